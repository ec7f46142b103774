"""BAM record unpacking on the device (csvgpu_bam_unpack / _dev, kernels/bamunpack.hip) against the host parser, alone and inside the run
from a file.

    python tools/bench_unpack.py --out profiles/device_unpack/device_unpack.json      # both chr22-sized files (30x ONT, 60x HiFi)
    python tools/bench_unpack.py --tech ont --alone-only --reps 10                     # e.g. under rocprofv3 --kernel-trace --stats

The file is tools/bench_inflate.py's: the bench's own chr22-sized contig written with the project's writer at --level.
alone: the decoded record stream of the file in pieces of about --piece-mib MiB cut at record boundaries (the reader's batches), anchors at
       every --anchor-every-th record (a BAI gives one per chunk and per 16 Kbp window) and, for comparison, ONE anchor per piece;
       `dev`        csvgpu_bam_unpack_dev with the bytes resident and the outputs on the device: device time (the context's CSV_K_MISC
                    timer) and wall time of the calls, GB/s of stream by device time;
       `host_ptr`   csvgpu_bam_unpack from host memory: wall time with the copies both ways;
       `reader_host` / `reader_device`  BamFile.read_contig with the host parser and with unpack_on_device, and `inflate_host` the host
                    inflate of the same file alone (csvhost_bgzf_inflate_file); `reader_device_chain` is the reader with inflate and unpack
                    both on the device (the decoded bytes stay there). `host_parser_beside_inflate_ms` = reader_host minus inflate_host is
                    DERIVED, a difference of two medians: it holds the record walk, BamReader::append, and whatever overlap of batches and
                    page faults the two runs do not share — the reader has no seam that times append alone.
file:  host.run_bam on the file with unpack_on_device off and on taking turns in one process: medians and p10-p90 of the wall time and of
       the time the run waited for decoded contigs (ms_decode). The rule of DESIGN.md §7 holds: the option stays off whatever comes out.
torch is imported first: it finds no device once the product library's copy of the HIP runtime is up in the process.
"""
import argparse
import gzip
import json
import os
import struct
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
torch.cuda.set_device(0)

import contextsv_amd as cs                      # noqa: E402
from contextsv_amd import host                  # noqa: E402
from bench import cpu_share, pin_to_gpu_numa, seed_of   # noqa: E402
from bench_inflate import CHR22, spread         # noqa: E402
from hmm_params import WGS_HMM                  # noqa: E402


def record_stream(path):
    """the file's decoded bytes behind the BAM header, and every record's offset"""
    with open(path, "rb") as f:
        data = gzip.decompress(f.read())
    l_text, = struct.unpack_from("<I", data, 4)
    o = 8 + l_text
    n_ref, = struct.unpack_from("<I", data, o)
    o += 4
    for _ in range(n_ref):
        l_name, = struct.unpack_from("<I", data, o)
        o += 8 + l_name
    stream = np.frombuffer(data, np.uint8)[o:]
    offs, p, n = [], 0, len(stream)
    while p + 4 <= n:
        bs = int(stream[p]) | int(stream[p + 1]) << 8 | int(stream[p + 2]) << 16 | int(stream[p + 3]) << 24
        offs.append(p)
        p += 4 + bs
    return stream, np.array(offs, np.int64)


def alone(args, path, ctx):
    stream, offs = record_stream(path)
    piece = args.piece_mib << 20
    cuts = [0]
    while cuts[-1] < len(offs):
        k = int(np.searchsorted(offs, offs[cuts[-1]] + piece))
        cuts.append(max(k, cuts[-1] + 1))
    pieces = []
    for a, b in zip(cuts[:-1], cuts[1:]):
        lo, hi = int(offs[a]), int(offs[b]) if b < len(offs) else len(stream)
        pieces.append((lo, hi, (offs[a:b:args.anchor_every] - lo).astype(np.uint32), b - a))
    out = {"records": int(len(offs)), "stream_bytes": int(len(stream)), "pieces": len(pieces), "anchor_every": args.anchor_every}
    want = host.BamFile(path).read_contig("chr22", want_seq=True, want_qnames=True, threads=args.threads)
    n, m, ns = want["reads"].n_reads, want["reads"].n_cigar, len(want["seq"])
    n_name = sum(len(q) for q in want["qnames"])
    assert n == len(offs)

    d_stream = [torch.from_numpy(np.ascontiguousarray(stream[lo:hi])).cuda() for lo, hi, _, _ in pieces]
    dev = dict(pos=torch.empty(n, dtype=torch.int32, device="cuda"), flag=torch.empty(n, dtype=torch.int16, device="cuda"),
               mapq=torch.empty(n, dtype=torch.uint8, device="cuda"), cigar_off=torch.empty(n + 1, dtype=torch.int64, device="cuda"),
               cigar=torch.empty(m, dtype=torch.int32, device="cuda"), seq_off=torch.empty(n + 1, dtype=torch.int64, device="cuda"),
               seq=torch.empty(max(ns, 1), dtype=torch.uint8, device="cuda"), name_off=torch.empty(n + 1, dtype=torch.int64, device="cuda"),
               name=torch.empty(max(n_name, 1), dtype=torch.uint8, device="cuda"), name_hash=torch.empty(n, dtype=torch.int64, device="cuda"))
    torch.cuda.synchronize()

    def dev_pass(one_anchor=False):
        at = [0, 0, 0, 0]                                   # records, CIGAR words, sequence bytes, name bytes so far
        for k, (lo, hi, anchors, _) in enumerate(pieces):
            view = {key: t[{"cigar": at[1], "seq": at[2], "name": at[3]}.get(key, at[0]):] for key, t in dev.items()}
            rc, c = ctx.bam_unpack_dev(d_stream[k], anchors[:1] if one_anchor else anchors, view, bases=(at[1], at[2], at[3]))
            if rc != 0 or c["consumed"] != hi - lo:
                raise SystemExit("piece %d: rc %d, %r" % (k, rc, c))
            at = [at[0] + c["n_kept"], at[1] + c["n_cigar"], at[2] + c["n_seq"], at[3] + c["n_name"]]
        return at
    assert dev_pass() == [n, m, ns, n_name]
    same = all(np.array_equal(dev[k].cpu().numpy().view(getattr(want["reads"], k).dtype), getattr(want["reads"], k)) for k in ("pos", "flag", "mapq", "cigar_off", "cigar"))
    same = same and np.array_equal(dev["seq"][:ns].cpu().numpy(), want["seq"]) and dev["name"][:n_name].cpu().numpy().tobytes() == "".join(want["qnames"]).encode()
    same = same and np.array_equal(dev["name_hash"].cpu().numpy().view(np.uint64), host.string_hashes(want["qnames"])[:n])
    for label, one in (("dev", False), ("dev_one_anchor", True)):
        t_wall = []
        ctx.timing_enable(1)
        ctx.timing_reset()
        reps = args.reps if not one else max(1, args.reps // 3)
        for _ in range(reps):
            t = time.perf_counter()
            dev_pass(one)
            t_wall.append((time.perf_counter() - t) * 1e3)
        ms_dev, groups = ctx.timing()["misc"]
        ctx.timing_enable(0)
        ms_dev /= reps
        out[label] = {"device_ms_per_pass": round(ms_dev, 4), "timer_groups_per_pass": groups / reps, "wall": spread(t_wall),
                      "GBps_stream": round(len(stream) / ms_dev / 1e6, 3), "Mrecords_per_s": round(len(offs) / ms_dev / 1e3, 3)}
    out["dev"]["equals_host_reader"] = bool(same)
    del d_stream, dev

    t_hp = []
    for _ in range(max(1, args.reps // 2) + 1):
        t = time.perf_counter()
        for lo, hi, anchors, _ in pieces:
            got = ctx.bam_unpack(stream[lo:hi], anchors, want_seq=True, want_names=True)
            assert got["status"] == 0
        t_hp.append((time.perf_counter() - t) * 1e3)
    out["host_ptr"] = {"wall": spread(t_hp[1:]), "note": "two calls per piece (sizing, then the arrays)"}

    t_rh, t_rd, t_rc, t_inf = [], [], [], []
    bam = host.BamFile(path)
    for _ in range(args.reps + 1):
        t = time.perf_counter(); bam.read_contig("chr22", want_seq=True, want_qnames=True, threads=args.threads); t_rh.append((time.perf_counter() - t) * 1e3)
        t = time.perf_counter(); bam.read_contig("chr22", want_seq=True, want_qnames=True, threads=args.threads, unpack_on_device=True); t_rd.append((time.perf_counter() - t) * 1e3)
        st_dev = bam.unpack_stats()
        t = time.perf_counter(); bam.read_contig("chr22", want_seq=True, want_qnames=True, threads=args.threads, unpack_on_device=True, inflate_on_device=True); t_rc.append((time.perf_counter() - t) * 1e3)
        st_chain = bam.unpack_stats()
        t_inf.append(host.bgzf_inflate_file(path, args.threads, None, 2048)["ms"])
    bam.close()
    out["reader_host"] = {"threads": args.threads, "wall": spread(t_rh[1:])}
    out["reader_device"] = {"threads": args.threads, "wall": spread(t_rd[1:]), "unpack_stats": st_dev}
    out["reader_device_chain"] = {"threads": args.threads, "wall": spread(t_rc[1:]), "unpack_stats": st_chain, "note": "inflate and unpack both on the device, kernel to kernel"}
    out["inflate_host"] = {"threads": args.threads, "wall": spread(t_inf[1:])}
    out["host_parser_beside_inflate_ms"] = round(out["reader_host"]["wall"]["median_ms"] - out["inflate_host"]["wall"]["median_ms"], 4)
    if not same:
        raise SystemExit("the device's arrays differ from the host reader's")
    return out


def from_file(args, path, ctx, hmm):
    settings = {"off": False, "on": True, "on_with_inflate": "chain"}
    rows = {k: [] for k in settings}
    digest = {}
    for i in range(len(settings) * (args.steps + args.warmup)):
        name = list(settings)[i % len(settings)]
        t = time.perf_counter()
        calls, tid, st = host.run_bam(ctx, path, hmm, chromosomes=["chr22"], threads=args.threads, unpack_on_device=settings[name] is not False,
                                      inflate_on_device=settings[name] == "chain")
        wall = (time.perf_counter() - t) * 1e3
        digest[name] = (calls.tobytes(), tid.tobytes())
        if i >= len(settings) * args.warmup:
            rows[name].append((wall, st["ms_decode"]))
    if len(set(digest.values())) != 1:
        raise SystemExit("the run's calls differ with the option")
    out = {name: {"wall": spread([r[0] for r in v]), "ms_decode": spread([r[1] for r in v])} for name, v in rows.items()}
    off = out["off"]["wall"]
    width = off["p90_ms"] - off["p10_ms"]
    out["same_calls"] = True
    out["off_p10_p90_spread_ms"] = round(width, 4)
    for name in ("on", "on_with_inflate"):
        out[name]["median_gain_ms"] = round(off["median_ms"] - out[name]["wall"]["median_ms"], 4)
        out[name]["beats_off_by_more_than_its_spread"] = bool(out[name]["median_gain_ms"] > width)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tech", choices=["ont", "hifi", "both"], default="both")
    ap.add_argument("--scale", type=float, default=1.0, help="of the chr22-sized contig")
    ap.add_argument("--level", type=int, default=1)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--piece-mib", type=int, default=128)
    ap.add_argument("--anchor-every", type=int, default=32)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--steps", type=int, default=7, help="timed runs from the file per setting (the settings take turns)")
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--alone-only", action="store_true")
    ap.add_argument("--no-alone", action="store_true")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    pinned = pin_to_gpu_numa(0)
    ctx = cs.Context(0)
    host.set_context(ctx)
    host.load().csvhost_set_quiet(1)
    hmm = cs.make_hmm(**WGS_HMM)
    res = {"tool": "tools/bench_unpack.py", "pinned_to": pinned, "cpu_share": cpu_share(), "level": args.level, "files": []}
    with tempfile.TemporaryDirectory(dir=os.environ.get("TMPDIR", "/tmp")) as d:
        for tech_name, tech, depth, config in (("ont", 0, 30.0, 3), ("hifi", 1, 60.0, 4)):
            if args.tech not in (tech_name, "both"):
                continue
            path = os.path.join(d, tech_name + ".bam")
            t0 = time.perf_counter()
            syn = host.SynthShard(seed_of(config, 21), int(CHR22 * args.scale), depth, tech, max(1, min(64, 2 * cpu_share())))
            nbytes = syn.write_bam(path, "chr22", level=args.level, threads=args.threads)
            one = {"tech": tech_name, "depth": depth, "scale": args.scale, "reads": int(syn.reads.n_reads), "bam_bytes": int(nbytes), "staging_s": round(time.perf_counter() - t0, 1)}
            syn.free()
            if not args.no_alone:
                one["alone"] = alone(args, path, ctx)
            if not args.alone_only:
                one["from_file"] = from_file(args, path, ctx, hmm)
            res["files"].append(one)
            print(json.dumps(one), flush=True)
            os.remove(path)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
    ctx.close()


if __name__ == "__main__":
    main()
