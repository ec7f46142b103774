"""Resident shards built on the device from BAM batches (csvgpu_shard_builder_*, RunParams::shard_on_device) against the upload route, inside
the run from a file and alone.

    python tools/bench_shard_build.py --out profiles/device_shard/device_shard.json      # both chr22-sized files (30x ONT, 60x HiFi)

The file is tools/bench_inflate.py's: the bench's own chr22-sized contig written with the project's writer at --level.
file:  host.run_bam on the file with four settings taking turns in one process — off, unpack_on_device, unpack + shard on the device, inflate +
       unpack + shard on the device: medians and p10-p90 of the wall time and of the time the run waited for decoded contigs (ms_decode); the
       calls must be identical. The rule of DESIGN.md §7 holds: an option goes on by default only if its gain is beyond the option-off spread on
       both files — and this one stays off whatever comes out.
alone: the file's decoded record stream appended to a builder in pieces of about --piece-mib MiB (`append`: wall time of all appends, the
       pieces' bytes resident), `finish` (the hand-over: pad, sortedness word, side arrays, the scan's split), `fetch_reads` (pos / flag / mapq)
       and `fetch_names` (offsets, bytes, hashes), `upload` of the host reader's arrays for comparison, and `alt_bases` for the contig's own
       pick list: every signature of the pipeline whose operation is 50 bases long, against the host loop on the same list (host.sig_alts).
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

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import contextsv_amd as cs                      # noqa: E402
from contextsv_amd import _lib, host            # noqa: E402
from bench import cpu_share, pin_to_gpu_numa, seed_of   # noqa: E402
from bench_inflate import CHR22, spread         # noqa: E402
from hmm_params import WGS_HMM                  # noqa: E402

SETTINGS = {"off": {}, "unpack": dict(unpack_on_device=True), "unpack_shard": dict(shard_on_device=True),
            "inflate_unpack_shard": dict(shard_on_device=True, inflate_on_device=True)}


def from_file(args, path, ctx, hmm):
    rows = {k: [] for k in SETTINGS}
    digest, resident = {}, {}
    names = list(SETTINGS)
    for i in range(len(names) * (args.steps + args.warmup)):
        name = names[i % len(names)]
        t = time.perf_counter()
        calls, tid, st = host.run_bam(ctx, path, hmm, chromosomes=["chr22"], threads=args.threads, **SETTINGS[name])
        wall = (time.perf_counter() - t) * 1e3
        digest[name] = (calls.tobytes(), tid.tobytes())
        resident[name] = int(st["contigs_resident"])
        if i >= len(names) * args.warmup:
            rows[name].append((wall, st["ms_decode"]))
    if len(set(digest.values())) != 1:
        raise SystemExit("the run's calls differ with the option")
    out = {name: {"wall": spread([r[0] for r in v]), "ms_decode": spread([r[1] for r in v]), "contigs_resident": resident[name]} for name, v in rows.items()}
    off = out["off"]["wall"]
    width = off["p90_ms"] - off["p10_ms"]
    out["same_calls"] = True
    out["n_calls"] = int(len(digest["off"][1]) // 4)
    out["off_p10_p90_spread_ms"] = round(width, 4)
    for name in names[1:]:
        out[name]["median_gain_ms"] = round(off["median_ms"] - out[name]["wall"]["median_ms"], 4)
        out[name]["beats_off_by_more_than_its_spread"] = bool(out[name]["median_gain_ms"] > width)
    return out


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
        offs.append(p)
        p += 4 + (int(stream[p]) | int(stream[p + 1]) << 8 | int(stream[p + 2]) << 16 | int(stream[p + 3]) << 24)
    return stream, np.array(offs, np.int64)


def timed(fn, reps):
    t_all, last = [], None
    for _ in range(reps):
        t = time.perf_counter()
        last = fn()
        t_all.append((time.perf_counter() - t) * 1e3)
    return spread(t_all), last


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
        pieces.append((lo, hi, (offs[a:b:args.anchor_every] - lo).astype(np.uint32)))
    bam = host.BamFile(path)
    want = bam.read_contig("chr22", want_seq=True, want_qnames=True, threads=args.threads)
    reads = cs.Reads(want["reads"].pos.copy(), want["reads"].flag.copy(), want["reads"].mapq.copy(), want["reads"].cigar_off.copy(), want["reads"].cigar.copy())
    seq_off, seq, depth_len = want["seq_off"].copy(), want["seq"].copy(), want["target_len"] + 1
    bam.close()
    out = {"records": int(len(offs)), "stream_bytes": int(len(stream)), "pieces": len(pieces), "cigar_words": int(reads.n_cigar), "seq_bytes": int(len(seq))}
    lib = ctx.lib
    dev = []
    for lo, hi, _ in pieces:                                   # the pieces' bytes resident, as behind csvgpu_bgzf_inflate_dev
        p = lib.csvgpu_dev_alloc(ctx.h, hi - lo)
        part = np.ascontiguousarray(stream[lo:hi])
        ctx._check(lib.csvgpu_upload(ctx.h, p, part.ctypes.data, hi - lo))
        dev.append(p)
    want_all = _lib.SB_SEQ | _lib.SB_NAMES | _lib.SB_NAME_HASH
    t_append, t_finish, t_free = [], [], []
    sh = None
    for rep in range(args.reps + 1):
        if sh is not None:
            sh.free()
        b = ctx.shard_builder(want_all, (len(offs), reads.n_cigar, len(seq), 64 * len(offs)) if args.reserve else None)
        t = time.perf_counter()
        for (lo, hi, anchors), p in zip(pieces, dev):
            rc, c = b.append_bam_ptr(p, hi - lo, anchors)
            if rc != 0 or c["consumed"] != hi - lo:
                raise SystemExit("append: rc %d, %r" % (rc, c))
        t_append.append((time.perf_counter() - t) * 1e3)
        t = time.perf_counter()
        sh = b.finish(depth_len)
        t_finish.append((time.perf_counter() - t) * 1e3)
    for p in dev:
        lib.csvgpu_dev_free(ctx.h, p)
    out["append"] = {"wall": spread(t_append[1:]), "reserve": bool(args.reserve), "note": "sizing pass + growth + writing pass per piece, bytes resident"}
    out["finish"] = {"wall": spread(t_finish[1:])}
    out["fetch_reads_small"], small = timed(lambda: sh.fetch_reads(want_cigar=False), args.reps)
    out["fetch_names"], nm = timed(sh.fetch_names, args.reps)
    same = all(np.array_equal(getattr(small, f), getattr(reads, f)) for f in ("pos", "flag", "mapq"))
    back = sh.fetch_reads()
    same = same and np.array_equal(back.cigar_off, reads.cigar_off) and np.array_equal(back.cigar, reads.cigar)
    same = same and [x.decode() for x in nm["names"]] == want["qnames"] and np.array_equal(nm["name_hash"], host.string_hashes(want["qnames"]))
    t_up = []
    for _ in range(args.reps + 1):
        t = time.perf_counter()
        up = ctx.upload(reads, depth_len)
        t_up.append((time.perf_counter() - t) * 1e3)
        up.free()
    out["upload_for_comparison"] = {"wall": spread(t_up[1:]), "note": "csvgpu_shard_upload of the host reader's arrays (pageable memory)"}
    # the contig's own pick list: every 50-base insertion / clip signature of the pipeline
    res = sh.pipeline()
    sig = sh.fetch(res)["sig_ins"]
    pick = sig[(sig["end"] - sig["start"] + 1) == 50]
    read, qpos = pick["read"].astype(np.uint32), (pick["qpos_kind"] >> 2).astype(np.uint32)
    ctx.timing_enable(1)
    ctx.timing_reset()
    out["alt_bases"], got = timed(lambda: ctx.alt_bases(sh, read, qpos, np.full(len(pick), 50)), args.reps)
    ms_dev, groups = ctx.timing()["misc"]
    ctx.timing_enable(0)
    out["alt_bases"].update(items=int(len(pick)), device_ms_per_call=round(ms_dev / max(groups, 1), 4))
    t = time.perf_counter()
    ref = host.sig_alts(pick, seq_off, seq)
    out["alt_bases"]["host_loop_ms"] = round((time.perf_counter() - t) * 1e3, 4)
    same = same and got == ref
    out["equals_host_route"] = bool(same)
    sh.free()
    if not same:
        raise SystemExit("the built shard differs from the host route")
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tech", choices=["ont", "hifi", "both"], default="both")
    ap.add_argument("--scale", type=float, default=1.0, help="of the chr22-sized contig")
    ap.add_argument("--level", type=int, default=1)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--piece-mib", type=int, default=128)
    ap.add_argument("--anchor-every", type=int, default=32)
    ap.add_argument("--reserve", action="store_true", help="alone: reserve the builder's arrays for the whole contig (no growth)")
    ap.add_argument("--with-seq", action="store_true", help="write the reads' sequences into the file (tools/bench_inflate.py's files have none: every ALT is N's)")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--steps", type=int, default=5, help="timed runs from the file per setting (the settings take turns)")
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
    res = {"tool": "tools/bench_shard_build.py", "with_seq": bool(args.with_seq), "pinned_to": pinned, "cpu_share": cpu_share(), "level": args.level, "files": []}
    with tempfile.TemporaryDirectory(dir=os.environ.get("TMPDIR", "/tmp")) as d:
        for tech_name, tech, depth, config in (("ont", 0, 30.0, 3), ("hifi", 1, 60.0, 4)):
            if args.tech not in (tech_name, "both"):
                continue
            path = os.path.join(d, tech_name + ".bam")
            t0 = time.perf_counter()
            syn = host.SynthShard(seed_of(config, 21), int(CHR22 * args.scale), depth, tech, max(1, min(64, 2 * cpu_share())), with_seq=args.with_seq)
            nbytes = syn.write_bam(path, "chr22", level=args.level, threads=args.threads)
            one = {"tech": tech_name, "depth": depth, "scale": args.scale, "reads": int(syn.reads.n_reads), "bam_bytes": int(nbytes), "staging_s": round(time.perf_counter() - t0, 1)}
            syn.free()
            if not args.alone_only:
                one["from_file"] = from_file(args, path, ctx, hmm)
            if not args.no_alone:
                one["alone"] = alone(args, path, ctx)
            res["files"].append(one)
            print(json.dumps(one), flush=True)
            os.remove(path)
            if args.out:                                      # (written after every file: a run cut short keeps what it measured)
                os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
                with open(args.out, "w") as f:
                    json.dump(res, f, indent=1)
                    f.write("\n")
    ctx.close()


if __name__ == "__main__":
    main()
