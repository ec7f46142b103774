"""BGZF inflate on the device (csvgpu_bgzf_inflate / _dev, kernels/inflate.hip) against the host's decoders, alone and inside the run from a
file.

    python tools/bench_inflate.py --out profiles/device_inflate/device_inflate.json      # both chr22-sized files (30x ONT, 60x HiFi)
    python tools/bench_inflate.py --tech ont --alone-only --reps 10                       # e.g. under rocprofv3 --kernel-trace --stats

The file is the bench's own chr22-sized contig (bench.py's seeds) written with the project's writer at --level.
alone: every BGZF block of the file, in batches of --window-blocks blocks as the reader takes them.
       `dev`     csvgpu_bgzf_inflate_dev with the compressed bytes already on the device: the kernel's device time (the context's CSV_K_MISC
                 timer) and wall time of the calls, GB/s in and out by device time;
       `host_ptr` csvgpu_bgzf_inflate from the mapped file: wall time with both copies;
       `mirror_device` / `mirror_host`  bgzf::inflate_range_device and bgzf::inflate_range on --threads threads over the same batches
                 (csvhost_bgzf_inflate_file): the host figure to hold the others against.
       The share of declined blocks is reported; on this project's writer's files it must be 0, or the run names the blocks.
file:  host.run_bam on the file with inflate_on_device off and on taking turns in one process: medians and p10-p90 of the wall time and of the
       time the run waited for decoded contigs (ms_decode). The rule of DESIGN.md §7: the option becomes the default only in a pull request
       of its own, and only if its median beats the option-off median by more than the option-off run's own p10-p90 spread, on both files.
torch is imported first: it finds no device once the product library's copy of the HIP runtime is up in the process.
"""
import argparse
import json
import os
import sys
import tempfile
import time
import zlib

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
torch.cuda.set_device(0)

import contextsv_amd as cs                      # noqa: E402
from contextsv_amd import _lib, host            # noqa: E402
from bench import cpu_share, pin_to_gpu_numa, seed_of   # noqa: E402
from hmm_params import WGS_HMM                  # noqa: E402

CHR22 = 50_818_468


def spread(ms):
    a = np.asarray(ms, np.float64)
    return {"median_ms": round(float(np.median(a)), 4), "p10_ms": round(float(np.percentile(a, 10)), 4), "p90_ms": round(float(np.percentile(a, 90)), 4), "n": int(len(a))}


def block_table(raw):
    """csv_bgzf_block records of every member of a BGZF file (offsets into the file, outputs back to back)"""
    rows, o, acc = [], 0, 0
    n = len(raw)
    while o < n:
        xlen = int(raw[o + 10]) | int(raw[o + 11]) << 8
        bsize, p = None, o + 12
        while p < o + 12 + xlen:
            slen = int(raw[p + 2]) | int(raw[p + 3]) << 8
            if raw[p] == 66 and raw[p + 1] == 67 and slen == 2:
                bsize = (int(raw[p + 4]) | int(raw[p + 5]) << 8) + 1
            p += 4 + slen
        data_off = 12 + xlen
        crc, isize = (int(x) for x in np.frombuffer(raw[o + bsize - 8: o + bsize].tobytes(), "<u4"))
        rows.append((o + data_off, acc, bsize - data_off - 8, isize, crc, 0))
        acc += isize
        o += bsize
    return np.array(rows, _lib.BGZF_BLOCK_DTYPE), acc


def alone(args, path, ctx):
    raw = np.memmap(path, np.uint8, "r")
    blocks, total_out = block_table(raw)
    W = max(args.window_blocks, 1)
    batches = []
    for i in range(0, len(blocks), W):
        b = blocks[i: i + W].copy()
        lo, hi = int(b["in_off"][0]), int(b["in_off"][-1]) + int(b["in_len"][-1])
        o0 = int(b["out_off"][0])
        b["in_off"] -= lo
        b["out_off"] -= o0
        batches.append((lo, hi, b, int(b["out_off"][-1]) + int(b["out_len"][-1])))
    largest_in, largest_out = max(h - l for l, h, _, _ in batches), max(n for _, _, _, n in batches)
    out = {"blocks": int(len(blocks)), "batches": len(batches), "in_bytes": int(len(raw)), "out_bytes": int(total_out), "window_blocks": W}

    # the reference bytes: zlib's decode of the first batch, against which both device forms are held once
    l0, h0, b0, n0 = batches[0]
    want = b"".join(zlib.decompress(raw[l0 + int(r["in_off"]): l0 + int(r["in_off"]) + int(r["in_len"])].tobytes(), -15) for r in b0)

    # dev: the compressed bytes of every batch on the device
    d_comp = [torch.from_numpy(np.ascontiguousarray(raw[l:h])).cuda() for l, h, _, _ in batches]
    d_out = torch.empty(max(largest_out, 1), dtype=torch.uint8, device="cuda")
    d_status = torch.empty(W, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    declined = []

    def dev_pass(record=False):
        for k, (l, h, b, n) in enumerate(batches):
            nd = ctx.bgzf_inflate_dev(d_comp[k], b, d_out, d_status)
            if record and nd:
                st = d_status[: len(b)].cpu().numpy()
                declined.extend(int(k * W + i) for i in np.flatnonzero(st))
    dev_pass(record=True)
    ctx.bgzf_inflate_dev(d_comp[0], b0, d_out, d_status)
    same_dev = d_out[:n0].cpu().numpy().tobytes() == want
    t_wall = []
    ctx.timing_enable(1)
    ctx.timing_reset()
    for _ in range(args.reps):
        t = time.perf_counter()
        dev_pass()
        t_wall.append((time.perf_counter() - t) * 1e3)
    ms_dev, groups = ctx.timing()["misc"]
    ctx.timing_enable(0)
    ms_dev /= args.reps
    out["dev"] = {"device_ms_per_pass": round(ms_dev, 4), "timer_groups_per_pass": groups / args.reps, "wall": spread(t_wall),
                  "GBps_in": round(len(raw) / ms_dev / 1e6, 3), "GBps_out": round(total_out / ms_dev / 1e6, 3), "equals_zlib_first_batch": bool(same_dev)}
    out["declined_blocks"] = len(declined)
    out["declined_share"] = len(declined) / max(len(blocks), 1)
    if declined:
        out["declined_block_indices"] = declined[:50]
    del d_comp

    # host_ptr: from the mapped file, both copies inside
    h_out = np.zeros(max(largest_out, 1), np.uint8)
    def host_ptr_pass():
        for l, h, b, n in batches:
            ctx.bgzf_inflate(raw[l:h], b, h_out)
    ctx.bgzf_inflate(raw[l0:h0], b0, h_out)
    same_host = h_out[:n0].tobytes() == want
    host_ptr_pass()
    t_hp = []
    for _ in range(args.reps):
        t = time.perf_counter()
        host_ptr_pass()
        t_hp.append((time.perf_counter() - t) * 1e3)
    out["host_ptr"] = {"wall": spread(t_hp), "GBps_out": round(total_out / np.median(t_hp) / 1e6, 3), "equals_zlib_first_batch": bool(same_host)}

    # the mirror's two routes over the same batches, taking turns
    t_md, t_mh = [], []
    for _ in range(args.reps + 1):
        t_md.append(host.bgzf_inflate_file(path, args.threads, ctx, W)["ms"])
        t_mh.append(host.bgzf_inflate_file(path, args.threads, None, W)["ms"])
    out["mirror_device"] = {"wall": spread(t_md[1:]), "GBps_out": round(total_out / np.median(t_md[1:]) / 1e6, 3)}
    out["mirror_host"] = {"threads": args.threads, "wall": spread(t_mh[1:]), "GBps_out": round(total_out / np.median(t_mh[1:]) / 1e6, 3)}
    if not (same_dev and same_host):
        raise SystemExit("the device's bytes differ from zlib's")
    return out


def from_file(args, path, ctx, hmm):
    settings = {"off": False, "on": True}
    rows = {k: [] for k in settings}
    digest = {}
    for i in range(len(settings) * (args.steps + args.warmup)):
        name = list(settings)[i % len(settings)]
        t = time.perf_counter()
        calls, tid, st = host.run_bam(ctx, path, hmm, chromosomes=["chr22"], threads=args.threads, inflate_on_device=settings[name])
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
    out["on"]["median_gain_ms"] = round(off["median_ms"] - out["on"]["wall"]["median_ms"], 4)
    out["on"]["beats_off_by_more_than_its_spread"] = bool(out["on"]["median_gain_ms"] > width)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tech", choices=["ont", "hifi", "both"], default="both")
    ap.add_argument("--scale", type=float, default=1.0, help="of the chr22-sized contig")
    ap.add_argument("--level", type=int, default=1)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--window-blocks", type=int, default=2048)
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
    res = {"tool": "tools/bench_inflate.py", "pinned_to": pinned, "cpu_share": cpu_share(), "level": args.level, "files": []}
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
