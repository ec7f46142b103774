"""mergeSVs' representatives on the device (csvgpu_chr_merge_select, SVCaller::merge_on_device) against the host merge.

    python tools/bench_merge_select.py --out profiles/merge_select        # every shard, every step, one child process per step

Without --step the tool only drives: every GPU step is a child process of its own under `timeout -k 10`, the steps chained with `&&` (a
step that faults or hangs ends the chain). The steps, per shard (chr1- and chr22-sized 30x ONT, chr22-sized 60x HiFi, generated):
select  the device select alone on the results of one pipeline: device time between events and per launch group (csvgpu_timing_get,
        CSV_K_MISC) and wall time of the call; SVCaller::mergeOrdered on the fetched signatures (host.merge_ordered: the pool form a lone
        contig takes, and with --host-threads 1 one thread); the bytes a contig's fetch moves either way (20 per signature against 32 per
        record + 32); the records must be the host's calls.
step    processResidentChromosomesPipelined over the one shard (the chr1-only rank of DESIGN.md §6.1), the option off / on taking turns in
        one process: at least five pairs, medians, and the off-off spread (p10-p90 of the off runs) that a difference has to beat.
Each step writes <out>/<shard>_<step>.json; profiles/merge_select/README.md holds the table and the sentence that decides a later default.
"""
import argparse
import json
import os
import shlex
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHARDS = {                                   # name: (contig length, depth, tech 0 ONT / 1 HiFi)
    "chr1_ont30": (248_956_422, 30.0, 0),
    "chr22_ont30": (50_818_468, 30.0, 0),
    "chr22_hifi60": (50_818_468, 60.0, 1),
}


def spread(x):
    x = np.sort(np.asarray(x, float))
    return dict(median=float(np.median(x)), p10=float(np.percentile(x, 10)), p90=float(np.percentile(x, 90)), n=len(x))


def staged(name, threads):
    import contextsv_amd as cs
    from contextsv_amd import host
    L, depth, tech = SHARDS[name]
    ctx = cs.Context(0)
    host.set_context(ctx)
    syn = host.SynthShard(0x5E1EC7 + tech, L, depth, tech, threads)
    sh = ctx.upload(syn.reads, syn.depth_len)
    syn.free()
    return ctx, sh


def step_select(name, args):
    from contextsv_amd import host
    ctx, sh = staged(name, args.threads)
    res = sh.pipeline()
    f = sh.fetch(res)
    sig, labels = np.concatenate([f["sig_del"], f["sig_ins"]]), np.concatenate([f["label_del"], f["label_ins"]])
    rec, counts = sh.merge_select(res)                       # warm: the shard's select scratch is allocated here
    calls, _ = host.merge_ordered(sig, labels, res.n_del, 1)
    assert len(calls) == len(rec) and np.array_equal(calls["start"], rec["start"]) and np.array_equal(calls["end"], rec["end"]) and \
        np.array_equal(calls["cluster_size"], rec["cluster_size"]), "the device's records are not the host's calls"
    wall = []
    ctx.timing_enable(1); ctx.timing_reset()
    for _ in range(args.reps):
        t0 = time.perf_counter(); sh.merge_select(res); wall.append((time.perf_counter() - t0) * 1e3)
    ms, n = ctx.timing()["misc"]
    ctx.timing_enable(0)
    _, host_ms = host.merge_ordered(sig, labels, res.n_del, args.reps)
    out = dict(shard=name, n_sig=int(res.n_sig), n_del=int(res.n_del), n_rep=len(rec), n_declined=list(counts["n_declined"]),
               largest_bucket=int(max(np.bincount(labels[: res.n_del] + 2).max(initial=0), np.bincount(labels[res.n_del:] + 2).max(initial=0))),
               device_select_ms_events=ms / max(n, 1), device_select_wall_ms=spread(wall), host_merge_ordered_ms=host_ms,
               host_threads=args.host_threads or "pool", bytes_fetch_off=int(res.n_sig) * 20, bytes_fetch_on=len(rec) * 32 + 32)
    sh.free(); ctx.close()
    return out


def step_step(name, args):
    from contextsv_amd import host
    ctx, sh = staged(name, args.threads)
    host.process_resident_pipelined(ctx, sh, 2, 0.1, 0.1)
    host.process_resident_pipelined(ctx, sh, 2, 0.1, 0.1, merge_on_device=True)
    off, on = [], []
    want = None
    host.merge_route_stats(reset=True)
    for _ in range(max(args.pairs, 5)):
        for flag, dst in ((False, off), (True, on)):
            calls, _, st, ms, _ = host.process_resident_pipelined(ctx, sh, args.steps, 0.1, 0.1, merge_on_device=flag)
            want = calls.tobytes() if want is None else want
            assert calls.tobytes() == want, "the option changed the calls"
            dst.append(ms / args.steps)
    o, n = spread(off), spread(on)
    out = dict(shard=name, steps_per_run=args.steps, ms_per_step_off=o, ms_per_step_on=n, off_off_spread=o["p90"] - o["p10"],
               gain_ms=o["median"] - n["median"], beats_spread=bool(o["median"] - n["median"] > o["p90"] - o["p10"]), routes=host.merge_route_stats())
    sh.free(); ctx.close()
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "merge_select"))
    ap.add_argument("--shards", default=",".join(SHARDS))
    ap.add_argument("--step", choices=("select", "step"))
    ap.add_argument("--shard")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--pairs", type=int, default=7)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--threads", type=int, default=16, help="generator threads")
    ap.add_argument("--host-threads", type=int, default=0, help="0: the host pool; 1: mergeOrdered on one thread (OMP-style cap of the pool)")
    ap.add_argument("--limit", type=int, default=900, help="seconds a step may take")
    args = ap.parse_args()
    os.makedirs(args.out, exist_ok=True)
    if args.step:
        if args.host_threads:
            os.environ["CSV_HOST_THREADS"] = str(args.host_threads)
        r = (step_select if args.step == "select" else step_step)(args.shard, args)
        with open(os.path.join(args.out, "%s_%s.json" % (args.shard, args.step)), "w") as fh:
            json.dump(r, fh, indent=1)
        print(json.dumps(r))
        return 0
    # the driver: every GPU step a process of its own under its own time limit, chained with &&
    me = shlex.quote(os.path.abspath(__file__))
    common = "--out %s --reps %d --pairs %d --steps %d --threads %d --host-threads %d" % (shlex.quote(args.out), args.reps, args.pairs, args.steps, args.threads,
                                                                                        args.host_threads)
    cmds = ["timeout -k 10 %d %s %s --step %s --shard %s %s" % (args.limit, shlex.quote(sys.executable), me, step, shlex.quote(name), common)
            for name in args.shards.split(",") for step in ("select", "step")]
    return subprocess.run(["bash", "-c", " && ".join(cmds)]).returncode


if __name__ == "__main__":
    sys.exit(main())
