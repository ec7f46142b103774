"""Overlap groups of the split-read pass: the host's interval tree (host.split_groups_host) against the device form
(Context.split_groups -> csvgpu_split_groups), alone and inside the whole-genome step.

    python tools/bench_split_groups.py --out profiles/<round>/split_groups.json            # both generated genomes (30x ONT, 60x HiFi)
    python tools/bench_split_groups.py --tech hifi --alone-only --reps 20                  # e.g. under rocprofv3 --kernel-trace --stats
    CSV_TRACE=1 python tools/bench_split_groups.py --tech hifi --steps 2 --no-alone        # the split chain's host sections on stderr

alone: the members of every contig of the genome — the primaries with a supplementary record, in the iteration order of the contig's
qname map (csvgpu_split_order on the staged shards), start = pos + 1, end = the scan's ref_end — as ONE call of 24 segments; wall time
of a warm call ending in a synchronise, `--reps` repetitions.
step: Genome.run (three lanes, like bench.py's step) with split_groups_on_device off and on, alternating in one process.
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import contextsv_amd as cs                      # noqa: E402
from contextsv_amd import host                  # noqa: E402
from bench import GRCH38, NAMES, cpu_share, pin_to_gpu_numa, seed_of   # noqa: E402
from hmm_params import WGS_HMM                  # noqa: E402


def spread(ms):
    a = np.sort(np.asarray(ms, dtype=np.float64))
    return {"n": int(len(a)), "median_ms": round(float(np.median(a)), 4), "min_ms": round(float(a[0]), 4), "p10_ms": round(float(np.quantile(a, 0.1)), 4),
            "p90_ms": round(float(np.quantile(a, 0.9)), 4), "max_ms": round(float(a[-1]), 4)}


class _Handle:
    def __init__(self, h):
        self.h = h


def members_of(ctx, g, pos_of, supp_hash):
    """-> (start, end, seg_off): every contig's surviving primaries in map iteration order. Needs one run behind it (the scan's intervals)."""
    shards = [_Handle(g.contig_info(i)["shard"]) for i in range(len(g))]
    order = ctx.split_order(shards, 20, supp_hash)
    ss, ee, off = [], [], [0]
    for i, rec in enumerate(order):
        rec = np.ascontiguousarray(rec, np.uint32)
        e, qs, qe = (np.zeros(max(len(rec), 1), np.int32) for _ in range(3))
        ctx._check(ctx.lib.csvgpu_aln_intervals_gather_resident(ctx.h, shards[i].h, rec.ctypes.data, len(rec), e.ctypes.data, qs.ctypes.data, qe.ctypes.data))
        ss.append(pos_of[i][rec] + 1)
        ee.append(e[: len(rec)])
        off.append(off[-1] + len(rec))
    return np.concatenate(ss).astype(np.int32), np.concatenate(ee).astype(np.int32), np.asarray(off, dtype=np.uint64)


def one_genome(args, tech_name, depth, ctx, lanes, hmm):
    tech = 0 if tech_name == "ont" else 1
    config = 3 if tech == 0 else 4
    n_contigs = max(1, min(args.contigs, 24))
    lens = [max(200_000, int(GRCH38[k] * args.scale)) for k in range(n_contigs)]
    gen_threads = max(1, min(64, 2 * cpu_share()))
    g = host.Genome()
    pos_of, supp_names = [], []
    n_reads = 0
    t0 = time.perf_counter()
    for k in range(n_contigs):
        syn = host.SynthShard(seed_of(config, k), lens[k], depth, tech, gen_threads)
        g.add_synth(ctx, NAMES[k], k, syn, snp_seed=seed_of(config, k), with_snps=True)
        r = syn.reads
        n_reads += int(r.n_reads)
        pos_of.append(r.pos.copy())
        keep = ((r.flag & 0x800) != 0) & ((r.flag & (0x100 | 0x4 | 0x400 | 0x200)) == 0) & (r.mapq >= 20)
        supp_names += ["r%d_%d" % (k, q) for q in syn.qname_id[keep].tolist()]
        syn.free()
    supp_hash = np.unique(host.string_hashes(supp_names)) if supp_names else np.zeros(0, np.uint64)
    out = {"tech": tech_name, "depth": depth, "contigs": n_contigs, "scale": args.scale, "reads": n_reads, "staging_s": round(time.perf_counter() - t0, 1)}
    cap = max(1 << 16, 4 * n_contigs * 4096)

    def step(on):
        t = time.perf_counter()
        calls, tid, st, _ = g.run(ctx, hmm, lanes=lanes, capacity=cap, copy=False, split_groups_on_device=on)
        ctx.synchronize()
        return (time.perf_counter() - t) * 1e3, st, calls, tid

    for _ in range(max(args.warmup, 1)):
        step(False)
        step(True)
    if not args.no_alone:
        s, e, off = members_of(ctx, g, pos_of, supp_hash)
        want = host.split_groups_host(s, e, off)
        got = ctx.split_groups(s, e, off)
        same = all(np.array_equal(np.asarray(a, np.uint64), np.asarray(b, np.uint64)) for a, b in zip(got, want))
        sizes = np.diff(want[1].astype(np.int64))
        t_host, t_dev = [], []
        for _ in range(args.reps):
            t = time.perf_counter()
            host.split_groups_host(s, e, off)
            t_host.append((time.perf_counter() - t) * 1e3)
            t = time.perf_counter()
            ctx.split_groups(s, e, off)
            ctx.synchronize()
            t_dev.append((time.perf_counter() - t) * 1e3)
        ctx.timing_enable(1)
        ctx.timing_reset()
        for _ in range(10):
            ctx.split_groups(s, e, off)
        ms, groups = ctx.timing()["split_groups"]
        ctx.timing_enable(0)
        out["alone"] = {"members": int(len(s)), "segments": int(len(off) - 1), "largest_segment": int(np.diff(off.astype(np.int64)).max()),
                        "groups": int(len(sizes)), "group_members": int(sizes.sum()), "largest_group": int(sizes.max()) if len(sizes) else 0,
                        "device_equals_host": bool(same), "host_tree_one_thread": spread(t_host), "device_call": spread(t_dev),
                        "device_event_ms_per_call": round(ms / 10, 4), "timer_groups_per_call": groups / 10}
        if not same:
            raise SystemExit("device groups differ from the host tree's")
    if not args.alone_only:
        rows = {False: [], True: []}
        digest = {}
        for i in range(2 * args.steps):
            on = bool(i & 1)
            wall, st, calls, tid = step(on)
            rows[on].append((wall, st.ms_total, st.ms_split, st.ms_split_prepare))
            digest[on] = (calls.tobytes(), tid.tobytes())
        if digest[False] != digest[True]:
            raise SystemExit("the step's records differ with the option")
        out["step"] = {("on" if on else "off"): {"wall": spread([r[0] for r in v]), "ms_total": spread([r[1] for r in v]), "ms_split": spread([r[2] for r in v]),
                                                 "ms_split_prepare": spread([r[3] for r in v])} for on, v in rows.items()}
        out["step"]["same_records"] = True
    g.free()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tech", choices=["ont", "hifi", "both"], default="both")
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--contigs", type=int, default=24)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--steps", type=int, default=20, help="timed steps per setting (off / on alternate)")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--lanes", type=int, default=3)
    ap.add_argument("--alone-only", action="store_true")
    ap.add_argument("--no-alone", action="store_true")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    pinned = pin_to_gpu_numa(0)
    gate = cs.Gate(0)
    ctx = cs.Context(0)
    host.set_context(ctx)
    host.load().csvhost_set_quiet(1)
    lanes = [cs.Context(0) for _ in range(args.lanes)] if args.lanes > 1 else []
    for c in lanes:
        c.set_gate(gate)
    hmm = cs.make_hmm(**WGS_HMM)
    res = {"tool": "tools/bench_split_groups.py", "pinned_to": pinned, "lanes": len(lanes), "genomes": []}
    for tech_name, depth in (("ont", 30.0), ("hifi", 60.0)):
        if args.tech in (tech_name, "both"):
            res["genomes"].append(one_genome(args, tech_name, depth, ctx, lanes, hmm))
            print(json.dumps(res["genomes"][-1]), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
    for c in lanes:
        c.set_gate(None)
        c.close()
    gate.close()
    ctx.close()


if __name__ == "__main__":
    main()
