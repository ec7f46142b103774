"""The evidence of the split-read pass's overlap groups (point sets, DBSCAN1D fits, largest clusters, medians, strand vote): the host route
(host.split_fits_host: sets and reductions on one thread, one csvgpu_dbscan_1d batch) against the device entry points
(Context.split_fits -> csvgpu_split_fits on given groups, csvgpu_split_groups_fits with the groups computed and kept on the device,
Context.split_resident_fits -> csvgpu_split_resident_fits with the tables built on the device from the resident shards too), alone and inside
the whole-genome step.

    python tools/bench_split_fits.py --out profiles/split_fits/split_fits.json             # both generated genomes (30x ONT, 60x HiFi)
    python tools/bench_split_fits.py --tech hifi --alone-only --reps 20                    # e.g. under rocprofv3 --kernel-trace --stats

alone: the members of every contig of the genome — the primaries with a supplementary record, in the iteration order of the contig's
qname map — with their supplementary records, as ONE call of 24 segments; wall time of a warm call ending in a synchronise.
       The tables' row: csvgpu_split_resident_fits on record references against the two device calls of the route it replaces — the
       interval gather and csvgpu_split_groups_fits — without the tables' assembly on the host between them (C++ on the pool in the run; not
       timed here, so the row is a lower bound of what is replaced).
step: Genome.run (three lanes, like bench.py's step) with split_fits_on_device off, on, on together with split_groups_on_device, and with
split_tables_on_device, taking turns in one process.
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
sys.path.insert(0, os.path.join(ROOT, "tools"))

import contextsv_amd as cs                      # noqa: E402
from contextsv_amd import host                  # noqa: E402
from bench import GRCH38, NAMES, cpu_share, pin_to_gpu_numa, seed_of   # noqa: E402
from bench_split_groups import _Handle, spread   # noqa: E402
from hmm_params import WGS_HMM                  # noqa: E402


def plan_of(ctx, g, per_contig, supp_hash):
    """Which records take part: -> (shards, per contig (members' records in map order, their supplementary records, entries per member), SplitRefs, seg_off).
    Every name of a generated genome lives on one contig, so every entry is a record of the member's own shard."""
    shards = [_Handle(g.contig_info(i)["shard"]) for i in range(len(g))]
    order = ctx.split_order(shards, 20, supp_hash)
    plan, seg_off, supp_off = [], [0], [np.zeros(1, np.int64)]
    n_supp = 0
    for i, rec in enumerate(order):
        pos, flag, qid, srec = per_contig[i]
        rec = np.ascontiguousarray(rec, np.uint32)
        srec = srec[np.argsort(qid[srec], kind="stable")]                       # by name, file order within a name
        lo, hi = np.searchsorted(qid[srec], qid[rec], "left"), np.searchsorted(qid[srec], qid[rec], "right")
        pick = np.concatenate([srec[a:b] for a, b in zip(lo, hi)]) if len(rec) else np.zeros(0, np.int64)
        plan.append((rec, np.ascontiguousarray(pick, np.uint32), hi - lo))
        supp_off.append(n_supp + np.cumsum(hi - lo))
        n_supp += len(pick)
        seg_off.append(seg_off[-1] + len(rec))
    refs = cs.SplitRefs(np.concatenate([p[0] for p in plan]), np.concatenate(supp_off).astype(np.uint64), np.concatenate([p[1] for p in plan]),
                        np.zeros(n_supp, np.uint8))
    return shards, plan, refs, np.asarray(seg_off, np.uint64)


def gather_of(ctx, shards, plan):
    """-> (call, rec_off, outputs): `call()` is csvgpu_aln_intervals_gather_batch for every record that takes part, on arrays made here."""
    want = np.ascontiguousarray(np.concatenate([np.concatenate([rec, pick]) for rec, pick, _ in plan]), np.uint32)
    rec_off = np.zeros(len(plan) + 1, np.uint64)
    rec_off[1:] = np.cumsum([len(rec) + len(pick) for rec, pick, _ in plan])
    out = tuple(np.zeros(max(len(want), 1), np.int32) for _ in range(3))
    hs = (C.c_void_p * len(shards))(*[sh.h for sh in shards])

    def call():
        ctx._check(ctx.lib.csvgpu_aln_intervals_gather_batch(ctx.h, len(shards), hs, want.ctypes.data, rec_off.ctypes.data, *[x.ctypes.data for x in out]))
        return hs, want
    return call, rec_off, out


def tables_of(ctx, shards, plan, per_contig, supp_off):
    """-> SplitTables: the interval gather and the tables assembled on the host (what csvgpu_split_resident_fits leaves out; the run's own host route
    assembles them in C++ on the pool, this one in numpy: it is not timed). Needs one run behind it (the scan's intervals are read from the resident
    shards)."""
    cols = {k: [] for k in ("start", "end", "q_start", "q_end", "reverse", "supp_start", "supp_end", "supp_q_start", "supp_q_end", "supp_flags")}
    call, rec_off, (e, qs, qe) = gather_of(ctx, shards, plan)
    call()
    for i, (rec, pick, _) in enumerate(plan):
        pos, flag, qid, srec = per_contig[i]
        a, m, b = int(rec_off[i]), int(rec_off[i]) + len(rec), int(rec_off[i + 1])
        cols["start"].append(pos[rec] + 1); cols["end"].append(e[a:m]); cols["q_start"].append(qs[a:m]); cols["q_end"].append(qe[a:m])
        cols["reverse"].append(((flag[rec] & 0x10) != 0).astype(np.uint8))
        cols["supp_start"].append(pos[pick] + 1); cols["supp_end"].append(e[m:b]); cols["supp_q_start"].append(qs[m:b])
        cols["supp_q_end"].append(qe[m:b]); cols["supp_flags"].append(((flag[pick] & 0x10) != 0).astype(np.uint8))
    return cs.SplitTables(supp_off=supp_off, **{k: np.concatenate(v) for k, v in cols.items()})


SETTINGS = {"off": {}, "fits": {"split_fits_on_device": True}, "fits+groups": {"split_fits_on_device": True, "split_groups_on_device": True},
            "tables": {"split_tables_on_device": True}}


def one_genome(args, tech_name, depth, ctx, lanes, hmm):
    tech = 0 if tech_name == "ont" else 1
    config = 3 if tech == 0 else 4
    n_contigs = max(1, min(args.contigs, 24))
    lens = [max(200_000, int(GRCH38[k] * args.scale)) for k in range(n_contigs)]
    gen_threads = max(1, min(64, 2 * cpu_share()))
    g = host.Genome()
    per_contig, supp_names = [], []
    n_reads = 0
    t0 = time.perf_counter()
    for k in range(n_contigs):
        syn = host.SynthShard(seed_of(config, k), lens[k], depth, tech, gen_threads)
        g.add_synth(ctx, NAMES[k], k, syn, snp_seed=seed_of(config, k), with_snps=True)
        r = syn.reads
        n_reads += int(r.n_reads)
        keep = ((r.flag & 0x800) != 0) & ((r.flag & (0x100 | 0x4 | 0x400 | 0x200)) == 0) & (r.mapq >= 20)
        per_contig.append((r.pos.copy(), r.flag.copy(), syn.qname_id.copy(), np.flatnonzero(keep)))
        supp_names += ["r%d_%d" % (k, q) for q in syn.qname_id[keep].tolist()]
        syn.free()
    supp_hash = np.unique(host.string_hashes(supp_names)) if supp_names else np.zeros(0, np.uint64)
    out = {"tech": tech_name, "depth": depth, "contigs": n_contigs, "scale": args.scale, "reads": n_reads, "staging_s": round(time.perf_counter() - t0, 1)}
    cap = max(1 << 16, 4 * n_contigs * 4096)

    def step(kw):
        t = time.perf_counter()
        calls, tid, st, _ = g.run(ctx, hmm, lanes=lanes, capacity=cap, copy=False, **kw)
        ctx.synchronize()
        return (time.perf_counter() - t) * 1e3, st, calls, tid

    for _ in range(max(args.warmup, 1)):
        for kw in SETTINGS.values():
            step(kw)
    if not args.no_alone:
        shards, plan, refs, off = plan_of(ctx, g, per_contig, supp_hash)
        T = tables_of(ctx, shards, plan, per_contig, refs.supp_off)
        groups = host.split_groups_host(T.start, T.end, off)
        want = host.split_fits_host(ctx, T, off, groups)
        same = ctx.split_fits(T, off, groups)[1].tobytes() == want.tobytes() and ctx.split_fits(T, off)[1].tobytes() == want.tobytes()
        same = same and ctx.split_resident_fits(shards, refs, off)[1].tobytes() == want.tobytes()
        gather, _, _ = gather_of(ctx, shards, plan)
        t_host, t_given, t_fused, t_groups, t_resident, t_gather = [], [], [], [], [], []
        for _ in range(args.reps):
            for times, f in ((t_host, lambda: host.split_fits_host(ctx, T, off, groups)), (t_given, lambda: ctx.split_fits(T, off, groups)),
                             (t_fused, lambda: ctx.split_fits(T, off)), (t_groups, lambda: ctx.split_groups(T.start, T.end, off)),
                             (t_resident, lambda: ctx.split_resident_fits(shards, refs, off)),
                             (t_gather, gather)):
                t = time.perf_counter()
                f()
                ctx.synchronize()
                times.append((time.perf_counter() - t) * 1e3)
        ctx.timing_enable(1)
        ctx.timing_reset()
        for _ in range(10):
            ctx.split_fits(T, off, groups)
        ms, launches = ctx.timing()["split_fits"]
        ctx.timing_reset()
        for _ in range(10):
            ctx.split_resident_fits(shards, refs, off)
        tm = ctx.timing()
        ctx.timing_enable(0)
        sizes = want["n_members"].astype(np.int64)
        out["alone"] = {"members": int(T.n_members), "supplementary": int(T.n_supp), "segments": int(len(off) - 1), "groups": int(len(want)),
                        "group_members": int(sizes.sum()), "largest_group": int(sizes.max()) if len(sizes) else 0,
                        "groups_with_a_cluster_per_set": (want["size"] > 0).sum(axis=0).tolist(), "device_equals_host": bool(same),
                        "host_route_one_thread": spread(t_host), "split_fits_given_groups": spread(t_given), "split_groups_fits_fused": spread(t_fused),
                        "split_groups_alone": spread(t_groups), "device_event_ms_per_call": round(ms / 10, 4), "timer_groups_per_call": launches / 10,
                        "split_resident_fits": spread(t_resident), "interval_gather": spread(t_gather),
                        # what split_resident_fits replaces, WITHOUT the tables' assembly on the host between the two (membersOf and the flattening, C++ on
                        # the pool in the run, are not timed here): a lower bound of the replaced route
                        "gather_plus_groups_fits_fused": spread([a + b for a, b in zip(t_gather, t_fused)]),
                        "resident_fits_timer_groups_per_call": {k: tm[k][1] / 10 for k in ("misc", "split_groups", "split_fits")},
                        "resident_fits_device_event_ms_per_call": {k: round(tm[k][0] / 10, 4) for k in ("misc", "split_groups", "split_fits")}}
        if not same:
            raise SystemExit("device fits differ from the host route's")
    if not args.alone_only:
        rows = {k: [] for k in SETTINGS}
        digest = {}
        for i in range(len(SETTINGS) * args.steps):
            name = list(SETTINGS)[i % len(SETTINGS)]
            wall, st, calls, tid = step(SETTINGS[name])
            rows[name].append((wall, st.ms_total, st.ms_split, st.ms_split_prepare))
            digest[name] = (calls.tobytes(), tid.tobytes())
        if len(set(digest.values())) != 1:
            raise SystemExit("the step's records differ with the option")
        out["step"] = {name: {"wall": spread([r[0] for r in v]), "ms_total": spread([r[1] for r in v]), "ms_split": spread([r[2] for r in v]),
                              "ms_split_prepare": spread([r[3] for r in v])} for name, v in rows.items()}
        off_t = out["step"]["off"]["ms_total"]
        width = off_t["p90_ms"] - off_t["p10_ms"]
        out["step"]["same_records"] = True
        out["step"]["off_p10_p90_spread_ms"] = round(width, 4)
        for name in [k for k in SETTINGS if k != "off"]:
            out["step"][name]["median_gain_ms"] = round(off_t["median_ms"] - out["step"][name]["ms_total"]["median_ms"], 4)
            out["step"][name]["beats_off_by_more_than_its_spread"] = bool(out["step"][name]["median_gain_ms"] > width)
    g.free()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tech", choices=["ont", "hifi", "both"], default="both")
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--contigs", type=int, default=24)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--steps", type=int, default=20, help="timed steps per setting (the settings take turns)")
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
    res = {"tool": "tools/bench_split_fits.py", "pinned_to": pinned, "lanes": len(lanes), "genomes": []}
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
