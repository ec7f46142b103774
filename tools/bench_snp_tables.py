"""Resident SNP tables: the copy-number passes with their SNPs looked up on the device (Genome.snp_tables_resident ->
csvgpu_cn_decode_tables_many) against the route that queries them on the host and sends them up, alone and inside the whole-genome step.

    python tools/bench_snp_tables.py --out profiles/snp_tables/snp_tables.json      # both generated genomes (30x ONT, 60x HiFi)

step:  Genome.run (three lanes, like bench.py's step) with the tables off / on taking turns in one process, each with
       cn_observations_on_device off and on: medians and p10-p90 of ms_total, ms_cigar_cn and ms_split_cn; the records must be identical.
       The rule of DESIGN.md §7: an option becomes the default only if its median ms_total beats the option-off median by more than the
       option-off run's own p10-p90 spread, on both genomes. The default stays off here either way; the file says which way the rule falls.
alone: the regions of one genome-wide copy-number pass (the step's calls of at least --min-cnv positions, contig by contig) against SNP
       tables of the generated genomes' density, two comparisons:
       calls   Context.cn_decode (csvgpu_cn_decode_resident_many; the SNP arrays are made beforehand, so the host's query section is NOT in
               this number — only the checks and the tables' way up are) against Context.cn_decode_tables with a capacity given
               (csvgpu_cn_decode_tables_many, one call). Wall time of warm calls ending in a synchronise, and the device time of the two
               timer groups between events.
       mirror  the host mirror's CIGAR copy-number pass, contig by contig (host.cn_prediction, observations_on_device=True): without a table
               it runs the `cn: snp queries` section on the pool, DeviceObs::add and csvgpu_cn_decode_resident_many; with snp_table= it runs
               csvgpu_cn_decode_tables_many. The candidates' votes are in both. This is the section plus the host-fed call against the table
               call; one call per contig on both sides, where a run makes one for all contigs.
"""
import argparse
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
from bench_cn_observations import snp_table     # noqa: E402
from bench_split_groups import _Handle, spread   # noqa: E402
from hmm_params import WGS_HMM                  # noqa: E402

# (tables resident, cn_observations_on_device)
SETTINGS = {"off": (False, False), "tables": (True, False), "device_obs": (False, True), "device_obs+tables": (True, True)}


def one_genome(args, tech_name, depth, ctx, lanes, hmm):
    tech = 0 if tech_name == "ont" else 1
    config = 3 if tech == 0 else 4
    n_contigs = max(1, min(args.contigs, 24))
    lens = [max(200_000, int(GRCH38[k] * args.scale)) for k in range(n_contigs)]
    gen_threads = max(1, min(64, 2 * cpu_share()))
    g = host.Genome()
    for k in range(n_contigs):
        syn = host.SynthShard(seed_of(config, k), lens[k], depth, tech, gen_threads)
        g.add_synth(ctx, NAMES[k], k, syn, snp_seed=seed_of(config, k), with_snps=True)
        syn.free()
    out = {"tech": tech_name, "depth": depth, "contigs": n_contigs, "scale": args.scale}
    cap = max(1 << 16, 4 * n_contigs * 4096)
    state = {"tables": False}

    def step(name):
        tables, on_device = SETTINGS[name]
        if tables != state["tables"]:
            g.snp_tables_resident(tables)
            state["tables"] = tables
        t = time.perf_counter()
        calls, tid, st, stats = g.run(ctx, hmm, lanes=lanes, capacity=cap, copy=False, cn_observations_on_device=on_device)
        ctx.synchronize()
        return (time.perf_counter() - t) * 1e3, st, calls, tid, stats

    for _ in range(max(args.warmup, 1)):
        for name in SETTINGS:
            last = step(name)
    if not args.no_alone:
        _, _, calls, tid, stats = last
        calls, tid = calls.copy(), tid.copy()
        shards = [_Handle(g.contig_info(i)["shard"]) for i in range(len(g))]
        mean_cov = [float(s.mean_cov) for s in stats]
        tables = [snp_table(seed_of(config, k), lens[k]) for k in range(n_contigs)]
        dev = [ctx.snp_table(t["pos"], t["baf"], t["pfb"], t["has_pfb"]) for t in tables]
        per = []
        for k in range(n_contigs):
            c = calls[(tid == k) & (calls["end"] >= calls["start"]) & ((calls["end"] - calls["start"]) >= args.min_cnv)]
            per.append((np.ascontiguousarray(c["start"], np.uint32), np.ascontiguousarray(c["end"], np.uint32)))
        reg_off = np.concatenate([[0], np.cumsum([len(p[0]) for p in per])]).astype(np.uint64)
        rs, re = np.concatenate([p[0] for p in per]), np.concatenate([p[1] for p in per])
        ss = np.full(len(rs), args.sample_size, np.int32)
        so, sp, sb = [0], [], []
        for k in range(n_contigs):
            pos = tables[k]["pos"]
            for a, b in zip(*per[k]):
                lo, hi = np.searchsorted(pos, a, "left"), np.searchsorted(pos, b, "right")
                sp.append(pos[lo:hi]); sb.append(tables[k]["baf"][lo:hi]); so.append(so[-1] + hi - lo)
        cat = lambda v, dt: np.concatenate(v).astype(dt) if v else np.zeros(0, dt)
        arrays = (np.asarray(so, np.uint64), cat(sp, np.uint32), cat(sb, np.float64), np.zeros(so[-1]))
        head = (shards, mean_cov, reg_off, rs, re, ss)
        bound = int(np.maximum(ss, np.diff(arrays[0]).astype(np.int64)).sum() + 3 * so[-1])
        fed = lambda: ctx.cn_decode(hmm, *head, *arrays)
        looked_up = lambda: ctx.cn_decode_tables(hmm, shards, dev, *head[1:], capacity=bound)
        a, b = fed(), looked_up()
        same = b is not None and all(a[f].tobytes() == b[f].tobytes() for f in ("obs_off", "pos", "states", "loglik"))
        t_fed, t_tab = [], []
        for _ in range(args.reps):
            for times, f in ((t_fed, fed), (t_tab, looked_up)):
                t = time.perf_counter()
                f()
                ctx.synchronize()
                times.append((time.perf_counter() - t) * 1e3)
        events = {}
        for name, f in (("cn_decode_resident_many", fed), ("cn_decode_tables_many", looked_up)):
            ctx.timing_enable(1)
            ctx.timing_reset()
            for _ in range(10):
                f()
            tm = ctx.timing()
            ctx.timing_enable(0)
            events[name] = {k: {"ms_per_call": round(tm[k][0] / 10, 4), "groups_per_call": tm[k][1] / 10} for k in ("window", "viterbi")}
        # the mirror's pass per contig: SNP queries on the pool + host-fed decode, against the table call
        cands = [host.make_calls(per[k][0], per[k][1], np.ones(len(per[k][0]), np.int32)) for k in range(n_contigs)]
        live = [k for k in range(n_contigs) if len(per[k][0])]

        def mirror(with_table):
            return [host.cn_prediction(ctx, shards[k], cands[k], hmm, mean_cov[k], tables[k], split=False, sample_size=args.sample_size, min_cnv=args.min_cnv,
                                       observations_on_device=True, snp_table=dev[k] if with_table else None) for k in live]

        m_off, m_on = mirror(False), mirror(True)
        mirror_same = all(x.tobytes() == y.tobytes() for x, y in zip(m_off, m_on))
        t_m_off, t_m_on = [], []
        for _ in range(args.reps):
            for times, flag in ((t_m_off, False), (t_m_on, True)):
                t = time.perf_counter()
                mirror(flag)
                ctx.synchronize()
                times.append((time.perf_counter() - t) * 1e3)
        out["alone_mirror"] = {"contigs_with_candidates": len(live), "same_calls": bool(mirror_same),
                               "snp_queries_plus_cn_decode_resident_many": spread(t_m_off), "cn_decode_tables_many": spread(t_m_on)}
        same = same and mirror_same
        out["alone"] = {"regions": int(len(rs)), "snp_records": int(so[-1]), "observations": int(len(a["pos"])), "bound": bound, "tables_equal_fed": bool(same),
                        "cn_decode_resident_many_wall": spread(t_fed), "cn_decode_tables_many_wall": spread(t_tab), "device_event_time": events}
        for t in dev:
            t.free()
        if not same:
            raise SystemExit("the table route's decode differs from the host-fed one")
    if not args.alone_only:
        rows = {k: [] for k in SETTINGS}
        digest = {}
        for i in range(len(SETTINGS) * args.steps):
            name = list(SETTINGS)[i % len(SETTINGS)]
            wall, st, calls, tid, _ = step(name)
            rows[name].append((wall, st.ms_total, st.ms_cigar_cn, st.ms_split_cn))
            digest[name] = (calls.tobytes(), tid.tobytes())
        if len(set(digest.values())) != 1:
            raise SystemExit("the step's records differ with the option")
        out["step"] = {name: {"wall": spread([r[0] for r in v]), "ms_total": spread([r[1] for r in v]), "ms_cigar_cn": spread([r[2] for r in v]),
                              "ms_split_cn": spread([r[3] for r in v])} for name, v in rows.items()}
        out["step"]["same_records"] = True
        for base, on in (("off", "tables"), ("device_obs", "device_obs+tables")):
            off_t = out["step"][base]["ms_total"]
            width = off_t["p90_ms"] - off_t["p10_ms"]
            gain = off_t["median_ms"] - out["step"][on]["ms_total"]["median_ms"]
            out["step"][on]["against"] = base
            out["step"][on]["base_p10_p90_spread_ms"] = round(width, 4)
            out["step"][on]["median_gain_ms"] = round(gain, 4)
            out["step"][on]["beats_base_by_more_than_its_spread"] = bool(gain > width)
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
    ap.add_argument("--sample-size", type=int, default=20)
    ap.add_argument("--min-cnv", type=int, default=2000)
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
    res = {"tool": "tools/bench_snp_tables.py", "pinned_to": pinned, "lanes": len(lanes), "genomes": []}
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
