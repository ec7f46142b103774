"""The copy-number pass's observation vectors: the route that returns to the host twice (window launch, windows back, the vectors
assembled on the host pool, vectors up, Viterbi, states back) against the fused device call (Context.cn_decode ->
csvgpu_cn_decode_resident_many: windows -> observations -> emissions -> Viterbi, one readback), alone and inside the whole-genome step.

    python tools/bench_cn_observations.py --out profiles/cn_observations/cn_observations.json      # both generated genomes (30x ONT, 60x HiFi)
    python tools/bench_cn_observations.py --tech hifi --alone-only --reps 20                       # e.g. under rocprofv3 --kernel-trace --stats

alone: the regions of one genome-wide copy-number pass — the step's calls of at least --min-cnv positions, contig by contig — against SNP
       tables of the generated genomes' density (a record every 500..1500 positions; the genome's own tables stay inside the staged
       genome). The replaced route's three pieces: `windows_and_assembly` = host.query_snp_regions(on_device=False) per contig (the window
       launch, its readback and the assembly on the pool; the run makes ONE window call for all contigs, so this is an upper bound of
       that piece), `viterbi` = Context.viterbi on the assembled vectors; the fused call = Context.cn_decode, one call for all contigs;
       the seam = Context.cn_observations. Wall time of warm calls ending in a synchronise; device time of the fused call's two timer
       groups beside it.
step:  Genome.run (three lanes, like bench.py's step) with cn_observations_on_device off and on taking turns in one process: medians and
       p10-p90 of ms_total, ms_cigar_cn and ms_split_cn. The rule of DESIGN.md §7: the option becomes the default only if its median
       ms_total beats the option-off median by more than the option-off run's own p10-p90 spread, on both genomes.
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
from bench_split_groups import _Handle, spread   # noqa: E402
from hmm_params import WGS_HMM                  # noqa: E402

SETTINGS = {"off": {}, "on": {"cn_observations_on_device": True}}


def snp_table(seed, length):
    rng = np.random.default_rng(seed)
    pos = np.cumsum(rng.integers(500, 1500, int(length // 1000) + 2))
    pos = pos[pos < length].astype(np.uint32)
    baf = np.where(rng.random(len(pos)) < 2.0 / 3.0, 0.45 + 0.1 * rng.random(len(pos)), 1.0)
    return {"pos": pos, "baf": baf, "pfb": np.zeros(len(pos)), "has_pfb": np.zeros(len(pos), np.uint8)}


def one_genome(args, tech_name, depth, ctx, lanes, hmm):
    tech = 0 if tech_name == "ont" else 1
    config = 3 if tech == 0 else 4
    n_contigs = max(1, min(args.contigs, 24))
    lens = [max(200_000, int(GRCH38[k] * args.scale)) for k in range(n_contigs)]
    gen_threads = max(1, min(64, 2 * cpu_share()))
    g = host.Genome()
    n_reads = 0
    t0 = time.perf_counter()
    for k in range(n_contigs):
        syn = host.SynthShard(seed_of(config, k), lens[k], depth, tech, gen_threads)
        g.add_synth(ctx, NAMES[k], k, syn, snp_seed=seed_of(config, k), with_snps=True)
        n_reads += int(syn.reads.n_reads)
        syn.free()
    out = {"tech": tech_name, "depth": depth, "contigs": n_contigs, "scale": args.scale, "reads": n_reads, "staging_s": round(time.perf_counter() - t0, 1)}
    cap = max(1 << 16, 4 * n_contigs * 4096)

    def step(kw):
        t = time.perf_counter()
        calls, tid, st, stats = g.run(ctx, hmm, lanes=lanes, capacity=cap, copy=False, **kw)
        ctx.synchronize()
        return (time.perf_counter() - t) * 1e3, st, calls, tid, stats

    for _ in range(max(args.warmup, 1)):
        for kw in SETTINGS.values():
            last = step(kw)
    if not args.no_alone:
        _, _, calls, tid, stats = last
        calls, tid = calls.copy(), tid.copy()
        shards = [_Handle(g.contig_info(i)["shard"]) for i in range(len(g))]
        mean_cov = [float(s.mean_cov) for s in stats]
        tables = [snp_table(seed_of(config, k), lens[k]) for k in range(n_contigs)]
        per = []
        for k in range(n_contigs):
            c = calls[(tid == k) & (calls["end"] >= calls["start"]) & ((calls["end"] - calls["start"]) >= args.min_cnv)]
            per.append((np.ascontiguousarray(c["start"], np.uint32), np.ascontiguousarray(c["end"], np.uint32)))
        reg_off = np.concatenate([[0], np.cumsum([len(p[0]) for p in per])]).astype(np.uint64)
        rs, re = np.concatenate([p[0] for p in per]), np.concatenate([p[1] for p in per])
        so, sp, sb, sf = [0], [], [], []
        for k in range(n_contigs):
            pos = tables[k]["pos"]
            for a, b in zip(*per[k]):
                lo, hi = np.searchsorted(pos, a, "left"), np.searchsorted(pos, b, "right")
                sp.append(pos[lo:hi]); sb.append(tables[k]["baf"][lo:hi]); sf.append(np.zeros(hi - lo)); so.append(so[-1] + hi - lo)
        cat = lambda v, dt: np.concatenate(v).astype(dt) if v else np.zeros(0, dt)
        a = (shards, mean_cov, reg_off, rs, re, np.full(len(rs), args.sample_size, np.int32), np.asarray(so, np.uint64), cat(sp, np.uint32), cat(sb, np.float64),
             cat(sf, np.float64))

        def host_route():
            parts = [host.query_snp_regions(ctx, shards[k], per[k][0], per[k][1], mean_cov[k], args.sample_size, tables[k], on_device=False)
                     for k in range(n_contigs) if len(per[k][0])]
            return {f: np.concatenate([p[f] for p in parts]) for f in ("pos", "baf", "pfb", "log2_cov", "is_snp")}, \
                np.concatenate([[0], np.cumsum(np.concatenate([np.diff(p["obs_off"].astype(np.int64)) for p in parts]))]).astype(np.uint64)

        want, want_off = host_route()
        seam = ctx.cn_observations(*a)
        st_ref, ll_ref = ctx.viterbi(hmm, want["log2_cov"], want["baf"], want["pfb"], want_off)
        dec = ctx.cn_decode(hmm, *a)
        same = np.array_equal(seam["obs_off"], want_off) and all(seam[f].astype(want[f].dtype).tobytes() == want[f].tobytes() for f in want) and \
            np.array_equal(dec["states"], st_ref) and dec["loglik"].tobytes() == ll_ref.tobytes() and np.array_equal(dec["pos"], want["pos"])
        t_host, t_vit, t_seam, t_fused = [], [], [], []
        for _ in range(args.reps):
            for times, f in ((t_host, host_route), (t_vit, lambda: ctx.viterbi(hmm, want["log2_cov"], want["baf"], want["pfb"], want_off)),
                             (t_seam, lambda: ctx.cn_observations(*a)), (t_fused, lambda: ctx.cn_decode(hmm, *a))):
                t = time.perf_counter()
                f()
                ctx.synchronize()
                times.append((time.perf_counter() - t) * 1e3)
        ctx.timing_enable(1)
        ctx.timing_reset()
        for _ in range(10):
            ctx.cn_decode(hmm, *a)
        tm = ctx.timing()
        ctx.timing_enable(0)
        n_win = np.maximum(a[5], np.diff(a[6]).astype(np.int64))
        out["alone"] = {"regions": int(len(rs)), "windows": int(n_win.sum()), "largest_region_windows": int(n_win.max()) if len(n_win) else 0,
                        "snp_records": int(so[-1]), "observations": int(len(want["pos"])), "device_equals_host": bool(same),
                        "windows_and_assembly_per_contig_calls": spread(t_host), "viterbi": spread(t_vit),
                        "replaced_route": spread([x + y for x, y in zip(t_host, t_vit)]), "cn_observations_seam": spread(t_seam), "cn_decode_fused": spread(t_fused),
                        "fused_device_event_ms_per_call": {k: round(tm[k][0] / 10, 4) for k in ("window", "viterbi")},
                        "fused_timer_groups_per_call": {k: tm[k][1] / 10 for k in ("window", "viterbi")}}
        if not same:
            raise SystemExit("the device observations or their decode differ from the host route's")
    if not args.alone_only:
        rows = {k: [] for k in SETTINGS}
        digest = {}
        for i in range(len(SETTINGS) * args.steps):
            name = list(SETTINGS)[i % len(SETTINGS)]
            wall, st, calls, tid, _ = step(SETTINGS[name])
            rows[name].append((wall, st.ms_total, st.ms_cigar_cn, st.ms_split_cn))
            digest[name] = (calls.tobytes(), tid.tobytes())
        if len(set(digest.values())) != 1:
            raise SystemExit("the step's records differ with the option")
        out["step"] = {name: {"wall": spread([r[0] for r in v]), "ms_total": spread([r[1] for r in v]), "ms_cigar_cn": spread([r[2] for r in v]),
                              "ms_split_cn": spread([r[3] for r in v])} for name, v in rows.items()}
        off_t = out["step"]["off"]["ms_total"]
        width = off_t["p90_ms"] - off_t["p10_ms"]
        out["step"]["same_records"] = True
        out["step"]["off_p10_p90_spread_ms"] = round(width, 4)
        out["step"]["on"]["median_gain_ms"] = round(off_t["median_ms"] - out["step"]["on"]["ms_total"]["median_ms"], 4)
        out["step"]["on"]["beats_off_by_more_than_its_spread"] = bool(out["step"]["on"]["median_gain_ms"] > width)
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
    res = {"tool": "tools/bench_cn_observations.py", "pinned_to": pinned, "lanes": len(lanes), "genomes": []}
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
