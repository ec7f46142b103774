#!/usr/bin/env python3
"""bench.py — hot-path benchmark (driver contract: one JSON line on rank 0).

Workload (BASELINE.json `metric`): 30x synthetic ONT WHOLE GENOME — the 24 primary GRCh38 contig lengths, generator of SURVEY.md §8d
(seed = 0x5EED0000 + 1000 * config + contig index) — staged once: every contig's records resident in HBM as a struct-of-arrays shard
(~37 GB of CIGAR words + 12 GB of depth maps on one MI355X), the 7 bytes per record + query-name hash / identity that the host-side passes
read kept on the host, one SNP table per contig.

A *step* is one pass of SVCaller::run's pass order (reference src/sv_caller.cpp:804-925) over all resident contigs:
  depth map + mean coverage + CIGAR scan + addSVCall ordering + per-type interval DBSCAN (device) + mergeSVs representative choice
  (host), every contig, several contigs in flight (lanes)  ->  CIGAR copy-number predictions (window kernel + Viterbi kernel; calls >= 2 kb)
  ->  split-read signatures (scan kernel's alignment intervals, the reference's qname hash-map order replayed on the host, ONE batched
  DBSCAN1D launch)  ->  their copy-number predictions  ->  mergeSVs(0.1, 2, keep_noise) on the split calls  ->  final mergeSVs on the union.
value = reads scanned / s = reads of the genome x K / wall time of the K timed steps (inputs resident when the timed region starts).

N > 1 (torch.distributed.run, one rank per GPU): STRONG scaling of the same genome — contigs are bin-packed over the ranks by read count
(longest processing time first; the reference schedules one pool task per chromosome, sv_caller.cpp:827-863), every rank steps through
its own contigs, and the only collective is the final gather of the merged call records to rank 0 (one fixed-size all_gather per step,
RCCL), inside the timed region. No data-path collective.

A plain run stages the genome, warms up, times the K steps and prints the line (headline, stage and kernel times of the timed steps,
roofline). --full adds, at N = 1, the legs that take runs of their own: `no_split_overlap` (the same steps without the split overlap),
`chr22_cigar_path` (BASELINE configs[1], an earlier round's headline configuration), `chr1_cnv` (configs[2]: chr1 alone, all passes, with the
window / Viterbi kernel times), `from_file` / `from_file_wgs` (from real BGZF BAMs), `hifi_wgs` (configs[4]) and `cpu_baseline` (the CPU
restatement on the same 24 contigs, one contig per thread as the reference schedules them, on a stated sample).

--dump-outputs DIR writes what the last timed step returned as float64 .npy files: the merged call records field by field with their
contig ids (`calls_*.npy`, gathered to rank 0 at N > 1) and rank 0's per-contig statistics (`contig_*.npy`).
"""
import argparse
import hashlib
import json
import os
import sys
import threading
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

GRCH38 = [248956422, 242193529, 198295559, 190214555, 181538259, 170805979, 159345973, 145138636, 138394717, 133797422, 135086622, 133275309,
          114364328, 107043718, 101991189, 90338345, 83257441, 80373285, 58617616, 64444167, 46709983, 50818468, 156040895, 57227415]
NAMES = ["chr%d" % i for i in range(1, 23)] + ["chrX", "chrY"]
HBM_PEAK_GBS = 8000.0          # MI355X_MICROARCH.md: 8.0 TB/s spec (6.29 TB/s measured streaming copy)
REC_I32 = 12                   # one merged call record = 48 B (host.CALL_DTYPE)
DUMP_MAX_BYTES = 64 << 20      # --dump-outputs: all files together; larger outputs are cut to a fixed, seeded sample of rows
CONTIG_DUMP_FIELDS = ("n_signatures", "n_del", "n_ins", "depth_sum", "depth_nonzero", "min_pts", "mean_cov", "n_calls")   # (not the timings)


def seed_of(config, contig):
    return 0x5EED0000 + 1000 * config + contig + 1


def cpu_share():
    """CPUs this process may actually use: the scheduler affinity, cut to the cgroup's CPU quota (a one-GPU box of the pool reports 256 CPUs
    and grants 16: cpu.max = "1600000 100000"); thread pools sized beyond it only add context switches."""
    n = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 8)
    try:
        quota, period = open("/sys/fs/cgroup/cpu.max").read().split()[:2]
        if quota != "max":
            n = min(n, max(1, int(int(quota) / int(period))))
    except Exception:
        pass
    return max(1, n)


def pin_to_gpu_numa(device_index):
    """Keep this process (its host pools, the lanes' threads, the arrays they first touch) on the CPUs of the NUMA node the GPU hangs off:
    the pool's boxes are two-socket machines whose scheduler otherwise spreads a rank's threads over both sockets (sections of the host
    passes then run 3-6x slower from one step to the next). CSV_BENCH_NO_PIN=1 leaves the affinity alone. Returns what was done."""
    if os.environ.get("CSV_BENCH_NO_PIN") == "1" or not hasattr(os, "sched_setaffinity"):
        return None
    try:
        import torch
        pr = torch.cuda.get_device_properties(device_index)
        bdf = "%04x:%02x:%02x.0" % (getattr(pr, "pci_domain_id", 0), pr.pci_bus_id, getattr(pr, "pci_device_id", 0))
        node = int(open("/sys/bus/pci/devices/%s/numa_node" % bdf).read())
        if node < 0:
            return None
        cpus = set()
        for part in open("/sys/devices/system/node/node%d/cpulist" % node).read().strip().split(","):
            a, _, b = part.partition("-")
            cpus.update(range(int(a), int(b or a) + 1))
        cpus &= os.sched_getaffinity(0)
        if len(cpus) < 4:
            return None
        os.sched_setaffinity(0, cpus)
        return {"numa_node": node, "cpus": len(cpus), "gpu": bdf}
    except Exception as e:          # best effort: an unknown sysfs layout changes nothing
        return {"error": str(e)[:80]}


def cpu_throttle():
    """(periods throttled, microseconds throttled) of this cgroup so far — a step that exceeds the CPU quota is stalled by the scheduler"""
    try:
        kv = dict(line.split() for line in open("/sys/fs/cgroup/cpu.stat"))
        return int(kv.get("nr_throttled", 0)), int(kv.get("throttled_usec", 0))
    except Exception:
        return None


def call_digest(tid, calls):
    """SHA-256 of a run's merged call records (48 B each, contig after contig in the run's order) with their contig ids."""
    h = hashlib.sha256()
    h.update(np.ascontiguousarray(tid).tobytes())
    h.update(np.ascontiguousarray(calls).tobytes())
    return h.hexdigest()


def dump_outputs(out_dir, tid, calls, contig_tid, per):
    """--dump-outputs: one float64 .npy per field of the merged call records (+ their contig ids) and per per-contig statistic. Every field
    is an integer below 2**53 or a double, so float64 holds it exactly."""
    arrays = {"calls_tid": tid}
    arrays.update({"calls_" + f: calls[f] for f in calls.dtype.names})
    rows = len(tid)
    row_bytes = 8 * len(arrays)
    contig = {"contig_tid": np.asarray(contig_tid)}
    contig.update({"contig_" + f: np.array([getattr(p, f) for p in per]) for f in CONTIG_DUMP_FIELDS})
    budget = DUMP_MAX_BYTES - 8 * len(contig) * len(per) - 256 * (len(arrays) + len(contig))      # (256 B: room for each file's .npy header)
    if rows * row_bytes > budget:
        keep = np.sort(np.random.default_rng(0).choice(rows, budget // row_bytes, replace=False))
        arrays = {k: v[keep] for k, v in arrays.items()}
    arrays.update(contig)
    os.makedirs(out_dir, exist_ok=True)
    for name, a in arrays.items():
        np.save(os.path.join(out_dir, name + ".npy"), np.asarray(a, dtype=np.float64))


def main():
    t_start = time.perf_counter()
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--depth", type=float, default=30.0)
    ap.add_argument("--tech", choices=["ont", "hifi"], default="ont")
    ap.add_argument("--scale", type=float, default=float(os.environ.get("CSV_BENCH_SCALE", "1.0")), help="scale every contig length (rehearsals and tests; the judged run is 1.0)")
    ap.add_argument("--contigs", type=int, default=24, help="first N contigs of the genome (rehearsals)")
    ap.add_argument("--eps", type=float, default=0.1)
    ap.add_argument("--min-pts-pct", type=float, default=0.1)
    ap.add_argument("--lanes", type=int, default=3, help="contigs in flight per GPU during the CIGAR pass (contexts sharing a gate)")
    ap.add_argument("--host-threads", type=int, default=0, help="host threads of the split-read / copy-number passes (0 = hardware)")
    ap.add_argument("--gen-threads", type=int, default=0, help="threads of the generator (0 = the CPU share of this rank, at most 32)")
    ap.add_argument("--gen-ahead", type=int, default=3, help="contigs generated at once while staging (each with --gen-threads; the same inputs at any value)")
    ap.add_argument("--no-split-overlap", action="store_true", help="run the split-read pass's first half after the CIGAR pass instead of beside it (A/B: the big kernels "
                    "then have the device to themselves)")
    ap.add_argument("--background", action="store_true", help="the caller's context at the LOWEST stream priority (csvgpu_create_background): the split pass's ordering "
                    "kernels then only fill the gaps of the CIGAR pass — measured: they no longer stretch the big kernels (depth 0.50 of peak instead of 0.48) but "
                    "finish 3.5 ms after the pass, 37.1 ms per step against 35.8")
    ap.add_argument("--full", action="store_true", help="also the legs and the CPU baseline at N = 1 (a plain run is the headline only); the --no-* options "
                    "below leave parts of them out")
    ap.add_argument("--dump-outputs", default="", metavar="DIR", help="write what the last timed step returned to DIR/<name>.npy (float64)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-legs", action="store_true", help="headline only (no chr22 / chr1 / from-file legs)")
    ap.add_argument("--no-from-file", action="store_true")
    ap.add_argument("--no-from-file-wgs", action="store_true", help="skip the whole-genome-from-one-BAM leg (stages an 11 GB BAM under TMPDIR: ~70 s on a 16-CPU share)")
    ap.add_argument("--no-hifi-leg", action="store_true", help="skip the 60x HiFi whole-genome leg (BASELINE.json configs[4] on this rank's GPU)")
    ap.add_argument("--cpu-sample-frac", type=float, default=0.25, help="leading fraction of every contig's reads given to the CPU baseline")
    ap.add_argument("--verify-against-single", action="store_true", help="rank 0 also stages the WHOLE genome, runs it alone and asserts that the gathered "
                    "call set of the sharded run is byte-identical (rehearsals / tests; costs rank 0 the whole staging)")
    ap.add_argument("--dump-calls", default="", help="rank 0: write the gathered merged calls (npy: tid + CALL_DTYPE) here")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be at least 1")
    legs = args.full and not args.no_legs

    import torch
    import contextsv_amd as cs
    from contextsv_amd import host, parallel
    from hmm_params import WGS_HMM

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    dist = None
    rehearse = False
    if world > 1:
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        # CSV_BENCH_REHEARSE=1: rehearsal of the N>1 driver logic on a box with fewer cards than ranks — gloo instead of RCCL,
        # ranks share the cards round-robin, collectives on host tensors. Never the judged configuration.
        rehearse = os.environ.get("CSV_BENCH_REHEARSE") == "1"
        if rehearse:
            local_rank %= torch.cuda.device_count()
            torch.cuda.set_device(local_rank)
            dist.init_process_group("gloo")
        else:
            torch.cuda.set_device(local_rank)
            dist.init_process_group("nccl", device_id=torch.device("cuda", local_rank))
    else:
        torch.cuda.set_device(0)
    dev = torch.device("cuda", local_rank if world > 1 else 0)
    pinned_to = pin_to_gpu_numa(dev.index)
    coll_dev = torch.device("cpu") if rehearse else dev
    tech = 0 if args.tech == "ont" else 1
    config_id = 3 if tech == 0 else 4                                   # BASELINE.json configs[3] / configs[4]
    n_contigs = max(1, min(args.contigs, 24))
    lens = [max(200_000, int(GRCH38[k] * args.scale)) for k in range(n_contigs)]
    gen_threads = args.gen_threads or max(1, min(64, 2 * max(1, cpu_share() // max(world, 1))))      # (the ranks of a node share its CPU quota)
    hmm = cs.make_hmm(**WGS_HMM)

    # ---- partition: contigs over ranks, longest first (read count is proportional to length for one depth) ----------------------
    mine = parallel.assign_shards(lens, world)[rank]

    # the caller's own context: split-read ordering (beside the CIGAR pass), copy-number pass, batched DBSCAN1D, final merges
    # Stream creation order decides who shares a hardware queue (the runtime deals its four queues round-robin): the gate's stream first, so
    # that the big kernels' queue is shared with the LAST lane at most; CSV_BENCH_STREAM_ORDER = lazy | caller_first for the A/B.
    n_lanes = max(1, args.lanes)
    order = os.environ.get("CSV_BENCH_STREAM_ORDER", "gate_first")
    gate = None
    if n_lanes > 1 and order == "gate_first":
        gate = cs.Gate(dev.index)
    ctx = cs.Context(dev.index, background=args.background)
    host.set_context(ctx)
    if n_lanes > 1 and order == "caller_first":
        gate = cs.Gate(dev.index)
    lane_ctx = [cs.Context(dev.index) for _ in range(n_lanes)] if n_lanes > 1 else []
    if n_lanes > 1 and gate is None:
        gate = cs.Gate()
    for c in lane_ctx:
        c.set_gate(gate)

    def stage(contig_ids, keep_sample, tech=tech, depth=args.depth, config_id=config_id):
        """Generate, upload and free one contig at a time, in contig order -> (Genome, per-contig info, CPU-baseline samples). Up to
        --gen-ahead contigs are generated at once beside the uploads (the generator's single-threaded merge is most of its time); a contig's
        reads depend on its seed and gen_threads only."""
        from concurrent.futures import ThreadPoolExecutor

        def gen(k):
            t0 = time.perf_counter()
            syn = host.SynthShard(seed_of(config_id, k), lens[k], depth, tech, gen_threads)
            return syn, time.perf_counter() - t0

        g = host.Genome()
        info, samples = [], []
        t_gen = t_up = 0.0
        h2d = 0
        t_stage = time.perf_counter()
        ahead = max(1, args.gen_ahead)
        with ThreadPoolExecutor(max_workers=ahead) as ex:
            pending = [ex.submit(gen, k) for k in contig_ids[:ahead]]
            for i, k in enumerate(contig_ids):
                syn, dt = pending.pop(0).result()
                if i + ahead < len(contig_ids):
                    pending.append(ex.submit(gen, contig_ids[i + ahead]))
                t1 = time.perf_counter()
                g.add_synth(ctx, NAMES[k], k, syn, snp_seed=seed_of(config_id, k), with_snps=True)
                t2 = time.perf_counter()
                r = syn.reads
                info.append({"contig": NAMES[k], "tid": k, "len": lens[k], "reads": int(r.n_reads), "cigar_ops": int(r.n_cigar)})
                h2d += r.cigar.nbytes + r.pos.nbytes + r.flag.nbytes + r.mapq.nbytes + r.cigar_off.nbytes
                if keep_sample:
                    n = max(1, int(r.n_reads * args.cpu_sample_frac))
                    m = int(r.cigar_off[n])
                    sub = cs.Reads.__new__(cs.Reads)
                    sub.pos, sub.flag, sub.mapq, sub.tid = r.pos[:n].copy(), r.flag[:n].copy(), r.mapq[:n].copy(), None
                    sub.cigar_off, sub.cigar = r.cigar_off[: n + 1].copy(), r.cigar[:m].copy()
                    samples.append((NAMES[k], sub, syn.depth_len, int(r.n_reads)))
                syn.free()
                t_gen += dt
                t_up += t2 - t1
        return g, info, samples, {"synth_s": round(t_gen, 2), "upload_s": round(t_up, 2), "h2d_bytes": int(h2d), "wall_s": round(time.perf_counter() - t_stage, 2)}

    want_cpu = world == 1 and args.full and not args.no_cpu_baseline
    genome, info, samples, staging = stage(mine, want_cpu)
    reads_mine = sum(i["reads"] for i in info)
    ops_mine = sum(i["cigar_ops"] for i in info)
    cap = max(1 << 16, 4 * len(mine) * 4096)
    gather_cap = [1 << 16]                                                # merged calls per rank carried by the final gather: a worst case for the
                                                                          # warm-up steps, then twice the largest rank's count (set below)

    def step():
        calls, tid, st, per = genome.run(ctx, hmm, lanes=lane_ctx, eps=args.eps, min_pts_pct=args.min_pts_pct, host_threads=args.host_threads, capacity=cap,
                                         overlap_split=not args.no_split_overlap, copy=False)
        gathered = None
        if world > 1:
            per_shard = {int(t): calls[tid == t] for t in np.unique(tid)}
            for k in mine:
                per_shard.setdefault(k, calls[:0])
            gathered = parallel.gather_calls(per_shard, cap=gather_cap[0], dist=dist, device=coll_dev)
        return calls, tid, st, per, gathered

    def barrier():
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()
        ctx.synchronize()
        for c in lane_ctx:
            c.synchronize()

    for _ in range(max(args.warmup, 0)):
        warm = step()
    if world > 1 and args.warmup > 0:
        # every rank receives world x cap records per step: the capacity follows what the warm-up produced (a step that outgrows it fails loudly)
        m = torch.tensor([float(len(warm[0]))], dtype=torch.float64, device=coll_dev)
        dist.all_reduce(m, op=dist.ReduceOp.MAX)
        gather_cap[0] = max(1024, (2 * int(m.item()) + 1023) // 1024 * 1024)
        step()                                                             # (one more untimed step: the gather's buffers at their final size)
    for c in lane_ctx or [ctx]:
        c.timing_enable(3)                                                 # scan + depth pairs, every launch (contigs differ in size)
        c.timing_reset()
    if lane_ctx:
        ctx.timing_enable(1)                                               # window / Viterbi / DBSCAN1D / final-merge DBSCAN groups on the main context
        ctx.timing_reset()
    barrier()
    thr0 = cpu_throttle()
    t0 = time.perf_counter()
    acc = None
    for _ in range(args.steps):
        calls, tid, st, per, gathered = step()
        vals = [getattr(st, f) for f, _ in host.stage_times._fields_]
        acc = vals if acc is None else [a + b for a, b in zip(acc, vals)]
    barrier()
    elapsed = time.perf_counter() - t0
    calls, tid = calls.copy(), tid.copy()                                  # (views of the genome's result buffers: the legs below run it again)
    thr1 = cpu_throttle()
    timing = {}
    for c in (lane_ctx or []) + [ctx]:
        for k, (ms, n) in c.timing().items():
            a = timing.get(k, (0.0, 0))
            timing[k] = (a[0] + ms, a[1] + n)
        c.timing_enable(0)

    el = torch.tensor([elapsed], dtype=torch.float64, device=coll_dev)
    tot = torch.tensor([float(reads_mine), float(ops_mine), float(sum(p.n_signatures for p in per)), float(len(calls))], dtype=torch.float64, device=coll_dev)
    if world > 1:
        dist.all_reduce(el, op=dist.ReduceOp.MAX)
        dist.all_reduce(tot, op=dist.ReduceOp.SUM)
    elapsed = float(el.item())
    reads_all, ops_all, sigs_all, calls_all = (float(x) for x in tot.tolist())

    verify = None
    if world > 1 and rank == 0 and args.verify_against_single:
        # the unsharded run of the same genome on this rank's card, compared record for record with what the gather delivered
        g1, _, _, _ = stage(list(range(n_contigs)), False)
        c1, t1, _, _ = g1.run(ctx, hmm, lanes=lane_ctx, eps=args.eps, min_pts_pct=args.min_pts_pct, host_threads=args.host_threads, capacity=max(cap, 1 << 18))
        g1.free()
        same = sorted(gathered) == sorted(int(t) for t in range(n_contigs))
        for k in range(n_contigs):
            same = same and gathered[k].tobytes() == np.ascontiguousarray(c1[t1 == k]).tobytes()
        verify = {"sharded_equals_single": bool(same), "calls": int(len(c1))}
        if not same:
            raise SystemExit("bench.py: the gathered call set of the sharded run differs from the single-rank run")
    if rank == 0 and args.dump_calls:
        if world > 1:
            ks = sorted(gathered)
            np.savez(args.dump_calls, tid=np.concatenate([np.full(len(gathered[k]), k, np.int32) for k in ks]), calls=np.concatenate([gathered[k] for k in ks]))
        else:
            np.savez(args.dump_calls, tid=tid, calls=calls)
    if rank == 0 and args.dump_outputs:
        if world > 1:
            ks = sorted(gathered)
            d_tid, d_calls = np.concatenate([np.full(len(gathered[k]), k, np.int32) for k in ks]), np.concatenate([gathered[k] for k in ks])
        else:
            d_tid, d_calls = tid, calls
        dump_outputs(args.dump_outputs, d_tid, d_calls, [i["tid"] for i in info], per)

    if rank == 0:
        K = args.steps
        stage_ms = {f: v / K for (f, _), v in zip(host.stage_times._fields_, acc) if f.startswith("ms_")}
        counts = {f: int(v / K) for (f, _), v in zip(host.stage_times._fields_, acc) if f.startswith("n_")}
        kern = {k: ms / K for k, (ms, n) in timing.items() if n}          # device time per step, summed over this rank's launches
        launches = {k: n / K for k, (ms, n) in timing.items() if n}
        n_sig_rank = sum(p.n_signatures for p in per)
        depth_lens = sum(i["len"] + 1 for i in info)
        n_obs = None
        alg_bytes = {                                                     # per step, this rank's contigs (SURVEY §8d per-unit figures x units)
            "cigar_scan": 4.0 * ops_mine + 23.0 * reads_mine + 16.0 * n_sig_rank,
            "depth": 4.0 * ops_mine + 4.0 * depth_lens,
            "sort": 32.0 * n_sig_rank,
            "dbscan": 12.0 * n_sig_rank,
        }
        big = [k for k in ("cigar_scan", "depth") if kern.get(k, 0) > 0]
        dominant = max(big, key=lambda k: kern[k]) if big else "depth"
        ach = alg_bytes[dominant] / (kern[dominant] * 1e-3) / 1e9 if kern.get(dominant, 0) > 0 else 0.0
        traffic, traffic_src = None, None
        pmc_path = os.path.join(ROOT, "profiles", "pmc_traffic.json")
        if os.path.exists(pmc_path) and world == 1 and args.scale == 1.0 and n_contigs == 24 and ((tech == 0 and args.depth == 30.0) or (tech == 1 and args.depth == 60.0)):
            try:
                pj = json.load(open(pmc_path))
                key = "wgs" if tech == 0 else "hifi_wgs"
                traffic = pj.get(key, {}).get(dominant)
                traffic_src = pj.get(key, {}).get("source")
            except Exception:
                traffic = None
        workload = (f"whole genome: {n_contigs} GRCh38 primary contig lengths" + (f" x {args.scale:g}" if args.scale != 1.0 else "") +
                    f", {args.depth:g}x synthetic {args.tech.upper()}, all contigs resident in HBM; step = SVCaller::run pass order over every contig "
                    "(depth + CIGAR scan + ordering + interval DBSCAN + mergeSVs -> CIGAR CN pass (window + Viterbi) -> split-read signatures (batched DBSCAN1D) "
                    f"-> split CN pass -> mergeSVs x2) — BASELINE.json configs[{config_id}]" + (f", contigs bin-packed over {world} ranks + final gather" if world > 1 else ""))
        out = {
            "metric": "long reads scanned/s (whole-genome step: scan + depth + cluster + merge + CN + split passes), synthetic 30x ONT WGS",
            "value": reads_all * K / elapsed,
            "unit": "reads/s",
            "n_gpus": world,
            "steps": K,
            "warmup": args.warmup,
            "ms_per_step": elapsed / K * 1e3,
            "higher_is_better": True,
            "scaling": "strong",                                                # the same genome at every N: its contigs are bin-packed over the ranks
            "vs_baseline": None,
            "dtype": "u32",
            "data": "synthetic",
            "config": {"workload": workload, "reads": int(reads_all), "cigar_ops": int(ops_all), "signatures": int(sigs_all), "merged_calls": int(calls_all),
                       "contigs": n_contigs, "contigs_on_rank0": [i["contig"] for i in info], "eps": args.eps, "min_pts_pct": args.min_pts_pct,
                       "parallelism": f"chromosome-shard x{world}", "lanes": n_lanes, "scale": args.scale},
            "signatures_clustered_per_s": sigs_all * K / elapsed,
            "cigar_ops_per_s": ops_all * K / elapsed,
            "call_set_sha256": (call_digest(tid, calls) if world == 1 else
                                call_digest(np.concatenate([np.full(len(gathered[k]), k, np.int32) for k in sorted(gathered)]), np.concatenate([gathered[k] for k in sorted(gathered)]))),
            "stage_ms_per_step_rank0": {k: round(v, 3) for k, v in stage_ms.items()},
            "stage_counts_rank0": counts,
            "kernel_ms_per_step_rank0": {k: round(v, 4) for k, v in kern.items()},
            "kernel_launches_per_step_rank0": {k: round(v, 1) for k, v in launches.items()},
            "host_cpu": {"cpus": os.cpu_count(), "share": cpu_share(), "pinned_to": pinned_to,
                         "throttled_in_timed_region": ({"periods": thr1[0] - thr0[0], "ms": round((thr1[1] - thr0[1]) / 1e3, 1)} if thr0 and thr1 else None)},
            "staging_rank0": dict(staging, pcie_inclusive_reads_per_s=reads_mine / (staging["upload_s"] + elapsed / K)),
            "roofline": {"bound": "hbm", "kernel": dominant, "achieved": ach, "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": ach / HBM_PEAK_GBS,
                         "traffic": traffic, "traffic_source": traffic_src,
                         "algorithmic_bytes_per_step": alg_bytes[dominant], "kernel_ms_per_step": kern.get(dominant, 0.0),
                         "launches_per_step": launches.get(dominant, 0), "launches_timed": int(timing.get(dominant, (0, 0))[1]),
                         "note": "one launch per contig (depth = depth_items_kernel + depth_tile_kernel: the tiles' work lists and the tiles); achieved = bytes of this rank's contigs per step / the kernel's summed HIP-event time per step "
                                 "(events on the gate's stream, every launch timed)",
                         "all": {k: {"ms": round(kern.get(k, 0.0), 4), "GBps": round(alg_bytes[k] / (kern[k] * 1e-3) / 1e9, 1) if kern.get(k, 0) > 0 else None}
                                 for k in alg_bytes}},
        }
        if verify:
            out["verify"] = verify
        if world == 1 and legs and lane_ctx and not args.no_split_overlap:
            # A/B of the one overlap that costs the big kernels something: the same steps with the split pass's first half AFTER the CIGAR pass
            for c in lane_ctx:
                c.timing_enable(3); c.timing_reset()
            k2 = max(3, min(K, 10))
            t0 = time.perf_counter()
            for _ in range(k2):
                c2, t2, _, _ = genome.run(ctx, hmm, lanes=lane_ctx, eps=args.eps, min_pts_pct=args.min_pts_pct, host_threads=args.host_threads, capacity=cap, overlap_split=False)
            ctx.synchronize()
            # the timed steps take the early batches inside the CIGAR pass (timing-dependent batch sizes), this leg takes none: same calls or the run fails
            if call_digest(t2, c2) != out["call_set_sha256"]:
                raise SystemExit("bench.py: the call set of the overlapped step differs from the step without the split overlap")
            el2 = time.perf_counter() - t0
            tm2 = {}
            for c in lane_ctx:
                for kk, (ms, n) in c.timing().items():
                    a = tm2.get(kk, (0.0, 0)); tm2[kk] = (a[0] + ms, a[1] + n)
                c.timing_enable(0)
            d_ms = tm2.get(dominant, (0.0, 0))[0] / k2
            out["no_split_overlap"] = {"call_set_equal": True, "value": reads_all * k2 / el2, "unit": "reads/s", "ms_per_step": el2 / k2 * 1e3, "steps": k2,
                                       "kernel_ms_per_step": {kk: round(v[0] / k2, 4) for kk, v in tm2.items() if v[1]},
                                       "roofline_frac": (alg_bytes[dominant] / (d_ms * 1e-3) / 1e9 / HBM_PEAK_GBS) if d_ms > 0 else None,
                                       "note": "the split-read pass's ordering kernels after the CIGAR pass instead of beside it: the big kernels have the device to "
                                               "themselves (plus the lanes' own small kernels), the step is longer"}
        if world == 1 and legs:
            out["chr1_cnv"] = leg_chr1(cs, host, ctx, lane_ctx, genome, info, hmm, args)
            # the same kernel with the device to itself (the chr1 leg runs one contig on one context: nothing beside the scan / depth pair)
            alone = out["chr1_cnv"].get("depth_GBps" if dominant == "depth" else "cigar_scan_GBps")
            if alone:
                out["roofline"]["alone_frac"] = alone / HBM_PEAK_GBS
                out["roofline"]["note"] += ("; in the genome step the split-read pass's ordering kernels share the device with the first half of the CIGAR pass "
                                            "(that overlap shortens the step by ~15 % and stretches the big kernels by ~12 %; `no_split_overlap` is the same genome without it): "
                                            "`alone_frac` is the same kernel on chr1 with nothing beside it")
            out["chr22_cigar_path"] = leg_chr22(cs, host, dev, args, tech, config_id, gen_threads)
            if not args.no_from_file:
                out["from_file"] = from_file(cs, host, ctx, args, tech, config_id, gen_threads)
                if not args.no_from_file_wgs and tech == 0 and n_contigs == 24 and time.perf_counter() - t_start < 200:
                    genome.free()                                                # (the resident genome's host mirror + HBM are not needed any more; HiFi leg staged its own)
                    genome = host.Genome()
                    out["from_file_wgs"] = from_file_wgs(cs, host, ctx, args, lens, config_id, gen_threads)
        if world == 1 and legs and tech == 0 and not args.no_hifi_leg:
            out["hifi_wgs"] = leg_hifi_wgs(stage, ctx, lane_ctx, hmm, args, n_contigs, cap)
        if want_cpu:
            out["cpu_baseline"] = cpu_baseline(samples, args, reads_all)
        print(json.dumps(out), flush=True)

    genome.free()
    for c in lane_ctx:
        c.set_gate(None)
        c.close()
    ctx.close()
    if gate:
        gate.close()
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


def _hifi_traffic():
    """HBM bytes per 60x HiFi genome step of the two big kernels from the committed PMC passes (profiles/pmc_traffic.json: tools/profile_round.sh ... hifi)"""
    try:
        pj = json.load(open(os.path.join(ROOT, "profiles", "pmc_traffic.json"))).get("hifi_wgs", {})
        return {"cigar_scan": pj.get("cigar_scan"), "depth": pj.get("depth"), "source": "profiles/pmc_traffic.json (separate rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes)"}
    except Exception:
        return None


def leg_hifi_wgs(stage, ctx, lane_ctx, hmm, args, n_contigs, cap):
    """BASELINE configs[4]'s workload on one GPU: the same 24 contig lengths at 60x synthetic PacBio HiFi (1.04e7 reads of ~37 CIGAR ops:
    ten times the reads of the ONT genome in a twentieth of the CIGAR words) through the same step. The scan and the depth walk take their
    short-read forms here (groups of 16 lanes per read, chosen per shard from the mean CIGAR words per read: scan.hip, depth.hip)."""
    from contextsv_amd import host
    g, info, _, staging = stage(list(range(n_contigs)), False, tech=1, depth=60.0, config_id=4)
    try:
        reads = sum(i["reads"] for i in info)
        ops = sum(i["cigar_ops"] for i in info)
        run = lambda: g.run(ctx, hmm, lanes=lane_ctx, eps=args.eps, min_pts_pct=args.min_pts_pct, host_threads=args.host_threads, capacity=cap)
        for _ in range(2):
            run()
        for c in lane_ctx or [ctx]:
            c.timing_enable(3); c.timing_reset()
        if lane_ctx:
            ctx.timing_enable(1); ctx.timing_reset()
        steps = max(3, min(args.steps, 10))
        ctx.synchronize()
        t0 = time.perf_counter()
        acc = None
        for _ in range(steps):
            calls, tid, st, per = run()
            vals = [getattr(st, f) for f, _ in host.stage_times._fields_]
            acc = vals if acc is None else [a + b for a, b in zip(acc, vals)]
        ctx.synchronize()
        el = time.perf_counter() - t0
        tm = {}
        for c in (lane_ctx or []) + [ctx]:
            for k, (ms, n) in c.timing().items():
                a = tm.get(k, (0.0, 0)); tm[k] = (a[0] + ms, a[1] + n)
            c.timing_enable(0)
        kern = {k: v[0] / steps for k, v in tm.items() if v[1]}
        n_sig = sum(p.n_signatures for p in per)
        b_scan = 4.0 * ops + 23.0 * reads + 16.0 * n_sig
        b_depth = 4.0 * ops + 4.0 * sum(i["len"] + 1 for i in info)
        stage_ms = {f: round(v / steps, 3) for (f, _), v in zip(host.stage_times._fields_, acc) if f.startswith("ms_")}
        return {"workload": f"whole genome, {n_contigs} contigs, 60x synthetic HiFi, resident; same step (BASELINE.json configs[4] on one GPU)",
                "value": reads * steps / el, "unit": "reads/s", "ms_per_step": el / steps * 1e3, "steps": steps, "reads": int(reads), "cigar_ops": int(ops),
                "signatures": int(n_sig), "merged_calls": int(len(calls)), "signatures_clustered_per_s": n_sig * steps / el,
                "stage_ms_per_step": stage_ms, "kernel_ms_per_step": {k: round(v, 4) for k, v in kern.items()},
                "cigar_scan_GBps": round(b_scan / (kern["cigar_scan"] * 1e-3) / 1e9, 1) if kern.get("cigar_scan") else None,
                "cigar_scan_frac": round(b_scan / (kern["cigar_scan"] * 1e-3) / 1e9 / HBM_PEAK_GBS, 4) if kern.get("cigar_scan") else None,
                "depth_GBps": round(b_depth / (kern["depth"] * 1e-3) / 1e9, 1) if kern.get("depth") else None,
                "depth_frac": round(b_depth / (kern["depth"] * 1e-3) / 1e9 / HBM_PEAK_GBS, 4) if kern.get("depth") else None,
                "staging": staging, "traffic_bytes_per_step": _hifi_traffic(),
                "note": "kernel times are HIP-event times on the gate's stream inside the step (the other lanes' small kernels and the split-read pass's ordering kernels "
                        "share the device); algorithmic bytes as for the headline: scan 4 m + 23 n + 16 n_sig, depth 4 m + 4 (L + 1)"}
    finally:
        g.free()


def leg_chr1(cs, host, ctx, lane_ctx, genome, info, hmm, args):
    """BASELINE configs[2]: the largest contig alone (chr1), all passes of the step, with the copy-number kernels' own times."""
    k = max(range(len(info)), key=lambda i: info[i]["reads"])
    ci = genome.contig_info(k)
    g = host.Genome()
    # a second handle over the same resident shard would free it twice: stage the contig again instead (one upload)
    syn = host.SynthShard(seed_of(3 if args.tech == "ont" else 4, info[k]["tid"]), info[k]["len"], args.depth, 0 if args.tech == "ont" else 1,
                          args.gen_threads or min(64, 2 * cpu_share()))
    g.add_synth(ctx, info[k]["contig"], info[k]["tid"], syn, snp_seed=seed_of(3 if args.tech == "ont" else 4, info[k]["tid"]), with_snps=True)
    syn.free()
    steps = max(3, min(args.steps, 10))
    g.run(ctx, hmm, lanes=[], eps=args.eps, min_pts_pct=args.min_pts_pct, host_threads=args.host_threads)
    ctx.timing_enable(1); ctx.timing_reset()
    ctx.synchronize()
    t0 = time.perf_counter()
    acc = None
    for _ in range(steps):
        calls, tid, st, per = g.run(ctx, hmm, lanes=[], eps=args.eps, min_pts_pct=args.min_pts_pct, host_threads=args.host_threads)
        vals = [getattr(st, f) for f, _ in host.stage_times._fields_]
        acc = vals if acc is None else [a + b for a, b in zip(acc, vals)]
    ctx.synchronize()
    el = time.perf_counter() - t0
    tm = {k2: (ms / steps, n / steps) for k2, (ms, n) in ctx.timing().items() if n}
    ctx.timing_enable(0)
    g.free()
    stage_ms = {f: round(v / steps, 3) for (f, _), v in zip(host.stage_times._fields_, acc) if f.startswith("ms_")}
    counts = {f: int(v / steps) for (f, _), v in zip(host.stage_times._fields_, acc) if f.startswith("n_")}
    sc, dp = tm.get("cigar_scan", (0, 0))[0], tm.get("depth", (0, 0))[0]
    bytes_scan = 4.0 * ci["n_cigar"] + 23.0 * ci["n_reads"] + 16.0 * counts["n_signatures"]
    bytes_depth = 4.0 * ci["n_cigar"] + 4.0 * ci["depth_len"]
    return {"workload": f"{info[k]['contig']} alone ({info[k]['len']} bp, {args.depth:g}x), all passes, one lane (BASELINE.json configs[2])",
            "value": ci["n_reads"] * steps / el, "unit": "reads/s", "ms_per_step": el / steps * 1e3, "steps": steps, "reads": int(ci["n_reads"]),
            "stage_ms_per_step": stage_ms, "counts": counts,
            "kernel_ms_per_step": {k2: round(v[0], 4) for k2, v in tm.items()},
            "cigar_scan_GBps": round(bytes_scan / (sc * 1e-3) / 1e9, 1) if sc > 0 else None,
            "depth_GBps": round(bytes_depth / (dp * 1e-3) / 1e9, 1) if dp > 0 else None}


def leg_chr22(cs, host, dev, args, tech, config_id, gen_threads):
    """BASELINE configs[1] = last round's headline: one chr22-sized contig, CIGAR path only (scan + depth + ordering + DBSCAN + mergeSVs),
    three copies in three lanes, 200 pipelined passes."""
    syn = host.SynthShard(0x5EED0000 + 1000 * 1 + 22, GRCH38[21] if args.scale == 1.0 else max(200_000, int(GRCH38[21] * args.scale)), args.depth, tech, gen_threads)
    reads, depth_len = syn.reads, syn.depth_len
    gate = cs.Gate(dev.index)                                  # (before the lanes' contexts: csvgpu_gate_open)
    lanes = [cs.Context(dev.index) for _ in range(3)]
    shards = []
    try:
        for c in lanes:
            shards.append(c.upload(reads, depth_len))
            c.synchronize()
            c.set_gate(gate)
        steps = 200
        split = lambda n: [n // 3 + (1 if l < n % 3 else 0) for l in range(3)]
        host.process_resident_lanes(lanes, shards, split(9), args.eps, args.min_pts_pct, capacity=8192)
        host.process_resident_lanes(lanes, shards, split(10), args.eps, args.min_pts_pct, capacity=8192)
        for c in lanes:
            c.timing_enable(2); c.timing_reset()
        t0 = time.perf_counter()
        calls, st, ms, tot = host.process_resident_lanes(lanes, shards, split(steps), args.eps, args.min_pts_pct, capacity=8192)
        for c in lanes:
            c.synchronize()
        el = time.perf_counter() - t0
        tm = {}
        for c in lanes:
            for k, (ms_, n) in c.timing().items():
                a = tm.get(k, (0.0, 0)); tm[k] = (a[0] + ms_, a[1] + n)
            c.timing_enable(0)
        per = {k: v[0] / v[1] for k, v in tm.items() if v[1]}
        b_scan = 4.0 * reads.n_cigar + 23.0 * reads.n_reads + 16.0 * st.n_signatures
        b_depth = 4.0 * reads.n_cigar + 4.0 * depth_len
        return {"workload": "chr22-sized contig, CIGAR path only, 3 lanes (BASELINE.json configs[1]; BENCH_r01's configuration)", "value": reads.n_reads * steps / el,
                "unit": "reads/s", "ms_per_step": el / steps * 1e3, "steps": steps, "reads": int(reads.n_reads), "signatures": int(st.n_signatures),
                "kernel_ms": {k: round(v, 5) for k, v in per.items()},
                "cigar_scan_GBps": round(b_scan / (per["cigar_scan"] * 1e-3) / 1e9, 1) if per.get("cigar_scan") else None,
                "depth_GBps": round(b_depth / (per["depth"] * 1e-3) / 1e9, 1) if per.get("depth") else None,
                "host_merge_ms_per_step": round(st.ms_host_merge, 4), "device_chain_ms_per_step": round(st.ms_device, 4)}
    finally:
        for sh in shards:
            sh.free()
        for c in lanes:
            c.set_gate(None)
            c.close()
        gate.close()
        syn.free()


def from_file(cs, host, ctx, args, tech, config_id, gen_threads):
    """SURVEY §8d's from-file number: one chr22-sized contig staged as a real coordinate-sorted BGZF BAM + BAI, then end to end through
    SVCaller::runBam — BGZF inflate on the host cores + BAM record decode + H2D + device chain + host merge. Never `value`: it is
    bound by inflate on the host, not by the GPU. (Whole genome from one BAM: tools/bench_genome.py.)"""
    import tempfile
    from hmm_params import WGS_HMM
    threads = max(2, cpu_share())                           # this rank's CPU share (htslib's hts_set_threads counterpart: sv_caller.cpp:80, cnv_caller.cpp:427)
    syn = host.SynthShard(0x5EED0000 + 1000 * 1 + 22, GRCH38[21] if args.scale == 1.0 else max(200_000, int(GRCH38[21] * args.scale)), args.depth, tech, gen_threads)
    try:
        with tempfile.TemporaryDirectory(dir=os.environ.get("TMPDIR", "/tmp")) as d:
            bam = os.path.join(d, "shard.bam")
            t0 = time.perf_counter()
            nbytes = syn.write_bam(bam, "chr22", level=1, threads=threads)
            t_write = time.perf_counter() - t0
            hmm = cs.make_hmm(**WGS_HMM)
            best = None
            for _ in range(2):                                                      # second pass: page cache warm, as a re-run would be
                t0 = time.perf_counter()
                calls, _, bs = host.run_bam(ctx, bam, hmm, chromosomes=["chr22"], threads=threads, eps=args.eps, min_pts_pct=args.min_pts_pct,
                                            split_svs=True, cigar_cn=True)
                t = time.perf_counter() - t0
                if best is None or t < best[0]:
                    best = (t, bs, len(calls))
        t, bs, n_calls = best
        return {"reads_per_s": bs["n_reads"] / t, "seconds": round(t, 4), "decode_wait_s": round(bs["ms_decode"] * 1e-3, 4),
                "bam_bytes": int(nbytes), "bam_write_s": round(t_write, 3), "inflate_threads": threads, "merged_calls": int(n_calls),
                "compressed_GBps": nbytes / t / 1e9,
                "note": "BGZF inflate + BAM decode (query names kept for the split-read pass) + upload + all passes for one contig; sequences not stored (l_seq = 0)"}
    finally:
        syn.free()


def from_file_wgs(cs, host, ctx, args, lens, config_id, gen_threads):
    """The whole 30x genome from ONE coordinate-sorted BGZF BAM + BAI through SVCaller::runBam (contig i + 1 is inflated and decoded while
    contig i is on the device; every shard stays resident until the passes at the end): BGZF inflate on this rank's CPU share is the bound —
    a one-GPU box of the pool grants 16 CPUs (cgroup cpu.max), so 11.4 GB of BGZF at ~100 MB/s per core cannot take less than ~7 s there.
    Never `value`. Staging (generation + BAM writing) is reported and is not part of the run time."""
    import tempfile
    from hmm_params import WGS_HMM
    threads = max(2, cpu_share())
    n = len(lens)
    with tempfile.TemporaryDirectory(dir=os.environ.get("TMPDIR", "/tmp")) as d:
        bam = os.path.join(d, "genome.bam")
        t0 = time.perf_counter()
        w = host.SynthBamWriter(bam, NAMES[:n], lens, level=1, threads=threads)
        reads = ops = 0
        for k in range(n):
            syn = host.SynthShard(seed_of(config_id, k), lens[k], args.depth, 0, gen_threads)
            w.append(syn, k)
            reads += int(syn.reads.n_reads); ops += int(syn.reads.n_cigar)
            syn.free()
        w.close()
        t1 = time.perf_counter()
        hmm = cs.make_hmm(**WGS_HMM)
        calls, tids, bs = host.run_bam(ctx, bam, hmm, threads=threads, eps=args.eps, min_pts_pct=args.min_pts_pct, split_svs=True, cigar_cn=True, capacity=1 << 22)
        t2 = time.perf_counter()
        nbytes = os.path.getsize(bam)
    return {"reads_per_s": reads / (t2 - t1), "seconds": round(t2 - t1, 3), "decode_wait_s": round(bs["ms_decode"] * 1e-3, 3), "bam_bytes": int(nbytes), "stage_s": round(t1 - t0, 1),
            "inflate_threads": threads, "host_cpu_share": cpu_share(), "reads": reads, "cigar_ops": ops, "merged_calls": int(len(calls)), "compressed_GBps": nbytes / (t2 - t1) / 1e9,
            "note": "one BAM, one runBam call, all passes; the file is in the page cache (just written); inflate threads = this rank's CPU share"}


def cpu_baseline(samples, args, reads_genome):
    """The CPU restatement (oracle, kind "port") on the SAME 24 contigs, scheduled as the reference schedules them: one pool task per contig
    (sv_caller.cpp:827-863, ThreadPool of --threads workers), largest first. Bounded sample: every task gets the leading `cpu_sample_frac` of
    its contig's reads (same depth, shorter region). Per contig: CIGAR scan -> depth -> per-type O(n^2) DBSCAN, the three loops where the
    reference's time goes. The DBSCAN is quadratic in the signature count, so the full-size contigs would run at a LOWER rate
    than this sample does (the figure flatters the CPU). The copy-number and split-read passes are not part of the CPU figure (they would
    only lower it further). ctypes releases the GIL, so the tasks run concurrently.
    Thread counts (sv_caller.cpp:822-826 takes --threads): `value` = 24 workers, one per contig, whatever the host grants (the reference's
    own default use); `by_threads` adds the host's CPU share (no oversubscription: its per-task times are the clean ones) and ONE thread —
    the sum of those clean per-task times, derived, not run (the tasks are independent and single-threaded; running them in a row would
    take a minute and measure the same thing)."""
    import oracle_lib
    from concurrent.futures import ThreadPoolExecutor
    orc = oracle_lib.load_oracle()

    def one(i):
        name, sub, depth_len, n_full = samples[i]
        t0 = time.perf_counter()
        sig = orc.cigar_scan(sub, depth_len)
        t1 = time.perf_counter()
        _, s, nz = orc.depth(sub, depth_len)
        t2 = time.perf_counter()
        mean = s / nz if nz else 0.0
        min_pts = int(np.ceil(mean * args.min_pts_pct)) if args.min_pts_pct > 0 else 5
        kind = sig["qpos_kind"] & 3
        for sel in (kind == 1, kind != 1):
            part = sig[sel]
            if len(part) >= 2 and min_pts >= 1:
                orc.dbscan_iv(part["start"], part["end"], args.eps, min_pts)
        t3 = time.perf_counter()
        return (name, sub.n_reads, len(sig), t1 - t0, t2 - t1, t3 - t2)

    order = sorted(range(len(samples)), key=lambda i: -samples[i][1].n_reads)

    def run(workers):
        t0 = time.perf_counter()
        with ThreadPoolExecutor(max_workers=workers) as ex:
            res = list(ex.map(one, order))
        return time.perf_counter() - t0, res

    share = cpu_share()
    wall, res = run(len(samples))                                           # one worker per contig (24): the reference's default
    n_reads = sum(r[1] for r in res)
    n_sig = sum(r[2] for r in res)
    slow = max(res, key=lambda r: r[3] + r[4] + r[5])
    by_threads = {str(len(samples)): {"value": n_reads / wall, "wall_s": round(wall, 2), "note": f"{len(samples)} workers on {share} granted CPUs"}}
    if share < len(samples):
        wall_s, res_s = run(share)
        by_threads[str(share)] = {"value": n_reads / wall_s, "wall_s": round(wall_s, 2), "note": "workers = the host's CPU share (cgroup cpu.max / affinity), contigs largest first"}
        clean = res_s
    else:
        clean = res
    serial_s = sum(r[3] + r[4] + r[5] for r in clean)
    by_threads["1"] = {"value": n_reads / serial_s, "wall_s": round(serial_s, 2), "note": "derived: the sum of the per-contig task times of the run without oversubscription (independent single-threaded tasks)"}
    out = {"value": n_reads / wall, "unit": "reads/s", "cores": len(samples), "kind": "port",
           "sample": f"leading {args.cpu_sample_frac:g} of every contig's reads ({n_reads} of {int(reads_genome)} reads, {n_sig} signatures), {len(samples)} contigs = "
                     f"{len(samples)} workers at once, one contig each as the reference schedules them; wall {wall:.1f} s = the slowest task ({slow[0]}: scan {slow[3]:.2f} s + "
                     f"depth {slow[4]:.2f} s + O(n^2) DBSCAN {slow[5]:.2f} s); oracle/csv_oracle.c -O2. DBSCAN is quadratic: at full contig size the CPU rate is lower",
           "wall_s": round(wall, 2), "host_cpus": os.cpu_count(), "host_cpu_share": share, "signatures_clustered_per_s": n_sig / wall, "by_threads": by_threads,
           "cpu_seconds_by_loop": {"scan": round(sum(r[3] for r in clean), 2), "depth": round(sum(r[4] for r in clean), 2), "dbscan": round(sum(r[5] for r in clean), 2)}}
    # cross-check of the port against the REFERENCE's own dbscan.cpp (oracle/_ref, where it was built): same signature set, one thread each —
    # at -O2 and at the reference's shipped flags (its Makefile:14 passes no -O)
    ref = oracle_lib.load_ref()
    if ref is not None:
        name, sub, depth_len, _ = min(samples, key=lambda s: s[1].n_reads)
        sig = orc.cigar_scan(sub, depth_len)
        part = sig[(sig["qpos_kind"] & 3) != 1]
        t0 = time.perf_counter(); a = orc.dbscan_iv(part["start"], part["end"], args.eps, 3); t1 = time.perf_counter()
        b = ref.dbscan_iv(part["start"], part["end"], args.eps, 3); t2 = time.perf_counter()
        out["ref_dbscan_s"] = round(t2 - t1, 3)
        out["port_dbscan_s"] = round(t1 - t0, 3)
        same = bool(np.array_equal(a, b))
        ref0 = oracle_lib.load_ref_O0()
        if ref0 is not None:
            t3 = time.perf_counter(); c = ref0.dbscan_iv(part["start"], part["end"], args.eps, 3); t4 = time.perf_counter()
            out["ref_dbscan_O0_s"] = round(t4 - t3, 3)
            same = same and bool(np.array_equal(a, c))
        out["ref_dbscan_note"] = (f"the reference's own src/dbscan.cpp (oracle/_ref: -O2, and -g without -O as its Makefile:14 ships it) vs the port on the {len(part)} INS "
                                  f"signatures of the {name} sample; labels equal: {same}")
    return out


if __name__ == "__main__":
    main()
