"""The VCF writer's record lines on the device (csvgpu_vcf_format, VCFOptions::format_on_device) against the host writer.

    python tools/bench_vcf_format.py --out profiles/vcf_format

One MI355X, one process. A generated genome (24 contigs, --contig-mb each) is written as FASTA and opened twice (host backing, device
backing); every contig gets a resident shard with its depth map; the call set is genome-wide and of the benchmark's size (--calls over the
24 contigs, a VCF-like length mix: most calls below 1 kb, a tail to 1e5, and --long deletions of 1e5 - 1e6 bases). Rows, the settings
taking turns inside every repetition:
  save_vcf_host_genome      host.save_vcf, host-backed genome, depth from the shards
  save_vcf_device_genome    the same with the device-backed genome, format_on_device off (a fetch per contig)
  save_vcf_device_format    the same with format_on_device on (one csvgpu_vcf_format call)
  vcf_format_call           Context.vcf_format alone (both of its calls: the sizing one and the writing one): wall time, and the CSV_K_MISC
                            kernels' time between events
The three files must be byte-identical. Medians with p10 - p90 go to <out>/vcf_format.json.
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def spread(x):
    x = np.sort(np.asarray(x, float))
    return dict(median=float(np.median(x)), p10=float(np.percentile(x, 10)), p90=float(np.percentile(x, 90)), n=len(x))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "vcf_format"))
    ap.add_argument("--calls", type=int, default=30_000)
    ap.add_argument("--long", type=int, default=6, help="deletions of 1e5 - 1e6 bases")
    ap.add_argument("--contig-mb", type=float, default=4.0)
    ap.add_argument("--reps", type=int, default=7)
    args = ap.parse_args()
    import contextsv_amd as cs
    from contextsv_amd import host
    from contextsv_amd.host import CALL_DTYPE
    import synth_small as ss

    rng = np.random.default_rng(2024)
    scratch = tempfile.TemporaryDirectory(prefix="vcf_format_bench_")      # the FASTA and the three output files: removed at the end
    tmp = scratch.name
    L = int(args.contig_mb * 1e6)
    names = ["chr%d" % (k + 1) for k in range(22)] + ["chrX", "chrY"]
    pool = np.frombuffer(b"ACGT" * 30 + b"acgtNnRYKMSWBDHV", np.uint8)
    path = os.path.join(tmp, "genome.fa")
    with open(path, "wb") as f:
        for n in names:
            s = pool[rng.integers(0, len(pool), L)]
            f.write(b">" + n.encode() + b"\n")
            f.write(np.insert(s, np.arange(60, L, 60), 10).tobytes() + b"\n")
    ctx, gctx = cs.Context(0), cs.Context(0)
    g_host, g_dev = host.ReferenceGenome(path), host.ReferenceGenome(path, load_on_device=True, ctx=gctx)
    assert g_dev.device_stats["on_device"] == 1
    b = ctx.genome_builder(os.path.getsize(path))
    b.append(open(path, "rb").read())
    genome = b.finish()

    per = args.calls // len(names)
    items, tab, shards = [], [], []
    for k, n in enumerate(names):
        reads, depth_len = ss.random_shard(100 + k, n_reads=300, mean_ops=30, chr_len=L)
        sh = ctx.upload(reads, depth_len)
        sh.pipeline()
        shards.append(sh)
        c = np.zeros(per, CALL_DTYPE)
        c["sv_type"] = rng.choice([0, 0, 0, 1, 2, 3, 3, 3, 4, -1], per)
        c["start"] = np.sort(rng.integers(2, L - 1_100_000, per))
        length = np.where(rng.random(per) < 0.9, rng.integers(50, 1000, per), (10 ** rng.uniform(3, 5, per)).astype(np.int64))
        if k < args.long:
            length[rng.integers(0, per)] = int(10 ** rng.uniform(5, 6))
            c["sv_type"][np.argmax(length)] = 0
        c["end"] = c["start"] + length
        c["cluster_size"], c["hmm_likelihood"] = rng.integers(2, 60, per), -rng.random(per) * 5000
        c["aln_flags"], c["genotype"], c["cn_state"] = 1 << rng.integers(0, 9, per), rng.integers(0, 4, per), rng.integers(0, 7, per)
        alts = [(b"<DEL>", b"<DUP>", b"<INV>", pool[rng.integers(0, 120, int(min(l, 2000)))].tobytes(), b"<BND>")[t] if t >= 0 else b"." for t, l in zip(c["sv_type"], length)]
        items.append((n, c, alts, sh))
        tab.append((n, per, sh, None))
    calls = np.concatenate([i[1] for i in items])
    alts = [a for i in items for a in i[2]]

    def save(tag, g, on):
        d = os.path.join(tmp, tag)
        os.makedirs(d, exist_ok=True)
        t0 = time.perf_counter()
        host.save_vcf(d, g, items, file_date="20250926", ctx=ctx, format_on_device=on)
        return (time.perf_counter() - t0) * 1e3, os.path.join(d, "output.vcf")

    rows = {k: [] for k in ("save_vcf_host_genome", "save_vcf_device_genome", "save_vcf_device_format", "vcf_format_call_wall", "vcf_format_call_kernels")}
    files = {}
    devnull = os.open(os.devnull, os.O_WRONLY)
    saved = os.dup(2), os.dup(1)
    os.dup2(devnull, 2); os.dup2(devnull, 1)                  # the writer's per-contig messages and warnings are not what is timed
    try:
        for rep in range(args.reps + 1):                      # (the first repetition warms arenas, the page-locked block and the page cache)
            for tag, g, on in (("save_vcf_host_genome", g_host, False), ("save_vcf_device_genome", g_dev, False), ("save_vcf_device_format", g_dev, True)):
                ms, files[tag] = save(tag, g, on)
                if rep:
                    rows[tag].append(ms)
            ctx.timing_enable(1); ctx.timing_reset()
            t0 = time.perf_counter()
            text, status, counts = ctx.vcf_format(genome, tab, calls, alts)
            wall = (time.perf_counter() - t0) * 1e3
            k_ms, _ = ctx.timing()["misc"]
            ctx.timing_enable(0)
            if rep:
                rows["vcf_format_call_wall"].append(wall); rows["vcf_format_call_kernels"].append(k_ms)
    finally:
        os.dup2(saved[0], 2); os.dup2(saved[1], 1)
    ref = open(files["save_vcf_host_genome"], "rb").read()
    same = all(open(p, "rb").read() == ref for p in files.values())
    body = ref[ref.index(b"FORMAT\tSAMPLE\n") + 14:]
    out = dict(device="one MI355X", contigs=len(names), contig_bases=L, calls=len(calls), lines=int(counts["n_lines"]), text_bytes=int(counts["text_bytes"]),
               longest_line=int(max(len(l) for l in body.split(b"\n"))), routes=host.vcf_route_stats(), files_identical=bool(same), text_is_the_files_body=bool(text == body),
               ms={k: spread(v) for k, v in rows.items()}, reps=args.reps)
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, "vcf_format.json"), "w") as fh:
        json.dump(out, fh, indent=1)
    print(json.dumps(out))
    for sh in shards:
        sh.free()
    genome.free(); g_dev.close(); g_host.close(); ctx.close(); gctx.close()
    scratch.cleanup()
    return 0 if same and text == body else 1


if __name__ == "__main__":
    sys.exit(main())
