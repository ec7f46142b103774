#!/usr/bin/env python
"""SNP tables built on the device (csvgpu_snp_builder_*, host.SNPFile(tables_on_device=True), host.run_bam(snp_tables_on_device=True))
against the host loader, in the manner of tools/bench_vcf_parse.py.

One generated sample VCF (--snp-lines, default 2e6, over --contigs contigs in file order) and a population file per contig
(--af-lines each). In one process, the settings taking turns call by call, medians of --reps calls with p10-p90:
  file      SNPFile() + table() of every contig end to end: the host parser, parse_on_device, tables_on_device
  builder   alone: Context.snp_builder append + finish of the whole text, against csvgpu_vcf_snp_parse plus a per-record merge of what it
            returns (the loop of SNPFile::load restated with numpy: one comparison per record for the contig, one stable grouping)
  run       --run-contig-len > 0: host.run_bam on a synthetic contig of that length (4e7: about chr22) with a SNP VCF, with and without
            snp_tables_on_device
Writes one JSON document (--out, e.g. profiles/snp_build/snp_build.json). The default of every switch stays off whatever this prints;
DESIGN.md section 7 has the rule for ever changing that: beat the option-off median by more than the option-off run's own p10-p90 spread."""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

from bench_vcf_parse import AF_HEADER, SNP_HEADER, af_text, snp_text  # noqa: E402


def stats(times):
    t = np.sort(np.asarray(times))
    return dict(median_s=float(np.median(t)), p10_s=float(np.percentile(t, 10)), p90_s=float(np.percentile(t, 90)), calls=len(t))


def turns(settings, reps, warm=1):
    """settings: name -> callable; every round runs each once, in an order that rotates, so that none is always first"""
    names = list(settings)
    out = {n: [] for n in names}
    for r in range(warm + reps):
        for n in names[r % len(names):] + names[:r % len(names)]:
            t0 = time.perf_counter()
            settings[n]()
            if r >= warm:
                out[n].append(time.perf_counter() - t0)
    return {n: stats(v) for n, v in out.items()}


def beats(on, off):
    """the rule of DESIGN.md section 7"""
    return bool(off["median_s"] - on["median_s"] > off["p90_s"] - off["p10_s"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--snp-lines", type=int, default=2_000_000)
    ap.add_argument("--contigs", type=int, default=24)
    ap.add_argument("--af-lines", type=int, default=20_000)
    ap.add_argument("--info-bytes", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--run-contig-len", type=int, default=0)
    ap.add_argument("--run-depth", type=float, default=30.0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import contextsv_amd as cs
    from contextsv_amd import host

    rng = np.random.default_rng(1)
    tmp = tempfile.mkdtemp()
    os.makedirs(os.path.join(tmp, "chr"))
    names = ["chr%d" % (k + 1) for k in range(a.contigs)]
    per = max(1, a.snp_lines // a.contigs)
    parts, gpaths = [], {}
    for name in names:                                           # bench_vcf_parse's lines, one stretch per contig
        text, pos = snp_text(per, rng)
        parts.append(text.replace(b"chr1\t", name.encode() + b"\t"))
        gpaths[name] = os.path.join(tmp, "chr", "g.%s.vcf" % name)
        open(gpaths[name], "wb").write(AF_HEADER.encode() + af_text(a.af_lines, a.info_bytes, pos, rng).replace(b"chr1\t", name.encode() + b"\t"))
    stext = b"".join(parts)
    spath = os.path.join(tmp, "sample.vcf")
    open(spath, "wb").write(SNP_HEADER.encode() + stext)
    res = dict(snp=dict(lines=per * a.contigs, bytes=len(stext), contigs=a.contigs), af=dict(lines_per_contig=a.af_lines), reps=a.reps)
    print("generated %.1f MB of sample text" % (len(stext) / 1e6), flush=True)

    with cs.Context(0) as ctx:
        def whole(**kw):
            f = host.SNPFile(spath, threads=1, ctx=ctx if kw else None, **kw)
            n = sum(len(f.table(c, gpaths[c], "nfe")[0]) for c in names)
            st = f.build_stats if kw.get("tables_on_device") else None
            f.close()
            return n, st
        n_off, _ = whole()
        n_on, st = whole(tables_on_device=True)
        assert n_off == n_on, (n_off, n_on)
        res["file"] = turns(dict(host=lambda: whole(), parse_on_device=lambda: whole(parse_on_device=True), tables_on_device=lambda: whole(tables_on_device=True)), a.reps)
        res["file"]["build_stats"] = st
        res["file"]["tables_beat_host"] = beats(res["file"]["tables_on_device"], res["file"]["host"])
        print("file: " + ", ".join("%s %.3f s" % (k, v["median_s"]) for k, v in res["file"].items() if isinstance(v, dict) and "median_s" in v), flush=True)

        buf = np.frombuffer(stext, np.uint8)

        def build():
            b = ctx.snp_builder(0)
            got = b.append(buf)
            ids, run_contig = {}, []
            for o, n in zip(got["run_line_off"].tolist(), got["run_chrom_len"].tolist()):
                run_contig.append(ids.setdefault(stext[o:o + n], len(ids)))
            b.finish(run_contig).free()

        def parse_and_merge():
            r = ctx.vcf_snp_parse(buf)
            off, ln = r["line_off"], r["chrom_len"]
            # SNPFile::load's loop: a record starts a new contig when its CHROM differs from the one before; then the records per contig
            first = stext[off[0]:off[0] + ln[0]] if len(off) else b""
            new = np.ones(len(off), bool)
            for k in range(1, len(off)):
                name = stext[off[k]:off[k] + ln[k]]
                new[k] = name != first
                first = name
            run = np.cumsum(new) - 1
            order = np.argsort(run, kind="stable")
            return r["pos"][order], r["value"][order]
        res["builder"] = turns(dict(append_finish=build, parse_plus_host_merge=parse_and_merge), max(3, a.reps // 3))
        res["builder"]["note"] = "parse_plus_host_merge restates the C++ loop in Python: an upper bound of its cost, not a measurement of it"
        print("builder: " + ", ".join("%s %.3f s" % (k, v["median_s"]) for k, v in res["builder"].items() if isinstance(v, dict)), flush=True)

        if a.run_contig_len > 0:
            from contextsv_amd import make_hmm
            from hmm_params import WGS_HMM
            syn = host.SynthShard(11, a.run_contig_len, a.run_depth, threads=8, with_seq=True)
            bam = os.path.join(tmp, "run.bam")
            syn.write_bam(bam, chr_name="chr22", threads=8)
            rtext, _ = snp_text(max(1000, a.run_contig_len // 1000), rng)
            rvcf = os.path.join(tmp, "run.vcf")
            open(rvcf, "wb").write(SNP_HEADER.encode() + rtext.replace(b"chr1\t", b"chr22\t"))
            hmm = make_hmm(**WGS_HMM)
            run = lambda **kw: host.run_bam(ctx, bam, hmm, threads=8, snp_vcf=rvcf, **kw)  # noqa: E731
            want, got = run()[0], run(snp_tables_on_device=True)[0]
            assert want.tobytes() == got.tobytes()
            res["run"] = turns(dict(off=lambda: run(), snp_tables_on_device=lambda: run(snp_tables_on_device=True)), a.reps)
            res["run"]["calls"] = int(len(want))
            res["run"]["tables_beat_off"] = beats(res["run"]["snp_tables_on_device"], res["run"]["off"])
            print("run: off %.3f s, tables %.3f s" % (res["run"]["off"]["median_s"], res["run"]["snp_tables_on_device"]["median_s"]), flush=True)

    line = json.dumps(res, indent=1)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
