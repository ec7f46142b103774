#!/usr/bin/env python
"""The device VCF parser (csvgpu_vcf_snp_parse / csvgpu_vcf_af_parse / _dev, host.SNPFile(parse_on_device=True)) against the host parser.

Two generated files: a sample VCF (--snp-lines, default 2e6) and a gnomAD-like population file (--af-lines, default 5e5, about --info-bytes
of INFO per line with AF_nfe behind a fifth of it). For each: bytes of text per second as the median of --reps warm calls with p10-p90, for
  host_1thread   host.SNPFile on one thread (what runs today: inflate does not exist for a plain file, the parse is serial anyway)
  dev            the _dev entry point with the text resident on the device: wall time of the call (its two read-backs included) and the
                 kernels' time by the context's timers (CSV_K_MISC: around the launches, not the read-backs), the latter also as a
                 fraction of the HBM peak over the bytes the kernels must read (the text twice for the line ends; once more by the
                 per-line kernel for the sample file; for the population file, whose lines are mostly left at their heads, only the
                 two line-end passes are counted and the figure is a lower bound, no roofline)
  host_ptr       the host-pointer entry point, upload included (a sizing call is not part of it: the arrays are large enough)
  file           SNPFile() / .table() end to end, option off and on
Writes one JSON document (--out). With --parent-tree (another built checkout, e.g. the parent commit's) SNPFile() is also timed
through that tree's package, the two taking turns, on the same sample file."""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.environ.get("BENCH_VCF_TREE") or ROOT)      # (the --parent-tree child imports that tree's package)
HBM_PEAK = 8.0e12            # bytes per second, MI355X

SNP_HEADER = ("##fileformat=VCFv4.2\n##FORMAT=<ID=GT,Number=1,Type=String,Description=\"g\">\n##FORMAT=<ID=DP,Number=1,Type=Integer,Description=\"d\">\n"
              "##FORMAT=<ID=AD,Number=R,Type=Integer,Description=\"a\">\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tSAMPLE\n")
AF_HEADER = "##fileformat=VCFv4.2\n##INFO=<ID=AF_nfe,Number=A,Type=Float,Description=\"f\">\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\n"


def snp_text(n, rng):
    """n sample lines of about 150 bytes, positions ascending; a tenth fails a filter"""
    pos = np.cumsum(rng.integers(1, 200, n))
    dp = rng.integers(8, 80, n)
    a0 = (dp * rng.random(n)).astype(int)
    q = rng.uniform(20, 90, n)
    bases = "ACGT"
    out = []
    for k in range(n):
        out.append("chr1\t%d\t.\t%s\t%s\t%.2f\tPASS\tAC=1;AF=0.5;AN=2;DP=%d;MQ=60.00;QD=12.3;SOR=0.693;FS=0.000;MLEAC=1;MLEAF=0.500\tGT:AD:DP:GQ:PL\t0/1:%d,%d:%d:99:255,0,255"
                   % (pos[k], bases[k & 3], bases[(k + 1 + (k >> 2) % 3) & 3], q[k], dp[k], a0[k], dp[k] - a0[k], dp[k]))
    return ("\n".join(out) + "\n").encode(), pos


def af_text(n, info_bytes, snp_pos, rng):
    """n population lines, every fourth on a sample position; INFO of about info_bytes with AF_nfe a fifth of the way in"""
    on = rng.choice(snp_pos, n // 4)
    pos = np.sort(np.concatenate([on, rng.integers(1, int(snp_pos[-1]), n - len(on))]))
    keys = ["AC", "AN", "AF", "AC_afr", "AN_afr", "AF_afr", "AC_amr", "AF_amr", "nhomalt", "AC_XX", "AF_XX", "faf95", "vep", "cadd", "revel", "popmax"]
    def fill(m, salt):
        parts, size, k = [], 0, salt
        while size < m:
            p = "%s_%d=%s" % (keys[k % len(keys)], k % 97, "0.%05d" % ((k * 7919) % 100000) if k % 3 else "x" * (k % 40 + 1))
            parts.append(p)
            size += len(p) + 1
            k += 1
        return ";".join(parts)
    pool = [(fill(info_bytes // 5, s), fill(info_bytes - info_bytes // 5, s + 1000)) for s in range(64)]
    afs = ["0.5", "0.25", "0.001", "0.0372", "1.2e-2", ".", "0.33,0.1", "0.998"]
    out = []
    for k in range(n):
        a, b = pool[k & 63]
        out.append("chr1\t%d\trs%d\tA\tG\t.\tPASS\t%s;AF_nfe=%s;%s" % (pos[k], k, a, afs[k & 7], b))
    return ("\n".join(out) + "\n").encode()


def stats(times, nbytes):
    t = np.sort(np.asarray(times))
    med, p10, p90 = float(np.median(t)), float(np.percentile(t, 10)), float(np.percentile(t, 90))
    return dict(median_s=med, p10_s=p10, p90_s=p90, gb_per_s=nbytes / med / 1e9, gb_per_s_p10_p90=[nbytes / p90 / 1e9, nbytes / p10 / 1e9], calls=len(t))


def timed(fn, reps, warm=2):
    for _ in range(warm):
        fn()
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        out.append(time.perf_counter() - t0)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--snp-lines", type=int, default=2_000_000)
    ap.add_argument("--af-lines", type=int, default=500_000)
    ap.add_argument("--info-bytes", type=int, default=4000)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=None)
    ap.add_argument("--parent-tree", default=None)
    ap.add_argument("--parent-child", default=None, help=argparse.SUPPRESS)      # internal: time SNPFile() in this process (BENCH_VCF_TREE: whose package)
    a = ap.parse_args()

    if a.parent_child:                                        # a process of its own per library: one copy of the mirror per process
        from contextsv_amd import host
        print(json.dumps(timed(lambda: host.SNPFile(a.parent_child, threads=1).close(), a.reps, 1)))
        return

    import contextsv_amd as cs
    from contextsv_amd import _lib, host
    rng = np.random.default_rng(1)
    tmp = tempfile.mkdtemp()
    os.makedirs(os.path.join(tmp, "chr"))
    t0 = time.perf_counter()
    stext, spos = snp_text(a.snp_lines, rng)
    gtext = af_text(a.af_lines, a.info_bytes, spos, rng)
    spath, gpath = os.path.join(tmp, "sample.vcf"), os.path.join(tmp, "chr", "g.vcf")
    open(spath, "wb").write(SNP_HEADER.encode() + stext)
    open(gpath, "wb").write(AF_HEADER.encode() + gtext)
    res = dict(snp=dict(lines=a.snp_lines, bytes=len(stext)), af=dict(lines=a.af_lines, bytes=len(gtext), info_bytes=a.info_bytes),
               generate_s=time.perf_counter() - t0, reps=a.reps, hbm_peak_bytes_per_s=HBM_PEAK)
    print("generated %.1f MB + %.1f MB in %.1f s" % (len(stext) / 1e6, len(gtext) / 1e6, res["generate_s"]), flush=True)

    with cs.Context(0) as ctx:
        lib, h = ctx.lib, ctx.h
        off = host.SNPFile(spath, threads=1)
        kept = np.sort(off.table("chr1")[0])
        n_af = len(host.SNPFile(spath, threads=1).table("chr1", gpath, "nfe")[2])      # (a file's population hits are built once, on the first use of the contig)
        res["snp"]["kept"], res["af"]["kept"] = int(off.records_kept), int(n_af)

        # ---- end to end through the file
        res["snp"]["file_off"] = stats(timed(lambda: host.SNPFile(spath, threads=1).close(), a.reps), len(stext))
        res["snp"]["file_on"] = stats(timed(lambda: host.SNPFile(spath, threads=1, parse_on_device=True, ctx=ctx).close(), a.reps), len(stext))
        on = host.SNPFile(spath, threads=1, parse_on_device=True, ctx=ctx)
        res["snp"]["device_stats"] = on.device_stats
        print("snp file: off %.2f GB/s, on %.2f GB/s" % (res["snp"]["file_off"]["gb_per_s"], res["snp"]["file_on"]["gb_per_s"]), flush=True)

        def table(dev):
            times = []
            for _ in range(a.reps + 1):                       # table() builds once per SNPFile: a fresh one per call, its load not timed
                f = host.SNPFile(spath, threads=1, parse_on_device=dev, ctx=ctx if dev else None)
                t = time.perf_counter()
                got = f.table("chr1", gpath, "nfe")
                times.append(time.perf_counter() - t)
                assert len(got[2]) == n_af
                f.close()
            return times[1:]
        res["af"]["file_off"] = stats(table(False), len(gtext))
        res["af"]["file_on"] = stats(table(True), len(gtext))
        print("af file: off %.2f GB/s, on %.2f GB/s" % (res["af"]["file_off"]["gb_per_s"], res["af"]["file_on"]["gb_per_s"]), flush=True)
        res["snp"]["host_1thread"], res["af"]["host_1thread"] = res["snp"]["file_off"], res["af"]["file_off"]        # a plain file: the parse is all there is

        # ---- the entry points alone
        for name, text in (("snp", stext), ("af", gtext)):
            af = name == "af"
            buf = np.frombuffer(text, np.uint8)
            cap = len(kept) + 16
            arrays = dict(line_off=np.zeros(cap, np.uint32), chrom_len=np.zeros(cap, np.uint32), pos=np.zeros(cap, np.uint32), value=np.zeros(cap, np.float64),
                          defer_off=np.zeros(1024, np.uint32))
            if af:
                del arrays["chrom_len"]
            call = (lambda: ctx.vcf_af_parse_into(buf, "chr1", "AF_nfe=", kept, arrays)) if af else (lambda: ctx.vcf_snp_parse_into(buf, arrays))
            rc, c = call()
            assert rc == 0 and c["n_kept"] == res[name]["kept"] and c["n_deferred"] == 0, (rc, c)
            res[name]["host_ptr"] = stats(timed(call, a.reps), len(text))
            # resident: text, positions and outputs in device memory
            d_text = lib.csvgpu_dev_alloc(h, len(text) + 16)
            d = {k: lib.csvgpu_dev_alloc(h, v.nbytes) for k, v in arrays.items()}
            d_pos = lib.csvgpu_dev_alloc(h, max(kept.nbytes, 4))
            assert d_text and d_pos and all(d.values())
            ctx._check(lib.csvgpu_upload(h, d_text, buf.ctypes.data, len(text)))
            ctx._check(lib.csvgpu_upload(h, d_pos, kept.ctypes.data, kept.nbytes))
            o = _lib.csv_vcf_out()
            for k, p in d.items():
                setattr(o, k, p)
            o.cap, o.cap_defer = cap, 1024
            cc = _lib.csv_vcf_counts()
            if af:
                dev = lambda: lib.csvgpu_vcf_af_parse_dev(h, d_text, len(text), b"chr1", 4, b"AF_nfe=", 7, d_pos, len(kept), C.byref(o), C.byref(cc))
            else:
                dev = lambda: lib.csvgpu_vcf_snp_parse_dev(h, d_text, len(text), 1, 1, C.byref(o), C.byref(cc))
            assert dev() == 0 and cc.n_kept == res[name]["kept"], (cc.n_kept, cc.status)
            res[name]["dev"] = stats(timed(dev, a.reps), len(text))
            ctx.timing_enable(1)
            ker = []
            for _ in range(a.reps):
                ctx.timing_reset()
                assert dev() == 0
                ker.append(ctx.timing()["misc"][0] / 1e3)
            ctx.timing_enable(0)
            k = stats(ker, len(text))
            # the line-end kernels read the text twice; the per-line kernel reads a sample line whole, of a population line only the head
            # and INFO up to the key on the lines that hit: for that file the bytes are a lower bound and the fraction is no roofline figure
            k["must_read_bytes"] = (2 if af else 3) * len(text)
            k["must_read_is_lower_bound"] = af
            k["hbm_fraction"] = k["must_read_bytes"] / k["median_s"] / HBM_PEAK
            res[name]["dev_kernels"] = k
            for p in [d_text, d_pos] + list(d.values()):
                lib.csvgpu_dev_free(h, p)
            print("%s: dev %.1f GB/s wall, %.1f GB/s kernels (%.3f of HBM peak over %d x text), host_ptr %.2f GB/s" %
                  (name, res[name]["dev"]["gb_per_s"], k["gb_per_s"], k["hbm_fraction"], 2 if af else 3, res[name]["host_ptr"]["gb_per_s"]), flush=True)

    if a.parent_tree:                                         # this tree's mirror and another's on the same file, taking turns
        turns = dict(branch=[], parent=[])
        for turn in range(8):                                 # parent, branch, branch, parent, ...: neither is always the one that goes first
            who = "parent" if turn % 4 in (0, 3) else "branch"
            env = dict(os.environ)
            if who == "parent":
                env["BENCH_VCF_TREE"] = os.path.abspath(a.parent_tree)
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--parent-child", spath, "--reps", str(max(a.reps // 2, 5))], env=env, capture_output=True,
                               text=True, check=True)
            turns[who] += json.loads(r.stdout.strip().splitlines()[-1])
        res["snp"]["file_off_branch"] = stats(turns["branch"], len(stext))
        res["snp"]["file_off_parent"] = stats(turns["parent"], len(stext))
        b, p = res["snp"]["file_off_branch"], res["snp"]["file_off_parent"]
        res["snp"]["branch_median_inside_parent_p10_p90"] = bool(p["p10_s"] <= b["median_s"] <= p["p90_s"])
        print("SNPFile() option off: parent %.3f s [%.3f, %.3f], branch %.3f s" % (p["median_s"], p["p10_s"], p["p90_s"], b["median_s"]), flush=True)

    line = json.dumps(res, indent=1)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
