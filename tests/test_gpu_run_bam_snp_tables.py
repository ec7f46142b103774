"""host.run_bam with snp_tables_on_device=True on the small from-file fixture of tests/test_gpu_bam.py: the same calls record for record
as without the switch, and the copy-number pass took the table route (host.cn_route_stats: its decode calls ran on resident tables, which
a from-file run could not reach before)."""
import numpy as np
import pytest

from contextsv_amd import Reads, host, make_hmm
from hmm_params import WGS_HMM
from test_gpu_e2e import CONTIG_LEN, _build

pytestmark = pytest.mark.gpu


def _fixture(tmp_path):
    """the contigs of test_gpu_bam.py's run: one BAM, and the SNPs as a VCF (no population file)"""
    contigs = _build(7)
    rng = np.random.default_rng(3)
    vcf = ["##fileformat=VCFv4.2", '##FORMAT=<ID=GT,Number=1,Type=String,Description="g">', '##FORMAT=<ID=DP,Number=1,Type=Integer,Description="d">',
           '##FORMAT=<ID=AD,Number=R,Type=Integer,Description="a">', "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tS"]
    for t, c in enumerate(contigs):
        pos = c["snps"]["pos"]
        dp = rng.integers(20, 60, len(pos))
        a1 = np.where(rng.random(len(pos)) < 0.6, dp // 2 + rng.integers(-3, 4, len(pos)), rng.choice([0, 1], len(pos)) * dp)
        vcf += ["contig%d\t%d\t.\tA\tG\t60\tPASS\t.\tGT:DP:AD\t0/1:%d:%d,%d" % (t, p, d, d - a, a) for p, d, a in zip(pos, dp, a1)]
        vcf.append("contig%d\t%d\t.\tA\tGT\t60\tPASS\t.\tGT:DP:AD\t0/1:30:15,15" % (t, int(pos[-1]) + 5))      # an indel: ignored
    snp_vcf = str(tmp_path / "snps.vcf")
    open(snp_vcf, "w").write("\n".join(vcf) + "\n")
    cat = lambda f, dt: np.ascontiguousarray(np.concatenate([getattr(c["reads"], f) for c in contigs]), dt)  # noqa: E731
    base = np.concatenate([[0], np.cumsum([c["reads"].n_cigar for c in contigs])]).astype(np.uint64)
    coff = np.concatenate([c["reads"].cigar_off[:-1] + base[i] for i, c in enumerate(contigs)] + [base[-1:]]).astype(np.uint64)
    reads = Reads(cat("pos", np.int32), cat("flag", np.uint16), cat("mapq", np.uint8), coff, cat("cigar", np.uint32))
    tid = np.concatenate([np.full(c["reads"].n_reads, t, np.int32) for t, c in enumerate(contigs)])
    qnames = ["r%d" % q for c in contigs for q in c["qname_id"]]
    bam = str(tmp_path / "reads.bam")
    host.write_bam(bam, ["contig%d" % t for t in range(len(contigs))], [CONTIG_LEN] * len(contigs), tid, reads, qnames, level=1, threads=8)
    return bam, snp_vcf, len(contigs)


def test_run_bam_with_snp_tables_on_device(ctx, tmp_path):
    bam, snp_vcf, n_contigs = _fixture(tmp_path)
    hmm = make_hmm(**WGS_HMM)
    host.cn_route_stats(reset=True)
    want, want_tid, st = host.run_bam(ctx, bam, hmm, threads=8, snp_vcf=snp_vcf)
    off = host.cn_route_stats(reset=True)
    assert st["n_contigs"] == n_contigs and len(want) > 20
    assert off["tables"] == 0 and off["queries"] > 0              # a from-file run without the switch has no resident table
    for kw in (dict(snp_tables_on_device=True), dict(snp_parse_on_device=True), dict(snp_parse_on_device=True, snp_tables_on_device=True)):
        got, got_tid, _ = host.run_bam(ctx, bam, hmm, threads=8, snp_vcf=snp_vcf, **kw)
        route = host.cn_route_stats(reset=True)
        assert np.array_equal(got_tid, want_tid) and got.tobytes() == want.tobytes(), kw
        if kw.get("snp_tables_on_device"):
            assert route["tables"] > 0 and route["queries"] == 0, (kw, route)      # every decode call looked its SNPs up on the device
        else:
            assert route["tables"] == 0 and route["queries"] == off["queries"], (kw, route)
    # the switch is restored: the next run is the plain one again
    host.run_bam(ctx, bam, hmm, threads=8, snp_vcf=snp_vcf)
    assert host.cn_route_stats(reset=True)["tables"] == 0
