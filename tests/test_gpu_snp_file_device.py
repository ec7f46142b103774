"""host.SNPFile with parse_on_device=True (SNPFile::load / ::table through csvgpu_vcf_snp_parse / csvgpu_vcf_af_parse, the deferred lines and
the declined batches through the host functions): the tables are those of the option-off SNPFile, bit for bit with NaN as NaN, on the
generated files of tests/test_snp_io.py, plain and bgzipped — with two 3 000-byte members per batch, so that lines straddle batches."""
import numpy as np
import pytest

import vcf_parse_inputs as inp
from contextsv_amd import host
from test_snp_io import files  # noqa: F401  (the module's fixture: sample.vcf[.gz] and gnomad_txt/g.chr*.vcf[.gz])

pytestmark = pytest.mark.gpu


def _same(a, b):
    """bit for bit; NaN as NaN"""
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype != np.float64:
        return np.array_equal(a, b)
    nan = np.isnan(a)
    return np.array_equal(nan, np.isnan(b)) and np.array_equal(a.view(np.uint64)[~nan], b.view(np.uint64)[~nan])


def _tables_equal(on, off, chrom, pfb=None, eth=""):
    got, want = on.table(chrom, pfb, eth), off.table(chrom, pfb, eth)
    for g, w, name in zip(got, want, ("pos", "baf", "af_pos", "af")):
        assert _same(g, w), (chrom, eth, name, len(g), len(w))
    return got


@pytest.mark.parametrize("compressed", [False, True])
def test_tables_equal_the_host_parsers(ctx, files, compressed):  # noqa: F811
    d, g = files
    ext = ".gz" if compressed else ""
    n_lines = open(d / "sample.vcf", "rb").read().count(b"\n") - inp.HEADER.count("\n")
    for eth in ("nfe", "", "int"):
        on = host.SNPFile(str(d / ("sample.vcf" + ext)), threads=3, parse_on_device=True, ctx=ctx, window_blocks=2)
        off = host.SNPFile(str(d / ("sample.vcf" + ext)), threads=3)
        st = on.device_stats
        assert st["lines"] == n_lines and st["kept"] == off.records_kept == on.records_kept > 700 and st["deferred"] == 0 and st["declined_batches"] == 0
        for c in ("chr1", "chr2", "chrX"):
            pos, baf, af_pos, af = _tables_equal(on, off, c, g[c] + ext if c in g else None, eth)
            assert c == "chrX" or (len(pos) > 200 and (len(af_pos) > 30) == (eth != "int"))
        assert on.device_stats["lines"] > st["lines"] or eth == "int"        # the population files went through the device too
        assert on.device_stats["deferred"] == 0 and on.device_stats["declined_batches"] == 0


@pytest.mark.parametrize("compressed", [False, True])
def test_regions_match_the_oracle(ctx, files, oracle, compressed):  # noqa: F811
    d, g = files
    ext = ".gz" if compressed else ""
    snp = host.SNPFile(str(d / ("sample.vcf" + ext)), threads=3, parse_on_device=True, ctx=ctx, window_blocks=2)
    rng = np.random.default_rng(5)
    n_pfb = 0
    for chrom, span in (("chr1", 400_000), ("chr2", 300_000)):
        regions = [(1, span), (span // 2, span // 2), (span + 10, span + 500), (500, 100)]
        for _ in range(25):
            a = int(rng.integers(1, span))
            regions.append((a, a + int(rng.choice([0, 50, 2000, 20_000, 150_000]))))
        for a, b in regions:
            pos, baf, pfb = snp.query(chrom, a, b, pfb_vcf=g[chrom] + ext, ethnicity="nfe", threads=3)
            epos, ebaf, epfb = oracle.read_snp_af(str(d / "sample.vcf"), g[chrom], chrom, chrom, a, b, "AF_nfe")
            assert np.array_equal(pos, epos) and np.array_equal(baf, ebaf, equal_nan=True) and (pfb is None) == (epfb is None), (chrom, a, b)
            if pfb is not None:
                assert pfb[0] == epfb[0] and (pfb[1] == epfb[1] or (np.isnan(pfb[1]) and np.isnan(epfb[1])))
                n_pfb += 1
    assert n_pfb > 20


def test_deferred_lines_and_a_declined_batch(ctx, tmp_path):
    text, snps, rng = inp.generated_snp_text()
    head = text[:text.index(b"\n", 5000) + 1]
    extra = [l for _, l in inp.DELIBERATE_SNP] + inp.NOT_DEFERRED_SNP + [inp.DEFERRED_BY_ORDER]
    full = head + ("\n".join(extra) + "\n").encode() + text[len(head):]
    for compress in (False, True):
        path = str(tmp_path / ("d.vcf" + (".gz" if compress else "")))
        inp.write_vcf(path, inp.HEADER, [(0, full.decode().rstrip("\n"))], compress)
        on = host.SNPFile(path, parse_on_device=True, ctx=ctx, window_blocks=2)
        off = host.SNPFile(path)
        assert on.device_stats["deferred"] == len(inp.DELIBERATE_SNP) + 1 and on.device_stats["declined_batches"] == 0
        assert on.records_kept == off.records_kept
        for c in ("chr1", "chr2"):
            _tables_equal(on, off, c)
    # the population file's deferred lines, one of them the STOP line
    positions = [900, 1000] + inp.DELIBERATE_AF_POS + [1500]
    spath = str(tmp_path / "s.vcf")
    inp.write_vcf(spath, inp.HEADER, [(p, inp.GOOD % (p, "50", "40", "10,30")) for p in positions], False)
    (tmp_path / "chr").mkdir()
    lines = [inp.GN % ("900", "AF_nfe=0.25"), inp.GN % ("1000", "AF=0.5;AF_nfe=.")] + [l for _, l in inp.DELIBERATE_AF] + [inp.GN % ("1500", "AF_nfe=0.75")]
    for compress in (False, True):
        gpath = str(tmp_path / "chr" / ("g.vcf" + (".gz" if compress else "")))
        inp.write_vcf(gpath, inp.GNOMAD_HEADER, [(0, l) for l in lines], compress)
        on, off = host.SNPFile(spath, parse_on_device=True, ctx=ctx, window_blocks=2), host.SNPFile(spath)
        _, _, af_pos, _ = _tables_equal(on, off, "chr1", gpath, "nfe")
        assert 1500 not in af_pos.tolist() and 1007 in af_pos.tolist() and on.device_stats["deferred"] == len(inp.DELIBERATE_AF)
    # a header line in mid-file: the device declines the batch, the host parser reads it (and obeys the line)
    mid = text[:text.index(b"\n", 40_000) + 1]
    body = mid + b"##FORMAT=<ID=AD,Number=R,Type=String,Description=\"not Integer from here on\">\n" + text[len(mid):]
    path = str(tmp_path / "mid.vcf")
    inp.write_vcf(path, inp.HEADER, [(0, body.decode().rstrip("\n"))], False)
    on, off = host.SNPFile(path, parse_on_device=True, ctx=ctx), host.SNPFile(path)
    assert on.device_stats["declined_batches"] == 1 and on.records_kept == off.records_kept < host.SNPFile(str(tmp_path / "d.vcf")).records_kept
    for c in ("chr1", "chr2"):
        _tables_equal(on, off, c)


def test_option_needs_a_context(tmp_path):
    with pytest.raises(ValueError, match="context"):
        host.SNPFile(str(tmp_path / "x.vcf"), parse_on_device=True)
