"""host.SNPFile with tables_on_device=True (SNPFile::load through csvgpu_snp_builder_*, SNPFile::table through csvgpu_snp_columns_af_parse /
_table): the tables and queries are those of the option-off SNPFile, bit for bit with NaN as NaN, on the generated files of
tests/test_snp_io.py, plain and bgzipped + indexed, with window_blocks=1 so that batches are many; build_stats shows that the device appended
most of the kept records (tests/test_snp_build_inputs.py: the text makes that possible) and which contigs' tables are resident."""
import numpy as np
import pytest

import vcf_parse_inputs as inp
from contextsv_amd import host
from test_gpu_snp_file_device import _same, _tables_equal
from test_snp_io import files  # noqa: F401  (the module's fixture: sample.vcf[.gz] and gnomad_txt/g.chr*.vcf[.gz])

pytestmark = pytest.mark.gpu


def _open(path, ctx):
    return host.SNPFile(path, threads=3, tables_on_device=True, ctx=ctx, window_blocks=1), host.SNPFile(path, threads=3)


@pytest.mark.parametrize("compressed", [False, True])
def test_tables_and_queries_equal_the_host_loaders(ctx, files, compressed):  # noqa: F811
    d, g = files
    ext = ".gz" if compressed else ""
    n_lines = open(d / "sample.vcf", "rb").read().count(b"\n") - inp.HEADER.count("\n")
    for eth in ("nfe", ""):
        on, off = _open(str(d / ("sample.vcf" + ext)), ctx)
        st, bs = on.device_stats, on.build_stats
        assert st["lines"] == n_lines and on.records_kept == off.records_kept > 700 and st["declined_batches"] == 0
        # the device's share: more than half of the kept records were appended by the device
        assert st["kept"] + bs["appended_host"] == on.records_kept and st["kept"] > on.records_kept / 2, (st, bs)
        assert bs["runs"] >= 2 and bs["tables_resident"] == 0
        if compressed:
            assert bs["runs"] > 10                                # many batches: a contig continues over many appends
        for c in ("chr1", "chr2", "chrX"):
            pos, baf, af_pos, af = _tables_equal(on, off, c, g[c] + ext if c in g else None, eth)
            assert c == "chrX" or (len(pos) > 200 and len(af_pos) > 30)
        assert on.build_stats["tables_resident"] == 2             # both contigs are ascending
        assert on.device_stats["lines"] > st["lines"]             # the population files went through the device too
        rng = np.random.default_rng(5)
        for chrom, span in (("chr1", 400_000), ("chr2", 300_000)):
            regions = [(1, span), (span // 2, span // 2), (span + 10, span + 500), (500, 100)]
            regions += [(a, a + int(rng.choice([0, 50, 2000, 150_000]))) for a in rng.integers(1, span, 8).tolist()]
            for a, b in regions:
                got = on.query(chrom, a, b, pfb_vcf=g[chrom] + ext, ethnicity=eth, threads=3)
                want = off.query(chrom, a, b, pfb_vcf=g[chrom] + ext, ethnicity=eth, threads=3)
                assert _same(got[0], want[0]) and _same(got[1], want[1]), (chrom, a, b)
                assert (got[2] is None) == (want[2] is None) and (got[2] is None or (got[2][0] == want[2][0] and _same(np.array([got[2][1]]), np.array([want[2][1]]))))
        on.close()


def test_deferred_lines_a_declined_batch_and_an_unsorted_contig(ctx, tmp_path):
    text, snps, rng = inp.generated_snp_text()
    head = text[:text.index(b"\n", 5000) + 1]
    extra = [l for _, l in inp.DELIBERATE_SNP] + inp.NOT_DEFERRED_SNP + [inp.DEFERRED_BY_ORDER]
    full = head + ("\n".join(extra) + "\n").encode() + text[len(head):]
    for compress in (False, True):
        path = str(tmp_path / ("d.vcf" + (".gz" if compress else "")))
        inp.write_vcf(path, inp.HEADER, [(0, full.decode().rstrip("\n"))], compress)
        on, off = _open(path, ctx)
        assert on.device_stats["deferred"] == len(inp.DELIBERATE_SNP) + 1 and on.records_kept == off.records_kept
        assert 0 < on.build_stats["appended_host"] <= len(inp.DELIBERATE_SNP) + 1
        for c in ("chr1", "chr2"):
            _tables_equal(on, off, c)
        # the deliberate lines sit among chr1's at positions of their own: chr1 is no longer ascending and keeps the host arrays only
        assert on.build_stats["tables_resident"] == 1
    # a header line in mid-file: the device declines the batch, it goes through the host parser (which obeys the line) and append_host
    mid = text[:text.index(b"\n", 40_000) + 1]
    body = mid + b"##FORMAT=<ID=AD,Number=R,Type=String,Description=\"not Integer from here on\">\n" + text[len(mid):]
    path = str(tmp_path / "mid.vcf")
    inp.write_vcf(path, inp.HEADER, [(0, body.decode().rstrip("\n"))], False)
    on, off = _open(path, ctx)
    assert on.device_stats["declined_batches"] == 1 and on.records_kept == off.records_kept < host.SNPFile(str(tmp_path / "d.vcf")).records_kept
    for c in ("chr1", "chr2"):
        _tables_equal(on, off, c)
    # one contig unsorted (two stretches of its lines swapped), one returning after another: the same tables, the unsorted one not resident
    lines = text.decode().rstrip("\n").split("\n")
    c1 = [l for l in lines if l.startswith("chr1\t")]
    c2 = [l for l in lines if l.startswith("chr2\t")]
    c2[100:110], c2[300:310] = c2[300:310], c2[100:110]
    path = str(tmp_path / "unsorted.vcf")
    inp.write_vcf(path, inp.HEADER, [(0, l) for l in c1[:400] + c2 + c1[400:]], False)
    on, off = _open(path, ctx)
    assert on.records_kept == off.records_kept and on.build_stats["runs"] >= 3
    for c in ("chr1", "chr2"):
        _tables_equal(on, off, c)
    assert on.build_stats["tables_resident"] == 1
    pos = on.table("chr2")[0]
    assert (pos[1:] < pos[:-1]).any() and not (on.table("chr1")[0][1:] < on.table("chr1")[0][:-1]).any()


def test_option_needs_a_context(tmp_path):
    with pytest.raises(ValueError, match="context"):
        host.SNPFile(str(tmp_path / "x.vcf"), tables_on_device=True)
