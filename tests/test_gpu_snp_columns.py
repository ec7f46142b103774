"""What is made from a contig's resident columns (csvgpu_snp_columns_af_parse / _table): the population parse against Context.vcf_af_parse
with the host-sorted positions, and the table against Context.snp_table_hits on the host arrays, over the region families of
tests/snp_table_inputs.py — byte for byte, the reference never being the builder."""
import numpy as np
import pytest

import snp_build_inputs as sb
import snp_table_inputs as sti
import vcf_parse_inputs as inp
from contextsv_amd import _lib

pytestmark = pytest.mark.gpu

AF_KEYS = ("line_off", "pos", "value", "defer_off")
COUNT_KEYS = ("n_lines", "n_kept", "n_deferred", "stop_off", "status", "declined")


@pytest.fixture(scope="module")
def generated(ctx):
    """the generated sample text as columns (one device append), the model beside them, and the population texts"""
    text, snps, rng = sb.generated()
    m, b = sb.Model(), ctx.snp_builder()
    m.append(text)
    got = b.append(text)
    assert got["n_kept"] == m.n_device > 700 and got["n_deferred"] == 0
    cols = b.finish(m.run_contig)
    gn = {c: inp.generated_gnomad_text(rng, snps, c)[0] for c in ("chr1", "chr2")}
    yield cols, m, gn
    cols.free()


def _same_parse(got, ref):
    assert {k: got[k] for k in COUNT_KEYS} == {k: ref[k] for k in COUNT_KEYS}
    if not ref["declined"]:
        for k in AF_KEYS:
            assert got[k].tobytes() == ref[k].tobytes(), k


@pytest.mark.parametrize("chrom", ("chr1", "chr2"))
@pytest.mark.parametrize("needle", ("AF=", "AF_nfe="))
def test_af_parse_of_the_generated_population_text(ctx, generated, chrom, needle):
    cols, m, gn = generated
    pos, _, asc = m.columns()[m.ids[chrom.encode()]]
    assert asc
    ref = ctx.vcf_af_parse(gn[chrom], chrom, needle, np.sort(pos))
    assert ref["n_kept"] > 20
    exp = inp.expected_af(gn[chrom], chrom, needle, np.sort(pos))
    assert ref["pos"].tobytes() == exp["pos"].tobytes() and ref["stop_off"] == exp["stop_off"]
    _same_parse(cols.af_parse(m.ids[chrom.encode()], gn[chrom], chrom, needle), ref)
    # the other contig's file on this contig's positions: nothing kept, the same counts
    other = gn["chr2" if chrom == "chr1" else "chr1"]
    _same_parse(cols.af_parse(m.ids[chrom.encode()], other, chrom, needle), ctx.vcf_af_parse(other, chrom, needle, np.sort(pos)))


def test_af_parse_of_the_deliberate_lines_capacity_and_decline(ctx):
    """the deferred kinds of tests/vcf_parse_inputs.py on columns that hold their positions; CSV_ECAPACITY with the exact counts; a '#' line
    declines"""
    b = ctx.snp_builder()
    b.append(sb.body([sb.good(p) for p in inp.DELIBERATE_AF_POS]))
    cols = b.finish([0])
    text = sb.body([l.encode() for _, l in inp.DELIBERATE_AF] + [(inp.GN % ("1003", "AF_nfe=0.25")).encode()])
    ref = ctx.vcf_af_parse(text, "chr1", "AF_nfe=", inp.DELIBERATE_AF_POS)
    exp = inp.expected_af(text, "chr1", "AF_nfe=", np.asarray(inp.DELIBERATE_AF_POS, np.uint32))
    assert ref["defer_off"].tobytes() == exp["defer_off"].tobytes() and ref["n_deferred"] >= 6 and ref["n_kept"] == 1
    _same_parse(cols.af_parse(0, text, "chr1", "AF_nfe="), ref)
    out = dict(line_off=np.zeros(0, np.uint32), pos=np.zeros(0, np.uint32), value=np.zeros(0), defer_off=np.zeros(1, np.uint32))
    rc, c = cols.af_parse_into(0, text, "chr1", "AF_nfe=", out)
    rc2, c2 = ctx.vcf_af_parse_into(text, "chr1", "AF_nfe=", np.asarray(inp.DELIBERATE_AF_POS, np.uint32), out)
    assert rc == rc2 == _lib.CSV_ECAPACITY and c == c2 and c["n_kept"] == 1
    bad = text + b"#late\n"
    _same_parse(cols.af_parse(0, bad, "chr1", "AF_nfe="), ctx.vcf_af_parse(bad, "chr1", "AF_nfe=", inp.DELIBERATE_AF_POS))
    assert cols.af_parse(0, bad, "chr1", "AF_nfe=")["declined"]
    with pytest.raises(_lib.CsvError, match="holds no record"):
        cols.af_parse(3, text, "chr1", "AF_nfe=")
    cols.free()


def test_af_parse_dev_with_the_text_and_the_outputs_on_the_device(ctx, generated):
    """csvgpu_snp_columns_af_parse_dev: the text in device memory at an odd address, the outputs device arrays; equal to the host-pointer
    form, which the tests above hold against Context.vcf_af_parse"""
    cols, m, gn = generated
    lib, cid = ctx.lib, m.ids[b"chr1"]
    ref = cols.af_parse(cid, gn["chr1"], "chr1", "AF_nfe=")
    k, d = ref["n_kept"], ref["n_deferred"]
    assert k > 20
    data = np.frombuffer(gn["chr1"], np.uint8)
    sizes = dict(line_off=4 * (k + 2), pos=4 * (k + 2), value=8 * (k + 2), defer_off=4 * (d + 2))
    dev = {name: lib.csvgpu_dev_alloc(ctx.h, n) for name, n in sizes.items()}
    d_text = lib.csvgpu_dev_alloc(ctx.h, len(data) + 16)
    assert d_text and all(dev.values())
    try:
        ctx._check(lib.csvgpu_upload(ctx.h, d_text + 5, data.ctypes.data, len(data)))
        o, c = _lib.csv_vcf_out(), _lib.csv_vcf_counts()
        for name in dev:
            setattr(o, name, dev[name])
        o.cap, o.cap_defer = k + 2, d + 2
        rc = lib.csvgpu_snp_columns_af_parse_dev(ctx.h, cols.h, cid, d_text + 5, len(data), b"chr1", 4, b"AF_nfe=", 7, o, c)
        assert rc == 0 and (c.n_lines, c.n_kept, c.n_deferred, c.stop_off, c.status) == (ref["n_lines"], k, d, ref["stop_off"], 0)
        for name, n in (("line_off", k), ("pos", k), ("value", k), ("defer_off", d)):
            got = np.zeros(n, ref[name].dtype)
            if n:
                ctx._check(lib.csvgpu_download(ctx.h, got.ctypes.data, dev[name], got.nbytes))
            assert got.tobytes() == ref[name].tobytes(), name
        o.cap = k - 1
        assert lib.csvgpu_snp_columns_af_parse_dev(ctx.h, cols.h, cid, d_text + 5, len(data), b"chr1", 4, b"AF_nfe=", 7, o, c) == _lib.CSV_ECAPACITY
        assert (c.n_kept, c.n_deferred) == (k, d)
    finally:
        for p in list(dev.values()) + [d_text]:
            lib.csvgpu_dev_free(ctx.h, p)


def _same_query(ctx, got_table, ref_table, t, seed):
    rs, re = sti.regions_for(t, seed)
    got, ref = ctx.snp_table_query(got_table, rs, re), ctx.snp_table_query(ref_table, rs, re)
    for k in ("snp_off", "pos", "baf", "pfb"):
        assert got[k].tobytes() == ref[k].tobytes(), k
    return len(ref["pos"])


def test_tables_of_the_hit_families(ctx):
    """every first-hit table of tests/snp_table_inputs.py that holds a record, each a contig of one builder (host-appended, the key its
    index): columns_table + snp_table_query equals snp_table_hits on the host arrays + snp_table_query"""
    tabs = {k: t for k, t in sti.hit_tables().items() if len(t["pos"])}
    b = ctx.snp_builder()
    for cid, t in enumerate(tabs.values()):
        n = len(t["pos"])
        b.append_host(np.full(n, 100 + 3 * cid, np.uint32), np.arange(n, dtype=np.uint64), t["pos"], t["baf"])
    cols = b.finish([])
    assert cols.describe()["ascending"].all() and cols.describe()["contig_id"].tolist() == [100 + 3 * c for c in range(len(tabs))]
    total = 0
    for cid, (name, t) in enumerate(tabs.items()):
        gp, gb = cols.fetch(100 + 3 * cid)
        assert gp.tobytes() == t["pos"].tobytes() and gb.tobytes() == np.asarray(t["baf"], np.float64).tobytes(), name      # NaN payloads too
        got, ref = cols.table(100 + 3 * cid, t["af_pos"], t["af"]), ctx.snp_table_hits(t["pos"], t["baf"], t["af_pos"], t["af"])
        assert got.n == ref.n == len(t["pos"])
        total += _same_query(ctx, got, ref, t, cid)
        got.free()
        ref.free()
    assert total > 1000
    cols.free()


def test_tables_of_the_generated_text(ctx, generated):
    """the columns the device cut, with the population records of the reference parse: the table is the host arrays' table; the columns may
    be freed before the table is used"""
    cols, m, gn = generated
    for chrom in ("chr1", "chr2"):
        cid = m.ids[chrom.encode()]
        pos, baf, _ = m.columns()[cid]
        af = ctx.vcf_af_parse(gn[chrom], chrom, "AF_nfe=", pos)
        t = dict(pos=pos, baf=baf, af_pos=af["pos"], af=af["value"])
        got, ref = cols.table(cid, t["af_pos"], t["af"]), ctx.snp_table_hits(pos, baf, t["af_pos"], t["af"])
        assert _same_query(ctx, got, ref, t, 3) > 100
        got.free()
        ref.free()
    with pytest.raises(_lib.CsvError, match="af_pos is not ascending"):
        cols.table(0, [5, 4], [0.5, 0.5])
