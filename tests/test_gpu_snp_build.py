"""Resident SNP columns built on the device (csvgpu_snp_builder_* / csvgpu_snp_columns_*, kernels/snpbuild.hip) through Context: every
append's report (counts, the run table, the deferred offsets) and, behind finish, every contig's columns byte for byte and the describe
table, against the Python model of tests/snp_build_inputs.py (tests/test_snp_build_inputs.py runs that model alone on the CPU); the larger
case also against the host loader (host.SNPFile without a device option)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import snp_build_inputs as sb
import vcf_parse_inputs as inp
from contextsv_amd import _lib, host

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T = _lib.VCF_TILE_BYTES
RUN_KEYS = ("run_first", "run_line_off", "run_chrom_len")


def _check_report(got, e, text):
    assert not got["declined"] and got["status"] == 0, got
    assert (got["n_lines"], got["n_kept"], got["n_deferred"], got["n_runs"], got["first_run"]) == (e["n_lines"], e["n_kept"], e["n_deferred"], e["n_runs"],
                                                                                                   e["first_run"]), (got, e["n_runs"])
    for k in RUN_KEYS + ("defer_off",):
        assert got[k].dtype == np.uint32 and np.array_equal(got[k], e[k]), (k, got[k][:8], e[k][:8])


def _check_columns(cols, m):
    exp = m.columns()
    d = cols.describe()
    assert d["contig_id"].tolist() == sorted(exp), (d, sorted(exp))
    assert d["count"].tolist() == [len(exp[c][0]) for c in sorted(exp)]
    assert d["ascending"].tolist() == [exp[c][2] for c in sorted(exp)]
    for cid, (pos, baf, _) in exp.items():
        gp, gb = cols.fetch(cid)
        assert gp.tobytes() == pos.tobytes(), (cid, gp[:8], pos[:8])
        assert gb.tobytes() == baf.tobytes(), (cid, gb[:8], baf[:8])
    return exp


def _drive(ctx, batches, reserve=0, defer_to_host=True):
    """batches: (text, text_base) in the order of the calls -> (columns, model): every device append checked against the model, the
    deferred lines' records through append_host, the run names mapped to ids from the device's own run table"""
    m, b = sb.Model(), ctx.snp_builder(reserve)
    run_contig = []
    for text, base in batches:
        e = m.append(text, base)
        got = b.append(text, base)
        _check_report(got, e, text)
        run_contig += [m.id_of(text[o:o + n]) for o, n in zip(got["run_line_off"].tolist(), got["run_chrom_len"].tolist())]
        if defer_to_host and len(got["defer_off"]):
            b.append_host(*m.host_records(text, got["defer_off"], base))
    assert run_contig == m.run_contig
    cols = b.finish(run_contig)
    return cols, m


def _whole(ctx, text, **kw):
    cols, m = _drive(ctx, [(text, 0)], **kw)
    exp = _check_columns(cols, m)
    cols.free()
    return m, exp


# ---- CHROM names -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", range(len(sb.NAME_FAMILIES)), ids=[l for l, _ in sb.NAME_FAMILIES])
def test_chrom_names(ctx, family):
    """neighbouring names that differ in length only, in the last byte only, behind the 16th byte only; at the text's start and behind padding
    lines that move them over 16-byte pieces"""
    names = sb.NAME_FAMILIES[family][1]
    for pad in (0, 1, 50, 100):
        m, exp = _whole(ctx, sb.name_text(names, per=3, pad=pad))
        assert len(exp) == len(set(names)) and m.n_device == 3 * len(names)


@pytest.mark.parametrize("family", (4, 5), ids=("17 bytes", "40 bytes"))
def test_chrom_names_across_the_tile_edge(ctx, family):
    """the first name's bytes on both sides of the CSV_VCF_TILE_BYTES edge, at every split"""
    names = sb.NAME_FAMILIES[family][1]
    for text in sb.tile_edge_texts(names):
        m, exp = _whole(ctx, text)
        assert m.n_device == 2 * len(names)


# ---- run structure ---------------------------------------------------------------------------------------------------------------------
def test_every_record_its_own_run(ctx):
    text = sb.body([sb.good(10 + k, ("chr1", "chr2")[k & 1]) for k in range(301)])
    m, exp = _whole(ctx, text)
    assert len(m.run_contig) == 301 and [len(exp[c][0]) for c in (0, 1)] == [151, 150]


def test_one_run_in_all(ctx):
    m, exp = _whole(ctx, sb.body([sb.good(10 + k) for k in range(300)]))
    assert m.run_contig == [0] and len(exp[0][0]) == 300


def test_a_contig_that_returns(ctx):
    """chr1, chr2, chr1: two runs with one id, stitched in file order"""
    text = sb.body([sb.good(10), sb.good(11), sb.good(5, "chr2"), sb.good(12), sb.good(13)])
    m, exp = _whole(ctx, text)
    assert m.run_contig == [0, 1, 0] and exp[0][0].tolist() == [10, 11, 12, 13] and exp[0][2]


def test_a_contig_continued_in_the_next_append(ctx):
    a = sb.body([sb.good(10), sb.good(11, "chr2"), sb.good(12, "chr2")])
    b = sb.body([sb.good(13, "chr2"), sb.good(14, "chr3")])
    c = sb.body([sb.skipped(1, "chr9")])                          # a batch that keeps nothing: no run
    cols, m = _drive(ctx, [(a, 0), (c, len(a)), (b, len(a) + len(c))])
    exp = _check_columns(cols, m)
    cols.free()
    assert m.run_contig == [0, 1, 1, 2] and exp[1][0].tolist() == [11, 12, 13]


# ---- deferred lines --------------------------------------------------------------------------------------------------------------------
def test_deferred_lines(ctx):
    """first in the batch, last, between two kept records of one CHROM (no run break), naming another contig (no run break either: its
    record comes from the host under that contig's id), kept or not by the host parser; all through append_host at their file position"""
    text = sb.body([sb.deferred(3), sb.good(5), sb.deferred(6), sb.good(7), sb.deferred(8, "chr2"), sb.good(9), sb.deferred(1, ref="N"),
                    sb.good(10, "chr2"), sb.deferred(11, "chr2")])
    m, exp = _whole(ctx, text)
    assert m.run_contig == [0, 1] and m.n_host == 4
    assert exp[0][0].tolist() == [3, 5, 6, 7, 9] and exp[0][1].tolist() == [sb.DEFER_BAF, 0.75, sb.DEFER_BAF, 0.75, 0.75]
    assert exp[1][0].tolist() == [8, 10, 11] and exp[0][2] and exp[1][2]


def test_a_batch_of_deferred_lines_only(ctx):
    a = sb.body([sb.good(4)])
    b = sb.body([sb.deferred(5 + k, ("chr1", "chr7")[k & 1]) for k in range(40)])
    cols, m = _drive(ctx, [(a, 0), (b, len(a))])
    exp = _check_columns(cols, m)
    cols.free()
    assert m.run_contig == [0] and m.n_host == 40 and len(exp[0][0]) == 21 and len(exp[1][0]) == 20


def test_the_deliberate_deferred_lines_among_the_generated_text(ctx):
    text, _, _ = sb.generated()
    lines = text.split(b"\n")[:-1]
    for k, (_, l) in enumerate(inp.DELIBERATE_SNP):
        lines.insert(37 * (k + 1), l.encode())
    m, exp = _whole(ctx, sb.body(lines))
    assert m.n_host == len(inp.DELIBERATE_SNP) and m.n_device > 700 and m.n_device > m.n_host


# ---- append order and host batches ------------------------------------------------------------------------------------------------------
def test_batches_in_reverse_order_of_text_base(ctx):
    text, _, _ = sb.generated()
    cut = text.find(b"\n", len(text) // 3) + 1
    cut2 = text.find(b"\n", 2 * len(text) // 3) + 1
    parts = [(text[:cut], 0), (text[cut:cut2], cut), (text[cut2:], cut2)]
    cols, m = _drive(ctx, parts[::-1])
    exp = _check_columns(cols, m)
    cols.free()
    cols, m2 = _drive(ctx, parts)                                 # the same columns in file order of the calls (ids are dealt out differently)
    exp2 = _check_columns(cols, m2)
    cols.free()
    for name in (b"chr1", b"chr2"):
        assert exp[m.ids[name]][0].tobytes() == exp2[m2.ids[name]][0].tobytes() and exp[m.ids[name]][1].tobytes() == exp2[m2.ids[name]][1].tobytes()


def test_a_declined_batch_goes_through_the_host(ctx):
    """a '#' line behind data declines the batch: status says where, nothing is appended, the run count stays; append_host takes it"""
    a = sb.body([sb.good(4), sb.good(5, "chr2")])
    bad = sb.body([sb.good(6, "chr2"), b"#late header", sb.good(7), sb.deferred(8)])
    c = sb.body([sb.good(9)])
    m, b = sb.Model(), ctx.snp_builder()
    run_contig = []
    ea, ga = m.append(a), b.append(a)
    _check_report(ga, ea, a)
    run_contig += [m.id_of(n) for n in ea["run_names"]]
    got = b.append(bad, len(a))
    assert got["declined"] and got["reason"] == _lib.VCF_HEADER_LINE and got["offset"] == len(sb.good(6, "chr2")) + 1 and got["first_run"] == 2
    assert got["n_kept"] == 0 and got["n_runs"] == 0
    b.append_host(*m.host_batch(bad, len(a)))
    ec, gc = m.append(c, len(a) + len(bad)), b.append(c, len(a) + len(bad))
    _check_report(gc, ec, c)
    assert gc["first_run"] == 2                                   # the declined batch left no run
    run_contig += [m.id_of(n) for n in ec["run_names"]]
    cols = b.finish(run_contig)
    exp = _check_columns(cols, m)
    cols.free()
    assert exp[0][0].tolist() == [4, 7, 8, 9] and exp[1][0].tolist() == [5, 6]


# ---- boundaries --------------------------------------------------------------------------------------------------------------------------
def test_empty_text_and_empty_builder(ctx):
    b = ctx.snp_builder()
    got = b.append(b"")
    assert not got["declined"] and (got["n_lines"], got["n_kept"], got["n_deferred"], got["n_runs"], got["first_run"]) == (0, 0, 0, 0, 0)
    got = b.append(b"\n\n\r\n")
    assert (got["n_lines"], got["n_kept"], got["n_runs"]) == (0, 0, 0)
    cols = b.finish([])
    d = cols.describe()
    assert len(d["contig_id"]) == 0 and len(d["count"]) == 0
    with pytest.raises(_lib.CsvError, match="holds no record"):
        cols.fetch(0)
    cols.free()


def test_last_line_without_its_line_end_and_crlf(ctx):
    lines = [sb.good(5), sb.good(6, "chr2"), sb.deferred(7, "chr2"), sb.good(8, "chr2")]
    for text in (sb.body(lines, last=False), sb.body(lines, end=b"\r\n"), sb.body(lines, end=b"\r\n", last=False) + b"\r"):
        m, exp = _whole(ctx, text)
        assert exp[0][0].tolist() == [5] and exp[1][0].tolist() == [6, 7, 8]


def test_duplicate_positions_are_kept(ctx):
    text = sb.body([sb.good(5, ad="1,3"), sb.good(5, ad="3,1"), sb.good(5), sb.good(6), sb.good(6, ad="2,2")])
    m, exp = _whole(ctx, text)
    assert exp[0][0].tolist() == [5, 5, 5, 6, 6] and exp[0][1].tolist() == [0.75, 0.25, 0.75, 0.75, 0.5] and exp[0][2]


def test_a_contig_with_one_descending_position(ctx):
    """flagged, fetchable; columns_table and columns_af_parse refuse it with a message; the other contig's table is made"""
    text = sb.body([sb.good(5), sb.good(9), sb.good(8), sb.good(20), sb.good(3, "chr2"), sb.good(4, "chr2")])
    cols, m = _drive(ctx, [(text, 0)])
    exp = _check_columns(cols, m)
    assert not exp[0][2] and exp[1][2] and cols.describe()["ascending"].tolist() == [False, True]
    with pytest.raises(_lib.CsvError, match="snp_columns_table: positions are not ascending"):
        cols.table(0, [], [])
    with pytest.raises(_lib.CsvError, match="not ascending"):
        cols.af_parse(0, b"chr1\t5\t.\tA\tG\t.\tPASS\tAF=0.5\n", "chr1", "AF=")
    t = cols.table(1, [], [])
    assert t.n == 2
    t.free()
    cols.free()


# ---- capacity and memory -----------------------------------------------------------------------------------------------------------------
def _arrays(r, d, fill=0xA5A5A5A5):
    a = {k: np.full(r, fill, np.uint32) for k in RUN_KEYS}
    a["defer_off"] = np.full(d, fill, np.uint32)
    return a


def test_capacity_too_small(ctx):
    """cap_runs, cap_defer, both: CSV_ECAPACITY with the exact counts, nothing written, nothing appended; then the same call with exactly
    enough room, which writes nothing behind the counts"""
    head = sb.body([sb.good(2, "chr5")])
    text = sb.body([sb.good(5), sb.deferred(6), sb.good(7, "chr2"), sb.deferred(8), sb.good(9, "chr3"), sb.deferred(10)])
    m, b = sb.Model(), ctx.snp_builder()
    _check_report(b.append(head), m.append(head), head)
    e = m.append(text, len(head))
    assert (e["n_runs"], e["n_deferred"]) == (3, 3)
    for r, d in ((2, 3), (3, 2), (0, 0), (2, 8), (8, 2)):
        a = _arrays(r, d)
        rc, c = b.append_into(text, a, len(head))
        assert rc == _lib.CSV_ECAPACITY and "capacity" in ctx.last_error()
        assert (c["n_lines"], c["n_kept"], c["n_deferred"], c["n_runs"], c["first_run"]) == (6, 3, 3, 3, 1), c
        assert all((v == 0xA5A5A5A5).all() for v in a.values())
    a = _arrays(5, 5)
    rc, c = b.append_into(text, a, len(head))
    assert rc == 0 and c["first_run"] == 1                        # the refused calls appended no run
    for k in RUN_KEYS + ("defer_off",):
        assert np.array_equal(a[k][:3], e[k]) and (a[k][3:] == 0xA5A5A5A5).all(), k
    b.append_host(*m.host_records(text, a["defer_off"][:3], len(head)))
    cols = b.finish(m.run_contig)
    _check_columns(cols, m)                                       # ... and no record
    cols.free()


def test_growth_from_nothing_and_from_a_reserve(ctx):
    """reserve 0 through more than three growths of 1.5x (batches of 1, 1, 2, 4, ... records), and a reserve that is outgrown once"""
    for reserve in (0, 100):
        batches, base, p = [], 0, 10
        for n in (1, 1, 2, 4, 8, 16, 64, 300):
            text = sb.body([sb.good(p + k, ("chr1", "chr2")[(p + k) % 3 == 0]) for k in range(n)])
            batches.append((text, base))
            base += len(text)
            p += n
        cols, m = _drive(ctx, batches, reserve=reserve)
        exp = _check_columns(cols, m)
        cols.free()
        assert sum(len(v[0]) for v in exp.values()) == 396


_INJECT = r"""
import sys
sys.path[:0] = [{root!r}, {tests!r}]
import numpy as np
import contextsv_amd as cs
from contextsv_amd import _lib
import snp_build_inputs as sb
first = sb.body([sb.good(5), sb.good(6, "chr2")])
second = sb.body([sb.good(10 + k, ("chr2", "chr1")[k > 200]) for k in range(400)])
third = sb.body([sb.good(500 + k, ("chr3", "chr1")[k > 100]) for k in range(300)])
with cs.Context(0) as ctx:
    if not hasattr(ctx.lib, "csvgpu_test_fail_next_alloc"):
        raise SystemExit("no hook in this build")
    m, b = sb.Model(), ctx.snp_builder(0)
    m.append(first); b.append(first)
    out = dict(run_first=np.zeros(4, np.uint32), run_line_off=np.zeros(4, np.uint32), run_chrom_len=np.zeros(4, np.uint32), defer_off=np.zeros(4, np.uint32))
    # `second` outgrows the run scratch first, then the arrays; `third` (fewer records than `second`, so the scratch holds) the arrays alone.
    # Three times each: the failed attempt appends nothing and keeps the contents (the array whose growth failed, and those behind it, are not grown).
    for text, base in ((second, len(first)), (third, len(first) + len(second))):
        for _ in range(3):
            ctx.lib.csvgpu_test_fail_next_alloc(1)
            rc, c = b.append_into(text, out, base)
            assert rc == _lib.CSV_ENOMEM and "snp builder growth" in ctx.last_error(), (rc, ctx.last_error())
        ctx.lib.csvgpu_test_fail_next_alloc(0)
        rc, c = b.append_into(text, out, base)                   # the same append again
        e = m.append(text, base)
        assert rc == 0 and (c["n_kept"], c["n_runs"], c["first_run"]) == (e["n_kept"], 2, e["first_run"]), c
    cols = b.finish(m.run_contig)
    exp = m.columns()
    for cid, (pos, baf, _) in exp.items():
        gp, gb = cols.fetch(cid)
        assert gp.tobytes() == pos.tobytes() and gb.tobytes() == baf.tobytes(), cid
    assert cols.describe()["count"].tolist() == [len(exp[c][0]) for c in sorted(exp)]
    cols.free()
    # finish: its one allocation (the columns' block) fails -> NULL with a message, the builder consumed
    b = ctx.snp_builder(0)
    b.append(first)
    ctx.lib.csvgpu_test_fail_next_alloc(1)
    try:
        b.finish([0, 1])
        raise SystemExit("the injected allocation failure did not surface in finish")
    except cs.CsvError as e:
        assert "snp_builder_finish: hipMalloc failed" in str(e), str(e)
    ctx.lib.csvgpu_test_fail_next_alloc(0)
    assert b.h is None
print("ok")
"""


def test_failed_growth_in_the_testhooks_build():
    """csvgpu_test_fail_next_alloc(1) in front of an append that must grow (libcsvgpu_testhooks.so, in a child process): CSV_ENOMEM with the
    contents kept, three times where the run scratch is the first to grow and three times where the arrays are; then the same append
    succeeds; the columns are the model's. Then finish's own allocation fails: NULL with a message"""
    lib = os.path.join(ROOT, "contextsv_amd", "lib", "libcsvgpu_testhooks.so")
    if not os.path.exists(lib):
        pytest.skip("no test-hook build")
    env = dict(os.environ, CSVGPU_LIB=lib)
    r = subprocess.run([sys.executable, "-c", _INJECT.format(root=ROOT, tests=os.path.join(ROOT, "tests"))], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.startswith("ok"), (r.stdout[-2000:], r.stderr[-3000:])


# ---- errors --------------------------------------------------------------------------------------------------------------------------------
def test_refused_arguments(ctx):
    """every CSV_EINVAL of the appends, with a message and nothing written or appended"""
    lib, text = ctx.lib, np.frombuffer(sb.body([sb.good(5)]), np.uint8)
    b = ctx.snp_builder()
    a = _arrays(4, 4)
    o = _lib.csv_snp_runs()
    for k in a:
        setattr(o, k, a[k].ctypes.data)
    o.cap_runs = o.cap_defer = 4
    c = _lib.csv_snp_append_counts()
    c.n_kept = 77

    def call(fn=lib.csvgpu_snp_builder_append, bh=b.h, t=text.ctypes.data, n=len(text), base=0, out=C.byref(o), cnt=C.byref(c)):
        return fn(ctx.h, bh, t, n, base, 1, 1, out, cnt)
    for fn in (lib.csvgpu_snp_builder_append, lib.csvgpu_snp_builder_append_dev):
        for kw, msg in ((dict(bh=None), "null pointer"), (dict(out=None), "null pointer"), (dict(cnt=None), "null pointer"), (dict(t=None), "null pointer"),
                        (dict(n=1 << 32), "2^32 bytes"), (dict(base=(1 << 48) - len(text) + 1), "2^48"), (dict(base=1 << 63), "2^48")):
            assert call(fn, **kw) == _lib.CSV_EINVAL and msg in ctx.last_error(), (kw, ctx.last_error())
    o.run_line_off = None
    assert call() == _lib.CSV_EINVAL and "null pointer" in ctx.last_error()
    o.run_line_off, o.defer_off = a["run_line_off"].ctypes.data, None
    assert call() == _lib.CSV_EINVAL
    o.defer_off = a["defer_off"].ctypes.data
    assert c.n_kept == 77 and all((v == 0xA5A5A5A5).all() for v in a.values())
    assert call(base=(1 << 48) - len(text)) == 0 and c.n_kept == 1 and c.first_run == 0        # the largest base there is
    # append_host
    one = (np.array([3], np.uint32), np.array([9], np.uint64), np.array([5], np.uint32), np.array([0.5]))
    for k, v, msg in ((0, 1 << 16, "2^16"), (1, 1 << 48, "2^48")):
        args = [x.copy() for x in one]
        args[k] = np.array([1, v], args[k].dtype)
        for j in range(4):
            if j != k:
                args[j] = np.repeat(args[j], 2)
        assert b.append_host_raw(*args) == _lib.CSV_EINVAL and msg in ctx.last_error()
    for k in range(4):
        p = [x.ctypes.data for x in one]
        p[k] = None
        assert lib.csvgpu_snp_builder_append_host(ctx.h, b.h, 1, *p) == _lib.CSV_EINVAL and "null array" in ctx.last_error()
    assert lib.csvgpu_snp_builder_append_host(ctx.h, b.h, 0, None, None, None, None) == 0
    cols = b.finish([0])                                          # ... and only the one record of the accepted call is there
    assert cols.describe()["count"].tolist() == [1]
    with pytest.raises(_lib.CsvError, match="holds no record"):
        cols.fetch(1)
    with pytest.raises(_lib.CsvError, match="holds no record"):
        cols.table(1, [], [])
    cols.free()


def _two_runs(ctx):
    b = ctx.snp_builder()
    b.append(sb.body([sb.good(5), sb.good(6, "chr2")]))
    return b


def test_finish_refuses(ctx):
    """NULL with a message, the builder consumed each time: a wrong n_runs, an id at or above 2^16, two records of a contig with one key"""
    for run_contig, msg in (([0], "run count"), ([0, 1, 2], "run count"), ([0, 1 << 16], r"at or above 2\^16")):
        b = _two_runs(ctx)
        with pytest.raises(_lib.CsvError, match=msg):
            b.finish(run_contig)
        assert b.h is None
    b = _two_runs(ctx)
    b.append_host([1, 1], [700, 700], [1, 2], [0.5, 0.5])
    with pytest.raises(_lib.CsvError, match="share an order key"):
        b.finish([0, 1])
    b = _two_runs(ctx)                                            # the same key in two contigs is no clash; a host record on a device record's key is
    b.append_host([0, 1], [700, 700], [1, 2], [0.5, 0.5])
    cols = b.finish([0, 1])
    assert cols.describe()["count"].tolist() == [2, 2]
    cols.free()
    b = _two_runs(ctx)
    b.append_host([0], [0], [1], [0.5])
    with pytest.raises(_lib.CsvError, match="share an order key"):
        b.finish([0, 1])
    b = _two_runs(ctx)                                            # ids may leave gaps and need not follow the runs' order
    cols = b.finish([40000, 7])
    d = cols.describe()
    assert d["contig_id"].tolist() == [7, 40000] and cols.fetch(7)[0].tolist() == [6] and cols.fetch(40000)[0].tolist() == [5]
    cols.free()
    b = _two_runs(ctx)
    b.destroy()                                                   # a builder that is never finished
    assert b.h is None


# ---- the device-pointer form ----------------------------------------------------------------------------------------------------------------
def test_append_dev_at_every_alignment(ctx):
    """the text in device memory at 16 byte shifts (what csvgpu_bgzf_inflate_dev leaves): the same report and columns"""
    text = sb.name_text(sb.NAME_FAMILIES[4][1], per=2, pad=T - 30) + sb.body([sb.deferred(9)])
    data = np.frombuffer(text, np.uint8)
    dev = ctx.lib.csvgpu_dev_alloc(ctx.h, len(data) + 16)
    assert dev
    try:
        for shift in range(16):
            ctx._check(ctx.lib.csvgpu_upload(ctx.h, dev + shift, data.ctypes.data, len(data)))
            m, b = sb.Model(), ctx.snp_builder()
            e = m.append(text, 1000)
            a = _arrays(e["n_runs"], e["n_deferred"])
            rc, c = b.append_ptr_into(dev + shift, len(data), a, 1000)
            assert rc == 0 and (c["n_kept"], c["n_runs"], c["n_deferred"]) == (e["n_kept"], e["n_runs"], 1), (shift, c)
            for k in a:
                assert np.array_equal(a[k], e[k]), (shift, k)
            b.append_host(*m.host_records(text, a["defer_off"], 1000))
            cols = b.finish(m.run_contig)
            _check_columns(cols, m)
            cols.free()
    finally:
        ctx.lib.csvgpu_dev_free(ctx.h, dev)


# ---- larger -----------------------------------------------------------------------------------------------------------------------------------
def test_seventy_thousand_records_against_the_host_loader(ctx, tmp_path):
    """more records than one radix tile and than the builder's capped grids hold lanes, in three batches out of order; per contig the
    columns are what host.SNPFile (no device option) holds for the same text"""
    text = sb.big_text()
    cuts = [0, text.find(b"\n", len(text) // 2) + 1, text.find(b"\n", 3 * len(text) // 4) + 1, len(text)]
    parts = [(text[cuts[i]:cuts[i + 1]], cuts[i]) for i in (2, 0, 1)]
    cols, m = _drive(ctx, parts)
    exp = _check_columns(cols, m)
    assert m.n_device > 70_000 and m.n_host == 0 and len(m.run_contig) > 100
    path = str(tmp_path / "big.vcf")
    with open(path, "wb") as f:
        f.write(inp.HEADER.encode() + text)
    ref = host.SNPFile(path, threads=4)
    assert ref.records_kept == m.n_device
    for name, cid in m.ids.items():
        pos, baf, _, _ = ref.table(name.decode())
        gp, gb = cols.fetch(cid)
        assert gp.tobytes() == pos.tobytes() and gb.tobytes() == baf.tobytes(), name
    ref.close()
    cols.free()
