"""BGZF members inflated on the device (csvgpu_bgzf_inflate / _dev, kernels/inflate.hip): exact against zlib on every block kind, on the
corners zlib never writes (tests/inflate_inputs.py builds them, and tests/test_inflate_core.py has run the same inputs through the decode
core on the CPU under the sanitizers), with guard bytes around every output range; a wrong size or CRC and damaged streams are declined,
never trusted; and through the reader and the run the option changes nothing but where the bytes are decoded.

Every test packs its members into one or a few calls. The 65 535-byte member of the CRC lengths is one stored block of 60 000 bytes and a
fixed block of 5 535: a single stored block of that length is 65 540 bytes of input, above the 65 536 a member (and the entry point)
allows."""
import os
import subprocess
import sys
import zlib

import numpy as np
import pytest

import inflate_inputs as inp

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_passed = set()            # the exactness tests that passed in this session: the damaged streams run only behind them


def _run(ctx, cases, out_lens=None, crcs=None):
    comp, blocks, out = inp.layout(cases, out_lens, crcs)
    n_declined, status = ctx.bgzf_inflate(comp, blocks, out)
    return n_declined, status, out, blocks


def _bytes_of(out, b):
    return out[int(b["out_off"]): int(b["out_off"]) + int(b["out_len"])].tobytes()


def _assert_exact(ctx, cases):
    n_declined, status, out, blocks = _run(ctx, cases)
    bad = [cases[i].name for i in np.flatnonzero(status)]
    assert n_declined == 0 and not bad, bad[:10]
    wrong = [c.name for c, b in zip(cases, blocks) if _bytes_of(out, b) != c.data]
    assert not wrong, wrong[:10]
    assert inp.guards_intact(out, blocks), "bytes outside the members' output ranges were written"


@pytest.fixture(scope="module")
def zlib_cases():
    return inp.zlib_cases()


def test_every_block_kind(ctx, zlib_cases):
    """(a) nine lengths x six content kinds x five levels x five strategies, as 1350 members of one call: none declined"""
    assert len(zlib_cases) == 54 * 25
    _assert_exact(ctx, zlib_cases)
    _passed.add("a")


def test_every_block_kind_on_device_tensors():
    """(a) the same members through csvgpu_bgzf_inflate_dev with torch tensors: compressed bytes, decoded bytes and status stay on the
    device. In a process of its own, torch first (tests/bgzf_inflate_dev_check.py)."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "bgzf_inflate_dev_check.py")], capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0 and "inflate_dev ok: 1350 members" in r.stdout, (r.stdout[-2000:], r.stderr[-3000:])
    _passed.add("a_dev")


def test_edges(ctx):
    """(b) 1-3, 5-10: several DEFLATE blocks per member, the longest match at the longest distance ending at out_len, length-3 matches,
    15-bit codes, one distance code, none, the EOF member, 65 536 bytes out; every offset odd (inflate_inputs.layout)"""
    cases = inp.edge_cases()
    comp, blocks, out = inp.layout(cases)
    assert (blocks["in_off"] % 2 == 1).sum() > len(cases) // 3 and (blocks["out_off"] % 4 != 0).sum() > len(cases) // 2
    assert any(b["in_len"] == 2 and b["out_len"] == 0 for b in blocks) and (blocks["out_len"] == 65536).any()
    _assert_exact(ctx, cases)
    _passed.add("b_edges")


def test_overlapping_copies(ctx):
    """(b) 4: every distance 1..70 with lengths 3, 64, 65, 258: either side of the wave width, and dist < len"""
    cases = inp.overlap_cases()
    assert len(cases) == 280
    _assert_exact(ctx, cases)
    _passed.add("b_overlap")


def test_more_members_than_the_grid(ctx):
    """(b) 11: 5000 small members in one call"""
    _assert_exact(ctx, inp.small_cases(5000))
    _passed.add("b_small")


def test_crc_of_every_length(ctx):
    """(b) 12, 13: the device's CRC-32 at every length 0..300, 511/512/513/4095/4096/65535 against zlib.crc32 — right: status 0; any other
    value in the field: status 1"""
    cases = inp.crc_cases()
    assert [len(c.data) for c in cases] == inp.CRC_LENGTHS
    _assert_exact(ctx, cases)                                                      # the field is zlib.crc32 of the data
    wrong = [(zlib.crc32(c.data) ^ (1 << (i % 32))) & 0xFFFFFFFF for i, c in enumerate(cases)]
    n_declined, status, out, blocks = _run(ctx, cases, crcs=wrong)
    assert n_declined == len(cases) and (status == 1).all()
    assert inp.guards_intact(out, blocks)
    _passed.add("b_crc")


def test_announced_size_off_by_one(ctx, zlib_cases):
    """(c) out_len one less and one more than the truth: declined, guards intact (the CRC field is the true data's: a decoder that
    truncated or padded would have to get past it, too)"""
    cases = [c for c in zlib_cases + inp.edge_cases() if len(c.data) <= 20_000]
    assert len(cases) > 1000
    for d in (-1, 1):
        sel = [c for c in cases if len(c.data) + d >= 0]
        n_declined, status, out, blocks = _run(ctx, sel, out_lens=[len(c.data) + d for c in sel])
        assert n_declined == len(sel) and (status == 1).all(), [sel[i].name for i in np.flatnonzero(status == 0)][:10]
        assert inp.guards_intact(out, blocks)
    _passed.add("c")


def test_damaged_streams_are_declined(ctx):
    """(d) the damaged and truncated streams the CPU check ran, each between intact neighbours, in one call: the call returns, a damaged
    member is declined or decodes to the original, the neighbours are right, the guards intact. Checks the decline path; runs only after
    the exactness tests of this session passed."""
    need = {"a", "a_dev", "b_edges", "b_overlap", "b_small", "b_crc", "c"}
    assert need <= _passed, "the exactness tests did not all pass in this session: %s missing" % sorted(need - _passed)
    damaged = inp.damaged_cases(300)
    good = [c for c in inp.edge_cases() if len(c.data) < 5000]
    cases, is_damaged = [], []
    for i, c in enumerate(damaged):
        cases += [good[i % len(good)], c]
        is_damaged += [False, True]
    cases.append(good[0]); is_damaged.append(False)
    n_declined, status, out, blocks = _run(ctx, cases)
    is_damaged = np.array(is_damaged)
    assert set(np.unique(status)) <= {0, 1} and n_declined == int(status.sum())
    assert not status[~is_damaged].any()
    for c, b, s in zip(cases, blocks, status):
        if s == 0:
            assert _bytes_of(out, b) == c.data, c.name
    assert status[is_damaged].sum() > 250
    assert inp.guards_intact(out, blocks)


def test_arguments(ctx):
    """(g) every CSV_EINVAL of the entry points, and n_blocks == 0"""
    from contextsv_amd import CsvError, _lib
    c = inp.edge_cases()[0]
    comp, blocks, out = inp.layout([c, c])
    lib, h = ctx.lib, ctx.h
    status = np.zeros(2, np.uint8)
    args = lambda **kw: [kw.get("comp", comp.ctypes.data), kw.get("comp_len", len(comp)), kw.get("blocks", blocks.ctypes.data), kw.get("n", 2),
                         kw.get("out", out.ctypes.data), kw.get("out_len", len(out)), kw.get("status", status.ctypes.data)]
    for fn in (lib.csvgpu_bgzf_inflate, lib.csvgpu_bgzf_inflate_dev):
        assert fn(None, *args()) == _lib.CSV_EINVAL
        for null in ("comp", "blocks", "out", "status"):
            assert fn(h, *args(**{null: None})) == _lib.CSV_EINVAL, null
        assert fn(h, *args(n=0)) == 0 and fn(h, None, 0, None, 0, None, 0, None) == 0
        for field, value in (("in_len", 65537), ("out_len", 65537), ("in_off", len(comp) - 1), ("out_off", len(out) - 1), ("in_off", 1 << 62), ("out_off", 1 << 62)):
            b2 = blocks.copy()
            b2[1][field] = value
            assert fn(h, *args(blocks=b2.ctypes.data)) == _lib.CSV_EINVAL, (field, value)
        assert fn(h, *args(comp_len=int(blocks[1]["in_off"]) + int(blocks[1]["in_len"]) - 1)) == _lib.CSV_EINVAL
        assert fn(h, *args(out_len=int(blocks[1]["out_off"]) + int(blocks[1]["out_len"]) - 1)) == _lib.CSV_EINVAL
        b2 = blocks.copy()
        b2[1]["out_off"] = int(blocks[0]["out_off"]) + int(blocks[0]["out_len"]) - 1         # overlaps member 0's range
        assert fn(h, *args(blocks=b2.ctypes.data)) == _lib.CSV_EINVAL
        assert fn(h, *args(blocks=blocks[::-1].copy().ctypes.data)) == _lib.CSV_EINVAL       # out_off decreases
        assert b"bgzf_inflate" in lib.csvgpu_last_error(h)
    assert (out == inp.GUARD).all()
    with pytest.raises(CsvError):
        b2 = blocks.copy()
        b2[0]["in_len"] = 70000
        ctx.bgzf_inflate(comp, b2, out)
    n_declined, st = ctx.bgzf_inflate(comp, blocks, out)                                   # and the same arguments, unspoilt, decode
    assert n_declined == 0 and not st.any() and _bytes_of(out, blocks[1]) == c.data


# ---- (e), (f): through the reader and the run --------------------------------------------------------------------------------------------
def _three_contigs():
    """the three contigs of tests/test_gpu_bam.py as one record set, with one CIGAR of more than 65 535 operations (it travels in a CG tag)"""
    from contextsv_amd import Reads
    from test_gpu_e2e import CONTIG_LEN, _build
    contigs = _build(7)
    cat = lambda f, dt: np.ascontiguousarray(np.concatenate([getattr(c["reads"], f) for c in contigs]), dt)
    base = np.concatenate([[0], np.cumsum([c["reads"].n_cigar for c in contigs])]).astype(np.uint64)
    coff = np.concatenate([c["reads"].cigar_off[:-1] + base[i] for i, c in enumerate(contigs)] + [base[-1:]]).astype(np.uint64)
    reads = Reads(cat("pos", np.int32), cat("flag", np.uint16), cat("mapq", np.uint8), coff, cat("cigar", np.uint32))
    tid = np.concatenate([np.full(c["reads"].n_reads, t, np.int32) for t, c in enumerate(contigs)])
    qnames = ["r%d" % q for c in contigs for q in c["qname_id"]]
    return contigs, reads, tid, qnames, CONTIG_LEN


def _with_long_cigar(reads, tid, qnames):
    """one more record in front of contig 0: 70 001 operations"""
    from contextsv_amd import Reads
    long_cigar = np.array([((1 + (j % 3)) << 4) | (0 if j % 2 == 0 else (1 if j % 4 == 1 else 2)) for j in range(70_001)], np.uint32)
    r = Reads(np.concatenate([[0], reads.pos]), np.concatenate([[0], reads.flag]), np.concatenate([[60], reads.mapq]),
              np.concatenate([[0], reads.cigar_off + np.uint64(len(long_cigar))]).astype(np.uint64), np.concatenate([long_cigar, reads.cigar]))
    return r, np.concatenate([[0], tid]).astype(np.int32), ["long0"] + qnames


def _same_shard(a, b):
    assert (a["tid"], a["name"], a["target_len"]) == (b["tid"], b["name"], b["target_len"])
    for f in ("pos", "flag", "mapq", "cigar_off", "cigar"):
        assert np.array_equal(getattr(a["reads"], f), getattr(b["reads"], f)), f
    assert np.array_equal(a["seq_off"], b["seq_off"]) and np.array_equal(a["seq"], b["seq"]) and a["qnames"] == b["qnames"]


@pytest.mark.parametrize("level", [0, 1, 6])
def test_reader_with_device_inflate_equals_host_route(tmp_path, level):
    """(e) read_contig and read_all with inflate_on_device: array for array what the host route reads, at window_blocks 1, 2 and default
    (records straddle blocks and batches: a record of 280 KiB lies in the file), with a CG-tag CIGAR"""
    from contextsv_amd import host
    _, reads, tid, qnames, contig_len = _three_contigs()
    reads, tid, qnames = _with_long_cigar(reads, tid, qnames)
    rng = np.random.default_rng(level)
    l_seq = rng.integers(0, 30, reads.n_reads).astype(np.int32)
    seq_off = np.concatenate([[0], np.cumsum((l_seq + 1) // 2)]).astype(np.uint64)
    seq = rng.integers(0, 256, int(seq_off[-1]), dtype=np.uint8)
    seq[seq_off[1:][l_seq % 2 == 1] - 1] &= 0xF0
    names = ["contig%d" % t for t in range(3)]
    path = str(tmp_path / "reads.bam")
    host.write_bam(path, names, [contig_len] * 3, tid, reads, qnames, seq_off, seq, l_seq, level=level, threads=8)
    bam = host.BamFile(path)
    want_all, want_unplaced = bam.read_all(want_seq=True, want_qnames=True, threads=8)
    want_all = [dict(s, reads=_copy_reads(s["reads"]), seq_off=s["seq_off"].copy(), seq=s["seq"].copy()) for s in want_all]
    assert len(want_all) == 3 and max(np.diff(want_all[0]["reads"].cigar_off)) > 65535
    for window in (1, 2, 0):
        got_all, got_unplaced = bam.read_all(want_seq=True, want_qnames=True, threads=8, window_blocks=window, inflate_on_device=True)
        assert got_unplaced == want_unplaced and len(got_all) == 3
        for g, w in zip(got_all, want_all):
            _same_shard(g, w)
        for t in (2, 0):
            _same_shard(bam.read_contig(names[t], want_seq=True, want_qnames=True, threads=8, window_blocks=window, inflate_on_device=True), want_all[t])
    # and back on the host with the same handle
    _same_shard(bam.read_contig(names[1], want_seq=True, want_qnames=True), want_all[1])
    bam.close()


def _copy_reads(r):
    from contextsv_amd import Reads
    return Reads(r.pos.copy(), r.flag.copy(), r.mapq.copy(), r.cigar_off.copy(), r.cigar.copy())


def test_reader_with_device_inflate_fails_like_the_host_route(tmp_path):
    """(e) one flipped byte inside a block: the same message either way; plain gzip and a cut file fail as before"""
    import gzip
    from contextsv_amd import host
    _, reads, tid, qnames, contig_len = _three_contigs()
    path = str(tmp_path / "reads.bam")
    host.write_bam(path, ["contig%d" % t for t in range(3)], [contig_len] * 3, tid, reads, qnames, level=6, threads=8)
    raw = open(path, "rb").read()

    def message(p, **kw):
        with pytest.raises(RuntimeError) as ei:
            host.BamFile(p, load_index=False).read_all(threads=4, **kw)
        return str(ei.value)

    for k, at in enumerate((len(raw) // 2, len(raw) // 3 + 17, len(raw) - 5000)):
        bad = bytearray(raw)
        bad[at] ^= 0x5A
        p = str(tmp_path / ("flip%d.bam" % k))
        open(p, "wb").write(bytes(bad))
        on_host = message(p)
        assert "BGZF" in on_host or "BAM" in on_host
        assert message(p, inflate_on_device=True) == on_host
    p = str(tmp_path / "cut.bam")
    open(p, "wb").write(raw[: len(raw) // 2])
    assert message(p, inflate_on_device=True) == message(p) and "truncated" in message(p)
    p = str(tmp_path / "plain.bam")
    with gzip.open(p, "wb") as f:
        f.write(b"BAM\1" + b"\0" * 100)
    with pytest.raises(RuntimeError, match="BGZF"):
        host.BamFile(p, load_index=False)


def test_run_from_bam_with_device_inflate_gives_the_same_calls(ctx, tmp_path):
    """(f) runBam with the option off and on, and on beside the other opt-in device forms: identical calls and per-contig statistics"""
    from contextsv_amd import host, make_hmm
    from hmm_params import WGS_HMM
    contigs, reads, tid, qnames, contig_len = _three_contigs()
    path = str(tmp_path / "reads.bam")
    host.write_bam(path, ["contig%d" % t for t in range(3)], [contig_len] * 3, tid, reads, qnames, level=1, threads=8)
    hmm = make_hmm(**WGS_HMM)
    want, want_tid, st = host.run_bam(ctx, path, hmm, threads=8)
    assert len(want) > 20 and st["n_contigs"] == 3
    got, got_tid, st_on = host.run_bam(ctx, path, hmm, threads=8, inflate_on_device=True)
    stats = lambda s: {k: s[k] for k in ("n_contigs", "n_reads", "n_cigar", "bam_bytes")}
    assert got.tobytes() == want.tobytes() and np.array_equal(got_tid, want_tid) and stats(st_on) == stats(st)
    got, got_tid, st_all = host.run_bam(ctx, path, hmm, threads=8, inflate_on_device=True, split_groups_on_device=True, split_fits_on_device=True,
                                        split_tables_on_device=True, cn_observations_on_device=True)
    assert got.tobytes() == want.tobytes() and np.array_equal(got_tid, want_tid) and stats(st_all) == stats(st)
