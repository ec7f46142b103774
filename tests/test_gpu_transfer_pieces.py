"""The pieced copies between pageable host memory and the device (Transfer, contextsv_amd/csrc/api/glue.hpp) at their piece boundaries,
through the entry points that use them: the two halves of the page-locked block taken in turn, the event wait from the third piece on,
the piece counter carried from one array to the next, and the runs of a download clipped where a piece ends. The device readers' own
tests use inputs of well under one piece."""
import os
import subprocess
import sys
import zlib

import numpy as np
import pytest

import fasta_dev
import fasta_inputs as fi
import inflate_inputs as zi
from contextsv_amd import Reads, _lib
from contextsv_amd._lib import ptr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = 4 << 20                      # kPiece of contextsv_amd/csrc/api/glue.hpp: bytes per copy through one half of the page-locked block
GUARD = 0xA5


@pytest.mark.parametrize("n", [1, P - 1, P, P + 1, 2 * P, 2 * P + 1, 3 * P + 5])
def test_upload_sizes(ctx, n):
    """csvgpu_upload of 1 byte up to 3 pieces + 5 bytes (from the third piece on a half is reused, behind a wait for its event) and
    csvgpu_download: the bytes come back as they went"""
    data = np.random.default_rng(n).integers(0, 256, n, dtype=np.uint8)
    back = np.full(n, 0x5A, np.uint8)
    dev = ctx.lib.csvgpu_dev_alloc(ctx.h, n)
    assert dev
    try:
        ctx._check(ctx.lib.csvgpu_upload(ctx.h, dev, ptr(data), n))
        ctx._check(ctx.lib.csvgpu_download(ctx.h, ptr(back), dev, n))
    finally:
        ctx.lib.csvgpu_dev_free(ctx.h, dev)
    assert np.array_equal(back, data)


def test_counter_carried_across_arrays(ctx):
    """One append_host batch whose ten arrays have odd sizes on both sides of a piece (flag, mapq under one; the CIGAR words three), so
    that an array starts on whichever half the one before it left off; fetch_reads / fetch_names (whole-range downloads of the same sizes)
    give the input back"""
    rng = np.random.default_rng(41)
    n = 300_001
    ops = rng.integers(1, 15, n)
    cigar_off = np.zeros(n + 1, np.uint64)
    cigar_off[1:] = np.cumsum(ops, dtype=np.uint64)
    m = int(cigar_off[-1])
    cigar = (rng.integers(1, 60, m).astype(np.uint32) << 4) | rng.choice([0, 1, 2, 4], m).astype(np.uint32)
    pos = np.sort(rng.integers(0, 1_000_000, n)).astype(np.int32)            # sorted: finish has nothing unusual to do
    flag, mapq = rng.integers(0, 1 << 12, n).astype(np.uint16), rng.integers(0, 61, n).astype(np.uint8)
    seq_off, name_off = np.zeros(n + 1, np.uint64), np.zeros(n + 1, np.uint64)
    seq_off[1:] = np.cumsum(rng.integers(0, 40, n), dtype=np.uint64)
    name_off[1:] = np.cumsum(rng.integers(10, 25, n), dtype=np.uint64)
    seq = rng.integers(0, 256, int(seq_off[-1]), dtype=np.uint8)
    name = rng.integers(33, 127, int(name_off[-1]), dtype=np.uint8)
    name_hash = rng.integers(0, 1 << 63, n).astype(np.uint64)
    assert 2 * P < cigar.nbytes < 3 * P and cigar.nbytes % P and flag.nbytes < P and mapq.nbytes < P and seq.nbytes > P and name.nbytes > P
    b = ctx.shard_builder(_lib.SB_SEQ | _lib.SB_NAMES | _lib.SB_NAME_HASH)
    try:
        b.append_host(Reads(pos, flag, mapq, cigar_off, cigar), seq_off, seq, name_off, name, name_hash)
        assert b.sizes() == dict(n_reads=n, n_cigar=m, n_seq=len(seq), n_name=len(name))
        sh = b.finish(1_100_000)
    finally:
        b.destroy()
    try:
        back, names = sh.fetch_reads(), sh.fetch_names()
    finally:
        sh.free()
    for f, want in (("pos", pos), ("flag", flag), ("mapq", mapq), ("cigar_off", cigar_off), ("cigar", cigar)):
        assert np.array_equal(getattr(back, f), want), f
    assert np.array_equal(names["name_off"], name_off) and np.array_equal(names["name"], name) and np.array_equal(names["name_hash"], name_hash)


def _member_data(rng, n):
    kind = int(rng.integers(0, 3))
    if kind == 0:
        return bytes(rng.integers(0, 256, n, dtype=np.uint8))               # incompressible: stored blocks
    if kind == 1:
        return bytes(rng.integers(0, 4, n, dtype=np.uint8))                 # short codes
    unit = bytes(rng.integers(0, 256, 37, dtype=np.uint8))
    return (unit * (n // 37 + 1))[:n]                                       # matches


def _members_between(cuts, biggest=65_000):
    """[start, end) ranges that tile [cuts[0], cuts[-1]), none longer than `biggest`, one of them ending and the next starting at every cut"""
    out = []
    for a, b in zip(cuts, cuts[1:]):
        while a < b:
            e = min(a + biggest, b)
            out.append([a, e])
            a = e
    return out


def _inflate_layout(ctx, ranges, bad=()):
    """Members at the given [start, end) offsets, counted from the first member's out_off, through the host form of csvgpu_bgzf_inflate;
    those listed in `bad` carry a wrong CRC. Every decoded member is zlib's bytes; every other byte of `out` is still the guard."""
    rng = np.random.default_rng(len(ranges))
    lead_in, lead_out = 11, 7
    comp, blocks, want = bytearray(b"\x5a" * lead_in), np.zeros(len(ranges), zi.BLOCK_DTYPE), []
    for i, (a, e) in enumerate(ranges):
        data = _member_data(rng, e - a)
        c = zi.deflate(data, 1)
        assert len(c) <= 65_536 and zlib.decompress(c, -15) == data
        blocks[i] = (len(comp), lead_out + a, len(c), len(data), zi.crc(data) ^ (1 if i in bad else 0), 0)
        comp += c + b"\x5a" * (i % 3)
        want.append(data)
    out = np.full(lead_out + ranges[-1][1] + 64, GUARD, np.uint8)
    rc, status = ctx.bgzf_inflate(np.frombuffer(bytes(comp), np.uint8), blocks, out)
    expect = np.full(len(out), GUARD, np.uint8)
    for i, (a, e) in enumerate(ranges):
        if i not in bad:
            expect[lead_out + a: lead_out + e] = np.frombuffer(want[i], np.uint8)
    assert rc == len(bad) and np.array_equal(status, np.array([1 if i in bad else 0 for i in range(len(ranges))], np.uint8))
    wrong = np.flatnonzero(out != expect)
    assert not len(wrong), (int(wrong[0]) - lead_out, len(wrong))


def test_runs_against_piece_boundaries(ctx):
    """The host form of csvgpu_bgzf_inflate copies back only the decoded members' ranges, adjacent ones as one run, piece by piece.
    Members that end and start at P - 1, P and P + 1 with nothing between them (two of them one byte long); a member that ends at
    2P - 1 before one guard byte, a one-byte member [2P, 2P + 1) before two guard bytes; elsewhere every fifth member three bytes short of
    its neighbour: runs that end, start and pass through the end of a piece."""
    cuts = [0, P - 1, P, P + 1, 2 * P, 2 * P + 3, 2 * P + 200_001]
    ranges = _members_between(cuts)
    for i, r in enumerate(ranges):
        if r[1] == 2 * P:
            r[1] -= 1                                                       # [.., 2P - 1), a guard byte, [2P, ..
        elif r[1] == 2 * P + 3:
            r[1] -= 2                                                       # [2P, 2P + 1), two guard bytes, [2P + 3, ..
        elif i % 5 == 0 and r[1] - r[0] > 100 and r[1] not in cuts:
            r[1] -= 3
    ends, starts = {r[1] for r in ranges}, {r[0] for r in ranges}
    assert {P - 1, P, P + 1, 2 * P - 1, 2 * P + 1} <= ends and {P - 1, P, P + 1, 2 * P} <= starts
    _inflate_layout(ctx, ranges)


def test_declined_member_across_a_piece_boundary(ctx):
    """One member with a wrong CRC whose range lies on both sides of P, its neighbours adjacent to it: status 1 for it alone, the call
    returns 1, and its whole range keeps the caller's bytes, in the piece before P and in the one behind"""
    ranges = _members_between([0, 2 * P + 12_345])
    for i, r in enumerate(ranges):
        if i % 7 == 3 and not r[0] < P < r[1]:
            r[1] -= 2
    bad = [i for i, r in enumerate(ranges) if r[0] < P < r[1]]
    assert len(bad) == 1 and ranges[bad[0]][1] == ranges[bad[0] + 1][0] and ranges[bad[0] - 1][1] == ranges[bad[0]][0]
    _inflate_layout(ctx, ranges, bad=set(bad))


def test_vcf_host_form_against_device_form_beyond_two_pieces():
    """A VCF text of more than two pieces through csvgpu_vcf_snp_parse (text up in three pieces, arrays back through the block) and
    through csvgpu_vcf_snp_parse_dev: equal counts and arrays, every generated line counted. In a process of its own, torch first
    (tests/transfer_pieces_dev_check.py)."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "transfer_pieces_dev_check.py")], capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0 and "transfer_pieces_dev ok" in r.stdout, (r.stdout[-2000:], r.stderr[-3000:])


def test_fasta_text_beyond_two_pieces(ctx):
    """A FASTA text of more than two pieces, 60-column lines, three records, appended as one piece: the genome is the Python statement's"""
    lengths = (5_000_001, 3_000_017, 600_003)
    text = fi.wrapped_text(np.random.default_rng(5), (("chr1", lengths[0]), ("chr2 extra words", lengths[1]), ("chrM", lengths[2])), width=60)
    assert len(text) > 2 * P
    exp = fasta_dev.check_text(ctx, text)
    assert [n for n, _ in exp] == [b"chr1", b"chr2", b"chrM"] and tuple(len(s) for _, s in exp) == lengths
