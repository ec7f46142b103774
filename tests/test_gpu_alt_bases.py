"""The 50-base ALT strings cut on the device from a built shard's packed sequences (csvgpu_alt_bases_resident, kernels/shardbuild.hip)
against a Python statement of the host rule (SVCaller::toSVCall's base loop; the code table and the ambiguity set of
tests/test_alt_sequence.py). tests/test_alt_bases_core.py has held the kernel's per-base header against the host loop itself under the
sanitizers; here the kernel runs: every length around the wave width, both nibble positions, sequences that start at odd addresses, the
byte bound with its pad nibble, items beyond one grid, and the refusals."""
import numpy as np
import pytest

import bam_py
from contextsv_amd import CsvError, Reads, _lib, host
from test_alt_sequence import AMBIG, NT16, pack
from test_gpu_alt_sequence import CASES, M, I, S

pytestmark = pytest.mark.gpu

CLEAN = "".join("N" if c in AMBIG else c for c in NT16)


def py_alt(seq: bytes, qpos: int, n: int) -> str:
    """the host rule on one record's packed sequence"""
    if (qpos + n + 1) // 2 > len(seq):
        return "N" * n
    return "".join(CLEAN[(seq[q >> 1] >> (0 if q & 1 else 4)) & 15] for q in range(qpos, qpos + n))


def build(ctx, seqs, depth_len=1000, want=_lib.SB_SEQ, batches=1):
    """a shard built on the device from one record per (packed sequence, l_seq) -> Shard"""
    recs = [bam_py.encode_record(0, 10 + k, 60, 0, b"r%d" % k, [(max(l, 1) << 4) | 0], bytes(s), l) for k, (s, l) in enumerate(seqs)]
    b = ctx.shard_builder(want)
    per = (len(recs) + batches - 1) // batches
    for a in range(0, len(recs), per):
        rc, _ = b.append_bam(b"".join(recs[a:a + per]), [0])
        assert rc == 0
    return b.finish(depth_len)


def check(ctx, sh, seqs, items):
    read, qpos, lens = (np.array([it[k] for it in items], np.int64) for k in range(3))
    got = ctx.alt_bases(sh, read, qpos, lens)
    for (r, q, n), g in zip(items, got):
        assert g == py_alt(bytes(seqs[r][0]), q, n), (r, q, n, g)


@pytest.fixture(scope="module")
def three(ctx):
    """three records: 600 bases of every code, an odd l_seq with a non-zero pad nibble behind an odd number of bytes, no sequence; then one
    of even length — the second and the fourth start at odd addresses"""
    rng = np.random.default_rng(5)
    a = np.array([(h << 4) | l for h in range(16) for l in range(16)] * 2, np.uint8)[:301]          # 602 bases -> l_seq 601: 301 bytes (odd)
    b = rng.integers(0, 256, 101, dtype=np.uint8)
    b[-1] = (b[-1] & 0xF0) | 0x8                                                                      # l_seq 201: the pad nibble holds T
    c = np.zeros(0, np.uint8)
    d = rng.integers(0, 256, 100, dtype=np.uint8)                                                     # l_seq 200
    seqs = [(a, 601), (b, 201), (c, 0), (d, 200)]
    sh = build(ctx, seqs, batches=2)
    assert sh.sizes()["n_seq"] == 301 + 101 + 100
    yield sh, seqs
    sh.free()


def test_lengths_offsets_and_codes(ctx, three):
    sh, seqs = three
    items = [(r, q, n) for r in (0, 1, 3) for q in (0, 1, 2, 7, 64, 65) for n in (1, 49, 50, 51, 64, 65, 200)]
    check(ctx, sh, seqs, items)
    # all sixteen codes at both nibble positions: 512 consecutive bases of the first record hold every byte value once
    got = ctx.alt_bases(sh, [0, 0], [0, 1], [512, 511])
    assert got[0] == py_alt(bytes(seqs[0][0]), 0, 512) and got[1] == got[0][1:]
    assert {got[0][2 * k] for k in range(256)} == set(CLEAN) and {got[0][2 * k + 1] for k in range(256)} == set(CLEAN)
    assert got[0][:32] == "".join("=" + c for c in CLEAN)                              # bytes 0x00 .. 0x0f: '=' and each code in turn


def test_the_byte_bound(ctx, three):
    sh, seqs = three
    for n in (1, 50, 200):
        # l_seq odd (201): up to l_seq inside; l_seq + 1 reads the pad nibble (the bound is on bytes); l_seq + 2 is outside
        items = [(1, 201 - n, n), (1, 202 - n, n), (1, 203 - n, n)]
        got = ctx.alt_bases(sh, *zip(*items))
        check(ctx, sh, seqs, items)
        assert got[1][-1] == "T" and got[2] == "N" * n
        # l_seq even (200): l_seq inside, l_seq + 1 outside
        items = [(3, 200 - n, n), (3, 201 - n, n)]
        got = ctx.alt_bases(sh, *zip(*items))
        check(ctx, sh, seqs, items)
        assert got[1] == "N" * n and got[0] == py_alt(bytes(seqs[3][0]), 200 - n, n)
    # no stored sequence: N whatever is asked; a query offset of 2^30 does not wrap
    assert ctx.alt_bases(sh, [2, 2, 0, 1], [0, 5, 1 << 30, (1 << 32) - 1], [50, 1, 50, 50]) == ["N" * 50, "N", "N" * 50, "N" * 50]


def test_interleaved_empty_and_many_items(ctx, three):
    sh, seqs = three
    items = [(0, 3, 50), (3, 4, 50), (1, 5, 0), (0, 6, 7), (2, 0, 0), (1, 100, 50), (3, 150, 51), (0, 0, 0), (1, 0, 64)]
    check(ctx, sh, seqs, items)
    assert ctx.alt_bases(sh, [], [], []) == [] and ctx.alt_bases(sh, [1, 3], [0, 0], [0, 0]) == ["", ""]
    # 70 000 items over the three records that hold bases: more waves than one grid has; guard bytes on both sides of `out`
    rng = np.random.default_rng(8)
    n = 70_000
    read = rng.choice([0, 1, 3], n).astype(np.uint32)
    qpos = rng.integers(0, 220, n).astype(np.uint32)
    lens = rng.integers(0, 12, n).astype(np.uint64)
    lens[::1000] = 50
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    G = 256
    buf = np.full(int(off[-1]) + 2 * G, 0xA5, np.uint8)
    ctx._check(ctx.lib.csvgpu_alt_bases_resident(ctx.h, sh.h, read.ctypes.data, qpos.ctypes.data, off.ctypes.data, n, buf[G:].ctypes.data))
    assert (buf[:G] == 0xA5).all() and (buf[-G:] == 0xA5).all()
    text = buf[G:-G].tobytes().decode("latin-1")
    want = "".join(py_alt(bytes(seqs[r][0]), int(q), int(k)) for r, q, k in zip(read, qpos, lens))
    assert text == want
    # offsets that do not start at 0: only [out_off[0], out_off[n]) is written
    buf[:] = 0xA5
    off2 = off[:101] + np.uint64(7)
    ctx._check(ctx.lib.csvgpu_alt_bases_resident(ctx.h, sh.h, read.ctypes.data, qpos.ctypes.data, off2.ctypes.data, 100, buf[G:].ctypes.data))
    assert (buf[:G + 7] == 0xA5).all() and (buf[G + int(off2[100]):] == 0xA5).all() and buf[G + 7:G + int(off2[100])].tobytes().decode("latin-1") == want[:int(off[100])]


def test_refusals_write_nothing(ctx, three):
    sh, seqs = three

    def refused(shard, read, qpos, off, what):
        read, qpos, off = np.asarray(read, np.uint32), np.asarray(qpos, np.uint32), np.asarray(off, np.uint64)
        out = np.full(256, 0xA5, np.uint8)
        rc = ctx.lib.csvgpu_alt_bases_resident(ctx.h, shard.h, read.ctypes.data, qpos.ctypes.data, off.ctypes.data, len(read), out.ctypes.data)
        assert rc == _lib.CSV_EINVAL and what in ctx.lib.csvgpu_last_error(ctx.h).decode(), (rc, ctx.lib.csvgpu_last_error(ctx.h))
        assert (out == 0xA5).all()
    refused(sh, [0, 4], [0, 0], [0, 10, 20], "beyond the shard")                         # read == n_reads
    refused(sh, [0, 1, 3], [0, 0, 0], [0, 20, 10, 30], "decreases")
    up = ctx.upload(Reads.from_cigar_lists([10], [0], [60], [[(M, 100)]]), 1000)
    try:
        refused(up, [0], [0], [0, 50], "no sequences")                                    # an uploaded shard holds none
    finally:
        up.free()
    without = build(ctx, seqs, want=0)
    try:
        assert without.sizes()["n_seq"] == 0
        refused(without, [0], [0], [0, 50], "no sequences")
    finally:
        without.free()
    dropped = build(ctx, seqs)
    try:
        assert ctx.alt_bases(dropped, [0], [2], [50]) == [py_alt(bytes(seqs[0][0]), 2, 50)]
        dropped.drop_sequences()
        assert dropped.sizes()["n_seq"] == 0
        refused(dropped, [0], [2], [0, 50], "no sequences")
        dropped.drop_sequences()                                                          # (nothing left to drop: still CSV_OK)
        with pytest.raises(CsvError):
            ctx.alt_bases(dropped, [0], [2], [50])
    finally:
        dropped.free()


@pytest.mark.parametrize("name,pos,cigar,depth_len,exp", CASES, ids=[c[0] for c in CASES])
def test_fifty_base_alt_from_the_shards_own_sequences(ctx, name, pos, cigar, depth_len, exp):
    """the six cases of tests/test_gpu_alt_sequence.py through processChromosome on a BUILT shard, the ALT cut from the sequences it holds:
    the strings of the seq_off / seq route"""
    host.set_context(ctx)
    qlen = sum(l for op, l in cigar if op in (M, I, S))
    rng = np.random.default_rng(len(name))
    bases = "".join(rng.choice(list(NT16), qlen))
    seq = pack(bases)
    words = [(l << 4) | op for op, l in cigar]
    rec = bam_py.encode_record(0, pos, 60, 0, b"read", words, seq.tobytes(), qlen)
    # a record in front whose sequence has an odd number of bytes: the read's own starts at an odd address
    front = bam_py.encode_record(0, max(pos - 5, 0), 60, 0x100, b"front", [(10 << 4) | 0], bytes([0x12] * 3), 5)
    b = ctx.shard_builder(_lib.SB_SEQ)
    assert b.append_bam(front + rec, [0])[0] == 0
    sh = b.finish(depth_len)
    up = ctx.upload(sh.fetch_reads(), depth_len)
    try:
        seq_off = np.array([0, 3, 3 + len(seq)], np.uint64)
        want = host.process_resident_chromosome_alts(ctx, up, 0.1, 0.1, seq_off, np.concatenate([np.array([0x12] * 3, np.uint8), seq]))
        start, end, q = exp
        assert want == [(start, end, "".join("N" if c in AMBIG else c for c in bases[q: q + 50]))]
        assert host.process_resident_chromosome_alts(ctx, sh, 0.1, 0.1, resident_seq=True) == want
        assert host.process_resident_chromosome_alts(ctx, sh, 0.1, 0.1) == [(start, end, "N" * 50)]      # not asked for: N's, as without sequences
    finally:
        up.free()
        sh.free()
