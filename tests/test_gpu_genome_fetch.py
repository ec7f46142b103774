"""csvgpu_genome_fetch (contextsv_amd/csrc/api/fasta.hip, kernels/fasta.hip fa_cut): cuts of a genome that lives on the device, against
ReferenceGenome::query's rule and the VCF writer's masking as tests/fasta_inputs.py states them."""
import numpy as np
import pytest

import fasta_dev as fd
import fasta_inputs as fi
from contextsv_amd import _lib

pytestmark = pytest.mark.gpu
GUARD = 0xA5


@pytest.fixture(scope="module")
def genome(ctx):
    """three records behind 5 residue bytes that fall to the first: the records start at 0, 1 405 and 1 405 + 2^20 + 77 of the array"""
    rng = np.random.default_rng(12)
    seqs = [b"ACGTA" + fi._bases(rng, 1400), fi._bases(rng, (1 << 20) + 77), bytes(range(256)).replace(b"\n", b"") * 3]
    text = b"ACGTA\n>r0 d\n" + seqs[0][5:] + b"\n>big\n" + seqs[1] + b"\n>bytes\n" + seqs[2]
    g = fd.build(ctx, [text], reserve=len(text))
    assert g.describe()["names"] == [b"r0", b"big", b"bytes"] and list(g.describe()["lengths"]) == [len(s) for s in seqs]
    yield g, seqs
    g.free()


def _fetch_between_guards(g, seqs, rec, ps, pe, mask, lead=37):
    rec, ps, pe = (np.asarray(a, np.uint32) for a in (rec, ps, pe))
    lens = np.array([fi.cut_len(len(seqs[r]), int(a), int(b)) for r, a, b in zip(rec, ps, pe)], np.uint64)
    off = np.full(len(rec) + 1, lead, np.uint64)
    off[1:] += np.cumsum(lens, dtype=np.uint64)
    out = np.full(int(off[-1]) + 41, GUARD, np.uint8)
    assert g.fetch_raw(rec, ps, pe, off, mask, out) == 0
    assert (out[:lead] == GUARD).all() and (out[int(off[-1]):] == GUARD).all(), "written outside [out_off[0], out_off[n])"
    raw = out.tobytes()
    return [raw[int(off[i]): int(off[i + 1])] for i in range(len(rec))]


def test_lengths_0_to_200_at_every_start(genome):
    g, seqs = genome
    rec, ps, pe = [], [], []
    for r in (0, 1):
        for start in range(1, 18):                      # every residue mod 16 of the source, and one more
            for n in range(201):
                rec.append(r); ps.append(start); pe.append(start + n - 1)      # (n == 0: start > end)
    for mask in (False, True):
        got = _fetch_between_guards(g, seqs, rec, ps, pe, mask)
        for k, (r, a, b) in enumerate(zip(rec, ps, pe)):
            assert got[k] == fi.cut(seqs[r], a, b, mask), (r, a, b, mask)


def test_range_edges(genome):
    g, seqs = genome
    L = len(seqs[0])
    cases = [(0, 0), (0, 5), (0, L), (5, 4), (L, 1), (1, L), (2, L), (1, L + 1), (L, L), (L, L + 1), (L + 1, L + 1), (1, 0xFFFFFFFF), (0xFFFFFFFF, 0xFFFFFFFF),
             (0xFFFFFFFF, 1), (1, 1), (L - 15, L), (L - 16, L)]
    got = _fetch_between_guards(g, seqs, [0] * len(cases), [a for a, _ in cases], [b for _, b in cases], False)
    for (a, b), s in zip(cases, got):
        assert s == fi.cut(seqs[0], a, b), (a, b)
    assert got[0] == got[1] == got[2] == b"" and got[5] == seqs[0] and got[7] == b"" and got[11] == b""        # the wrap of 0; end past the contig
    assert g.fetch([0, 0], [3, 1], [10, L]) == [seqs[0][2:10], seqs[0]]


def test_every_byte_value_with_and_without_the_mask(genome):
    g, seqs = genome
    s = seqs[2]
    assert len(set(s)) == 255 and len(s) == 765
    for mask in (False, True):
        whole, = _fetch_between_guards(g, seqs, [2], [1], [len(s)], mask)
        assert whole == (s.translate(fi.MASK_TABLE) if mask else s)
        each = _fetch_between_guards(g, seqs, [2] * 255, range(1, 256), range(1, 256), mask)
        assert b"".join(each) == (s[:255].translate(fi.MASK_TABLE) if mask else s[:255])
    assert sum(a != b for a, b in zip(s[:255], s[:255].translate(fi.MASK_TABLE))) == 20


def test_70000_items_between_guard_bytes(genome):
    g, seqs = genome
    rng = np.random.default_rng(2)
    n = 70_000
    rec = rng.integers(0, 2, n).astype(np.uint32)
    ps = np.array([rng.integers(0, len(seqs[r]) + 2) for r in rec], np.uint32)
    pe = (ps + rng.choice([0, 0, 1, 2, 15, 16, 17, 40, 300], n) - rng.integers(0, 2, n)).astype(np.uint32)
    got = _fetch_between_guards(g, seqs, rec, ps, pe, True, lead=3)
    exp = [fi.cut(seqs[r], int(a), int(b), True) for r, a, b in zip(rec, ps, pe)]
    assert got == exp and sum(map(len, exp)) > 1_000_000 and exp.count(b"") > 5_000


def test_one_item_of_a_mebibyte(genome):
    g, seqs = genome
    for start in (1, 2, 17, 78):
        got, = _fetch_between_guards(g, seqs, [1], [start], [start + (1 << 20) - 1], False, lead=start)
        assert len(got) == 1 << 20 and got == seqs[1][start - 1: start - 1 + (1 << 20)]


def test_the_last_record_of_a_name(ctx):
    g = fd.build(ctx, [b">x\nAAAA\n>y\nCC\n>x\nGGGGGG\n>\nTT\n>x\nTTTTTTTTT\n>y d\nC\n"])
    assert g.describe()["names"] == [b"x", b"y", b"x", b"x", b"y"]             # (the empty-named header is no record)
    assert g.record_of("x") == 3 and g.record_of(b"y") == 4
    with pytest.raises(KeyError):
        g.record_of("z")
    assert g.fetch([g.record_of("x"), g.record_of("y"), 0], [1, 1, 2], [11, 1, 3]) == [b"TTTTTTTTTTT", b"C", b"AA"]
    g.free()


def test_refusals_at_known_indices(genome):
    g, seqs = genome
    L = len(seqs[0])
    out = np.full(64, GUARD, np.uint8)

    def rc(rec, ps, pe, off):
        r = g.fetch_raw(rec, ps, pe, np.asarray(off, np.uint64), False, out)
        assert (out == GUARD).all(), "written despite the refusal"
        return r

    assert rc([0, 3, 0], [1, 1, 1], [4, 4, 4], [0, 4, 8, 12]) == _lib.CSV_EINVAL                    # a record index beyond the genome, item 1
    assert rc([0, 0, 0xFFFFFFFF], [1, 1, 1], [4, 4, 4], [0, 4, 8, 12]) == _lib.CSV_EINVAL
    assert rc([0, 0, 0], [1, 1, 1], [4, 4, 4], [0, 4, 3, 7]) == _lib.CSV_EINVAL                      # out_off decreases at item 1
    assert rc([0, 0, 0], [1, 1, 1], [4, 4, 4], [0, 4, 9, 13]) == _lib.CSV_EINVAL                     # item 1: room for 5, the cut has 4
    assert rc([0, 0, 0], [1, 1, 1], [4, 4, 4], [0, 4, 7, 11]) == _lib.CSV_EINVAL                     # item 1: room for 3
    assert rc([0, 0], [1, 1], [4, L + 1], [0, 4, 8]) == _lib.CSV_EINVAL                              # item 1: an empty cut (end past the contig) given room
    assert rc([0, 0], [1, 0], [4, 4], [0, 4, 8]) == _lib.CSV_EINVAL                                  # item 1: pos_start 0 wraps: empty
    assert g.ctx.lib.csvgpu_genome_fetch(g.ctx.h, g.h, None, None, None, None, 2, 0, out.ctypes.data) == _lib.CSV_EINVAL
    assert g.ctx.lib.csvgpu_genome_fetch(g.ctx.h, g.h, None, None, None, None, 0, 0, None) == 0
    assert g.fetch([0], [1], [4]) == [seqs[0][:4]]
