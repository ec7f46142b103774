"""What the GPU tests of the device genome share: a text through Context.genome_builder() in pieces, and a Genome read back whole."""
import numpy as np

import fasta_inputs as fi


def pieces_of(text: bytes, cuts):
    """text cut at the given offsets (any order, duplicates and the ends allowed: empty pieces are appended too)"""
    at = [0] + sorted(cuts) + [len(text)]
    return [text[a:b] for a, b in zip(at, at[1:])]


def even_pieces(text: bytes, n: int):
    return pieces_of(text, [len(text) * k // n for k in range(1, n)])


class DevText:
    """bytes at a device address with a chosen residue mod 16 (csvgpu_dev_alloc / csvgpu_upload): line ends lie all around the text, and
    none of them may count"""

    def __init__(self, ctx, text: bytes, shift: int = 0):
        self.ctx, self.n = ctx, len(text)
        buf = np.full(len(text) + 64, 0x0A, np.uint8)
        self.base = ctx.lib.csvgpu_dev_alloc(ctx.h, len(buf))
        assert self.base
        lead = (-self.base) % 16 + shift
        buf[lead: lead + len(text)] = np.frombuffer(text, np.uint8)
        ctx._check(ctx.lib.csvgpu_upload(ctx.h, self.base, buf.ctypes.data, len(buf)))
        self.ptr = self.base + lead
        assert self.ptr % 16 == shift % 16

    def free(self):
        self.ctx.lib.csvgpu_dev_free(self.ctx.h, self.base)


def build(ctx, pieces, dev: bool = False, shift: int = 0, reserve: int = 0):
    """the pieces appended in order -> Genome"""
    b = ctx.genome_builder(reserve)
    for p in pieces:
        if dev:
            t = DevText(ctx, p, shift)
            try:
                b.append_ptr(t.ptr, t.n)
            finally:
                t.free()
        else:
            b.append(p)
    return b.finish()


def device_records(g):
    """[(name, sequence)] of a Genome: describe, and every record fetched whole in one call"""
    d = g.describe()
    n = d["n_records"]
    lengths = d["lengths"]
    assert len(d["names"]) == n == len(lengths) and int(lengths.astype(np.uint64).sum()) == d["total_bases"]
    seqs = g.fetch(np.arange(n, dtype=np.uint32), np.ones(n, np.uint32), lengths) if n else []
    return list(zip(d["names"], seqs))


def check_text(ctx, text: bytes, pieces=None, **kw):
    """the device genome of `text` = the Python statement: names, lengths and every base"""
    g = build(ctx, [text] if pieces is None else pieces, **kw)
    try:
        got, exp = device_records(g), fi.records(text)
        assert [n for n, _ in got] == [n for n, _ in exp]
        assert [len(s) for _, s in got] == [len(s) for _, s in exp]
        assert got == exp
        c = g.describe()
        assert c["n_text_bytes"] == len(text) and c["n_lines"] == text.count(b"\n")
    finally:
        g.free()
    return exp
