"""csvgpu_genome_builder_* (contextsv_amd/csrc/api/fasta.hip, kernels/fasta.hip): a FASTA's text appended on the device, whole and in pieces
cut anywhere, against the Python statement of the loader's rules (tests/fasta_inputs.py, itself held against the host loader and the oracle
in tests/test_fasta_inputs.py) and against the host backing — names, lengths and every base. A tile is 4 096 bytes."""
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

import bam_py
import fasta_dev as fd
import fasta_inputs as fi
from contextsv_amd import _lib, host

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def tiles():
    return fi.tile_texts(np.random.default_rng(5))


def _host_table(tmp_path, text):
    """name -> sequence of the host backing (the last record of a name)"""
    path = str(tmp_path / "t.fa")
    with open(path, "wb") as f:
        f.write(text)
    g = host.ReferenceGenome(path)
    out = {}
    for name in set(g.getChromosomes()):
        n = g.getChromosomeLength(name.decode("latin-1"))
        out[name] = g.query(name.decode("latin-1"), 1, n) if n else b""
    g.close()
    return out


def _check_both(ctx, tmp_path, text, **kw):
    exp = fd.check_text(ctx, text, **kw)
    assert _host_table(tmp_path, text) == {n: s for n, (_, s) in fi.lookup(exp).items()}


# ---- 1. small texts -----------------------------------------------------------------------------------------------------------------------
def test_small_texts(ctx, tmp_path):
    for text in fi.small_texts():
        _check_both(ctx, tmp_path, text)
        fd.check_text(ctx, text, dev=True, shift=3)


# ---- 2. headers and names -----------------------------------------------------------------------------------------------------------------
def test_header_and_name_edges(ctx, tmp_path):
    for text in fi.header_texts():
        _check_both(ctx, tmp_path, text)
        fd.check_text(ctx, text, pieces=fd.even_pieces(text, 3))
    recs = fd.check_text(ctx, b">x\nAA\n>y\nT\n>x\nCC\n>x\nGGG\n")
    assert [n for n, _ in recs] == [b"x", b"y", b"x", b"x"]                   # two and three records of one name, all kept


# ---- 3. tile edges ------------------------------------------------------------------------------------------------------------------------
def test_line_ends_around_a_tile_edge(ctx, tiles):
    keys = [k for k in tiles if k.startswith("edge")]
    assert len(keys) == 35
    for k in keys:
        fd.check_text(ctx, tiles[k])


@pytest.mark.parametrize("key", ["lengths0-70", "three_tiles", "long_residues", "long_header", "many_short"])
def test_line_lengths(ctx, tiles, tmp_path, key):
    _check_both(ctx, tmp_path, tiles[key])


# ---- 4. alignment -------------------------------------------------------------------------------------------------------------------------
def test_text_pointer_at_every_residue_mod_16(ctx, tiles):
    text = tiles["lengths0-70"] + tiles["edge+3"]
    for shift in range(1, 16):
        fd.check_text(ctx, text, dev=True, shift=shift)


def test_genome_tail_at_every_residue_mod_16(ctx):
    """the second batch's first kept byte lands at every residue mod 16 of the array: the compaction's 16-byte, 4-byte and single-byte stores"""
    rng = np.random.default_rng(8)
    body = fi.wrapped_text(rng) + b">u\n" + fi._bases(rng, 5000) + b"\n"
    for k in range(16):
        first = b">a\n" + b"ACGTNRYKACGTNRYK"[:k] + (b"\n" if k % 2 else b"")
        fd.check_text(ctx, first + body, pieces=[first, body])
        fd.check_text(ctx, first + body, pieces=[first, body], dev=True, shift=k)


# ---- 5. cuts ------------------------------------------------------------------------------------------------------------------------------
def test_a_text_cut_at_each_offset(ctx):
    text = fi.feature_text()
    exp = fd.check_text(ctx, text)
    assert len(exp) >= 6
    for at in range(len(text) + 1):
        assert fd.check_text(ctx, text, pieces=fd.pieces_of(text, [at])) == exp, at
    for n in (1, 3, 7):
        assert fd.check_text(ctx, text, pieces=fd.even_pieces(text, n)) == exp, n
    for at in range(0, len(text), 7):                                          # the same on device pointers
        assert fd.check_text(ctx, text, pieces=fd.pieces_of(text, [at]), dev=True, shift=at % 16) == exp, at


def test_cuts_inside_long_lines(ctx, tiles):
    for key in ("long_header", "three_tiles"):
        text = tiles[key]
        for n in (2, 5):
            fd.check_text(ctx, text, pieces=fd.even_pieces(text, n))
    text = b">abc def\r\nAC\r\nGT\r\n"
    for a in range(len(text)):                                                 # three pieces: between '\r' and '\n', inside the name, one byte each
        for b in range(a, len(text)):
            fd.check_text(ctx, text, pieces=fd.pieces_of(text, [a, b]))


# ---- 6. growth and failure ----------------------------------------------------------------------------------------------------------------
def test_growth_from_no_reserve_and_with_the_files_size(ctx):
    rng = np.random.default_rng(3)
    text = fi.wrapped_text(rng, contigs=(("g1", 40_000), ("g2", 90_000), ("g3", 7)))
    for reserve in (0, len(text)):
        fd.check_text(ctx, text, pieces=fd.even_pieces(text, 9), reserve=reserve)


def test_empty_builders(ctx):
    for pieces in ([], [b""], [b"", b""]):
        g = fd.build(ctx, pieces)
        d = g.describe()
        assert d["n_records"] == 0 and d["total_bases"] == 0 and d["names"] == [] and g.fetch([], [], []) == []
        g.free()
    b = ctx.genome_builder()
    b.append(b">a\nAC")
    b.destroy()                                                                # a builder that is never finished
    with pytest.raises(ValueError):
        b.append(b"x")


def test_capacity_and_refusals(ctx):
    g = fd.build(ctx, [b">one\nACGT\n>three\nAC\n"])
    rc, c, off, names, lengths = g.describe_raw(0, 0)
    assert rc == _lib.CSV_ECAPACITY and (c["n_records"], c["n_name_bytes"], c["total_bases"]) == (2, 8, 6)
    for caps in ((1, 8), (2, 7), (0, 8), (2, 0)):
        rc, c, off, names, lengths = g.describe_raw(*caps)
        assert rc == _lib.CSV_ECAPACITY and (c["n_records"], c["n_name_bytes"], c["total_bases"]) == (2, 8, 6), caps
        assert not off.any() and not names.any() and not lengths.any(), "written despite CSV_ECAPACITY"
    rc, c, off, names, lengths = g.describe_raw(5, 20)
    assert rc == 0 and list(off[:3]) == [0, 3, 8] and names.tobytes()[:8] == b"onethree" and list(lengths[:2]) == [4, 2]
    g.free()
    b = ctx.genome_builder()
    lib = ctx.lib
    buf = np.frombuffer(b">a\nAC\n", np.uint8)
    assert lib.csvgpu_genome_builder_append(ctx.h, b.h, None, 4) == _lib.CSV_EINVAL
    assert lib.csvgpu_genome_builder_append_dev(ctx.h, b.h, None, 4) == _lib.CSV_EINVAL
    assert lib.csvgpu_genome_builder_append(ctx.h, b.h, buf.ctypes.data, 1 << 32) == _lib.CSV_EINVAL        # (refused before a byte is read)
    assert lib.csvgpu_genome_builder_append_dev(ctx.h, b.h, 256, 1 << 32) == _lib.CSV_EINVAL
    assert lib.csvgpu_genome_builder_append(ctx.h, None, buf.ctypes.data, 4) == _lib.CSV_EINVAL
    assert lib.csvgpu_genome_builder_append(ctx.h, b.h, None, 0) == 0
    b.append(b">a\nAC\n")                                                      # the refusals left the builder as it was
    g = b.finish()
    assert fd.device_records(g) == [(b"a", b"AC")]
    g.free()


_INJECT = r"""
import sys
sys.path.insert(0, {root!r}); sys.path.insert(0, {tests!r})
import numpy as np
import contextsv_amd as cs
from contextsv_amd import _lib
import fasta_dev as fd, fasta_inputs as fi
rng = np.random.default_rng(4)
first = b">a d\nACGT\n>b"
second = b"b\n" + fi._bases(rng, 50_000) + b"\n>c\nGG"
with cs.Context(0) as ctx:
    ctx.lib.csvgpu_test_fail_next_alloc(1)
    try:
        ctx.genome_builder(100)
        raise SystemExit("the injected allocation failure did not surface in create")
    except cs.CsvError as e:
        assert "genome builder growth" in str(e), str(e)
    b = ctx.genome_builder(0)
    b.append(first)
    for _ in range(3):
        ctx.lib.csvgpu_test_fail_next_alloc(1)
        try:
            b.append(second)
            raise SystemExit("the injected allocation failure did not surface")
        except cs.CsvError as e:
            assert e.status == _lib.CSV_ENOMEM and "genome builder growth" in str(e), str(e)
    ctx.lib.csvgpu_test_fail_next_alloc(0)
    b.append(second)                                                           # the same append again
    g = b.finish()
    assert fd.device_records(g) == fi.records(first + second)
    g.free()
print("ok")
"""


def test_failed_growth_in_the_testhooks_build():
    """csvgpu_test_fail_next_alloc(1) in front of an append that must grow (libcsvgpu_testhooks.so, in a child process): CSV_ENOMEM three
    times over, the builder unchanged — the open header line `>b` of the first append is still open —, then the same append succeeds"""
    env = dict(os.environ, CSVGPU_LIB=os.path.join(ROOT, "contextsv_amd", "lib", "libcsvgpu_testhooks.so"))
    r = subprocess.run([sys.executable, "-c", _INJECT.format(root=ROOT, tests=os.path.join(ROOT, "tests"))], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout + r.stderr


# ---- 7. the seam --------------------------------------------------------------------------------------------------------------------------
def test_inflate_dev_then_append_dev(ctx):
    """one bgzipped text: csvgpu_bgzf_inflate_dev leaves the members' bytes on the device, csvgpu_genome_builder_append_dev takes them where
    they lie, one member a call (the members end anywhere in a line)"""
    rng = np.random.default_rng(6)
    text = fi.wrapped_text(rng, contigs=(("s1 seam", 20_000), ("s2", 13_001)))
    raw, blocks, o, out_off = b"", [], 0, 0
    for a in range(0, len(text), 3001):
        raw += bam_py.bgzf_block(text[a:a + 3001])
    while o < len(raw):
        bsize = struct.unpack_from("<H", raw, o + 16)[0] + 1
        crc, isize = struct.unpack_from("<II", raw, o + bsize - 8)
        blocks.append((o + 18, out_off, bsize - 26, isize, crc, 0))
        o += bsize
        out_off += isize
    blocks = np.array(blocks, _lib.BGZF_BLOCK_DTYPE)
    assert out_off == len(text) and len(blocks) > 5
    lib = ctx.lib
    d_comp, d_bytes, d_status = (lib.csvgpu_dev_alloc(ctx.h, n) for n in (len(raw), out_off + 16, len(blocks)))
    assert d_comp and d_bytes and d_status
    comp = np.frombuffer(raw, np.uint8)
    ctx._check(lib.csvgpu_upload(ctx.h, d_comp, comp.ctypes.data, len(comp)))
    assert lib.csvgpu_bgzf_inflate_dev(ctx.h, d_comp, len(raw), blocks.ctypes.data, len(blocks), d_bytes, out_off, d_status) == 0
    b = ctx.genome_builder(len(text))
    for blk in blocks:
        b.append_ptr(d_bytes + int(blk["out_off"]), int(blk["out_len"]))
    g = b.finish()
    assert fd.device_records(g) == fi.records(text)
    g.free()
    for p in (d_comp, d_bytes, d_status):
        lib.csvgpu_dev_free(ctx.h, p)
