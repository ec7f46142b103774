"""The FASTA loader's rules restated in Python, and the texts the FASTA tests share. The rules are those of ReferenceGenome::setFilepath
and ::query (contextsv_amd/csrc/host/fasta_query.cpp; the device states them in csrc/fasta_core.hpp):

  lines      split on b"\\n" only; a final unterminated line counts; b"\\r" stays in the data and in a name; an empty line adds nothing
  headers    a non-empty line whose first byte is b">"; the name runs from the byte behind it to the first blank or the line's end
  residues   every other line. The loader appends them to ONE pending sequence, which it stores (and clears) only under a named header,
             when the next header line or the file's end arrives: residues in front of the first header or under an empty-named header
             fall to the first named header behind them, and are dropped when none follows
  records    one per named header, in file order; a lookup by name takes the last record of that name
  a cut      [pos_start, pos_end] 1-based inclusive, both decremented with uint32 wrap; empty when pos_end >= length or start > end
"""
import numpy as np

TILE = 4096
AMBIGUOUS = b"RYKMSWBDHVrykmswbdhv"
MASK_TABLE = bytes(ord("N") if c in AMBIGUOUS else c for c in range(256))


def records(text: bytes):
    """[(name, sequence)] in file order, duplicates kept: what the loader stores, store by store."""
    out, name, seq = [], b"", bytearray()
    for line in text.split(b"\n"):                     # (the piece behind a final b"\n" is empty and adds nothing)
        if line[:1] == b">":
            if name:
                out.append((name, bytes(seq)))
                seq = bytearray()
            name = line[1:].split(b" ", 1)[0]
        else:
            seq += line
    if name:
        out.append((name, bytes(seq)))
    return out


def lookup(recs):
    """name -> (record index, sequence): the last record of a name wins, as the loader's map overwrite does."""
    return {n: (i, s) for i, (n, s) in enumerate(recs)}


def chromosomes(recs):
    return sorted(n for n, _ in recs)


def contig_header(recs):
    return b"\n".join(b"##contig=<ID=" + n + b",length=" + str(len(s)).encode() + b">" for n, (_, s) in sorted(lookup(recs).items()))


def cut(seq: bytes, pos_start: int, pos_end: int, mask: bool = False) -> bytes:
    ps, pe = (pos_start - 1) & 0xFFFFFFFF, (pos_end - 1) & 0xFFFFFFFF
    if pe >= len(seq) or ps > pe:
        return b""
    s = seq[ps: pe + 1]
    return s.translate(MASK_TABLE) if mask else s


def cut_len(length: int, pos_start: int, pos_end: int) -> int:
    ps, pe = (pos_start - 1) & 0xFFFFFFFF, (pos_end - 1) & 0xFFFFFFFF
    return 0 if pe >= length or ps > pe else pe - ps + 1


# ---- the texts ------------------------------------------------------------------------------------------------------------------------

def _bases(rng, n):
    return bytes(rng.choice(np.frombuffer(b"ACGTNacgtnRYKMSWBDHV", np.uint8), n).tobytes())


def small_texts():
    """Texts of 0-17 bytes and the degenerate shapes: no final newline, only headers, only residues, only empty lines, \\r\\n endings."""
    out = [b"", b"\n", b">", b">\n", b"A", b"A\n", b">a", b">a\n", b">a\nA", b">a\nA\n", b"\n\n\n", b">a\r\nAC\r\nGT\r\n", b">a\r\n\r\nAC\r",
           b"ACGT\nACGT\n", b"ACGT", b">a\n>b\n>c\n", b">a\n>b\n>c", b">a\n\n\nAC\n\n", b"\n>a\nAC", b">a b c\nACGTACGTA", b"> \n>\n> x\n", b"\r\n\r\n",
           b">a\nACG\n>b\nTTT\n>a\nG", b"AC\n>\nGT\n>z\nA\n"]
    for n in range(18):
        out.append((b">q\n" + b"ACGTACGTACGTACGT")[:n])
        out.append(b"ACGTACG\nACGTACGTAC"[:n])
    return out


def header_texts():
    """`>` alone, `> desc`, residues in front of the first header and under empty-named headers, repeated names, long names, \\r in a name."""
    out = [b">\nACGT\n>x\nTT\n", b"> desc\nACGT\n>x y\nTT\n", b"ACGT\nAC\n>x\nTT\n", b">x\nAA\n>\nCC\n>y\nGG\n", b">x\nAA\n>\nCC\n", b">x\nAA\n> d\nCC",
           b">x\nAA\n>x\nCC\n", b">x\nAA\n>y\nT\n>x\nCC\n>x\nGGG\n", b">x\r\nAA\r\n>y\rz w\nCC\n", b">x\r y\nAC\n", b"AA\n>\nCC\n> \nGG\n",
           b">a\n>b\nAC\n>\n>c\n", b">\n>\n>\nAC\n>k\n"]
    for n in (1, 2, 15, 16, 17, 63, 64, 65, 255, 256, 300):
        name = (b"n%03d_" % n + b"x" * 300)[:n]
        out.append(b">" + name + b"\nACGT\n>" + name + b" description here\nTTTT\nGG")
    return out


def tile_texts(rng):
    """Line ends around tile edges, line lengths 0-70, long lines, many short lines."""
    out = {}
    for d in range(-17, 18):                           # a line end at every offset within 17 bytes of the first tile edge (and so of the second)
        first = b">c1 d\n" + _bases(rng, TILE + d - 6 - 1) + b"\n"
        assert len(first) == TILE + d
        out[f"edge{d:+d}"] = first + _bases(rng, TILE - 1) + b"\n>c2\n" + _bases(rng, 37)
    lines = [b">len"]
    for n in list(range(71)) + list(range(70, -1, -1)):
        lines.append(_bases(rng, n))
    out["lengths0-70"] = b"\n".join(lines) + b"\n>next\n" + _bases(rng, 61) + b"\n"
    out["three_tiles"] = b">t\nAC\n" + _bases(rng, 2 * TILE + 300) + b"\nGT\n"
    out["long_residues"] = b">r\n" + _bases(rng, 70_000) + b"\n>s\nAC\n"
    out["long_header"] = b">h " + b"d" * 70_000 + b"\nACGT\n>" + b"N" * 70_000 + b"\nTT\n"
    out["many_short"] = b">m\n" + b"A\n" * 302_000 + b">n\nC\n"
    return out


def wrapped_text(rng, contigs=(("chr1", 9000), ("chr2 extra words", 5000), ("chr3", 0), ("chrM", 61)), width=60):
    parts = []
    for name, n in contigs:
        parts.append(b">" + name.encode())
        seq = _bases(rng, n)
        parts += [seq[i: i + width] for i in range(0, n, width)]
    return b"\n".join(parts) + b"\n"


def feature_text():
    """300 bytes with every feature above: the text the cut tests feed at every offset."""
    t = (b"ACG\nT\n\n> lead desc\nNN\r\n>chrA some description\r\nACGTRYKM\nacgtrykm\n\n>\nSWB\n>chrB\nDHV\n\n>chrA\nTTTTTTTTTTGGGGGGGGGG\n"
         b">name\rwith cr x\nAC\n>chrC\n" + b"ACGTNNNNAC" * 9 + b"\n> \nGG\n>last no newline at the end of this text\nCCCCCCCCCCAAAAAAAAAATTTTT")
    t = t + b"G" * (300 - len(t))
    assert len(t) == 300
    return t


def all_texts(rng):
    d = {f"small{i}": t for i, t in enumerate(small_texts())}
    d.update({f"header{i}": t for i, t in enumerate(header_texts())})
    d.update(tile_texts(rng))
    d["wrapped"] = wrapped_text(rng)
    d["features"] = feature_text()
    return d
