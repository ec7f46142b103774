"""Inputs of the device's BAM record unpacking (csvgpu_bam_unpack, kernels/bamunpack.hip) with the expected arrays computed here, in pure
Python, from the rules of the host reader (BamReader::stream / append / find_cg and readContig's run): a third statement of them beside
host/bam_io.cpp and contextsv_amd/csrc/bam_record_core.hpp. tests/test_bam_unpack_inputs.py pins these expectations against the host reader
on the CPU; tests/test_gpu_bam_unpack.py runs the kernels on the same streams. Records come from tests/bam_py.py's encode_record; what it
cannot write (a CG:B,i tag, a refused length) is patched into its bytes."""
import struct

import numpy as np

import bam_py

SHORT, LONG, NEG_LSEQ, FIELDS, ANCHOR = 1, 2, 3, 4, 5
MESSAGES = {SHORT: "BAM: record shorter than its fixed fields", LONG: "BAM: implausible record length", NEG_LSEQ: "BAM: negative sequence length",
            FIELDS: "BAM: record fields exceed the record length"}
GUARD = 0xA5


class Declined(Exception):
    def __init__(self, reason, offset):
        super().__init__("declined: reason %d at %d" % (reason, offset))
        self.reason, self.offset = reason, offset


# ---- libstdc++'s std::hash<std::string> (64-bit _Hash_bytes) ---------------------------------------------------------------------------
_M64 = (1 << 64) - 1
_MUL = (0xc6a4a793 << 32) + 0x5bd1e995


def _mix(v):
    return v ^ (v >> 47)


def hash_bytes(b: bytes) -> int:
    h = (0xc70f6907 ^ (len(b) * _MUL)) & _M64
    n8 = len(b) & ~7
    for i in range(0, n8, 8):
        d = (_mix((int.from_bytes(b[i:i + 8], "little") * _MUL) & _M64) * _MUL) & _M64
        h = ((h ^ d) * _MUL) & _M64
    if len(b) & 7:
        h = ((h ^ int.from_bytes(b[n8:], "little")) * _MUL) & _M64
    h = (_mix(h) * _MUL) & _M64
    return _mix(h)


# ---- the rules, in Python ---------------------------------------------------------------------------------------------------------------
def walk(stream: bytes, start=0):
    """-> (record offsets, consumed); Declined for a refused block_size (the host's order: both length checks, then completeness)"""
    offs, o, n = [], start, len(stream)
    while o + 4 <= n:
        bs, = struct.unpack_from("<I", stream, o)
        if bs < 32:
            raise Declined(SHORT, o)
        if bs > (1 << 30):
            raise Declined(LONG, o)
        if o + 4 + bs > n:
            break
        offs.append(o)
        o += 4 + bs
    return offs, o


def find_cg(rec: bytes, p: int):
    """find_cg of host/bam_io.cpp: -> (offset of the first element, count) or None; rec is one record body, p where its aux fields start"""
    end = len(rec)
    while p + 3 <= end:
        is_cg, t = rec[p:p + 2] == b"CG", rec[p + 2:p + 3]
        p += 3
        if t in (b"A", b"c", b"C"):
            ln = 1
        elif t in (b"s", b"S"):
            ln = 2
        elif t in (b"i", b"I", b"f"):
            ln = 4
        elif t == b"d":
            ln = 8
        elif t in (b"Z", b"H"):
            z = rec.find(b"\0", p)
            if z < 0:
                return None
            ln = z - p + 1
        elif t == b"B":
            if p + 5 > end:
                return None
            es = {b"c": 1, b"C": 1, b"s": 2, b"S": 2, b"i": 4, b"I": 4, b"f": 4}.get(rec[p:p + 1])
            n, = struct.unpack_from("<I", rec, p + 1)
            if es is None or end - p - 5 < n * es:
                return None
            if is_cg:
                return (p + 5, n) if rec[p:p + 1] in (b"I", b"i") else None
            ln = 5 + n * es
        else:
            return None
        if is_cg or end - p < ln:
            return None
        p += ln
    return None


def fields(stream: bytes, o: int):
    """one record at o -> dict of the host reader's values; Declined as append refuses"""
    bs, = struct.unpack_from("<I", stream, o)
    rec = stream[o + 4:o + 4 + bs]
    tid, pos, l_name, mapq, _bin, n_cigar, flag, l_seq = struct.unpack_from("<iiBBHHHi", rec, 0)
    if l_seq < 0:
        raise Declined(NEG_LSEQ, o)
    fixed = 32 + l_name + 4 * n_cigar + (l_seq + 1) // 2 + l_seq
    if fixed > bs:
        raise Declined(FIELDS, o)
    name = rec[32:32 + l_name].split(b"\0")[0]
    c0 = 32 + l_name
    cigar = rec[c0:c0 + 4 * n_cigar]
    if n_cigar > 0 and tid >= 0 and pos >= 0:
        w0, = struct.unpack_from("<I", rec, c0)
        if (w0 & 15) == 4 and (w0 >> 4) == l_seq:
            cg = find_cg(rec, fixed)
            if cg is not None and n_cigar <= cg[1] < (1 << 29):
                cigar = rec[cg[0]:cg[0] + 4 * cg[1]]
    seq = rec[c0 + 4 * n_cigar:c0 + 4 * n_cigar + (l_seq + 1) // 2]
    return dict(tid=tid, pos=pos, mapq=mapq, flag=flag, name=name, cigar=cigar, seq=seq)


def expected(stream: bytes, tid=-1, end=0, bases=(0, 0, 0)):
    """what csvgpu_bam_unpack must return for the whole stream (anchors change nothing): counts and arrays; Declined otherwise"""
    offs, consumed = walk(stream)
    tp = [struct.unpack_from("<ii", stream, o + 4) for o in offs]
    a = 0
    if tid >= 0:
        while a < len(offs) and 0 <= tp[a][0] < tid:
            a += 1
    b = a
    while b < len(offs) and (tid < 0 or (tp[b][0] == tid and tp[b][1] < end)):
        b += 1
    recs = [fields(stream, o) for o in offs[a:b]]                       # (the lowest offset first)
    cum = lambda lens, base: np.concatenate([[0], np.cumsum(lens, dtype=np.uint64)]).astype(np.uint64) + np.uint64(base)
    names = [r["name"] for r in recs]
    return dict(n_records=len(offs), kept_first=a, n_kept=b - a, stopped=b < len(offs), consumed=consumed, rec_off=offs,
                pos=np.array([r["pos"] for r in recs], np.int32), flag=np.array([r["flag"] for r in recs], np.uint16),
                mapq=np.array([r["mapq"] for r in recs], np.uint8),
                cigar_off=cum([len(r["cigar"]) // 4 for r in recs], bases[0]), cigar=np.frombuffer(b"".join(r["cigar"] for r in recs), np.uint32),
                seq_off=cum([len(r["seq"]) for r in recs], bases[1]), seq=np.frombuffer(b"".join(r["seq"] for r in recs), np.uint8),
                name_off=cum([len(x) for x in names], bases[2]), name=np.frombuffer(b"".join(names), np.uint8), names=names,
                name_hash=np.array([hash_bytes(x) for x in names], np.uint64))


# ---- records -----------------------------------------------------------------------------------------------------------------------------
def _cigar(rng, n):
    return [(int(rng.integers(1, 200)) << 4) | int(rng.choice([0, 1, 2, 4, 7, 8])) for _ in range(n)]


def record(rng, tid=0, pos=100, qname=b"read", n_cigar=3, l_seq=7, aux=b"", force_cg=False, cigar=None, mapq=None, flag=None):
    cigar = _cigar(rng, n_cigar) if cigar is None else cigar
    seq4 = bytes(rng.integers(1, 256, (l_seq + 1) // 2, dtype=np.uint8))
    return bam_py.encode_record(tid, pos, int(rng.integers(0, 61)) if mapq is None else mapq, int(rng.integers(0, 4096)) if flag is None else flag,
                                qname, cigar, seq4, l_seq, aux, force_cg)


def _name(n, k=0):
    return bytes(97 + (i * 7 + k) % 26 for i in range(n))


def patch(rec: bytes, at: int, fmt: str, value) -> bytes:
    """a field of one encoded record overwritten (at: offset from the record's start, block_size field included)"""
    return rec[:at] + struct.pack(fmt, value) + rec[at + struct.calcsize(fmt):]


def alignment_stream(seed=1):
    """(a) l_name 1..8 and 255 (the CIGAR at every byte alignment), n_cigar 0, l_seq 0 and odd, the empty name, a NUL inside l_name, and
    name lengths of every residue mod 8 up to 254 for the hashes"""
    rng = np.random.default_rng(seed)
    recs = []
    for k, n in enumerate(list(range(0, 8)) + [254]):
        recs.append(record(rng, pos=10 + k, qname=_name(n, k), n_cigar=1 + k % 4, l_seq=2 * k + 1))
    recs.append(record(rng, pos=30, qname=b"nocigar", n_cigar=0, l_seq=5))
    recs.append(record(rng, pos=31, qname=b"noseq", n_cigar=2, l_seq=0))
    recs.append(record(rng, pos=32, qname=b"", n_cigar=0, l_seq=0))
    recs.append(record(rng, pos=33, qname=b"ab\0cd", n_cigar=2, l_seq=3))
    recs.append(record(rng, pos=34, qname=b"\0xyz", n_cigar=1, l_seq=1))
    for k, n in enumerate(list(range(8, 26)) + [63, 64, 65, 127, 128, 247, 248, 249, 250, 251, 252, 253, 254]):
        recs.append(record(rng, pos=40 + k, qname=_name(n, k + 3), n_cigar=k % 3, l_seq=k % 5))
    return b"".join(recs)


AUX_FIELDS = [b"XAAx", b"Xcc\x81", b"XCC\x01", b"Xss\x01\x80", b"XSS\x01\x02", b"Xii\x01\x02\x03\x84", b"XII\x01\x02\x03\x04", b"Xff\x00\x00\x80\x3f",
              b"Xdd" + struct.pack("<d", 2.5), b"XZZa text\0", b"XHH1A2B\0"] + \
             [b"XB" + b"B" + s + struct.pack("<I", 3) + bytes(range(1, 1 + 3 * e)) for s, e in ((b"c", 1), (b"C", 1), (b"s", 2), (b"S", 2), (b"i", 4), (b"I", 4), (b"f", 4))]


def cg_stream(seed=2):
    """(b) the CG rule. -> (stream, names of the cases in record order, indices of the records whose CG tag counts)"""
    rng = np.random.default_rng(seed)
    recs, names, taken = [], [], []

    def add(name, rec, is_taken):
        if is_taken:
            taken.append(len(recs))
        recs.append(rec)
        names.append(name)
    l_seq = 9
    placeholder = [(l_seq << 4) | 4, (500 << 4) | 3]
    add("taken", record(rng, qname=b"cg0", n_cigar=5, l_seq=l_seq, force_cg=True), True)
    r = record(rng, qname=b"cg1", n_cigar=4, l_seq=l_seq, force_cg=True)
    add("B,i taken", r[:r.rfind(b"CGBI")] + b"CGBi" + r[r.rfind(b"CGBI") + 4:], True)
    add("count below n_cigar", record(rng, qname=b"cg2", n_cigar=1, l_seq=l_seq, force_cg=True), False)
    add("count equal to n_cigar", record(rng, qname=b"cg2b", n_cigar=2, l_seq=l_seq, force_cg=True), True)
    add("CG:Z", record(rng, qname=b"cg3", cigar=placeholder, l_seq=l_seq, aux=b"CGZ5M\0"), False)
    add("no tag", record(rng, qname=b"cg4", cigar=placeholder, l_seq=l_seq), False)
    add("another tag only", record(rng, qname=b"cg5", cigar=placeholder, l_seq=l_seq, aux=b"NMi\x01\0\0\0"), False)
    add("pos negative", record(rng, pos=-1, qname=b"cg7", n_cigar=5, l_seq=l_seq, force_cg=True), False)
    add("first op not S", record(rng, qname=b"cg8", cigar=[(l_seq << 4) | 0, (5 << 4) | 3], l_seq=l_seq, aux=b"CGBI" + struct.pack("<III", 2, 0x10, 0x20)), False)
    add("S of another length", record(rng, qname=b"cg9", cigar=[((l_seq + 1) << 4) | 4], l_seq=l_seq, aux=b"CGBI" + struct.pack("<III", 2, 0x10, 0x20)), False)
    for k, f in enumerate(AUX_FIELDS):
        add("behind %r" % f[:4], record(rng, qname=b"aux%d" % k, n_cigar=3 + k, l_seq=l_seq, aux=f, force_cg=True), True)
    add("behind all of them", record(rng, qname=b"auxall", n_cigar=7, l_seq=l_seq, aux=b"".join(AUX_FIELDS), force_cg=True), True)
    add("Z without NUL", record(rng, qname=b"bad0", cigar=placeholder, l_seq=l_seq, aux=b"XZZ" + b"CGBI\x02\x01\x01\x01" + b"\x10\x01\x01\x01" * 3), False)
    add("B count past the record", record(rng, qname=b"bad1", n_cigar=3, l_seq=l_seq, aux=b"XBBc" + struct.pack("<I", 1000) + b"abc", force_cg=True), False)
    add("B of an unknown subtype", record(rng, qname=b"bad2", n_cigar=3, l_seq=l_seq, aux=b"XBBq" + struct.pack("<I", 1) + b"a", force_cg=True), False)
    add("unknown type", record(rng, qname=b"bad3", n_cigar=3, l_seq=l_seq, aux=b"XQ?ab", force_cg=True), False)
    add("a scalar cut by the record's end", record(rng, qname=b"bad4", cigar=placeholder, l_seq=l_seq, aux=b"Xii\x01\x02"), False)
    add("CG count past the record", record(rng, qname=b"bad5", cigar=placeholder, l_seq=l_seq, aux=b"CGBI" + struct.pack("<II", 3, 0x10)), False)
    add("two aux bytes", record(rng, qname=b"bad6", cigar=placeholder, l_seq=l_seq, aux=b"CG"), False)
    add("taken again", record(rng, qname=b"cg10", n_cigar=6, l_seq=l_seq, force_cg=True), True)
    add("tid negative", record(rng, tid=-1, qname=b"cg6", n_cigar=5, l_seq=l_seq, force_cg=True), False)       # (last: the host reader's run of contig 0 ends here)
    return b"".join(recs), names, taken


def long_cigar_stream(n_small=5000, n_ops=70_000, seed=3):
    """(b) one real 70 000-operation record (a CG tag because it must be one) among 5 000 one-operation records"""
    rng = np.random.default_rng(seed)
    small = [record(rng, pos=10 + k, qname=b"s%d" % k, n_cigar=1, l_seq=k % 4) for k in range(n_small)]
    big = record(rng, pos=4000, qname=b"long", cigar=[((1 + j % 5) << 4) | (0 if j % 2 == 0 else 1 + j % 2) for j in range(n_ops)], l_seq=11)
    at = n_small // 2 + 1
    return b"".join(small[:at] + [big] + small[at:]), at


def plain_stream(n=60, seed=4, tid=0):
    rng = np.random.default_rng(seed)
    return b"".join(record(rng, tid=tid, pos=5 + 3 * k, qname=_name(3 + k % 11, k), n_cigar=k % 6, l_seq=k % 9, force_cg=(k % 13 == 5)) for k in range(n))


def filter_stream(seed=5):
    """(e) three records of contig 0, five of contig 1 at positions 10, 20, 30, 40, 50, two of contig 2, two without a contig"""
    rng = np.random.default_rng(seed)
    recs = [record(rng, tid=0, pos=900 + k, qname=b"a%d" % k) for k in range(3)]
    recs += [record(rng, tid=1, pos=10 * (k + 1), qname=b"b%d" % k, force_cg=(k == 2)) for k in range(5)]
    recs += [record(rng, tid=2, pos=7 + k, qname=b"c%d" % k) for k in range(2)]
    recs += [record(rng, tid=-1, pos=-1, qname=b"u%d" % k, n_cigar=0) for k in range(2)]
    return b"".join(recs)


def refusal_records(seed=6):
    """the twelve intact records the refused streams are made of"""
    rng = np.random.default_rng(seed)
    return [record(rng, pos=10 + 20_000 * k, qname=b"r%d" % k, n_cigar=2, l_seq=4) for k in range(12)]


def refusal_streams(seed=6):
    """(f) -> [(name, stream, reason, offset)]: each of the host's four checks failing at record 7 of 12"""
    recs = refusal_records(seed)
    at = sum(len(r) for r in recs[:7])
    with_rec = lambda r: b"".join(recs[:7] + [r] + recs[8:])
    return [("block_size 31", with_rec(patch(recs[7], 0, "<I", 31)), SHORT, at),
            ("block_size 0", with_rec(patch(recs[7], 0, "<I", 0)), SHORT, at),
            ("block_size 2^30 + 1", with_rec(patch(recs[7], 0, "<I", (1 << 30) + 1)), LONG, at),
            ("block_size 2^32 - 1", with_rec(patch(recs[7], 0, "<I", 0xFFFFFFFF)), LONG, at),
            ("l_seq -1", with_rec(patch(recs[7], 4 + 16, "<i", -1)), NEG_LSEQ, at),
            ("n_cigar 60000", with_rec(patch(recs[7], 4 + 12, "<H", 60000)), FIELDS, at),
            ("l_seq 2^31 - 1", with_rec(patch(recs[7], 4 + 16, "<i", (1 << 31) - 1)), FIELDS, at),
            ("l_name 255", with_rec(patch(recs[7], 4 + 8, "<B", 255)), FIELDS, at)]


def index_entries(stream: bytes):
    """the (bytes, tid, beg, end, flag) tuples bam_py.write_bam takes, for a well-formed stream"""
    out = []
    for o in walk(stream)[0]:
        bs, = struct.unpack_from("<I", stream, o)
        tid, pos = struct.unpack_from("<ii", stream, o + 4)
        flag, = struct.unpack_from("<H", stream, o + 4 + 14)
        out.append((stream[o:o + 4 + bs], tid, max(pos, 0), max(pos, 0) + 1, flag))
    return out
