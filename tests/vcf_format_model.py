"""A Python statement of the VCF writer's per-record rule (contextsv_amd/csrc/vcf_format_core.hpp; host/vcf_writer.cpp:144-227): lines,
status bytes and counts for a batch of contigs. tests/test_vcf_format_model.py holds it against host.save_vcf and the oracle on the CPU;
the GPU tests compare csvgpu_vcf_format against it, so a disagreement can be located without a device.

A contig is a dict: name (bytes), seq (bytes, or None: the genome has no such record), calls (host.CALL_DTYPE), alts (list of bytes),
depth (uint32 array, or None), gaps (list of (start, end) BED rows in file order)."""
import struct

import numpy as np

WRITTEN, SKIP_UNCLASSIFIED, SKIP_FIRST_POSITION, DISPOSITION, EMPTY_REF, GAP_FILTERED, DEPTH_OUT_OF_RANGE = 0, 1, 2, 3, 4, 8, 16
WHY_LIKELIHOOD, WHY_DEL_LENGTH, WHY_ENUM, WHY_NO_RECORD, WHY_DEL_START, WHY_TEXT_BYTES = 1, 2, 3, 4, 5, 6
METHOD = b"ContextSV v1.0.0"
TYPES = {-1: b"UNKNOWN", 0: b"DEL", 1: b"DUP", 2: b"INV", 3: b"INS", 4: b"BND", 5: b"NEUTRAL", 6: b"LOH"}
GENOTYPES = [b"0/0", b"0/1", b"1/1", b"./."]
EVIDENCE = [b"CIGARINS", b"CIGARDEL", b"CIGARCLIP", b"SPLIT", b"SPLITDIST1", b"SPLITDIST2", b"SPLITINV", b"SUPPINV", b"HMM", b"UNKNOWN"]
MASK = bytes.maketrans(b"RYKMSWBDHVrykmswbdhv", b"N" * 20)
U32 = 0xFFFFFFFF


def i32(x: int) -> int:
    x &= U32
    return x - (1 << 32) if x >= 1 << 31 else x


def cut(seq: bytes, pos_start: int, pos_end: int) -> bytes:
    """ReferenceGenome::query: 1-based inclusive, both decremented with uint32 wrap."""
    ps, pe = (pos_start - 1) & U32, (pos_end - 1) & U32
    return b"" if pe >= len(seq) or ps > pe else seq[ps: pe + 1]


def to_string_double(x: float):
    """std::to_string(double), glibc's "%f"; None where the rule refuses (finite, |x| >= 2^63)."""
    bits = struct.unpack("<Q", struct.pack("<d", x))[0]
    sign = b"-" if bits >> 63 else b""
    if (bits >> 52) & 0x7FF == 0x7FF:
        return sign + (b"nan" if bits & ((1 << 52) - 1) else b"inf")
    if abs(x) >= 2.0 ** 63:
        return None
    return ("%f" % x).encode()                            # (Python rounds the exact binary value to nearest, ties to even, as glibc does)


def gap_hit(start: int, end: int, sv_length: int, gaps) -> bool:
    for gs, ge in gaps:
        ov_start, ov_end = max(start, (gs + 1) & U32), min(end, (ge + 1) & U32)
        if ov_start <= ov_end:
            n = float(((ov_end - ov_start + 1) & U32))
            ratio = n / sv_length if sv_length else (float("inf") if n > 0 else float("nan"))
            if ratio > 0.2:
                return True
    return False


def decide(call, alt: bytes, seq, gaps, depth):
    """-> (why, status, line or None)"""
    t, g, cn = int(call["sv_type"]), int(call["genotype"]), int(call["cn_state"])
    if not (-1 <= t <= 6 and 0 <= g <= 3 and 0 <= cn <= 6):
        return WHY_ENUM, 0, None
    if t in (-1, 5):
        return 0, SKIP_UNCLASSIFIED, None
    start, end = int(call["start"]), int(call["end"])
    ulen = (end - start + 1) & U32
    sv_length = i32(ulen)
    status = GAP_FILTERED if gap_hit(start, end, sv_length, gaps) else 0
    istart = i32(start)
    if t == 0:
        if ulen > 0x7FFFFFFF:
            return WHY_DEL_LENGTH, 0, None
        if start == 1 << 31:
            return WHY_DEL_START, 0, None
        if seq is None:
            return WHY_NO_RECORD, 0, None
        pos = max(1, istart - 1)
        ref = cut(seq, pos, end)
        if ref:
            alt_out = ref[:1]
        else:
            ref, alt_out, status = b"N", b"<DEL>", status | EMPTY_REF
        svlen, end_out = -sv_length, end
    elif t == 3:
        if istart <= 1:
            return 0, SKIP_FIRST_POSITION | status, None
        if seq is None:
            return WHY_NO_RECORD, 0, None
        pos = start - 1
        ref = cut(seq, pos, pos)
        if ref:
            alt_out = alt if alt == b"<INS>" else ref + alt
        else:
            ref, alt_out, status = b"N", b"<INS>", status | EMPTY_REF
        svlen, end_out = sv_length, pos
    else:
        pos, end_out, svlen, ref, alt_out = start, end, sv_length, b"N", alt
    hmm = to_string_double(float(call["hmm_likelihood"]))
    if hmm is None:
        return WHY_LIKELIHOOD, 0, None
    d = i32(int(depth[pos])) if depth is not None and pos < len(depth) else -1      # (csvgpu_depth_lookup_resident's int32 value)
    if d < 0:
        d, status = 0, status | DEPTH_OUT_OF_RANGE
    aln = b",".join(EVIDENCE[b] for b in range(10) if int(call["aln_flags"]) >> b & 1)
    info = b"END=%d;SVTYPE=%s;SVLEN=%d;SVMETHOD=%s;ALN=%s;HMM=%s;SUPPORT=%d;CLUSTER=%d;ALNOFFSET=%d;CN=%d%s" % (
        end_out, TYPES[t], svlen, METHOD, aln, hmm, d, int(call["cluster_size"]), int(call["aln_offset"]), cn, b";LOH" if cn == 4 else b"")
    return 0, status, (pos, ref.translate(MASK), alt_out, b"AssemblyGap" if status & GAP_FILTERED else b"PASS", info, b"%s:%d" % (GENOTYPES[g], d))


def model(contigs):
    """-> (text or None when the batch is declined, status uint8[n], counts dict). The first refused call, in call order, names the reason."""
    lines, status, why = [], [], 0
    counts = dict(text_bytes=0, n_lines=0, total=0, unclassified=0, gap_filtered=0, declined_why=0)
    for c in contigs:
        for call, alt in zip(c["calls"], c["alts"]):
            w, st, line = decide(call, alt, c["seq"], c.get("gaps") or [], c["depth"])
            status.append(st)
            if w:
                why = why or w
                continue
            if st & DISPOSITION == SKIP_UNCLASSIFIED:
                counts["unclassified"] += 1
            else:
                counts["total"] += 1
            counts["gap_filtered"] += bool(st & GAP_FILTERED)
            if line is not None:
                pos, ref, alt_out, flt, info, sample = line
                lines.append(b"%s\t%d\t.\t%s\t%s\t.\t%s\t%s\tGT:DP\t%s\n" % (c["name"], pos, ref, alt_out, flt, info, sample))
    if why:
        return None, np.array(status, np.uint8), dict(text_bytes=0, n_lines=0, total=0, unclassified=0, gap_filtered=0, declined_why=why)
    text = b"".join(lines)
    counts["text_bytes"], counts["n_lines"] = len(text), len(lines)
    return text, np.array(status, np.uint8), counts


def body_of(vcf: bytes) -> bytes:
    """The record lines of an output.vcf: what lies behind the #CHROM line."""
    mark = b"FORMAT\tSAMPLE\n"
    return vcf[vcf.index(mark) + len(mark):]
