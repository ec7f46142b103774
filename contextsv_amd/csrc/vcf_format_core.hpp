// vcf_format_core.hpp — the per-record rule of the VCF writer (host/vcf_writer.cpp:144-227; the reference's SVCaller::saveToVCF,
// sv_caller.cpp:1067-1330, and ::getReadDepth, :1332-1344), stated once for the device (kernels/vcfformat.hip, api/vcf_format.hip) and for the
// CPU check (tools/fuzz/vcf_format_core_check.cpp). Compiles with g++ alone; no allocation, no std::string.
//   Disposition   by the order of writeVCF's loop: the enums are looked up first (a value outside its table refuses the batch: the host
//                 throws), UNKNOWN / NEUTRAL are skipped and counted as unclassified, every other call is counted in total and run against the
//                 contig's gap rows, and an INS with (int)start <= 1 then leaves without a line.
//   Fields        POS / END / SVLEN with preceding = max(1, (int)start - 1); REF is the cut [preceding, end] (DEL) or [start - 1, start - 1]
//                 (INS) by ReferenceGenome::query's rule, "N" where that is empty and for every other type; ALT takes REF's first base before
//                 REF is masked. SUPPORT and DP are the depth at POS, 0 where POS lies outside the map.
//   A line        one function, emit_line, over a sink: a counting sink gives the exact length, a storing sink the bytes, a window sink the
//                 bytes of one piece of the output. What a sink is given never depends on the sink, so the length is the text's.
//   %f            std::to_string(double) in integers: fmt_f6.
//   Refused       what the host cannot print without undefined behaviour or an exception, or what this rule does not cover: see Why.
#pragma once
#include <stdint.h>

#include "fasta_core.hpp"

namespace vcffmt {

// csvhost_call's layout (host/abi/csvhost_abi.h), csv_vcf_call's (include/csvgpu.h)
struct Call {
    uint32_t start, end;
    int32_t sv_type, cluster_size;
    double hmm_likelihood;
    int64_t id;
    uint32_t aln_flags;
    int32_t genotype, cn_state, aln_offset;
};
static_assert(sizeof(Call) == 48, "csvhost_call's layout");

// the status byte of a call: its disposition in the low two bits, flags above
enum : uint8_t { WRITTEN = 0, SKIP_UNCLASSIFIED = 1, SKIP_FIRST_POSITION = 2, DISPOSITION = 3, EMPTY_REF = 4, GAP_FILTERED = 8, DEPTH_OUT_OF_RANGE = 16 };
// why a batch is declined (0: it is not)
enum Why : uint32_t {
    WHY_NONE = 0,
    WHY_LIKELIHOOD = 1,      // a written line's likelihood is finite with |x| >= 2^63
    WHY_DEL_LENGTH = 2,      // a DEL whose end - start + 1 (uint32) does not fit a positive int: the host negates it
    WHY_ENUM = 3,            // sv_type outside -1..6, genotype outside 0..3, cn_state outside 0..6: the host throws
    WHY_NO_RECORD = 4,       // a DEL, or an INS with (int)start > 1, on a contig the genome has not: the host's queryMany throws
    WHY_DEL_START = 5,       // a DEL at start == 2^31: (int)start - 1 overflows on the host
    WHY_TEXT_BYTES = 6,      // the text has 2^32 bytes or more
};

constexpr uint32_t kMethodMax = 64;                       // bytes of the SVMETHOD string the entry point takes

enum : uint8_t { REF_GENOME = 0, REF_N = 1 };
enum : uint8_t { ALT_CALLER = 0, ALT_BASE = 1, ALT_BASE_CALLER = 2, ALT_DEL_SYMBOL = 3, ALT_INS_SYMBOL = 4 };

struct Line {
    uint8_t status = 0, why = 0, ref_kind = REF_N, alt_kind = ALT_CALLER;
    uint8_t gap_hit = 0;                                  // a gap row matched (also for a first-position INS: the host counts it before it leaves)
    uint32_t pos = 0, end = 0;
    int32_t svlen = 0;
    uint32_t ref_first = 0, ref_len = 1;                  // REF_GENOME: the cut's first byte in the contig, its bytes
    uint32_t depth = 0;                                   // as printed
};

FA_HD inline uint32_t dec_digits_u32(uint32_t v)
{
    uint32_t n = 1;
    while (v >= 10) { v /= 10; n++; }
    return n;
}
FA_HD inline uint32_t dec_chars_i32(int32_t v) { return v < 0 ? 1 + dec_digits_u32(0u - (uint32_t)v) : dec_digits_u32((uint32_t)v); }

FA_HD inline const char *type_string(int32_t t)
{
    switch (t) {
    case -1: return "UNKNOWN"; case 0: return "DEL"; case 1: return "DUP"; case 2: return "INV"; case 3: return "INS"; case 4: return "BND";
    case 5: return "NEUTRAL"; default: return "LOH";
    }
}
FA_HD inline const char *genotype_string(int32_t g) { return g == 0 ? "0/0" : g == 1 ? "0/1" : g == 2 ? "1/1" : "./."; }
FA_HD inline const char *evidence_name(int bit)
{
    switch (bit) {
    case 0: return "CIGARINS"; case 1: return "CIGARDEL"; case 2: return "CIGARCLIP"; case 3: return "SPLIT"; case 4: return "SPLITDIST1";
    case 5: return "SPLITDIST2"; case 6: return "SPLITINV"; case 7: return "SUPPINV"; case 8: return "HMM"; default: return "UNKNOWN";
    }
}

FA_HD inline uint64_t double_bits(double x)
{
    uint64_t b;
    __builtin_memcpy(&b, &x, 8);
    return b;
}
// finite with |x| >= 2^63: fmt_f6 does not print it
FA_HD inline bool f6_refused(double x)
{
    const uint32_t e = (uint32_t)(double_bits(x) >> 52) & 0x7ff;
    return e != 0x7ff && e >= 1023 + 63;
}

// ---- sinks: put(byte) and bytes(p, n, mask) in the line's order
struct CountSink {
    uint64_t at = 0;
    FA_HD void put(uint8_t) { at++; }
    FA_HD void bytes(const uint8_t *, uint64_t n, bool) { at += n; }
    FA_HD bool done() const { return false; }
};
// stores the bytes whose offset lies in [lo, hi): out[offset]. `at` starts at the line's offset in the text.
struct WindowSink {
    uint8_t *out;
    uint64_t at, lo, hi;
    FA_HD void put(uint8_t c) { if (at >= lo && at < hi) out[at] = c; at++; }
    FA_HD void bytes(const uint8_t *p, uint64_t n, bool mask)
    {
        const uint64_t a = at > lo ? at : lo, b = at + n < hi ? at + n : hi;
        for (uint64_t o = a; o < b; o++) { const uint8_t c = p[o - at]; out[o] = mask ? fastacore::mask_base(c) : c; }
        at += n;
    }
    FA_HD bool done() const { return at >= hi; }
};

template <class Sink> FA_HD inline void put_str(Sink &s, const char *t) { while (*t) s.put((uint8_t)*t++); }
template <class Sink> FA_HD inline void put_u64(Sink &s, uint64_t v)
{
    char d[20];
    int n = 0;
    do { d[n++] = (char)('0' + v % 10); v /= 10; } while (v);
    while (n) s.put((uint8_t)d[--n]);
}
template <class Sink> FA_HD inline void put_i32(Sink &s, int32_t v)
{
    if (v < 0) { s.put('-'); put_u64(s, (uint64_t)(0u - (uint32_t)v)); } else put_u64(s, (uint64_t)v);
}

// glibc's "%f" of x, for x not f6_refused: sign, integer part, the fraction times 10^6 rounded to nearest, ties to even, on the exact binary value
template <class Sink> FA_HD inline void fmt_f6(Sink &s, double x)
{
    const uint64_t b = double_bits(x);
    const uint32_t ef = (uint32_t)(b >> 52) & 0x7ff;
    uint64_t m = b & ((1ull << 52) - 1);
    if (b >> 63) s.put('-');
    if (ef == 0x7ff) { put_str(s, m ? "nan" : "inf"); return; }
    uint64_t ip = 0, fr = 0;                              // integer part, round(fraction * 10^6)
    const int e = (int)ef - 1023;                         // the value is (2^52 + m) * 2^(e - 52) (a denormal is far below 2^-21)
    if (ef != 0 && e >= -21) {
        m |= 1ull << 52;
        if (e >= 52) ip = m << (e - 52);                  // (e <= 62: below 2^63)
        else {
            const int sh = 52 - e;                        // 1 .. 73 fraction bits
            const uint64_t f = sh >= 64 ? m : m & ((1ull << sh) - 1);
            ip = sh >= 64 ? 0 : m >> sh;
            // f * 10^6 as (hi, lo): f < 2^53, the product below 2^73
            const uint64_t p_lo = (f & 0xffffffffull) * 1000000ull, p_hi = (f >> 32) * 1000000ull;      // < 2^52, < 2^41
            const uint64_t lo = p_lo + (p_hi << 32), hi = (p_hi >> 32) + (lo < p_lo ? 1 : 0);
            // q = product >> sh, with the bit below and whether anything lies under that
            uint64_t q, half, sticky;
            if (sh < 64) {
                q = (lo >> sh) | (hi << (64 - sh));
                half = (lo >> (sh - 1)) & 1;
                sticky = lo & ((1ull << (sh - 1)) - 1);
            } else {
                q = hi >> (sh - 64);
                half = sh == 64 ? lo >> 63 : (hi >> (sh - 65)) & 1;
                sticky = sh == 64 ? lo & ~(1ull << 63) : (lo | (hi & ((1ull << (sh - 65)) - 1)));
            }
            if (half && (sticky || (q & 1))) q++;
            if (q == 1000000) { q = 0; ip++; }
            fr = q;
        }
    }
    put_u64(s, ip);
    s.put('.');
    for (uint32_t div = 100000; div; div /= 10) s.put((uint8_t)('0' + fr / div % 10));
}

FA_HD inline bool alt_is_ins_symbol(const uint8_t *alt, uint64_t n) { return n == 5 && alt[0] == '<' && alt[1] == 'I' && alt[2] == 'N' && alt[3] == 'S' && alt[4] == '>'; }

// The call's disposition, flags and fields. contig_len: the contig's length in the genome, -1: the genome has no such record. gap_start /
// gap_end: the contig's BED rows in file order. alt: the caller's ALT string. The depth is not in it yet (set_depth): it is read at L.pos.
FA_HD inline Line decide(const Call &c, int64_t contig_len, const uint32_t *gap_start, const uint32_t *gap_end, uint32_t n_gaps, const uint8_t *alt, uint64_t alt_len)
{
    Line L;
    if (c.sv_type < -1 || c.sv_type > 6 || c.genotype < 0 || c.genotype > 3 || c.cn_state < 0 || c.cn_state > 6) { L.why = WHY_ENUM; return L; }
    if (c.sv_type == -1 || c.sv_type == 5) { L.status = SKIP_UNCLASSIFIED; return L; }
    const uint32_t start = c.start, end = c.end, ulen = end - start + 1;
    const int32_t sv_length = (int32_t)ulen;
    for (uint32_t g = 0; g < n_gaps; g++) {
        const uint32_t gs = gap_start[g] + 1, ge = gap_end[g] + 1;
        const uint32_t ov_start = start > gs ? start : gs, ov_end = end < ge ? end : ge;
        if (ov_start <= ov_end && (double)(ov_end - ov_start + 1) / (double)sv_length > 0.2) { L.gap_hit = 1; break; }
    }
    if (L.gap_hit) L.status |= GAP_FILTERED;
    const int64_t istart = (int32_t)start;                // the host's (int)start
    if (c.sv_type == 0) {
        if (ulen > 0x7fffffffu) { L.why = WHY_DEL_LENGTH; return L; }
        if (start == 0x80000000u) { L.why = WHY_DEL_START; return L; }
        if (contig_len < 0) { L.why = WHY_NO_RECORD; return L; }
        const uint32_t preceding = istart - 1 < 1 ? 1u : (uint32_t)(istart - 1);
        L.ref_len = fastacore::cut_len((uint32_t)contig_len, preceding, end, L.ref_first);
        if (L.ref_len) { L.ref_kind = REF_GENOME; L.alt_kind = ALT_BASE; }
        else { L.ref_len = 1; L.alt_kind = ALT_DEL_SYMBOL; L.status |= EMPTY_REF; }
        L.svlen = (int32_t)(0u - ulen);
        L.pos = preceding; L.end = end;
    } else if (c.sv_type == 3) {
        if (istart <= 1) { L.status = (uint8_t)(SKIP_FIRST_POSITION | (L.status & GAP_FILTERED)); return L; }
        if (contig_len < 0) { L.why = WHY_NO_RECORD; return L; }
        L.pos = start - 1;
        L.ref_len = fastacore::cut_len((uint32_t)contig_len, L.pos, L.pos, L.ref_first);
        if (L.ref_len) { L.ref_kind = REF_GENOME; L.alt_kind = alt_is_ins_symbol(alt, alt_len) ? ALT_CALLER : ALT_BASE_CALLER; }
        else { L.ref_len = 1; L.alt_kind = ALT_INS_SYMBOL; L.status |= EMPTY_REF; }
        L.svlen = sv_length;
        L.end = L.pos;
    } else {
        L.pos = start; L.end = end; L.svlen = sv_length;  // DUP / INV / BND / LOH: REF "N", the caller's ALT
    }
    if (f6_refused(c.hmm_likelihood)) L.why = WHY_LIKELIHOOD;
    return L;
}

// depth: the map's value at L.pos, negative: outside the map
FA_HD inline void set_depth(Line &L, int32_t depth)
{
    if (depth < 0) { L.status |= DEPTH_OUT_OF_RANGE; L.depth = 0; } else L.depth = (uint32_t)depth;
}

// where the fields of a written line begin (and the line's length), from the same emission that writes them
struct Layout { uint64_t pos = 0, ref = 0, alt = 0, filter = 0, info = 0, format = 0, len = 0; };

// The line of a WRITTEN call. ref_src: the genome's byte at the cut's first base (REF_GENOME; not read otherwise). Returns nothing: the
// sink has the bytes. lay: the fields' offsets relative to the sink's position on entry, or null.
template <class Sink>
FA_HD inline void emit_line(Sink &s, const Call &c, const Line &L, const uint8_t *name, uint32_t name_len, const uint8_t *ref_src, const uint8_t *alt, uint64_t alt_len,
                            const uint8_t *method, uint32_t method_len, Layout *lay = nullptr)
{
    const uint64_t at0 = s.at;
    s.bytes(name, name_len, false);
    s.put('\t');
    if (lay) lay->pos = s.at - at0;
    put_u64(s, L.pos);
    put_str(s, "\t.\t");
    if (lay) lay->ref = s.at - at0;
    if (L.ref_kind == REF_GENOME) s.bytes(ref_src, L.ref_len, true); else s.put('N');
    s.put('\t');
    if (lay) lay->alt = s.at - at0;
    switch (L.alt_kind) {
    case ALT_BASE: s.bytes(ref_src, 1, false); break;
    case ALT_BASE_CALLER: s.bytes(ref_src, 1, false); s.bytes(alt, alt_len, false); break;
    case ALT_DEL_SYMBOL: put_str(s, "<DEL>"); break;
    case ALT_INS_SYMBOL: put_str(s, "<INS>"); break;
    default: s.bytes(alt, alt_len, false); break;
    }
    if (s.done()) return;                                 // (a window that ends in front of the short fields; never a counting sink)
    put_str(s, "\t.\t");
    if (lay) lay->filter = s.at - at0;
    put_str(s, L.gap_hit ? "AssemblyGap" : "PASS");
    s.put('\t');
    if (lay) lay->info = s.at - at0;
    put_str(s, "END="); put_u64(s, L.end);
    put_str(s, ";SVTYPE="); put_str(s, type_string(c.sv_type));
    put_str(s, ";SVLEN="); put_i32(s, L.svlen);
    put_str(s, ";SVMETHOD="); s.bytes(method, method_len, false);
    put_str(s, ";ALN=");
    bool first = true;
    for (int bit = 0; bit < 10; bit++)
        if (c.aln_flags >> bit & 1) { if (!first) s.put(','); first = false; put_str(s, evidence_name(bit)); }
    put_str(s, ";HMM="); fmt_f6(s, c.hmm_likelihood);
    put_str(s, ";SUPPORT="); put_u64(s, L.depth);
    put_str(s, ";CLUSTER="); put_i32(s, c.cluster_size);
    put_str(s, ";ALNOFFSET="); put_i32(s, c.aln_offset);
    put_str(s, ";CN="); put_i32(s, c.cn_state);
    if (c.cn_state == 4) put_str(s, ";LOH");
    s.put('\t');
    if (lay) lay->format = s.at - at0;
    put_str(s, "GT:DP\t"); put_str(s, genotype_string(c.genotype)); s.put(':'); put_u64(s, L.depth);
    s.put('\n');
    if (lay) lay->len = s.at - at0;
}

// where REF begins in a WRITTEN call's line (Layout::ref without the emission: the pieces inside a long REF ask only this)
FA_HD inline uint64_t ref_offset(const Line &L, uint32_t name_len) { return (uint64_t)name_len + 1 + dec_digits_u32(L.pos) + 3; }
// a call that asks for a depth value: it is written, unless a value of it is refused
FA_HD inline bool asks_depth(const Call &c) { return c.sv_type != -1 && c.sv_type != 5 && !(c.sv_type == 3 && (int32_t)c.start <= 1); }
// bytes of a line beside its name, REF, ALT and method: the longest the short fields can be
constexpr uint32_t kShortMax = 320;

// the exact byte length of a WRITTEN call's line (no byte of name, genome, ALT or method is read)
FA_HD inline uint64_t line_length(const Call &c, const Line &L, uint32_t name_len, uint64_t alt_len, uint32_t method_len, Layout *lay = nullptr)
{
    CountSink s;
    emit_line(s, c, L, nullptr, name_len, nullptr, nullptr, alt_len, nullptr, method_len, lay);
    return s.at;
}

}  // namespace vcffmt
