// vcf_record_core.hpp — the decisions of one VCF text line, as the host reader takes them (host/snp_io.cpp: snp_record_of_line,
// af_record_of_line), in a form that compiles with g++ and with hipcc: no allocation, no libc. The device parser (kernels/vcfparse.hip)
// and the stand-alone check (tools/fuzz/vcf_record_core_check.cpp) run the same functions.
//
// A line is KEPT, SKIPPED, or DEFERRED; the population-frequency form can also STOP the file. DEFER is what keeps the result exact: a
// number is converted here only when the conversion provably equals libc's, and a line whose decision hangs on anything else goes back
// to the host reader.
//   integers (POS, the first DP value, the first two AD values): the whole token matches [+-]?[0-9]{1,9}
//   reals (QUAL, the INFO value): the whole token, of at most 64 bytes, matches [+-]?D*(.D*)?([eE][+-]?D+)? with a digit in front of
//     the exponent; the digits without leading zeros are at most 15 (an integer w < 2^53); the exponent less the fraction's length, e, is
//     within +-22 (10^|e| is a double). The value is the one correctly rounded operation w * 10^e or w / 10^-e, which equals a correctly
//     rounded strtod (Clinger, "How to read floating point numbers accurately", 1990).
//   more than one sample column: format_ints pads across samples, so the line defers at the first FORMAT lookup it reaches.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define VCF_HD __host__ __device__
#else
#define VCF_HD
#endif

namespace vcfcore {

enum : int { VCF_SKIP = 0, VCF_KEEP = 1, VCF_DEFER = 2, VCF_STOP = 3, VCF_MORE = 4 };   // MORE: af_line_head alone (the INFO search follows)
constexpr int32_t kIntMissing = INT32_MIN;               // bcf_int32_missing
constexpr uint32_t kNone = 0xffffffffu;
constexpr uint32_t kMaxRealToken = 64;
constexpr int kSnpTabs = 10, kAfTabs = 7;                 // tabs the two forms look for: 9 fields + a second sample's; CHROM..FILTER

struct Rec { uint32_t pos = 0, chrom_len = 0; double value = 0; };

VCF_HD inline bool bytes_eq(const uint8_t *p, uint32_t n, const char *s, uint32_t m)
{
    if (n != m) return false;
    for (uint32_t i = 0; i < n; i++) if (p[i] != (uint8_t)s[i]) return false;
    return true;
}
VCF_HD inline bool is_digit(uint8_t c) { return c >= '0' && c <= '9'; }

// [+-]?[0-9]{1,9}
VCF_HD inline bool tok_int(const uint8_t *p, uint32_t n, int64_t &v)
{
    uint32_t i = 0;
    bool neg = false;
    if (n && (p[0] == '+' || p[0] == '-')) { neg = p[0] == '-'; i = 1; }
    if (n - i < 1 || n - i > 9) return false;
    int64_t a = 0;
    for (; i < n; i++) { if (!is_digit(p[i])) return false; a = a * 10 + (p[i] - '0'); }
    v = neg ? -a : a;
    return true;
}

// the real-number rule of the header comment
VCF_HD inline bool tok_real(const uint8_t *p, uint32_t n, double &v)
{
    const double p10[23] = {1e0, 1e1, 1e2, 1e3, 1e4, 1e5, 1e6, 1e7, 1e8, 1e9, 1e10, 1e11, 1e12, 1e13, 1e14, 1e15, 1e16, 1e17, 1e18, 1e19, 1e20, 1e21, 1e22};
    if (n == 0 || n > kMaxRealToken) return false;
    uint32_t i = 0;
    bool neg = false;
    if (p[0] == '+' || p[0] == '-') { neg = p[0] == '-'; i = 1; }
    uint64_t w = 0;
    int n_sig = 0, n_dig = 0, n_frac = 0;
    for (; i < n && is_digit(p[i]); i++) { n_dig++; if (w || p[i] != '0') { w = w * 10 + (p[i] - '0'); if (++n_sig > 15) return false; } }
    if (i < n && p[i] == '.') {
        for (i++; i < n && is_digit(p[i]); i++) { n_dig++; n_frac++; if (w || p[i] != '0') { w = w * 10 + (p[i] - '0'); if (++n_sig > 15) return false; } }
    }
    if (n_dig == 0) return false;
    int ex = 0;
    if (i < n && (p[i] == 'e' || p[i] == 'E')) {
        i++;
        bool eneg = false;
        if (i < n && (p[i] == '+' || p[i] == '-')) { eneg = p[i] == '-'; i++; }
        if (i >= n) return false;
        for (; i < n; i++) { if (!is_digit(p[i])) return false; if (ex < 100000) ex = ex * 10 + (p[i] - '0'); }
        if (eneg) ex = -ex;
    }
    if (i != n) return false;
    const int e = ex - n_frac;
    if (e < -22 || e > 22) return false;
    const double d = e >= 0 ? (double)w * p10[e] : (double)w / p10[-e];
    v = neg ? -d : d;
    return true;
}

// the first `want` tabs of a line -> how many there are (at most want)
VCF_HD inline int find_tabs(const uint8_t *p, uint32_t len, uint32_t *tab, int want)
{
    int n = 0;
    for (uint32_t i = 0; i < len && n < want; i++) if (p[i] == '\t') tab[n++] = i;
    return n;
}

// bcf_is_snp: every allele is one base other than '*', or the symbolic <X> / <*>; ALT "." has no allele
VCF_HD inline bool allele_is_base(const uint8_t *p, uint32_t n) { return (n == 1 && p[0] != '*') || bytes_eq(p, n, "<X>", 3) || bytes_eq(p, n, "<*>", 3); }
VCF_HD inline bool is_snp(const uint8_t *ref, uint32_t n_ref, const uint8_t *alt, uint32_t n_alt)
{
    if (!allele_is_base(ref, n_ref)) return false;
    if (n_alt == 1 && alt[0] == '.') return true;
    uint32_t a = 0;
    for (;;) {
        uint32_t c = a;
        while (c < n_alt && alt[c] != ',') {
            if (c - a >= 3) return false;                 // an allele of four bytes or more is none of the three forms
            c++;
        }
        if (!allele_is_base(alt + a, c - a)) return false;
        if (c >= n_alt) return true;
        a = c + 1;
    }
}

// index of `key` (two bytes) among the ':'-separated FORMAT keys, first match, or -1
VCF_HD inline int format_index(const uint8_t *f, uint32_t n, const char *key)
{
    int idx = 0;
    uint32_t a = 0;
    for (;;) {
        uint32_t c = a;
        while (c < n && f[c] != ':') c++;
        if (c - a == 2 && f[a] == (uint8_t)key[0] && f[a + 1] == (uint8_t)key[1]) return idx;
        if (c >= n) return -1;
        a = c + 1;
        idx++;
    }
}

// field `idx` of the one sample column [s, s + n): its start and length (length 0 when the sample has fewer fields)
VCF_HD inline void sample_field(const uint8_t *s, uint32_t n, int idx, uint32_t &at, uint32_t &flen)
{
    uint32_t a = 0;
    for (int i = 0; i < idx; i++) {
        while (a < n && s[a] != ':') a++;
        if (a >= n) { at = n; flen = 0; return; }
        a++;
    }
    uint32_t c = a;
    while (c < n && s[c] != ':') c++;
    at = a; flen = c - a;
}

// one value of an integer FORMAT field: "" / "." -> missing; false: the token is outside the integer rule
VCF_HD inline bool format_int(const uint8_t *p, uint32_t n, int32_t &v)
{
    if (n == 0 || (n == 1 && p[0] == '.')) { v = kIntMissing; return true; }
    int64_t w;
    if (!tok_int(p, n, w)) return false;
    v = (int32_t)w;
    return true;
}

// ---- the sample's SNP records (SNPFile::load): tab[0 .. n_tab) from find_tabs(.., kSnpTabs)
VCF_HD inline int snp_line_tabs(const uint8_t *p, uint32_t len, const uint32_t *tab, int n_tab, bool dp_int, bool ad_int, Rec &r)
{
    if (n_tab < 8) return VCF_SKIP;                                        // fewer than 9 fields
    const uint8_t *ref = p + tab[2] + 1, *alt = p + tab[3] + 1, *qual = p + tab[4] + 1, *flt = p + tab[5] + 1, *fmt = p + tab[7] + 1;
    const uint32_t n_ref = tab[3] - tab[2] - 1, n_alt = tab[4] - tab[3] - 1, n_qual = tab[5] - tab[4] - 1, n_flt = tab[6] - tab[5] - 1;
    const uint32_t fmt_end = n_tab >= 9 ? tab[8] : len, n_fmt = fmt_end - tab[7] - 1;
    const uint8_t *smp = n_tab >= 9 ? p + tab[8] + 1 : p + len;
    const uint32_t n_smp = n_tab >= 9 ? len - tab[8] - 1 : 0;
    const bool more_samples = n_tab >= 10;
    if (!is_snp(ref, n_ref, alt, n_alt)) return VCF_SKIP;
    if (n_qual == 1 && qual[0] == '.') return VCF_SKIP;
    double q;
    if (!tok_real(qual, n_qual, q)) return VCF_DEFER;
    if ((float)q <= 30) return VCF_SKIP;
    if (!dp_int) return VCF_SKIP;
    int idx = format_index(fmt, n_fmt, "DP");
    if (idx < 0) return VCF_SKIP;
    if (more_samples) return VCF_DEFER;
    uint32_t at, fl;
    sample_field(smp, n_smp, idx, at, fl);
    {
        uint32_t c = 0;
        while (c < fl && smp[at + c] != ',') c++;
        int32_t dp;
        if (!format_int(smp + at, c, dp)) return VCF_DEFER;
        if (dp <= 10) return VCF_SKIP;
    }
    if (!(n_flt == 1 && flt[0] == '.') && !bytes_eq(flt, n_flt, "PASS", 4)) {
        bool pass = false;
        uint32_t a = 0;
        for (;;) {
            uint32_t c = a;
            while (c < n_flt && flt[c] != ';') c++;
            if (bytes_eq(flt + a, c - a, "PASS", 4)) pass = true;
            if (c >= n_flt) break;
            a = c + 1;
        }
        if (!pass) return VCF_SKIP;
    }
    if (!ad_int) return VCF_SKIP;
    idx = format_index(fmt, n_fmt, "AD");
    if (idx < 0) return VCF_SKIP;
    sample_field(smp, n_smp, idx, at, fl);
    uint32_t c0 = 0;
    while (c0 < fl && smp[at + c0] != ',') c0++;
    if (c0 >= fl) return VCF_SKIP;                                         // one value (or none): ad.size() < 2
    uint32_t c1 = c0 + 1;
    while (c1 < fl && smp[at + c1] != ',') c1++;
    int32_t ad0, ad1;
    if (!format_int(smp + at, c0, ad0) || !format_int(smp + at + c0 + 1, c1 - c0 - 1, ad1)) return VCF_DEFER;
    int64_t pos;
    if (!tok_int(p + tab[0] + 1, tab[1] - tab[0] - 1, pos)) return VCF_DEFER;
    r.value = (double)ad1 / (double)(int32_t)((uint32_t)ad0 + (uint32_t)ad1);
    r.pos = (uint32_t)pos;
    r.chrom_len = tab[0];
    return VCF_KEEP;
}

VCF_HD inline int vcf_snp_line(const uint8_t *p, uint32_t len, bool dp_int, bool ad_int, Rec &r)
{
    uint32_t tab[kSnpTabs];
    const int n = find_tabs(p, len, tab, kSnpTabs);
    return snp_line_tabs(p, len, tab, n, dp_int, ad_int, r);
}

// ---- the population file's records (SNPFile::table): tab[0 .. n_tab) from find_tabs(.., kAfTabs)
// Everything in front of INFO: SKIP / DEFER / STOP, or MORE with r.pos set (the INFO field starts at tab[6] + 1).
VCF_HD inline int af_line_head(const uint8_t *p, uint32_t len, const uint32_t *tab, int n_tab, const uint8_t *contig, uint32_t contig_len,
                               const uint32_t *sorted_pos, uint64_t n, uint32_t last_pos, Rec &r)
{
    if (n_tab < 7) return VCF_SKIP;                                        // fewer than 8 fields
    if (tab[0] != contig_len) return VCF_SKIP;
    for (uint32_t i = 0; i < contig_len; i++) if (p[i] != contig[i]) return VCF_SKIP;
    int64_t pos;
    if (!tok_int(p + tab[0] + 1, tab[1] - tab[0] - 1, pos)) return VCF_DEFER;
    const uint32_t q = (uint32_t)pos;
    if (q > last_pos) return VCF_STOP;
    uint64_t lo = 0, hi = n;
    while (lo < hi) { const uint64_t mid = (lo + hi) / 2; if (sorted_pos[mid] < q) lo = mid + 1; else hi = mid; }
    if (lo >= n || sorted_pos[lo] != q) return VCF_SKIP;
    if (!is_snp(p + tab[2] + 1, tab[3] - tab[2] - 1, p + tab[3] + 1, tab[4] - tab[3] - 1)) return VCF_SKIP;
    r.pos = q;
    r.chrom_len = tab[0];
    return VCF_MORE;
}

// whether the needle stands at p[k ..) inside [info, info_end), at the field's start or behind ';'
VCF_HD inline bool needle_at(const uint8_t *p, uint32_t info, uint32_t info_end, uint32_t k, const uint8_t *needle, uint32_t needle_len)
{
    if (k < info || k + needle_len > info_end || (k != info && p[k - 1] != ';')) return false;
    for (uint32_t i = 0; i < needle_len; i++) if (p[k + i] != needle[i]) return false;
    return true;
}

// the value behind the needle found at k (kNone: not found) -> SKIP / KEEP / DEFER
VCF_HD inline int af_line_value(const uint8_t *p, uint32_t info_end, uint32_t k, uint32_t needle_len, Rec &r)
{
    if (k == kNone) return VCF_SKIP;
    const uint32_t a = k + needle_len;
    uint32_t e = a;
    while (e < info_end && p[e] != ';' && p[e] != ',') e++;
    if (e == a) return VCF_SKIP;
    if (e - a == 1 && p[a] == '.') {
        const uint64_t bits = 0x7ff8000000000000ull;                      // NaN: passes both comparisons, as on the host
        union { uint64_t u; double d; } x;
        x.u = bits;
        r.value = x.d;
        return VCF_KEEP;
    }
    double d;
    if (!tok_real(p + a, e - a, d)) return VCF_DEFER;
    const double v = (double)(float)d;
    if (v <= 0.01 || v >= 0.99) return VCF_SKIP;
    r.value = v;
    return VCF_KEEP;
}

VCF_HD inline int vcf_af_line(const uint8_t *p, uint32_t len, const uint8_t *contig, uint32_t contig_len, const uint8_t *needle, uint32_t needle_len,
                              const uint32_t *sorted_pos, uint64_t n, uint32_t last_pos, Rec &r)
{
    uint32_t tab[kAfTabs];
    const int nt = find_tabs(p, len, tab, kAfTabs);
    const int code = af_line_head(p, len, tab, nt, contig, contig_len, sorted_pos, n, last_pos, r);
    if (code != VCF_MORE) return code;
    const uint32_t info = tab[6] + 1;
    uint32_t info_end = info;
    while (info_end < len && p[info_end] != '\t') info_end++;
    uint32_t k = kNone;
    for (uint32_t i = info; i + needle_len <= info_end; i++) if (needle_at(p, info, info_end, i, needle, needle_len)) { k = i; break; }
    return af_line_value(p, info_end, k, needle_len, r);
}

}  // namespace vcfcore
