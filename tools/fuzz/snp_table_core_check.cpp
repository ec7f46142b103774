// snp_table_core_check.cpp — the per-region rules of a resident SNP table (contextsv_amd/csrc/snp_table_core.hpp) on the CPU, against the
// host mirror's two SNPSource forms: SNPTable::queryFlat (the per-record kind) and the default SNPSource::queryFlat over
// SNPFileTable::query (the first-hit kind). A program of its own, built with AddressSanitizer + UBSan
// (make -C contextsv_amd/csrc snp-table-check; driven by tests/test_snp_table_core.py). The header's rules are applied the way the kernels of
// kernels/snptable.hip apply them: a table is resolved once (run ends by binary search, the runs' pfb from an inclusive prefix maximum over
// the marks), a region is a range, and its records are gathered with the hit's rule; every array lives in a heap block of exactly its size.
//
//   snp_table_core_check [n_random_tables] [regions_per_table]
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <random>
#include <vector>

#include "../../contextsv_amd/csrc/host/cnv_caller.h"
#include "../../contextsv_amd/csrc/host/snp_io.h"
#include "../../contextsv_amd/csrc/snp_table_core.hpp"

static long g_fail = 0, g_tables = 0, g_regions = 0, g_records = 0;
#define CHECK(c, ...) do { if (!(c)) { if (g_fail < 20) { fprintf(stderr, "FAIL: " __VA_ARGS__); fprintf(stderr, "\n"); } g_fail++; } } while (0)

static uint64_t bits(double v) { uint64_t b; memcpy(&b, &v, 8); return b; }
static double from_bits(uint64_t b) { double v; memcpy(&v, &b, 8); return v; }
static const uint32_t POS_MAX = 0x7ffffffeu;

// exact-size heap copies: a read past an array's end is the sanitizer's
template <class T> struct Exact {
    T *p; size_t n;
    explicit Exact(const std::vector<T> &v) : p(v.empty() ? nullptr : (T *)malloc(v.size() * sizeof(T))), n(v.size()) { if (n) memcpy(p, v.data(), n * sizeof(T)); }
    ~Exact() { free(p); }
    Exact(const Exact &) = delete;
};

// what the device holds for a table, made the way launch_snp_resolve makes it
struct Resolved { std::vector<uint64_t> baf, pfb; };
static Resolved resolve(const uint32_t *pos, const uint64_t *baf, const uint64_t *pfb, const uint8_t *has, uint32_t n, bool want_pfb)
{
    Resolved r;
    r.baf.resize(n); if (want_pfb) r.pfb.assign(n, 0);
    std::vector<int32_t> pm(n);
    if (want_pfb && has) {
        int32_t run = INT32_MIN;
        for (uint32_t i = 0; i < n; i++) { run = std::max(run, snpcore::mark(i, has[i] != 0)); pm[i] = run; }       // (launch_prefix_max: inclusive)
    }
    for (uint32_t i = 0; i < n; i++) {
        const uint32_t j = snpcore::run_last(pos, n, i);
        r.baf[i] = baf[j];
        if (want_pfb) r.pfb[i] = has ? snpcore::resolved_pfb_bits(pos, pfb, i, pm[j]) : 0;
    }
    return r;
}

struct Flat { std::vector<uint32_t> pos; std::vector<uint64_t> baf, pfb; };
static Flat host_flat(const SNPSource &s, uint32_t start, uint32_t end)
{
    std::vector<uint32_t> p; std::vector<double> b, f;
    s.queryFlat(start, end, p, b, f);
    Flat o; o.pos = p;
    for (double v : b) o.baf.push_back(bits(v));
    for (double v : f) o.pfb.push_back(bits(v));
    return o;
}
static void same(const Flat &got, const Flat &want, const char *kind, uint32_t start, uint32_t end)
{
    CHECK(got.pos == want.pos, "%s [%u, %u]: %zu positions, the host gives %zu", kind, start, end, got.pos.size(), want.pos.size());
    CHECK(got.baf == want.baf, "%s [%u, %u]: baf differs", kind, start, end);
    CHECK(got.pfb == want.pfb, "%s [%u, %u]: pfb differs", kind, start, end);
    g_regions++; g_records += (long)want.pos.size();
}

static void check_records(const SNPTable &t, const std::vector<std::pair<uint32_t, uint32_t>> &regions)
{
    const uint32_t n = (uint32_t)t.pos.size();
    std::vector<uint64_t> bb, fb;
    for (double v : t.baf) bb.push_back(bits(v));
    for (double v : t.pfb) fb.push_back(bits(v));
    Exact<uint32_t> pos(t.pos); Exact<uint64_t> baf(bb), pfb(fb); Exact<uint8_t> has(t.has_pfb);
    const Resolved r = resolve(pos.p, baf.p, pfb.p, t.has_pfb.empty() ? nullptr : has.p, n, true);
    Exact<uint64_t> rbaf(r.baf), rpfb(r.pfb);
    g_tables++;
    for (const auto &reg : regions) {
        uint32_t first, count;
        snpcore::range(pos.p, n, reg.first, reg.second, first, count);
        CHECK((uint64_t)first + count <= n, "records [%u, %u]: range leaves the table", reg.first, reg.second);
        Flat got;
        for (uint32_t k = 0; k < count && first + k < n; k++) { got.pos.push_back(pos.p[first + k]); got.baf.push_back(rbaf.p[first + k]); got.pfb.push_back(rpfb.p[first + k]); }
        Flat want;
        if (reg.first <= reg.second) want = host_flat(t, reg.first, reg.second);             // (start > end: the callers filter it; the table yields nothing)
        same(got, want, "records", reg.first, reg.second);
        CHECK(snpcore::window_count(20, count) == (uint32_t)std::max<int64_t>(20, (int64_t)want.pos.size()), "window count");
    }
}

static void check_hits(const SNPFileTable &t, const std::vector<std::pair<uint32_t, uint32_t>> &regions)
{
    const uint32_t n = (uint32_t)t.pos.size(), n_af = (uint32_t)t.af_pos.size();
    std::vector<uint64_t> bb, ab;
    for (double v : t.baf) bb.push_back(bits(v));
    for (double v : t.af) ab.push_back(bits(v));
    Exact<uint32_t> pos(t.pos), af_pos(t.af_pos); Exact<uint64_t> baf(bb), af(ab);
    const Resolved r = resolve(pos.p, baf.p, nullptr, nullptr, n, false);
    Exact<uint64_t> rbaf(r.baf);
    g_tables++;
    for (const auto &reg : regions) {
        uint32_t first, count;
        snpcore::range(pos.p, n, reg.first, reg.second, first, count);
        CHECK((uint64_t)first + count <= n, "hits [%u, %u]: range leaves the table", reg.first, reg.second);
        const uint32_t hit = n_af ? snpcore::first_hit(pos.p, first, count, af_pos.p, n_af) : snpcore::NO_HIT;
        CHECK(hit == snpcore::NO_HIT || hit < n_af, "hits [%u, %u]: hit leaves the table", reg.first, reg.second);
        Flat got;
        for (uint32_t k = 0; k < count && first + k < n; k++) {
            got.pos.push_back(pos.p[first + k]); got.baf.push_back(rbaf.p[first + k]);
            got.pfb.push_back(snpcore::hit_pfb_bits(pos.p[first + k], hit, af_pos.p, af.p));
        }
        Flat want;
        if (reg.first <= reg.second) want = host_flat(t, reg.first, reg.second);
        same(got, want, "hits", reg.first, reg.second);
    }
}

static std::vector<std::pair<uint32_t, uint32_t>> regions_for(const std::vector<uint32_t> &pos, const std::vector<uint32_t> &af_pos, std::mt19937_64 &rng, int n_random)
{
    std::vector<uint32_t> pts = {0, 1, POS_MAX - 1, POS_MAX};
    auto around = [&](uint32_t p) { if (p) pts.push_back(p - 1); pts.push_back(p); if (p < POS_MAX) pts.push_back(p + 1); };
    for (size_t i = 0; i < pos.size(); i += std::max<size_t>(1, pos.size() / 6)) around(pos[i]);
    if (!pos.empty()) around(pos.back());
    for (size_t i = 0; i < af_pos.size(); i += std::max<size_t>(1, af_pos.size() / 4)) around(af_pos[i]);
    std::sort(pts.begin(), pts.end());
    pts.erase(std::unique(pts.begin(), pts.end()), pts.end());
    std::vector<std::pair<uint32_t, uint32_t>> out;
    for (size_t i = 0; i < pts.size(); i++)                                  // a twelfth of the pairs, start == end always, some with start > end
        for (size_t j = 0; j < pts.size(); j++)
            if (i == j || (i < j ? (i + 5 * j) % 12 == 0 : (i * 3 + j) % 23 == 0)) out.emplace_back(pts[i], pts[j]);
    const uint32_t hi = pos.empty() ? 100 : std::min<uint32_t>(POS_MAX, pos.back() + 10);
    for (int k = 0; k < n_random; k++) {
        const uint32_t a = (uint32_t)(rng() % ((uint64_t)hi + 1));
        out.emplace_back(a, (uint32_t)std::min<uint64_t>(POS_MAX, (uint64_t)a + rng() % (hi / 3 + 2)));
    }
    return out;
}

static double value(std::mt19937_64 &rng)
{
    const uint64_t k = rng() % 40;
    if (k == 0) return from_bits(0x7ff8000000001234ull);                      // NaNs with payloads of their own
    if (k == 1) return from_bits(0xfff00000deadbeefull);
    if (k == 2) return -0.0;
    return (double)(rng() % 1000001) / 1000000.0;
}

static std::vector<uint32_t> positions(std::mt19937_64 &rng, size_t n, uint32_t span, int dup_pct)
{
    std::vector<uint32_t> p(n);
    for (auto &x : p) x = (uint32_t)(rng() % ((uint64_t)span + 1));
    std::sort(p.begin(), p.end());
    for (size_t i = 1; i < n; i++) if ((int)(rng() % 100) < dup_pct) p[i] = p[i - 1];
    std::sort(p.begin(), p.end());
    return p;
}

static SNPTable make_records(std::mt19937_64 &rng, size_t n, uint32_t span, int dup_pct, int flag_pct)
{
    SNPTable t;
    t.pos = positions(rng, n, span, dup_pct);
    for (size_t i = 0; i < n; i++) { t.baf.push_back(value(rng)); t.pfb.push_back(value(rng)); t.has_pfb.push_back((int)(rng() % 100) < flag_pct); }
    return t;
}
static SNPFileTable make_hits(std::mt19937_64 &rng, size_t n, size_t n_af, uint32_t span, int dup_pct)
{
    SNPFileTable t;
    t.pos = positions(rng, n, span, dup_pct);
    for (size_t i = 0; i < n; i++) t.baf.push_back(value(rng));
    for (size_t i = 0; i < n_af; i++) t.af_pos.push_back(n && rng() % 2 ? t.pos[rng() % n] : (uint32_t)(rng() % ((uint64_t)span + 1)));
    std::sort(t.af_pos.begin(), t.af_pos.end());
    for (size_t i = 0; i < n_af; i++) t.af.push_back(value(rng));
    return t;
}

int main(int argc, char **argv)
{
    const int n_random = argc > 1 ? atoi(argv[1]) : 3000, per_table = argc > 2 ? atoi(argv[2]) : 40;
    std::mt19937_64 rng(20240611);

    // the families: empty, one record, one position, runs of 2 and 3 with the flag on the first / middle / last / none, the coordinate extremes
    {
        SNPTable t;
        check_records(t, regions_for(t.pos, {}, rng, 10));
        t.pos = {500}; t.baf = {0.25}; t.pfb = {0.7}; t.has_pfb = {1};
        check_records(t, regions_for(t.pos, {}, rng, 10));
        SNPTable one;
        for (int i = 0; i < 300; i++) { one.pos.push_back(1234); one.baf.push_back(i / 300.0); one.pfb.push_back(1.0 - i / 300.0); one.has_pfb.push_back(i == 17); }
        check_records(one, regions_for(one.pos, {}, rng, 10));
        SNPTable runs;
        const int shapes[][4] = {{2, 1, 0, 0}, {2, 0, 1, 0}, {2, 0, 0, 0}, {2, 1, 1, 0}, {3, 1, 0, 0}, {3, 0, 1, 0}, {3, 0, 0, 1}, {3, 0, 0, 0}, {3, 1, 0, 1}};
        uint32_t p = 100;
        for (const auto &s : shapes) {
            for (int k = 0; k < s[0]; k++) { runs.pos.push_back(p); runs.has_pfb.push_back((uint8_t)s[1 + k]); }
            runs.pos.push_back(p + 5); runs.has_pfb.push_back((uint8_t)(s[0] % 2));
            p += 10;
        }
        for (size_t i = 0; i < runs.pos.size(); i++) { runs.baf.push_back((double)i / 64); runs.pfb.push_back(0.5 + (double)i / 256); }
        std::vector<std::pair<uint32_t, uint32_t>> every;
        for (uint32_t a = 95; a < 200; a++) for (uint32_t b = a; b < 200; b += 3) every.emplace_back(a, b);
        check_records(runs, every);
        SNPTable no_flags = runs;
        no_flags.has_pfb.clear();
        check_records(no_flags, regions_for(runs.pos, {}, rng, 20));
        SNPTable ext;
        ext.pos = {0, 0, 7, POS_MAX, POS_MAX}; ext.baf = {0.1, 0.2, value(rng), 0.4, from_bits(0xfff00000deadbeefull)};
        ext.pfb = {0.5, from_bits(0x7ff8000000001234ull), 0.7, 0.8, 0.9}; ext.has_pfb = {1, 1, 0, 1, 0};
        check_records(ext, regions_for(ext.pos, {}, rng, 20));

        SNPFileTable h;
        h.af_pos = {5}; h.af = {0.5};
        check_hits(h, regions_for(h.pos, h.af_pos, rng, 10));
        h.pos = {100, 200, 200, 300, 400, 400, 400, 500}; h.baf = {0.1, 0.2, 0.3, from_bits(0x7ff8000000001234ull), 0.5, 0.6, 0.7, 0.8};
        h.af_pos.clear(); h.af.clear();
        check_hits(h, regions_for(h.pos, h.af_pos, rng, 10));
        // no record of the population file inside [lo, hi]; the first one at lo; at hi; one just outside on each side; a NaN; a hit that is no record
        h.af_pos = {50, 99, 100, 250, 300, 400, 400, 501, 900}; h.af = {0.01, 0.02, 0.03, 0.04, from_bits(0xfff00000deadbeefull), 0.06, 0.07, 0.08, 0.09};
        std::vector<std::pair<uint32_t, uint32_t>> every_h;
        for (uint32_t a = 40; a < 520; a += 7) for (uint32_t b = a; b < 560; b += 11) every_h.emplace_back(a, b);
        for (uint32_t a : {99u, 100u, 101u, 199u, 200u, 201u, 249u, 250u, 251u, 300u, 399u, 400u, 401u, 500u, 501u})
            for (uint32_t b : {100u, 199u, 200u, 250u, 299u, 300u, 400u, 499u, 500u, 501u, 900u}) every_h.emplace_back(a, b);
        check_hits(h, every_h);
        h.pos = {0, 0, POS_MAX}; h.baf = {0.1, 0.2, 0.3}; h.af_pos = {0, POS_MAX}; h.af = {0.4, 0.6};
        check_hits(h, regions_for(h.pos, h.af_pos, rng, 10));
    }

    // random tables: sizes around the wave and workgroup boundaries among them, dense and sparse, with few and many duplicates
    const size_t sizes[] = {0, 1, 2, 3, 63, 64, 65, 255, 256, 257};
    for (int k = 0; k < n_random; k++) {
        const size_t n = k % 3 == 0 ? sizes[(size_t)(k / 3) % 10] : (size_t)(rng() % 400);
        const uint32_t span = k % 5 == 0 ? POS_MAX : (uint32_t)(rng() % (4 * n + 8));
        const int dup = (int)(rng() % 3) * 30, flag = (int)(rng() % 4) * 33;
        if (k % 2 == 0) {
            const SNPTable t = make_records(rng, n, span, dup, flag);
            check_records(t, regions_for(t.pos, {}, rng, per_table));
        } else {
            const SNPFileTable t = make_hits(rng, n, (size_t)(rng() % (n / 2 + 3)), span, dup);
            check_hits(t, regions_for(t.pos, t.af_pos, rng, per_table));
        }
    }
    printf("snp_table_core_check: %ld tables, %ld regions, %ld records, %ld failures\n", g_tables, g_regions, g_records, g_fail);
    return g_fail ? 1 : 0;
}
