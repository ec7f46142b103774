// sort_select_core_check — the lane-wise slot replay (contextsv_amd/csrc/sort_select_core.hpp) on the CPU. A program of its own, built by
// `make -C contextsv_amd/csrc merge-select-check` with g++ under AddressSanitizer + UBSan. It drives the core's rounds the way the kernel
// does — a map over the range, two prefix counts, a scatter of the swapped positions, one swap per pair — but over "virtual lanes", one
// after the other, with the two pair lists in heap blocks of exactly the size the kernel reserves, and holds
//   * the chosen id against std::sort's slot, on the patterns and sizes of tests/test_sort_select.py and on a 200 003-member bucket;
//   * one partition step against lib_unguarded_partition (host/sort_select.h), cut and arrangement, on random ranges with random tie counts;
//   * the partitions of every chain against the library's own loops, a chain that runs into the library's depth limit being declined;
//   * a caller's bound on the partitions: declined exactly when the chain needs more, never answered otherwise.
// Driven by tests/test_merge_select_core.py.
#include <stdint.h>
#include <stdio.h>

#include <algorithm>
#include <random>
#include <string>
#include <vector>

#include "../../contextsv_amd/csrc/host/sort_select.h"
#include "../../contextsv_amd/csrc/sort_select_core.hpp"

namespace ssc = sort_select_core;
using ssc::Ent;

// one partition of [lo + 1, hi) against the pivot at lo, lane by lane; returns the cut
static uint32_t core_partition(Ent *x, uint32_t lo, uint32_t hi)
{
    const uint32_t m = hi - lo - 1, pv = ssc::len_of(x[lo]);
    uint32_t *a_before = new uint32_t[m], *b_after = new uint32_t[m];
    uint32_t *list_a = new uint32_t[m / 2], *list_b = new uint32_t[m / 2];           // no position is in two pairs: K <= m / 2
    uint32_t run = 0;
    for (uint32_t t = 0; t < m; t++) { a_before[t] = run; run += ssc::in_a(ssc::len_of(x[lo + 1 + t]), pv); }
    run = 0;
    for (uint32_t t = m; t-- > 0;) { b_after[t] = run; run += ssc::in_b(ssc::len_of(x[lo + 1 + t]), pv); }
    uint32_t K = 0, cut = hi;
    for (uint32_t t = 0; t < m; t++) {                                               // every lane on its own position
        const uint32_t p = lo + 1 + t, len = ssc::len_of(x[p]);
        const bool a = ssc::in_a(len, pv), b = ssc::in_b(len, pv);
        if (ssc::swaps_a(a, a_before[t], b_after[t])) { list_a[a_before[t]] = p; K++; }
        if (ssc::swaps_b(b, a_before[t], b_after[t])) list_b[b_after[t]] = p;
        if (ssc::cut_candidate(a, b, a_before[t], b_after[t])) cut = std::min(cut, p);
    }
    for (uint32_t k = 0; k < K; k++) std::swap(x[list_a[k]], x[list_b[k]]);          // lane k
    delete[] a_before; delete[] b_after; delete[] list_a; delete[] list_b;
    return cut;
}

struct Chain { uint32_t idx; int rounds; bool declined; };
static Chain core_select(std::vector<Ent> x, uint32_t nth, uint32_t max_partitions)
{
    uint32_t lo = 0, hi = (uint32_t)x.size(), limit = ssc::depth_limit(x.size(), max_partitions);
    int rounds = 0;
    while (hi - lo > ssc::SMALL) {
        if (limit == 0) return Chain{ssc::NONE, rounds, true};
        --limit; rounds++;
        ssc::median_to_first(x.data(), lo, hi);
        ssc::keep_side(lo, hi, core_partition(x.data(), lo, hi), nth);
    }
    uint32_t idx = ssc::NONE;
    for (uint32_t i = lo; i < hi; i++) if (ssc::closing_rank(x.data(), lo, hi, i) == nth - lo) idx = ssc::idx_of(x[i]);
    return Chain{idx, rounds, false};
}

// the library's own chain for the slot (host/sort_select.h's loops): its partitions, or -1 where the depth limit runs out
static int lib_rounds(std::vector<Ent> x, uint32_t nth)
{
    auto cmp = [](Ent a, Ent b) { return ssc::comp(a, b); };
    Ent *lo = x.data(), *hi = x.data() + x.size(), *target = x.data() + nth;
    uint32_t limit = ssc::depth_limit(x.size(), 0);
    int rounds = 0;
    while (hi - lo > (std::ptrdiff_t)ssc::SMALL) {
        if (limit == 0) return -1;
        --limit; rounds++;
        csvhost::lib_move_median_to_first(lo, lo + 1, lo + (hi - lo) / 2, hi - 1, cmp);
        Ent *cut = csvhost::lib_unguarded_partition(lo + 1, hi, lo, cmp);
        if (target >= cut) lo = cut; else hi = cut;
    }
    return rounds;
}

static std::vector<uint32_t> pattern(int which, size_t n, std::mt19937_64 &rng, std::string &name)
{
    std::vector<uint32_t> k(n);
    switch (which) {
        case 0: name = "few_values"; for (auto &v : k) v = (uint32_t)(rng() % 4); break;
        case 1: name = "clip_lengths"; for (auto &v : k) v = 50 + (uint32_t)(rng() % 251); break;
        case 2: name = "random"; for (auto &v : k) v = (uint32_t)(rng() % (1u << 30)); break;
        case 3: name = "all_equal"; for (auto &v : k) v = 7; break;
        case 4: name = "ascending"; for (size_t i = 0; i < n; i++) k[i] = (uint32_t)i; break;
        case 5: name = "descending"; for (size_t i = 0; i < n; i++) k[i] = (uint32_t)(n - 1 - i); break;
        case 6: name = "organ_pipe"; for (size_t i = 0; i < n; i++) k[i] = (uint32_t)(i < n / 2 ? i : n - 1 - i); break;
        case 7: name = "sawtooth"; for (size_t i = 0; i < n; i++) k[i] = (uint32_t)(i % 17); break;
        default: {
            name = "median3_killer_like";
            std::vector<uint32_t> v;
            for (size_t i = 0; i < n; i += 2) v.push_back((uint32_t)i);
            std::vector<uint32_t> odd;
            for (size_t i = 1; i < n; i += 2) odd.push_back((uint32_t)i);
            v.insert(v.end(), odd.rbegin(), odd.rend());
            k.assign(v.begin(), v.begin() + n);
        }
    }
    return k;
}

int main()
{
    std::mt19937_64 rng(20261021);
    unsigned long long n_slots = 0, n_fail = 0, n_lib_limit = 0, n_part = 0, n_bound = 0;
    auto cmp = [](Ent a, Ent b) { return ssc::comp(a, b); };

    // ---- the chosen id against std::sort, every pattern and size
    for (size_t n : {(size_t)2, (size_t)15, (size_t)16, (size_t)17, (size_t)18, (size_t)33, (size_t)100, (size_t)1000, (size_t)4097, (size_t)200003}) {
        for (int which = 0; which < 9; which++) {
            std::string name;
            const std::vector<uint32_t> keys = pattern(which, n, rng, name);
            std::vector<Ent> x(n);
            for (size_t i = 0; i < n; i++) x[i] = ssc::make_ent(keys[i], (uint32_t)i);
            std::vector<Ent> sorted = x;
            std::sort(sorted.begin(), sorted.end(), cmp);
            std::vector<uint32_t> slots;
            if (n <= 100) for (size_t p = 0; p < n; p++) slots.push_back((uint32_t)p);
            else {
                for (size_t p : {(size_t)0, (size_t)1, n / 10, n / 5, n / 2, n - 2, n - 1, (size_t)ssc::nth_of(n)}) slots.push_back((uint32_t)p);
                for (int r = 0; r < 25; r++) slots.push_back((uint32_t)(rng() % n));
            }
            int rmin = 1 << 30, rmax = 0;
            for (uint32_t nth : slots) {
                const Chain c = core_select(x, nth, 0);
                n_slots++;
                rmin = std::min(rmin, c.rounds); rmax = std::max(rmax, c.rounds);
                const int want_rounds = lib_rounds(x, nth);
                if (c.declined != (want_rounds < 0) || (!c.declined && c.rounds != want_rounds)) {
                    if (n_fail++ < 10) printf("MISMATCH: %s n=%zu slot %u: the library's chain takes %d partitions, the core %d (declined %d)\n", name.c_str(), n, nth, want_rounds, c.rounds, (int)c.declined);
                }
                if (c.declined) { n_lib_limit++; continue; }      // (the library heap-sorts here: organ pipe and the interleaved pattern reach it)
                if (c.idx != ssc::idx_of(sorted[nth])) {
                    if (n_fail++ < 10) printf("MISMATCH: %s n=%zu slot %u: std::sort %u, core %u\n", name.c_str(), n, nth, ssc::idx_of(sorted[nth]), c.idx);
                }
                // a caller's bound: declined exactly when the chain needs more partitions, the same answer otherwise
                if (n <= 4097) for (uint32_t bound = 1; bound <= 3; bound++) {
                    const Chain d = core_select(x, nth, bound);
                    n_bound++;
                    if (d.declined != (c.rounds > (int)bound) || (!d.declined && d.idx != c.idx) || (d.declined && d.idx != ssc::NONE)) {
                        if (n_fail++ < 10) printf("MISMATCH: %s n=%zu slot %u bound %u: %d partitions, declined %d\n", name.c_str(), n, nth, bound, c.rounds, (int)d.declined);
                    }
                }
            }
            printf("partitions per chain: %-20s n=%-7zu %d .. %d (library limit %u)\n", name.c_str(), n, rmin, rmax, ssc::depth_limit(n, 0));
        }
    }

    // ---- one partition step against the library's loop: cut and arrangement
    for (int it = 0; it < 20000; it++) {
        const uint32_t n = 17 + (uint32_t)(rng() % (it % 50 == 0 ? 5000 : 64));
        const uint32_t vals = 2 + (uint32_t)(rng() % (it % 2 ? 999 : 6));
        std::vector<Ent> a(n);
        for (uint32_t i = 0; i < n; i++) a[i] = ssc::make_ent((uint32_t)(rng() % vals), i);
        std::vector<Ent> b = a;
        csvhost::lib_move_median_to_first(a.data(), a.data() + 1, a.data() + n / 2, a.data() + n - 1, cmp);
        const uint32_t cut_lib = (uint32_t)(csvhost::lib_unguarded_partition(a.data() + 1, a.data() + n, a.data(), cmp) - a.data());
        ssc::median_to_first(b.data(), 0u, n);
        const uint32_t cut_core = core_partition(b.data(), 0, n);
        n_part++;
        if (cut_lib != cut_core || a != b) {
            if (n_fail++ < 10) printf("MISMATCH: partition of %u members, %u values: cut %u (library) %u (core), arrangement %s\n", n, vals, cut_lib, cut_core, a == b ? "equal" : "differs");
        }
    }

    // ---- mergeSVs' slot as the host computes it
    for (uint64_t sz = 1; sz < 2000000; sz += (sz < 100000 ? 1 : 997)) {
        const uint64_t top = (uint64_t)std::max(1, (int)(sz * 0.2));
        if (ssc::top_of(sz) != top || ssc::nth_of(sz) != top / 2) { if (n_fail++ < 10) printf("MISMATCH: top of %llu\n", (unsigned long long)sz); }
    }

    printf("sort_select_core_check: %llu slots, %llu partitions, %llu bounded chains, %llu declined at the library limit, %llu failures\n", n_slots, n_part, n_bound,
           n_lib_limit, n_fail);
    return n_fail ? 1 : 0;
}
