// checks.cpp — test hooks over the host mirror's own building blocks (sort_select.h, par.h, umap_order.h, fast_inflate.h, shard assignment)
#include <atomic>
#include <thread>

#include "abi.hpp"
#include "../fast_inflate.h"
#include "../par.h"
#include "../sort_select.h"
#include "../umap_order.h"

extern "C" {

// test hook for sort_select.h: ids that std::sort and std_sort_select leave at slot nth when sorting `keys`
// descending by key only (ties make the difference between stable and unstable visible through the ids)
int csvhost_sort_select_check(const uint32_t *keys, uint64_t n, uint64_t nth, int64_t *id_std, int64_t *id_sel)
{
    GUARD({
        std::vector<uint32_t> a(n), b(n);
        for (uint64_t i = 0; i < n; i++) a[i] = b[i] = (uint32_t)i;
        auto cmp = [&](uint32_t x, uint32_t y) { return keys[x] > keys[y]; };
        std::sort(a.begin(), a.end(), cmp);
        *id_std = a[nth];
        *id_sel = *csvhost::std_sort_select(b.data(), b.data() + n, (std::ptrdiff_t)nth, cmp);       // (pointers: the block-wise partition for large ranges)
    })
}

// test hook: one partition step of sort_select.h on ids sorted descending by key — the library's loop and the block-wise form must leave
// the same cut and the same arrangement. *differ = 0 when they agree (ranges of more than 16, as in std::sort: the unguarded loops need the
// median-of-three's sentinels).
int csvhost_partition_check(const uint32_t *keys, uint64_t n, int *differ)
{
    GUARD({
        std::vector<uint32_t> a(n), b(n);
        for (uint64_t i = 0; i < n; i++) a[i] = b[i] = (uint32_t)i;
        auto cmp = [&](uint32_t x, uint32_t y) { return keys[x] > keys[y]; };
        *differ = 0;
        if (n > 16) {
            csvhost::lib_move_median_to_first(a.data(), a.data() + 1, a.data() + n / 2, a.data() + n - 1, cmp);
            csvhost::lib_move_median_to_first(b.data(), b.data() + 1, b.data() + n / 2, b.data() + n - 1, cmp);
            uint32_t *ca = csvhost::lib_unguarded_partition(a.data() + 1, a.data() + n, a.data(), cmp);
            uint32_t *cb = csvhost::lib_unguarded_partition_blocks(b.data() + 1, b.data() + n, b.data(), cmp);
            *differ = (ca - a.data() != cb - b.data()) || a != b;
        }
    })
}

// How many partitions the library's chain for slot nth takes on `keys` (descending by key, ids in input order: the loop of std_sort_select
// with the library's own partition, counted), or -1 where std::sort's depth limit runs out first and the library heap-sorts. The device's
// slot replay (csvgpu_sort_slot) declines exactly the chains that need more than its bound: the GPU tests predict its declines with this.
int64_t csvhost_sort_select_rounds(const uint32_t *keys, uint64_t n, uint64_t nth)
{
    try {
        if (n == 0 || nth >= n) return 0;
        std::vector<uint32_t> a(n);
        for (uint64_t i = 0; i < n; i++) a[i] = (uint32_t)i;
        auto cmp = [&](uint32_t x, uint32_t y) { return keys[x] > keys[y]; };
        int depth_limit = 0;
        for (uint64_t k = n; k > 1; k >>= 1) depth_limit++;
        depth_limit *= 2;
        uint32_t *lo = a.data(), *hi = a.data() + n, *target = a.data() + nth;
        int64_t rounds = 0;
        while (hi - lo > 16) {
            if (depth_limit == 0) return -1;
            --depth_limit; rounds++;
            csvhost::lib_move_median_to_first(lo, lo + 1, lo + (hi - lo) / 2, hi - 1, cmp);
            uint32_t *cut = csvhost::lib_unguarded_partition(lo + 1, hi, lo, cmp);
            if (target >= cut) lo = cut; else hi = cut;
        }
        return rounds;
    } catch (...) { return -2; }
}

// std::hash<std::string> of n '\n'-joined names (what the staging code attaches to a shard as its query-name column)
int csvhost_string_hashes(const char *names, uint64_t n, uint64_t *out)
{
    GUARD({
        const char *p = names;
        for (uint64_t i = 0; i < n; i++) {
            const char *e = strchr(p, '\n');
            const size_t len = e ? (size_t)(e - p) : strlen(p);
            out[i] = csvhost::std_string_hash(p, len);
            p = e ? e + 1 : p + len;
        }
    })
}

// SVCaller::assignShards: rank_of[i] for every shard weight
int csvhost_assign_shards(const double *weights, uint64_t n, int world, int32_t *rank_of)
{
    GUARD({
        const std::vector<int> r = SVCaller::assignShards(std::vector<double>(weights, weights + n), world);
        for (uint64_t i = 0; i < n; i++) rank_of[i] = r[i];
    })
}

// Test hook for par.h (CPU): parallel_for visits every index exactly once whatever the thread count, runs nested sections inline, hands
// the first exception to the caller and stays usable; WorkerThreads runs tasks side by side and reuses its threads. 0 = all held.
int csvhost_par_selftest(int n_items, int threads)
{
    GUARD({
        std::vector<std::atomic<int>> hit((size_t)n_items);
        for (auto &h : hit) h = 0;
        csvhost::parallel_for((size_t)n_items, threads, [&](size_t i) {
            hit[i]++;
            csvhost::parallel_for(3, threads, [&](size_t) {});                     // nested: inline
        });
        for (auto &h : hit) if (h != 1) throw std::runtime_error("parallel_for: an index was not visited exactly once");
        bool thrown = false;
        try { csvhost::parallel_for((size_t)n_items, threads, [&](size_t i) { if (i == (size_t)n_items / 2) throw std::runtime_error("x"); }); }
        catch (const std::runtime_error &) { thrown = true; }
        if (!thrown && n_items > 0) throw std::runtime_error("parallel_for: exception lost");
        std::atomic<long> sum{0};
        csvhost::parallel_for((size_t)n_items, threads, [&](size_t i) { sum += (long)i; });
        if (sum != (long)n_items * (n_items - 1) / 2) throw std::runtime_error("parallel_for: wrong sum after an exception");
        csvhost::WorkerThreads &w = csvhost::WorkerThreads::instance();
        for (int round = 0; round < 3; round++) {
            std::atomic<int> inside{0}, peak{0};
            std::vector<csvhost::WorkerThreads::Ticket> t;
            for (int k = 0; k < 4; k++)
                t.push_back(w.start([&] {
                    const int now = ++inside;
                    int p = peak.load();
                    while (now > p && !peak.compare_exchange_weak(p, now)) {}
                    const auto until = std::chrono::steady_clock::now() + std::chrono::milliseconds(20);
                    while (std::chrono::steady_clock::now() < until && peak.load() < 4) std::this_thread::yield();
                    --inside;
                }));
            for (auto x : t) w.wait(x);
            if (peak != 4) throw std::runtime_error("WorkerThreads: tasks did not run side by side");
        }
        // several threads in parallel sections at once, two on each pool (the one that finds a pool taken runs its items itself and
        // leaves the owner's flag alone)
        std::atomic<long> bad{0};
        std::vector<csvhost::WorkerThreads::Ticket> t;
        for (int k = 0; k < 4; k++)
            t.push_back(w.start([&, k] {
                if (k & 1) csvhost::HostPool::second_pool_flag() = true;
                for (int rep = 0; rep < 50; rep++) {
                    const size_t n = (size_t)n_items / 4 + (size_t)rep + 1;
                    std::vector<std::atomic<int>> seen(n);
                    for (auto &h : seen) h = 0;
                    csvhost::parallel_for(n, threads, [&](size_t i) { seen[i]++; });
                    for (auto &h : seen) if (h != 1) bad++;
                }
                csvhost::HostPool::second_pool_flag() = false;
            }));
        for (auto x : t) w.wait(x);
        if (bad) throw std::runtime_error("parallel_for: concurrent sections lost or repeated an index");
    })
}

// Test hook for umap_order.h (CPU): keys = n names ('\n'-joined) inserted in order with operator[], then every key with
// erase_mask[i] != 0 is erased. order_real = for every surviving node of a real std::unordered_map<std::string,int>, the index of
// the key's first insertion, in iteration order; order_emu = the same from csvhost::UMapOrder. Returns the count through *n_out
// (both have the same length when the emulation is right; the caller compares).
int csvhost_umap_order_check(const char *names, uint64_t n, const uint8_t *erase_mask, int64_t *order_real, int64_t *order_emu, uint64_t *n_real, uint64_t *n_emu,
                             uint64_t *buckets_real, uint64_t *buckets_emu)
{
    GUARD({
        const std::vector<std::string> keys = split_lines(names, (int64_t)n);
        std::unordered_map<std::string, int> real;
        csvhost::UMapOrder emu;
        std::vector<int64_t> first;
        for (uint64_t i = 0; i < n; i++) {
            real.emplace(keys[i], (int)i);                 // keeps the first index, as the emulation's `first` does
            real[keys[i]];                                 // (operator[] on an existing key: no structural change)
            const uint64_t h = csvhost::std_string_hash(keys[i].data(), keys[i].size());
            if (emu.find(h, [&](uint32_t nd) { return keys[(size_t)first[nd]] == keys[i]; }) < 0) { emu.insert_new(h); first.push_back((int64_t)i); }
        }
        *buckets_real = real.bucket_count(); *buckets_emu = emu.bucket_count();
        for (uint64_t i = 0; i < n; i++) if (erase_mask && erase_mask[i]) { real.erase(keys[i]); }
        uint64_t a = 0, b = 0;
        for (const auto &kv : real) order_real[a++] = kv.second;
        emu.for_each([&](uint32_t nd) { if (real.count(keys[(size_t)first[nd]])) order_emu[b++] = first[nd]; });
        *n_real = a; *n_emu = b;
    })
}

// ---- fast inflate / CRC (fast_inflate.h) on their own, for the tests
// 1 = decoded (out filled), 0 = declined (the caller would use zlib); never touches memory outside the two buffers
int csvhost_fast_inflate(const uint8_t *in, uint64_t in_len, uint8_t *out, uint64_t out_len) { return fastz::inflate(in, in_len, out, out_len) ? 1 : 0; }
uint32_t csvhost_fast_crc32(const uint8_t *buf, uint64_t len) { return fastz::crc32(buf, len); }

}  // extern "C"
