// arena_layouts_check.cpp — every carve function of contextsv_amd/csrc/layouts.hpp on the CPU, at the rounding edges of its counts.
// For each layout and shape: plan; allocate exactly the planned bytes; carve for real; fill every slice over its full requested size
// with a byte of its own; read all slices back (two slices that overlap show as a wrong byte, a slice that reaches past the
// reservation is caught by AddressSanitizer); the real carve must use what the plan said, every slice must be 256-byte aligned, and the
// ordering workspace's two key arrays must lie back to back. A layout named in kLayoutNames without a case here — or the reverse —
// fails the run. Built by `make layouts-check` (g++, -fsanitize=address,undefined, -DCSV_ARENA_LOG); a program of its own, no GPU.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <functional>
#include <map>
#include <set>
#include <string>
#include <vector>

#include "../../contextsv_amd/csrc/layouts.hpp"

namespace csv {
// Stand-ins for the per-primitive sizes that live beside their kernels (sort.hip, depth.hip, dbscan.hip, splitorder.hip). Deliberately
// odd, never a multiple of 256: a layout must hold whatever a primitive asks for.
size_t radix_sort_tmp_bytes(uint64_t n) { return 259 + n * 3; }
size_t exclusive_sum_tmp_bytes(uint64_t n) { return (n / 512 + 1) * 4 + 1; }
size_t prefix_max_tmp_bytes(uint64_t n) { return (n / 1024 + 1) * 4 + 3; }
size_t depth_tiles_tmp_bytes(uint32_t depth_len) { return ((size_t)depth_n_tiles(depth_len) + 1) * 16 + 5; }
size_t st_filter_bytes() { return 8191; }
constexpr uint64_t kUfTile = 256;
size_t dbscan_tmp_bytes(uint64_t n) { return arena_plan_bytes([&](Arena &a) { DbscanTmp t; return carve_dbscan_tmp(a, n, kUfTile, t); }); }
size_t dbscan1d_big_tmp_bytes(uint64_t n) { return dbscan_tmp_bytes(n); }

struct Slice { char *p; size_t bytes; };
static std::vector<Slice> g_log;
void arena_log(const Arena &a, void *p, size_t bytes) { if (a.base != arena_plan().base) g_log.push_back(Slice{(char *)p, bytes}); }      // (not the planning passes, nested ones included)
}  // namespace csv

using namespace csv;

static int g_fail = 0;
static long g_cases = 0;
#define CHECK(cond, ...) do { if (!(cond)) { fprintf(stderr, "FAIL %s: ", what.c_str()); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); g_fail++; return; } } while (0)

// `after` sees the carved workspace of the real pass (sub-slices that the log does not see)
static void run_case(const std::string &what, const std::function<bool(Arena &)> &carve, const std::function<bool(char *, char *)> &after = nullptr)
{
    g_cases++;
    Arena plan = arena_plan();
    CHECK(carve(plan), "the planning carve failed");
    const size_t need = plan.used;
    void *mem = nullptr;
    CHECK(posix_memalign(&mem, 256, need ? need : 1) == 0, "out of memory (%zu bytes)", need);
    Arena real; real.base = (char *)mem; real.cap = need;
    g_log.clear();
    const bool ok = carve(real);
    if (ok && real.used == need) {
        for (size_t i = 0; i < g_log.size(); i++) if (g_log[i].bytes) memset(g_log[i].p, (int)(i % 251) + 1, g_log[i].bytes);
    }
    bool clean = true, aligned = true;
    for (size_t i = 0; ok && i < g_log.size(); i++) {
        aligned &= ((uintptr_t)g_log[i].p & 255) == 0;
        for (size_t b = 0; b < g_log[i].bytes; b++) if ((unsigned char)g_log[i].p[b] != (unsigned char)((i % 251) + 1)) { clean = false; break; }
    }
    const bool after_ok = ok && after ? after((char *)mem, (char *)mem + need) : true;
    free(mem);
    CHECK(ok, "the real carve failed over exactly the planned %zu bytes", need);
    CHECK(real.used == need, "real used %zu, planned %zu", real.used, need);
    CHECK(aligned, "a slice is not 256-byte aligned");
    CHECK(clean, "two slices overlap");
    CHECK(after_ok, "a sub-slice lies outside its slice or overlaps another");
}

static bool sort_adjacent(const SortWs &w, uint64_t n) { return (char *)w.k1 == (char *)w.k0 + align_up(n * 8, 256) && (char *)w.sig_tmp == (char *)w.k0; }

int main()
{
    const uint64_t counts[] = {0, 1, 63, 64, 65, 255, 256, 257, 100003};
    const uint64_t big[] = {DBSCAN1D_MAX_SEG, DBSCAN1D_MAX_SEG + 1};
    const uint32_t depth_lens[] = {0, 1, DEPTH_TILE, DEPTH_TILE + 1};
    std::set<std::string> seen;
    std::map<std::string, std::vector<std::set<uint64_t>>> args;          // by layout and argument position: the values it was run with
    auto tag = [&](const char *name, std::initializer_list<uint64_t> v) {
        seen.insert(name);
        std::string s = name;
        std::vector<std::set<uint64_t>> &a = args[name];
        if (a.size() < v.size()) a.resize(v.size());
        size_t i = 0;
        for (uint64_t x : v) { s += " " + std::to_string(x); a[i++].insert(x); }
        return s;
    };

    for (uint64_t n : counts) {
        { SortWs w; run_case(tag("sortws", {n}), [&](Arena &a) { return sortws_carve(a, n, w); }, [&](char *, char *) { return sort_adjacent(w, n); }); }
        { DbscanIvWs w; run_case(tag("dbscan_iv", {n}), [&](Arena &a) { return carve_dbscan_iv(a, n, w); }, [&](char *, char *) { return sort_adjacent(w.w, n); }); }
        { JobScratch w; run_case(tag("job_scratch", {n}), [&](Arena &a) { return carve_job_scratch(a, n, w); }, [&](char *, char *) { return sort_adjacent(w.w, n); }); }
        { MergeSelectWs w; run_case(tag("merge_select", {n}), [&](Arena &a) { return carve_merge_select(a, n, w); }, [&](char *, char *) { return sort_adjacent(w.sw, n); }); }
        { DbscanTmp w; run_case(tag("dbscan_tmp", {n}), [&](Arena &a) { return carve_dbscan_tmp(a, n, kUfTile, w); }); }
        { ViterbiTmp w; run_case(tag("viterbi_tmp", {n}), [&](Arena &a) { return carve_viterbi_tmp(a, n, 1000, w); }); }
        for (uint32_t dl : depth_lens) { DepthWs w; run_case(tag("depth", {n, dl}), [&](Arena &a) { return carve_depth(a, n, dl, w); }, [&](char *, char *) { return sort_adjacent(w.w, n); }); }
        for (uint64_t B : big) { SfRunWs w; run_case(tag("sf_run", {n, B}), [&](Arena &a) { return carve_sf_run(a, n, B, w); }, [&](char *, char *) { return B <= DBSCAN1D_MAX_SEG || sort_adjacent(w.w, B); }); }
        for (uint64_t m : counts) {
            { ReadsWs w; run_case(tag("reads", {n, m}), [&](Arena &a) { return carve_reads(a, n, m, w); }); }
            { SplitNodesWs w; run_case(tag("split_nodes", {n, m}), [&](Arena &a) { return carve_split_nodes(a, n, m, w); }); }
            { MergeRunWs w; run_case(tag("merge_run", {n, m}), [&](Arena &a) { return carve_merge_run(a, n, m, w); }, [&](char *, char *) { return sort_adjacent(w.ms.sw, std::max(n, m)); }); }
            { SortSlotWs w; run_case(tag("sort_slot", {n, m}), [&](Arena &a) { return carve_sort_slot(a, n, m, w); }); }
            { WindowWs w; run_case(tag("window", {n, m}), [&](Arena &a) { return carve_window(a, n, m, w); }); }
            // (both copy-number routes end with the same back half: from its first slice to the reservation's end it is as large in either)
            auto back_bytes = [&](uint64_t S, bool dec) { return arena_plan_bytes([&](Arena &a) { CnBack b; return carve_cn_back(a, n, m, S, dec, b); }); };
            for (int dec : {0, 1}) { CnBack b; run_case(tag("cn_back", {n, m, (n + m) % 1009, (uint64_t)dec}), [&](Arena &a) { return carve_cn_back(a, n, m, (n + m) % 1009, dec != 0, b); }); }
            for (int dec : {0, 1}) {   // n regions, m windows; shards and SNP records run along
                CnWs w;
                const uint64_t n_sh = n % 5 + 1, S = (n + m) % 1009;
                run_case(tag("cn_obs", {n, m, n_sh, S, (uint64_t)dec}), [&](Arena &a) { return carve_cn_obs(a, n, m, n_sh, S, dec != 0, w); }, [&](char *, char *hi) {
                    const CnInLayout L(n, n_sh, S);
                    const size_t at[] = {L.rs, L.re, L.ss, L.wo, L.wbase, L.soff, L.spos, L.sbaf, L.spfb, L.small, L.big, L.bytes};
                    const size_t need[] = {n * 4, n * 4, n * 4, (n + n_sh) * 8, (n + 1) * 4, (n + 1) * 4, S * 4, S * 8, S * 8, n * 4, n * 4};
                    for (int i = 0; i < 11; i++) if (at[i] % 256 || at[i] + need[i] > at[i + 1]) return false;
                    return (size_t)(hi - (char *)w.b.l2) == back_bytes(S, dec != 0);
                });
            }
            for (int dec : {0, 1}) {   // n regions, m windows (0: the first carve); shards and SNP records run along. The second carve must leave the first one's slices where they were
                CnTabWs w, w0;
                const uint64_t n_sh = n % 5 + 1, S = m ? (n + m) % 1009 : 0;
                Arena p0 = arena_plan();
                (void)carve_cn_tables(p0, n, n_sh, 0, 0, dec != 0, w0);
                run_case(tag("cn_tables", {n, m, n_sh, S, (uint64_t)dec}), [&](Arena &a) { return carve_cn_tables(a, n, n_sh, m, S, dec != 0, w); }, [&](char *lo, char *hi) {
                    const CnUpLayout L(n, n_sh);
                    const size_t at[] = {L.rs, L.re, L.ssf, L.rsh, L.tabs, L.roff, L.bytes};
                    const size_t need[] = {n * 4, n * 4, n * 4, n * 4, n_sh * sizeof(SnpTabDev), (n_sh + 1) * 4};
                    for (int i = 0; i < 6; i++) if (at[i] % 256 || at[i] + need[i] > at[i + 1]) return false;
                    if (m && (size_t)(hi - (char *)w.b.l2) != back_bytes(S, dec != 0)) return false;
                    return w.up == lo && (char *)w.p.head - w.up == (char *)w0.p.head - w0.up && (char *)w.b.sl.tot - w.up == (char *)w0.b.sl.tot - w0.up &&
                           (char *)w.p.shard_w0 == (char *)w.p.head + CN_PLAN_HEAD_BYTES && sizeof(CnPlanHead) <= CN_PLAN_HEAD_BYTES;
                });
            }
            for (int io : {0, 1}) { BgzfWs w; run_case(tag("bgzf", {n, m, (uint64_t)io}), [&](Arena &a) { return carve_bgzf(a, n, io != 0, m, (n + m) % 1009 * 65, w); }); }   // n members, m compressed bytes
            for (int io : {0, 1}) {   // a stream of n * 36 + m % 36 bytes (n records at most) cut at m anchors; the outputs' capacities run along
                BamUnpackWs w;
                const uint64_t len = n * 36 + m % 36;
                run_case(tag("bam_unpack", {n, m, (uint64_t)io}), [&](Arena &a) { return carve_bam_unpack(a, len, m, io != 0, (n + m) % 1009, m, n % 3 ? m : 0, m % 3 ? n : 0, (n + m) % 2 != 0, w); },
                         [&](char *lo, char *hi) {
                             return bam_unpack_max_records(len) == n && (char *)w.res >= lo && (char *)(w.bounds + 2) <= (char *)w.res + BU_HEAD_BYTES && (char *)w.res + 256 <= hi &&
                                    (char *)w.status == (char *)w.res + 32 && ((uintptr_t)w.status & 7) == 0;
                         });
            }
            for (int io : {0, 1}) {   // n tiles, m line slots (0: the first carve); strings, form and capacities run along. The second carve must leave the first one's slices where they were
                VcfWs w, w0;
                const bool af = (n + m) % 2 != 0;
                Arena p0 = arena_plan();
                (void)carve_vcf(p0, n, m % 90, 0, io != 0, af, n, m, w0);
                run_case(tag("vcf", {n, m, (uint64_t)io}), [&](Arena &a) { return carve_vcf(a, n, m % 90, m, io != 0, af, (n + m) % 1009, n % 7, w); },
                         [&](char *lo, char *) {
                             return (char *)w.head == lo && (char *)w.tile_cnt - (char *)w.head == (char *)w0.tile_cnt - (char *)w0.head &&
                                    (char *)w.strings - (char *)w.head == (char *)w0.strings - (char *)w0.head && sizeof(VcfHead) <= 256;
                         });
            }
            { VcfTextWs w; run_case(tag("vcf_text", {n, m}), [&](Arena &a) { return carve_vcf_text(a, n, m, w); }); }
            { SplitTablesOut w; run_case(tag("sr_tables", {n, m}), [&](Arena &a) { return sr_carve(a, n, m, w); }); }
            for (int with : {0, 1}) { SplitFitsIn w; run_case(tag("sf_tables", {n, m, (uint64_t)with}), [&](Arena &a) { return carve_sf_tables(a, n, m, with != 0, w); }); }
            {   // n members in m segments; the block cleared by one memset holds six sub-slices
                SgWs w;
                run_case(tag("split_groups", {n, m}), [&](Arena &a) { return carve_split_groups(a, (uint32_t)n, m, w); }, [&](char *, char *) {
                    if (!sort_adjacent(w.sw, n)) return false;
                    const Slice sub[] = {{(char *)w.w.hist, (n + 1) * 4}, {(char *)w.w.cnt, (n + 1) * 4}, {(char *)w.w.keep, (n + 1) * 4}, {(char *)w.w.state, n},
                                         {(char *)w.w.total, 8}, {(char *)w.w.err, 4}};
                    for (int i = 0; i < 6; i++) {
                        if (sub[i].p < w.zero || sub[i].p + sub[i].bytes > w.zero + w.zero_bytes) return false;
                        memset(sub[i].p, 0x10 + i, sub[i].bytes);
                    }
                    for (int i = 0; i < 6; i++) for (size_t b = 0; b < sub[i].bytes; b++) if (sub[i].p[b] != 0x10 + i) return false;
                    return true;
                });
            }
            // every n_seg with every member count; the entry count runs along with them (every value of the list, not every triple)
            for (size_t k = 0; k < sizeof(counts) / sizeof(counts[0]); k++) {
                const uint64_t n_seg = n, nm = m, ns = counts[(k + (size_t)(n % 7) + (size_t)(m % 5)) % (sizeof(counts) / sizeof(counts[0]))];
                if (k >= 2 && (n_seg == 100003) + (nm == 100003) + (ns == 100003) >= 2) continue;      // (two entry counts per pair suffice where the slices are megabytes)
                SplitTablesIn w;
                run_case(tag("sr_refs", {n_seg, nm, ns}), [&](Arena &a) { return carve_sr_refs(a, n_seg, nm, ns, w); });
            }
            for (int D = 0; D <= (int)SO_TAIL_MAX; D++) {   // scratch bytes n, m nodes (the sorts take the larger of the two counts), bitmaps of n / 32 + 8 words
                SplitEpochsWs w;
                const uint64_t n_sort = n > m ? n : m;
                run_case(tag("split_epochs", {n, m, (uint64_t)D}), [&](Arena &a) { return carve_split_epochs(a, n, n_sort, m, D, (size_t)(n / 32 + 8), w); },
                         [&](char *, char *) { return sort_adjacent(w.w, n_sort); });
            }
        }
    }
    for (uint64_t len : {(uint64_t)0, (uint64_t)1, (uint64_t)DBSCAN1D_MAX_SEG, (uint64_t)DBSCAN1D_MAX_SEG + 1, (uint64_t)100003}) {
        Dbscan1dWs w;
        run_case(tag("dbscan1d", {len}), [&](Arena &a) { return carve_dbscan1d(a, (uint32_t)len, w); }, [&](char *, char *) { return len <= DBSCAN1D_MAX_SEG || sort_adjacent(w.w, len); });
    }

    // every count of a layout (n, n_seg, G, nm, ns: its leading arguments) has taken every value of the list
    const std::map<std::string, size_t> n_counts = {{"sortws", 1}, {"merge_select", 1}, {"sort_slot", 2}, {"merge_run", 2}, {"dbscan_iv", 1}, {"job_scratch", 1}, {"dbscan_tmp", 1}, {"viterbi_tmp", 1}, {"depth", 1}, {"sf_run", 1},
                                                    {"reads", 2}, {"split_nodes", 2}, {"window", 2}, {"cn_back", 2}, {"cn_obs", 2}, {"cn_tables", 2},{"bgzf", 2}, {"bam_unpack", 2}, {"vcf", 2}, {"vcf_text", 2}, {"sr_tables", 2}, {"sf_tables", 2}, {"split_groups", 2},
                                                    {"split_epochs", 2}, {"sr_refs", 3}, {"dbscan1d", 0}};
    for (const auto &kv : args) {
        const auto it = n_counts.find(kv.first);
        if (it == n_counts.end()) { fprintf(stderr, "FAIL: layout '%s' has no entry in the coverage table\n", kv.first.c_str()); g_fail++; continue; }
        for (size_t i = 0; i < it->second; i++)
            for (uint64_t c : counts)
                if (i >= kv.second.size() || !kv.second[i].count(c)) { fprintf(stderr, "FAIL: layout '%s' never ran with %llu as count %zu\n", kv.first.c_str(), (unsigned long long)c, i); g_fail++; }
    }
    // every layout of the header has a case above, and every case names a layout of the header
    std::set<std::string> listed(kLayoutNames, kLayoutNames + kLayoutCount);
    for (const std::string &name : listed) if (!seen.count(name)) { fprintf(stderr, "FAIL: layout '%s' of layouts.hpp has no case in this program\n", name.c_str()); g_fail++; }
    for (const std::string &name : seen) if (!listed.count(name)) { fprintf(stderr, "FAIL: case '%s' names no layout of layouts.hpp\n", name.c_str()); g_fail++; }
    if (listed.size() != kLayoutCount) { fprintf(stderr, "FAIL: a name twice in kLayoutNames\n"); g_fail++; }
    printf("arena_layouts_check: %zu layouts, %ld cases, %d failures\n", listed.size(), g_cases, g_fail);
    return g_fail ? 1 : 0;
}
