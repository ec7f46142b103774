// split_order.hip — the order in which the reference's hash table hands out the split-read candidates (kernels/splitorder.hip).
#include <unordered_map>

#include "glue.hpp"

namespace csv {

// the epochs of a libstdc++ hash table that grows by single insertions: node index at which each rehash happens, and the bucket
// count from there on — asked of the library's own policy object (what std::unordered_map itself consults)
void split_order_epochs(uint64_t n_max, std::vector<uint64_t> &first_node, std::vector<uint64_t> &buckets)
{
    static std::mutex mu;
    static std::vector<uint64_t> c_first, c_bkt;
    static uint64_t covered = 0;                              // the plan is known for tables of up to `covered` nodes
    std::lock_guard<std::mutex> l(mu);
    if (n_max > covered) {
        c_first.clear(); c_bkt.clear();
        std::__detail::_Prime_rehash_policy pol;
        std::size_t nb = 1;
        const uint64_t want = std::max<uint64_t>(n_max, 1u << 20);
        for (uint64_t i = 0; i < want;) {
            const std::pair<bool, std::size_t> g = pol._M_need_rehash(nb, i, 1);
            if (g.first) { nb = g.second; c_first.push_back(i); c_bkt.push_back(nb); }
            // nothing can happen before the table is full again (max_load_factor 1): jump there
            i = (g.first || i + 1 >= nb) ? i + 1 : std::min<uint64_t>(want, (uint64_t)nb);
        }
        covered = want;
    }
    first_node = c_first; buckets = c_bkt;
}

}  // namespace csv

using namespace csv;

// What csvgpu_split_order_begin leaves for csvgpu_split_order_finish (one pending order per context; device pointers into ctx->arena / ctx->work).
struct csv_split_state : SplitNodesWs, SplitEpochsWs {
    int n_contigs = 0;
    SplitOrderTab tab;
    std::vector<uint64_t> N;
    uint64_t n_nodes = 0, n_max = 0, total_reads = 0;
    int D = 0;
    SplitTailHost th;
    size_t bm_words = 0;
    bool finished = false;
    bool self = false;                 // the supplementary hashes are taken from the same shards: the whole order was queued by _begin
    uint64_t self_bound = 0;           // survivors the page-locked block has room for (self)
    std::vector<csv_split_survivor> surv;
    std::vector<uint64_t> off;
};

void csv::split_state_free(csv_ctx *ctx) { if (ctx) { delete ctx->split_state; ctx->split_state = nullptr; } }

// the survivors in their final order: the last D epochs for them and the nodes their order depends on (or, D = 0, the chain's final
// positions). devn: the set sizes stay on the device (everything is queued, nothing waited for).
static int split_order_tail(csv_ctx *ctx, csv_split_state *st, const uint64_t *d_supp, uint64_t n_supp, bool devn)
{
    hipStream_t s = ctx->stream;
    const int D = st->D;
    const int n_contigs = st->n_contigs;
    SplitTailHost &th = st->th;
    SortWs &w = st->w;
    const uint64_t n_nodes = st->n_nodes, cap = n_nodes;
    if (D == 0) {
        // ---- survivors: nodes whose name hash is a supplementary record's; their final position orders them ----
        launch_so_survivors(s, st->tab, n_nodes, st->node_hash, st->node_rec, st->list, d_supp, n_supp, st->d_out, cap, st->d_count);
        return CSV_OK;
    }
    // ---- top-down: who takes part in the last D epochs (hashes only) ----
    unsigned int *d_setn = (unsigned int *)((char *)st->d_count + 64);
    uint32_t set_n[SO_TAIL_MAX + 1] = {0, 0, 0, 0};
    for (int j = 0; j < D; j++) CSV_HIP(ctx, hipMemsetAsync(st->bitmap[j], 0, st->bm_words * 4, s));
    CSV_HIP(ctx, hipMemsetAsync(st->filter, 0, st_filter_bytes(), s));
    launch_st_survivors(s, th, (uint32_t)n_nodes, st->node_hash, d_supp, n_supp, st->filter, st->is_surv, st->bitmap[0]);
    for (int j = 1; j <= D; j++)
        launch_st_member(s, th, (uint32_t)n_nodes, j, st->node_hash, st->bitmap[j - 1], j < D ? st->bitmap[j] : nullptr, st->set[j], d_setn + j);
    if (!devn) {
        CSV_HIP(ctx, hipMemcpyAsync(ctx->pinned, d_setn, 16, hipMemcpyDeviceToHost, s));
        CSV_HIP(ctx, wait_stream(s));
        for (int j = 1; j <= D; j++) set_n[j] = ((const uint32_t *)ctx->pinned)[j];
        // a t value is a list position or an insertion index (below the largest contig's node count) or a rank in a level's order (below the set's size)
        uint64_t t_max = st->n_max;
        for (int j = 1; j <= D; j++) t_max = std::max<uint64_t>(t_max, set_n[j]);
        th.wv = std::max(1, bits_of(t_max));
    } else {
        for (int j = 1; j <= D; j++) set_n[j] = (uint32_t)n_nodes;           // (bounds: the kernels read the sizes)
        th.wv = std::max(1, bits_of(n_nodes));
    }
    // ---- bottom-up: order S_D with the chain's positions, then each smaller set with the ranks of the order before ----
    const int key_bits = th.wa + 2 * (th.wv + 1);
    for (int j = D - 1; j >= 0; j--) {
        const uint32_t n = set_n[j + 1];
        const uint32_t *n_dev = devn ? d_setn + (j + 1) : nullptr;
        if (n == 0) continue;
        CSV_HIP(ctx, hipMemsetAsync(st->minT, 0xff, (size_t)th.boff[j][n_contigs] * 4, s));
        launch_st_mint(s, th, j, st->set[j + 1], n, n_dev, st->node_hash, st->prevrank, st->minT);
        launch_st_keys(s, th, j, st->set[j + 1], n, n_dev, st->node_hash, st->prevrank, st->minT, w.k0, w.v0);
        const int io = devn ? launch_radix_sort_u64_devn(s, w.k0, w.v0, w.k1, w.v1, n, n_dev, key_bits, w.tmp)
                            : launch_radix_sort_u64(s, w.k0, w.v0, w.k1, w.v1, n, key_bits, w.tmp, onesweep(ctx));
        if (io < 0) { ctx->err = "split_order: set too large for the queued sort"; return CSV_EINVAL; }
        const uint32_t *sorted = (devn || n > 1) ? (io ? w.v1 : w.v0) : w.v0;
        if (j > 0) launch_st_rank(s, sorted, n, n_dev, st->prevrank);
        else launch_st_emit(s, th, sorted, n, n_dev, st->is_surv, st->node_rec, st->d_out, cap, st->d_count);
    }
    return CSV_OK;
}

// nodes + every epoch that does not depend on the supplementary records: queued, not waited for (beyond the node counts)
static int split_order_begin(csv_ctx *ctx, int n_contigs, csv_shard *const *shards, uint8_t min_mapq, int64_t n_supp_hint /* < 0: unknown */, bool self = false)
{
    if (!ctx) return CSV_EINVAL;
    delete ctx->split_state; ctx->split_state = nullptr;
    if (n_contigs < 0 || (uint32_t)n_contigs > SO_MAX_CONTIGS) { ctx->err = "split_order: at most 32 contigs per call"; return CSV_EINVAL; }
    if (n_contigs && !shards) { ctx->err = "split_order: null array"; return CSV_EINVAL; }
    std::unique_ptr<csv_split_state> st(new csv_split_state());
    st->n_contigs = n_contigs;
    st->off.assign((size_t)n_contigs + 1, 0);
    if (n_contigs == 0) { st->finished = true; ctx->split_state = st.release(); return CSV_OK; }
    (void)hipSetDevice(ctx->device);
    hipStream_t s = ctx->stream;
    SplitOrderTab &tab = st->tab;
    tab.A = (uint32_t)n_contigs;
    uint64_t total_reads = 0, n_blocks = 0;
    for (int c = 0; c < n_contigs; c++) {
        const csv_shard *sh = shards[c];
        if (!sh || (sh->d.n_reads && !sh->qhash)) { ctx->err = "split_order: a shard without query-name hashes (csvgpu_shard_set_qname_hash)"; return CSV_EINVAL; }
        tab.blk_off[c] = n_blocks;
        tab.n_reads[c] = sh->d.n_reads; tab.flag[c] = sh->d.flag; tab.mapq[c] = sh->d.mapq; tab.qhash[c] = sh->qhash;
        n_blocks += (sh->d.n_reads + 1023) / 1024;
        total_reads += sh->d.n_reads;
    }
    tab.blk_off[n_contigs] = n_blocks;
    st->total_reads = total_reads;
    if (total_reads == 0 || n_supp_hint == 0) { st->finished = true; ctx->split_state = st.release(); return CSV_OK; }
    if (total_reads >= 0xfffffff0ull) { ctx->err = "split_order: too many records in one call"; return CSV_EINVAL; }
    TimerScope ts(ctx, CSV_K_SPLIT_ORDER);

    // ---- nodes: the filter-passing primaries of every contig, file order ----
    // (the supplementary hashes arrive with _finish: at most one per record)
    int rc = arena_reserve_for(ctx, ctx->arena, "split order", [&](Arena &a) { return carve_split_nodes(a, n_blocks, total_reads, *st); });
    if (rc) return rc;
    unsigned int *d_nsupp = st->d_nsupp;
    uint32_t *blk = st->blk, *node_rec = st->node_rec, *list = st->list;
    void *es_tmp = st->es_tmp;
    uint64_t *node_hash = st->node_hash;
    CSV_HIP(ctx, hipMemsetAsync(blk + n_blocks, 0, 4, s));
    launch_so_count(s, tab, (uint32_t)n_blocks, min_mapq, blk);
    launch_exclusive_sum_u32(s, blk, n_blocks + 1, es_tmp);
    launch_so_scatter(s, tab, (uint32_t)n_blocks, min_mapq, blk, node_hash, node_rec);
    if ((rc = ensure_pinned(ctx, (n_blocks + 1) * 4 + 64 + 256))) return rc;
    CSV_HIP(ctx, hipMemcpyAsync(ctx->pinned, blk, (n_blocks + 1) * 4, hipMemcpyDeviceToHost, s));
    const size_t nsupp_at = align_up((n_blocks + 1) * 4, 64);
    if (self) {                                  // the supplementary records' hashes of the same shards (their count comes back with the node counts)
        CSV_HIP(ctx, hipMemsetAsync(d_nsupp, 0, 4, s));
        launch_so_supp(s, tab, (uint32_t)n_blocks, min_mapq, st->d_supp, d_nsupp);
        CSV_HIP(ctx, hipMemcpyAsync((char *)ctx->pinned + nsupp_at, d_nsupp, 4, hipMemcpyDeviceToHost, s));
    }
    CSV_HIP(ctx, wait_stream(s));
    const uint32_t *h_blk = (const uint32_t *)ctx->pinned;
    uint64_t n_supp_self = 0;
    if (self) {
        n_supp_self = *(const uint32_t *)((const char *)ctx->pinned + nsupp_at);
        n_supp_hint = (int64_t)n_supp_self;
        st->self = true;
        if (n_supp_self == 0) { st->finished = true; ctx->split_state = st.release(); return CSV_OK; }          // nothing survives
    }
    std::vector<uint64_t> &N = st->N;
    N.assign((size_t)n_contigs, 0);
    uint64_t n_nodes = h_blk[n_blocks], n_max = 0;
    for (int c = 0; c < n_contigs; c++) {
        tab.nbase[c] = h_blk[tab.blk_off[c]];
        N[(size_t)c] = (uint64_t)h_blk[tab.blk_off[c + 1]] - h_blk[tab.blk_off[c]];
        n_max = std::max(n_max, N[(size_t)c]);
    }
    tab.nbase[n_contigs] = (uint32_t)n_nodes;
    st->n_nodes = n_nodes; st->n_max = n_max;
    if (n_nodes == 0) { st->finished = true; ctx->split_state = st.release(); return CSV_OK; }

    // ---- the chain of epochs: a contig takes part in epoch k while it still has nodes inserted at or after the epoch's first node ----
    std::vector<uint64_t> first_node, buckets;
    split_order_epochs(n_max, first_node, buckets);
    // The last D epochs of every contig are ordered for the survivors (and the nodes their order depends on) only: splitorder.hip.
    // The sets double per level and the epochs halve, so D levels pay while 4^D <= nodes per supplementary record (about a hundred
    // in a long-read run: D = 3, also taken when the caller has not counted its supplementary records yet).
    int D = 0;
    {
        const uint64_t ratio = n_supp_hint > 0 ? n_nodes / (uint64_t)n_supp_hint : (n_nodes >= 4096 ? 64 : 1);
        while (D < (int)SO_TAIL_MAX && (ratio >> (2 * (D + 1))) >= 1) D++;
        if (ctx->tuning.split_tail != CSV_TAIL_AUTO) D = ctx->tuning.split_tail;
    }
    SplitTailHost &th = st->th;
    th.A = (uint32_t)n_contigs; th.wv = std::max(1, bits_of(n_nodes)); th.wa = std::max(1, bits_of((uint64_t)n_contigs - 1));
    if (n_nodes >= (1ull << 31) || th.wa + 2 * (th.wv + 1) > 64 || (self && n_nodes >= (1ull << 30))) D = 0;      // (self: the queued sorts count in 30 bits)
    th.D = (uint32_t)D;
    std::vector<int> K((size_t)n_contigs, -1);                       // a contig's last epoch
    for (int c = 0; c < n_contigs; c++) {
        for (size_t k = 0; k < first_node.size() && N[(size_t)c] > first_node[k]; k++) K[(size_t)c] = (int)k;
        th.nbase[c] = tab.nbase[c];
    }
    th.nbase[n_contigs] = (uint32_t)n_nodes;
    uint64_t tail_buckets = 0;
    for (int j = 0; j < D; j++) {
        uint64_t off = 0;
        for (int c = 0; c < n_contigs; c++) {
            const int e = K[(size_t)c] - j;
            th.B[j][c] = e >= 0 ? (uint32_t)buckets[(size_t)e] : 1u;
            th.F[j][c] = e >= 0 ? (uint32_t)first_node[(size_t)e] : 0u;
            th.boff[j][c] = (uint32_t)off;
            off += th.B[j][c];
        }
        if (off >= 0xffffffe0ull) { D = 0; th.D = 0; break; }
        for (int c = n_contigs; c <= (int)SO_MAX_CONTIGS; c++) th.boff[j][c] = (uint32_t)off;
        tail_buckets = std::max(tail_buckets, off);
    }
    st->D = D;
    auto in_chain = [&](int c, size_t k) { return N[(size_t)c] > first_node[k] && (int)k <= K[(size_t)c] - D; };
    uint64_t scratch = tail_buckets * 4;
    for (size_t k = 0; k < first_node.size(); k++) {
        uint64_t A = 0;
        for (int c = 0; c < n_contigs; c++) A += in_chain(c, k);
        scratch = std::max(scratch, A * buckets[k] * 4);
    }
    const size_t bm_words = st->bm_words = (size_t)((tail_buckets + 31) / 32 + 8);
    const uint64_t n_sort = std::max(n_nodes, n_supp_self);
    if ((rc = arena_reserve_for(ctx, ctx->work, "split order epochs", [&](Arena &a) { return carve_split_epochs(a, scratch, n_sort, n_nodes, D, bm_words, *st); }))) return rc;
    uint32_t *minT = st->minT;
    SortWs &w = st->w;
    CSV_HIP(ctx, hipMemsetAsync(st->d_count, 0, 256, s));

    // the first epochs (nodes and buckets in LDS) in one launch, one workgroup per contig
    size_t n_small = 0;
    {
        SplitSmallHost sm;
        while (n_small < first_node.size() && n_small < SO_SMALL_EPOCHS && buckets[n_small] <= SO_SMALL_B) n_small++;
        if (ctx->tuning.split_chain_only) n_small = 0;                          // (A/B and tests: every epoch through the chain's sorts)
        sm.A = (uint32_t)n_contigs; sm.n_epochs = (uint32_t)n_small;
        bool any = false;
        for (int c = 0; c <= n_contigs; c++) sm.nbase[c] = th.nbase[c];
        for (int c = 0; c < n_contigs; c++) {
            int kl = -1;
            for (size_t k = 0; k < n_small && in_chain(c, k); k++) kl = (int)k;
            sm.k_last[c] = kl; any |= kl >= 0;
        }
        for (size_t k = 0; k <= n_small && k < first_node.size(); k++) sm.first[k] = (uint32_t)std::min<uint64_t>(first_node[k], 0xffffffffu);
        if (n_small >= first_node.size()) sm.first[n_small] = 0xffffffffu;
        for (size_t k = 0; k < n_small; k++) sm.B[k] = (uint32_t)buckets[k];
        if (n_small && any) launch_so_small_epochs(s, sm, node_hash, list);
    }
    for (size_t k = n_small; k < first_node.size(); k++) {
        SplitOrderTab e;
        e.A = 0;
        uint64_t M = 0, m_max = 0;
        const uint64_t next_first = k + 1 < first_node.size() ? first_node[k + 1] : ~0ull;
        for (int c = 0; c < n_contigs; c++) {
            if (!in_chain(c, k)) continue;
            const uint64_t m = std::min(N[(size_t)c], next_first);                 // nodes present at the end of this epoch
            e.work_off[e.A] = M; e.nbase[e.A] = tab.nbase[c]; e.m_old[e.A] = (uint32_t)first_node[k];
            e.A++; M += m; m_max = std::max(m_max, m);
        }
        if (e.A == 0) break;
        e.work_off[e.A] = M;
        if (m_max <= 1) continue;                                                   // a single node: nothing to order
        const uint32_t B = (uint32_t)buckets[k];
        const int wbits = std::max(1, bits_of(m_max - 1));
        for (uint32_t a = 0; a < e.A; a++) e.rev_off[a] = M - e.work_off[a + 1];
        const int key_bits = std::max(1, bits_of(M - 1));
        CSV_HIP(ctx, hipMemsetAsync(minT, 0xff, (size_t)e.A * B * 4, s));
        launch_so_mint(s, e, M, B, node_hash, list, minT);
        launch_so_keys(s, e, M, B, wbits, node_hash, list, minT, w.k0, w.v0);
        const int io = launch_radix_sort_u64(s, w.k0, w.v0, w.k1, w.v1, M, key_bits, w.tmp, onesweep(ctx));
        launch_so_setlist(s, e, M, io ? w.v1 : w.v0, list);
    }
    if (D > 0) launch_st_inverse(s, th, (uint32_t)n_nodes, D - 1, list, st->prevrank);
    if (self) {
        // everything else too: the hashes sorted (64-bit keys, the values are not used), the survivors-only levels with the set sizes read on
        // the device, the survivors copied to the page-locked block — _finish only waits
        const int io = launch_radix_sort_u64(s, st->d_supp, w.v0, w.k1, w.v1, n_supp_self, 64, w.tmp, onesweep(ctx));
        if (io != 0) { ctx->err = "split_order: unexpected sort parity"; return CSV_EHIP; }
        if ((rc = split_order_tail(ctx, st.get(), st->d_supp, n_supp_self, true))) return rc;
        st->self_bound = std::min<uint64_t>(n_supp_self, n_nodes);
        if ((rc = ensure_pinned(ctx, 64 + st->self_bound * sizeof(csv_split_survivor) + 64))) return rc;
        CSV_HIP(ctx, hipMemcpyAsync(ctx->pinned, st->d_count, 8, hipMemcpyDeviceToHost, s));
        CSV_HIP(ctx, hipMemcpyAsync((char *)ctx->pinned + 64, st->d_out, st->self_bound * sizeof(csv_split_survivor), hipMemcpyDeviceToHost, s));
    }
    if (hipGetLastError() != hipSuccess) { ctx->err = "split_order: launch failed"; return CSV_EHIP; }
    ctx->split_state = st.release();
    return CSV_OK;
}

static int split_order_finish(csv_ctx *ctx, const uint64_t *supp_hash, uint64_t n_supp, uint32_t *out_rec, uint64_t capacity, uint64_t *out_off)
{
    if (!ctx) return CSV_EINVAL;
    csv_split_state *st = ctx->split_state;
    if (!st) { ctx->err = "split_order_finish without split_order_begin"; return CSV_EINVAL; }
    const int n_contigs = st->n_contigs;
    if (!out_off || (!st->self && n_supp && !supp_hash) || (capacity && !out_rec)) { ctx->err = "split_order: null array"; return CSV_EINVAL; }
    if (!st->self)
        for (uint64_t i = 1; i < n_supp; i++) if (supp_hash[i] <= supp_hash[i - 1]) { ctx->err = "split_order: supp_hash must be sorted and distinct"; return CSV_EINVAL; }
    for (int c = 0; c <= n_contigs; c++) out_off[c] = 0;
    (void)hipSetDevice(ctx->device);
    hipStream_t s = ctx->stream;
    if (!st->finished && !st->self) {
        if (n_supp == 0) {               // nothing survives
            CSV_HIP(ctx, wait_stream(s));
            st->finished = true;
        }
    }
    if (!st->finished) {
        TimerScope ts(ctx, CSV_K_SPLIT_ORDER);
        std::vector<csv_split_survivor> &surv = st->surv;
        int prc;
        if (st->self) {
            // everything was queued by _begin: the count and the survivors are in (or on their way to) the page-locked block
            CSV_HIP(ctx, wait_stream(s));
            const uint64_t n_surv = *(const unsigned long long *)ctx->pinned;
            if (n_surv > st->self_bound) { ctx->err = "split_order: more survivors than supplementary records"; return CSV_EHIP; }
            surv.resize(n_surv);
            if (n_surv) memcpy(surv.data(), (const char *)ctx->pinned + 64, n_surv * sizeof(csv_split_survivor));
        } else {
            const uint64_t n_nodes = st->n_nodes;
            // (room for one hash per record of these contigs was set aside by _begin; a run's other contigs can add more)
            struct TmpBuf { void *p = nullptr; ~TmpBuf() { if (p) (void)hipFree(p); } } big_supp;
            uint64_t *d_supp = st->d_supp;
            if (n_supp > st->total_reads) {
                if (hipMalloc(&big_supp.p, n_supp * 8) != hipSuccess) { (void)hipGetLastError(); big_supp.p = nullptr; ctx->err = "hipMalloc failed (supplementary hashes)"; return CSV_ENOMEM; }
                d_supp = (uint64_t *)big_supp.p;
            }
            // (through the context's page-locked block: a pageable copy is staged by the runtime under a lock the lanes' launches also take)
            prc = ensure_pinned(ctx, std::max<size_t>(n_supp * 8, 4096) + 64);
            if (prc) return prc;
            memcpy(ctx->pinned, supp_hash, n_supp * 8);
            CSV_HIP(ctx, hipMemcpyAsync(d_supp, ctx->pinned, n_supp * 8, hipMemcpyHostToDevice, s));
            CSV_HIP(ctx, wait_stream(s));                    // (the block is reused for the set sizes below)
            if ((prc = split_order_tail(ctx, st, d_supp, n_supp, false))) return prc;
            CSV_HIP(ctx, hipMemcpyAsync(ctx->pinned, st->d_count, 8, hipMemcpyDeviceToHost, s));
            CSV_HIP(ctx, wait_stream(s));
            const uint64_t n_surv = *(const unsigned long long *)ctx->pinned;
            if (n_surv > n_nodes) { ctx->err = "split_order: survivor count out of range"; return CSV_EHIP; }
            surv.resize(n_surv);
            if (n_surv) {
                if ((prc = ensure_pinned(ctx, n_surv * sizeof(csv_split_survivor) + 64))) return prc;
                CSV_HIP(ctx, hipMemcpyAsync(ctx->pinned, st->d_out, n_surv * sizeof(csv_split_survivor), hipMemcpyDeviceToHost, s));
                CSV_HIP(ctx, wait_stream(s));
                memcpy(surv.data(), ctx->pinned, n_surv * sizeof(csv_split_survivor));
            }
        }
        std::sort(surv.begin(), surv.end(), [](const csv_split_survivor &a, const csv_split_survivor &b) { return a.contig != b.contig ? a.contig < b.contig : a.pos < b.pos; });
        for (const csv_split_survivor &v : surv) st->off[v.contig + 1]++;
        for (int c = 0; c < n_contigs; c++) st->off[(size_t)c + 1] += st->off[(size_t)c];
        st->finished = true;
    }
    for (int c = 0; c <= n_contigs; c++) out_off[c] = st->off[(size_t)c];
    if (st->surv.size() > capacity) { ctx->err = "split_order: output capacity too small"; return CSV_ECAPACITY; }      // (the state stays: _finish again with more room)
    for (size_t i = 0; i < st->surv.size(); i++) out_rec[i] = st->surv[i].rec;
    delete st; ctx->split_state = nullptr;
    return CSV_OK;
}

int csvgpu_split_order_begin(csv_ctx *ctx, int n_contigs, csv_shard *const *shards, uint8_t min_mapq)
{
    return split_order_begin(ctx, n_contigs, shards, min_mapq, -1);
}

int csvgpu_split_order_begin_self(csv_ctx *ctx, int n_contigs, csv_shard *const *shards, uint8_t min_mapq)
{
    return split_order_begin(ctx, n_contigs, shards, min_mapq, -1, true);
}

int csvgpu_split_order_finish(csv_ctx *ctx, const uint64_t *supp_hash, uint64_t n_supp, uint32_t *out_rec, uint64_t capacity, uint64_t *out_off)
{
    return split_order_finish(ctx, supp_hash, n_supp, out_rec, capacity, out_off);
}

int csvgpu_split_order(csv_ctx *ctx, int n_contigs, csv_shard *const *shards, uint8_t min_mapq, const uint64_t *supp_hash, uint64_t n_supp,
                       uint32_t *out_rec, uint64_t capacity, uint64_t *out_off)
{
    if (!ctx) return CSV_EINVAL;
    if (!out_off || (n_contigs > 0 && !shards) || (n_supp && !supp_hash) || (capacity && !out_rec)) { ctx->err = "split_order: null array"; return CSV_EINVAL; }
    if (n_contigs >= 0 && (uint32_t)n_contigs <= SO_MAX_CONTIGS) for (int c = 0; c <= n_contigs; c++) out_off[c] = 0;
    for (uint64_t i = 1; i < n_supp; i++) if (supp_hash[i] <= supp_hash[i - 1]) { ctx->err = "split_order: supp_hash must be sorted and distinct"; return CSV_EINVAL; }
    int rc = split_order_begin(ctx, n_contigs, shards, min_mapq, (int64_t)n_supp);
    if (rc) return rc;
    rc = split_order_finish(ctx, supp_hash, n_supp, out_rec, capacity, out_off);
    if (rc) { delete ctx->split_state; ctx->split_state = nullptr; }         // (one call: nothing is kept for a retry, the caller repeats it with the size from out_off)
    return rc;
}
