// snp_table.hip — resident SNP tables: creation (host and device arrays), release, and the query seam (kernels/snptable.hip). The copy-number
// pass that reads them is in copynumber.hip.
#include <new>

#include "glue.hpp"

using namespace csv;

namespace {

struct BuildWs { uint64_t *baf = nullptr, *pfb = nullptr; uint8_t *has = nullptr; int32_t *marks = nullptr, *pm = nullptr; void *pm_tmp = nullptr; unsigned int *flag = nullptr; };

// dev: the records are device arrays (copied device to device); else host arrays (through the page-locked block, in pieces). dev_af: the
// same for the population arrays of the first-hit kind.
csv_snp_table *table_create(csv_ctx *ctx, const char *what, bool dev, bool dev_af, bool hits, const uint32_t *pos, const double *baf, const double *pfb, const uint8_t *has_pfb,
                            const uint32_t *af_pos, const double *af, uint64_t n, uint64_t n_af)
{
    if (!ctx) return nullptr;
    auto fail = [&](const std::string &msg) { ctx->err = std::string(what) + ": " + msg; return (csv_snp_table *)nullptr; };
    if (n >= 0xffffffffull || n_af >= 0xffffffffull) return fail("2^32 - 1 or more records");
    if ((n && (!pos || !baf)) || (n_af && (!af_pos || !af))) return fail("null array");
    if (hipSetDevice(ctx->device) != hipSuccess) { (void)hipGetLastError(); return fail("no device"); }
    const bool flagged = !hits && has_pfb && n;
    BuildWs w;
    if (arena_reserve_for(ctx, ctx->arena, what, [&](Arena &a) {
            return take(a, w.flag, 256) && take(a, w.baf, n * 8) && (!flagged || (take(a, w.pfb, pfb ? n * 8 : 0) && take(a, w.has, n) && take(a, w.marks, n * 4) &&
                                                                                take(a, w.pm, n * 4) && take(a, w.pm_tmp, prefix_max_tmp_bytes(n))));
        })) return nullptr;
    std::unique_ptr<csv_snp_table> t(new (std::nothrow) csv_snp_table());
    if (!t) return fail("no memory");
    t->device = ctx->device; t->hits = hits; t->n = n; t->n_af = n_af;
    const size_t o_pos = 0, o_baf = align_up(n * 4, 256), o_pfb = o_baf + align_up(n * 8, 256), o_afp = o_pfb + (hits ? 0 : align_up(n * 8, 256)),
                 o_af = o_afp + align_up(n_af * 4, 256), bytes = o_af + align_up(n_af * 8, 256);
    if (test_fail_alloc() || hipMalloc((void **)&t->block, bytes ? bytes : 256) != hipSuccess) { (void)hipGetLastError(); return fail("hipMalloc failed"); }
    char *const blk = t->block;
    auto release = [&](const std::string &msg) { (void)hipStreamSynchronize(ctx->stream); (void)hipFree(blk); return fail(msg); };
    uint32_t *d_pos = (uint32_t *)(blk + o_pos), *d_afp = (uint32_t *)(blk + o_afp);
    uint64_t *d_baf = (uint64_t *)(blk + o_baf), *d_pfb = hits ? nullptr : (uint64_t *)(blk + o_pfb), *d_af = (uint64_t *)(blk + o_af);
    hipStream_t s = ctx->stream;
    Transfer tr(ctx);
    if (tr.open(what)) { (void)hipFree(blk); return nullptr; }
    auto put = [&](void *dst, const void *src, size_t b, bool on_dev) -> bool {
        if (!b) return true;
        if (!on_dev) return tr.up(dst, src, b) == CSV_OK;
        if (hipMemcpyAsync(dst, src, b, hipMemcpyDeviceToDevice, s) == hipSuccess) return true;
        ctx->err = std::string(what) + ": device copy failed"; (void)hipGetLastError();
        return false;
    };
    if (hipMemsetAsync(w.flag, 0, 256, s) != hipSuccess) return release("memset failed");
    if (!put(d_pos, pos, n * 4, dev) || !put(w.baf, baf, n * 8, dev) || !put(d_afp, af_pos, n_af * 4, dev_af) || !put(d_af, af, n_af * 8, dev_af) ||
        (flagged && (!put(w.has, has_pfb, n, dev) || (pfb && !put(w.pfb, pfb, n * 8, dev))))) {
        const std::string why = ctx->err;                                       // (the copy's own text)
        release("");
        ctx->err = why;
        return nullptr;
    }
    if (!hits && !flagged && n && hipMemsetAsync(d_pfb, 0, n * 8, s) != hipSuccess) return release("memset failed");
    {
        TimerScope ts(ctx, CSV_K_MISC);
        launch_check_sorted_u32(s, d_pos, n, w.flag);
        launch_check_sorted_u32(s, d_afp, n_af, w.flag + 1);
        launch_snp_resolve(s, d_pos, w.baf, pfb ? w.pfb : nullptr, flagged ? w.has : nullptr, (uint32_t)n, w.marks, w.pm, w.pm_tmp, d_baf, flagged ? d_pfb : nullptr);
    }
    if (hipGetLastError() != hipSuccess) return release("a kernel launch failed");
    unsigned int unsorted[2] = {0, 0};
    if (tr.peek(unsorted, w.flag, sizeof unsorted)) { (void)hipFree(blk); return nullptr; }          // (waits: the table is complete behind it)
    if (unsorted[0]) return release("positions are not ascending");
    if (unsorted[1]) return release("af_pos is not ascending");
    t->pos = d_pos; t->baf = d_baf; t->pfb = d_pfb; t->af_pos = n_af ? d_afp : nullptr; t->af = n_af ? d_af : nullptr;
    return t.release();
}

}  // namespace

csv_snp_table *csvgpu_snp_table_create(csv_ctx *ctx, const uint32_t *pos, const double *baf, const double *pfb, const uint8_t *has_pfb, uint64_t n)
{
    return table_create(ctx, "snp_table_create", false, false, false, pos, baf, pfb, has_pfb, nullptr, nullptr, n, 0);
}
csv_snp_table *csvgpu_snp_table_create_hits(csv_ctx *ctx, const uint32_t *pos, const double *baf, const uint32_t *af_pos, const double *af, uint64_t n, uint64_t n_af)
{
    return table_create(ctx, "snp_table_create_hits", false, false, true, pos, baf, nullptr, nullptr, af_pos, af, n, n_af);
}
csv_snp_table *csvgpu_snp_table_create_dev(csv_ctx *ctx, const uint32_t *d_pos, const double *d_baf, const double *d_pfb, const uint8_t *d_has_pfb, uint64_t n)
{
    return table_create(ctx, "snp_table_create_dev", true, true, false, d_pos, d_baf, d_pfb, d_has_pfb, nullptr, nullptr, n, 0);
}
csv_snp_table *csvgpu_snp_table_create_hits_dev(csv_ctx *ctx, const uint32_t *d_pos, const double *d_baf, const uint32_t *d_af_pos, const double *d_af, uint64_t n,
                                                uint64_t n_af)
{
    return table_create(ctx, "snp_table_create_hits_dev", true, true, true, d_pos, d_baf, nullptr, nullptr, d_af_pos, d_af, n, n_af);
}

void csvgpu_snp_table_free(csv_ctx *ctx, csv_snp_table *table)
{
    if (!table) return;
    (void)hipSetDevice(table->device);
    if (ctx) (void)hipStreamSynchronize(ctx->stream);
    (void)hipFree(table->block);
    delete table;
}

uint64_t csvgpu_snp_table_size(const csv_snp_table *table) { return table ? table->n : 0; }

namespace csv {
csv_snp_table *snp_table_hits_mixed(csv_ctx *ctx, const char *what, const uint32_t *d_pos, const double *d_baf, const uint32_t *af_pos, const double *af, uint64_t n,
                                    uint64_t n_af)
{
    return table_create(ctx, what, true, false, true, d_pos, d_baf, nullptr, nullptr, af_pos, af, n, n_af);
}
SnpTabDev snp_table_dev(const csv_snp_table *t)
{
    SnpTabDev d{};
    if (!t || !t->n) return d;
    d.pos = t->pos; d.baf = t->baf; d.pfb = t->pfb; d.af_pos = t->af_pos; d.af = t->af; d.n = (uint32_t)t->n; d.n_af = (uint32_t)t->n_af;
    return d;
}
}  // namespace csv

int csvgpu_snp_table_query(csv_ctx *ctx, const csv_snp_table *table, const uint32_t *region_start, const uint32_t *region_end, uint64_t n_regions,
                           uint64_t *snp_off, uint32_t *pos, double *baf, double *pfb, uint64_t *n)
{
    if (!ctx) return CSV_EINVAL;
    auto bad = [&](const char *msg) { ctx->err = std::string("snp_table_query: ") + msg; return (int)CSV_EINVAL; };
    if (!table || !snp_off || !n) return bad("null argument");
    if (table->device != ctx->device) return bad("a table of another device");
    if (n_regions >= 0xffffffffull) return bad("2^32 - 1 or more regions");
    if (n_regions && (!region_start || !region_end)) return bad("null array");
    if (*n && (!pos || !baf || !pfb)) return bad("null array with a capacity");
    const uint64_t R = n_regions, cap = *n;
    if (R == 0) { *n = 0; snp_off[0] = 0; return CSV_OK; }
    (void)hipSetDevice(ctx->device);
    CnTabWs w;
    uint64_t S = 0;
    // (the copy-number layout's first part is the plan's; the records behind it are this call's own)
    auto carve = [&](Arena &a) { return carve_cn_tables(a, R, 1, 0, 0, false, w) && take(a, w.spos, S * 4) && take(a, w.sbaf, S * 8) && take(a, w.spfb, S * 8); };
    int rc;
    if ((rc = arena_reserve_for(ctx, ctx->arena, "snp_table_query", carve))) return rc;
    Transfer t(ctx);
    if ((rc = t.open("snp_table_query"))) return rc;
    hipStream_t s = ctx->stream;
    const CnUpLayout L(R, 1);
    const SnpTabDev td = snp_table_dev(table);
    const uint32_t roff[2] = {0, (uint32_t)R};
    auto plan = [&]() -> int {
        int rc2;
        if ((rc2 = t.up(w.up + L.rs, region_start, R * 4)) || (rc2 = t.up(w.up + L.re, region_end, R * 4)) || (rc2 = t.up(w.up + L.tabs, &td, sizeof td)) ||
            (rc2 = t.up(w.up + L.roff, roff, sizeof roff))) return rc2;
        CnPlan p = w.p;
        p.ssf = nullptr; p.rsh = nullptr;
        TimerScope ts(ctx, CSV_K_MISC);
        launch_cn_plan(s, p, (uint32_t)R, 1);
        return CSV_OK;
    };
    if ((rc = plan())) return rc;
    CnPlanHead h;
    if ((rc = t.peek(&h, w.p.head, sizeof h))) return rc;
    if (h.S >= 0xffffffffull) return bad("2^32 - 1 or more records");
    *n = h.S;
    if (h.S > cap) { ctx->err = "snp_table_query: capacity too small"; return CSV_ECAPACITY; }
    S = h.S;
    // (a grown arena is a new allocation, possibly at the old address: the pointer says nothing, the capacity rises with every growth)
    const size_t cap_before = ctx->arena.cap;
    if ((rc = arena_reserve_for(ctx, ctx->arena, "snp_table_query", carve))) return rc;
    if (ctx->arena.cap != cap_before && (rc = plan())) return rc;            // the arena grew: the plan again, into the new one
    {
        CnPlan p = w.p;
        p.ssf = nullptr; p.rsh = nullptr;
        TimerScope ts(ctx, CSV_K_MISC);
        launch_snp_gather(s, p, (uint32_t)R, (uint32_t)S, w.spos, w.sbaf, w.spfb);
    }
    CSV_HIP(ctx, hipGetLastError());
    std::vector<uint32_t> off32(R + 1);
    if ((rc = t.down(off32.data(), w.p.soff, (R + 1) * 4)) || (rc = t.down(pos, w.spos, S * 4)) || (rc = t.down(baf, w.sbaf, S * 8)) || (rc = t.down(pfb, w.spfb, S * 8))) return rc;
    if ((rc = t.wait())) return rc;
    for (uint64_t r = 0; r <= R; r++) snp_off[r] = off32[r];
    return CSV_OK;
}
