// split.cpp — split-read signatures (findSplitSVSignatures mirror) and the tables, groups and fits behind them
#include "abi.hpp"
#include "../dbscan.h"

// the three table hooks answer with the device library's codes: -1 (CSV_EINVAL) for std::invalid_argument, -100 for anything else
#define GUARD_CODES(...) try { __VA_ARGS__; return 0; } catch (const std::invalid_argument &e) { set_error(e.what()); return CSV_EINVAL; \
    } catch (const std::exception &e) { set_error(e.what()); return -100; }

extern "C" {

struct csvhost_split_call { uint32_t start, end; int32_t sv_type, cluster_size, aln_offset; uint32_t aln_flags; int32_t tid; };

// records in file order; qname = "r<qname_id>". Output sorted by contig id, each contig's calls in the reference's order.
// device_groups != 0: the overlap groups come from csvgpu_split_groups on `ctx` (SplitParams::device_groups) instead of the host tree.
// device_fits != 0: the groups' point sets, fits, largest clusters and medians come from csvgpu_split_fits (SplitParams::device_fits) — with both
// set, groups and fits from csvgpu_split_groups_fits.
int csvhost_split_signatures_dev(csv_ctx *ctx, uint64_t n, const int32_t *tid, const int32_t *pos, const uint16_t *flag, const uint8_t *mapq,
                                 const int32_t *ref_end, const int32_t *q_start, const int32_t *q_end, const uint32_t *qname_id, int n_targets,
                                 int min_mapq, int device_groups, int device_fits, csvhost_split_call *out, uint64_t cap, uint64_t *n_out)
{
    GUARD({
        csvhost::set_context(ctx);
        std::vector<SplitRecord> rec(n);
        std::vector<std::string> qn(n), targets((size_t)n_targets);
        for (int t = 0; t < n_targets; t++) targets[(size_t)t] = "contig" + std::to_string(t);
        for (uint64_t i = 0; i < n; i++) {
            rec[i] = SplitRecord{tid[i], pos[i], flag[i], mapq[i], ref_end[i], q_start[i], q_end[i]};
            qn[i] = "r" + std::to_string(qname_id[i]);
        }
        SplitParams p; p.min_mapq = min_mapq;
        std::unique_ptr<SplitGroupSource> dev_groups;
        if (device_groups) { dev_groups = makeDeviceGroupSource(ctx); p.device_groups = dev_groups.get(); }
        std::unique_ptr<SplitFitSource> dev_fits;
        if (device_fits) { dev_fits = makeDeviceFitSource(ctx); p.device_fits = dev_fits.get(); }
        std::unordered_map<std::string, std::vector<SVCall>> calls;
        findSplitSVSignatures(rec, qn, targets, p, calls);
        uint64_t k = 0;
        for (int t = 0; t < n_targets; t++) {
            auto it = calls.find(targets[(size_t)t]);
            if (it == calls.end()) continue;
            for (const SVCall &c : it->second) {
                if (k < cap) out[k] = csvhost_split_call{c.start, c.end, (int32_t)c.sv_type, c.cluster_size, c.aln_offset, (uint32_t)c.aln_type.to_ulong(), t};
                k++;
            }
        }
        *n_out = k;
    })
}

int csvhost_split_signatures_opts(csv_ctx *ctx, uint64_t n, const int32_t *tid, const int32_t *pos, const uint16_t *flag, const uint8_t *mapq,
                                  const int32_t *ref_end, const int32_t *q_start, const int32_t *q_end, const uint32_t *qname_id, int n_targets,
                                  int min_mapq, int device_groups, csvhost_split_call *out, uint64_t cap, uint64_t *n_out)
{
    return csvhost_split_signatures_dev(ctx, n, tid, pos, flag, mapq, ref_end, q_start, q_end, qname_id, n_targets, min_mapq, device_groups, 0, out, cap, n_out);
}

int csvhost_split_signatures(csv_ctx *ctx, uint64_t n, const int32_t *tid, const int32_t *pos, const uint16_t *flag, const uint8_t *mapq,
                             const int32_t *ref_end, const int32_t *q_start, const int32_t *q_end, const uint32_t *qname_id, int n_targets,
                             int min_mapq, csvhost_split_call *out, uint64_t cap, uint64_t *n_out)
{
    return csvhost_split_signatures_opts(ctx, n, tid, pos, flag, mapq, ref_end, q_start, q_end, qname_id, n_targets, min_mapq, 0, out, cap, n_out);
}

// The record references that SplitPass::prepare() computes (csv_split_refs' arrays, what SplitParams::device_tables is given), from the inputs of
// csvhost_split_signatures without the intervals; needs no GPU. Segment t = tid t: seg_off [n_targets + 1]; record indices count within the tid's
// records in file order (a contig uploaded as its own shard); supp_rec / supp_tid say which record an entry on another tid is (no device call reads
// them). The member arrays have room for n entries (supp_off: n + 1), the entry arrays for `cap`; n_out[0] = members, n_out[1] = entries; -5 (CSV_ECAPACITY)
// with only n_out written when there are more entries than `cap`.
int csvhost_split_refs(uint64_t n, const int32_t *tid, const int32_t *pos, const uint16_t *flag, const uint8_t *mapq, const uint32_t *qname_id, int n_targets,
                       int min_mapq, uint64_t *seg_off, uint32_t *member_rec, uint64_t *supp_off, uint32_t *supp_rec, uint8_t *supp_where, int32_t *supp_tid,
                       uint64_t cap, uint64_t *n_out)
{
    GUARD_CODES({
        std::vector<SplitRecord> rec(n);
        std::vector<std::string> qn(n);
        for (uint64_t i = 0; i < n; i++) {
            rec[i] = SplitRecord{tid[i], pos[i], flag[i], mapq[i], 0, 0, 0};
            qn[i] = "r" + std::to_string(qname_id[i]);
        }
        SplitParams p; p.min_mapq = min_mapq;
        SplitRefTables R;
        std::vector<uint64_t> so;
        splitReferences(rec, qn, (size_t)(n_targets > 0 ? n_targets : 0), p, R, so);
        n_out[0] = R.member_rec.size(); n_out[1] = R.supp_rec.size();
        if (R.member_rec.size() > n) { set_error("split_refs: more members than records"); return -100; }
        if (R.supp_rec.size() > cap) { set_error("split_refs: entry capacity too small"); return CSV_ECAPACITY; }
        std::copy(so.begin(), so.end(), seg_off);
        std::copy(R.member_rec.begin(), R.member_rec.end(), member_rec);
        std::copy(R.supp_off.begin(), R.supp_off.end(), supp_off);
        std::copy(R.supp_rec.begin(), R.supp_rec.end(), supp_rec);
        std::copy(R.supp_where.begin(), R.supp_where.end(), supp_where);
        std::copy(R.supp_tid.begin(), R.supp_tid.end(), supp_tid);
    })
}

// The outputs of csvgpu_split_groups computed by the host's interval tree (the path without SplitParams::device_groups); needs no GPU.
// seg_group_off [n_seg + 1]; group_off [seg_off[n_seg] + 1] (entries 0 .. seg_group_off[n_seg] written); *n_members: in capacity, out count
// required; -5 (CSV_ECAPACITY) when members[] is too small, -1 (CSV_EINVAL) on end < start or descending offsets.
int csvhost_split_groups_host(const int32_t *start, const int32_t *end, const uint64_t *seg_off, uint64_t n_seg, uint64_t *seg_group_off,
                              uint64_t *group_off, uint32_t *members, uint64_t *n_members)
{
    GUARD_CODES({
        std::vector<uint64_t> sgo, go;
        std::vector<uint32_t> mem;
        splitGroupsHost(start, end, seg_off, n_seg, sgo, go, mem);
        const uint64_t cap = *n_members;
        *n_members = mem.size();
        if (mem.size() > cap) { set_error("split_groups_host: members capacity too small"); return CSV_ECAPACITY; }
        std::copy(sgo.begin(), sgo.end(), seg_group_off);
        std::copy(go.begin(), go.end(), group_off);
        std::copy(mem.begin(), mem.end(), members);
    })
}

// The records of csvgpu_split_fits by the host route (splitFitsHost: point sets and reductions on this thread, one csvgpu_dbscan_1d batch on `ctx`);
// out[seg_group_off[n_seg]] records of 64 bytes (csv_split_fit). -1 (CSV_EINVAL) on tables that do not fit.
int csvhost_split_fits_host(csv_ctx *ctx, const csv_split_tables *t, const uint64_t *seg_off, uint64_t n_seg, const uint64_t *seg_group_off, const uint64_t *group_off,
                            const uint32_t *members, double eps, int min_pts, csv_split_fit *out)
{
    GUARD_CODES({
        csvhost::set_context(ctx);
        static_assert(sizeof(SplitFit) == sizeof(csv_split_fit), "SplitFit is csv_split_fit");
        SplitFitTables T;
        const uint64_t nm = t->n_members, ns = t->n_supp;
        T.start.assign(t->start, t->start + nm); T.end.assign(t->end, t->end + nm); T.q_start.assign(t->q_start, t->q_start + nm); T.q_end.assign(t->q_end, t->q_end + nm);
        T.reverse.assign(t->reverse, t->reverse + nm); T.supp_off.assign(t->supp_off, t->supp_off + nm + 1);
        T.supp_start.assign(t->supp_start, t->supp_start + ns); T.supp_end.assign(t->supp_end, t->supp_end + ns);
        T.supp_q_start.assign(t->supp_q_start, t->supp_q_start + ns); T.supp_q_end.assign(t->supp_q_end, t->supp_q_end + ns);
        T.supp_flags.assign(t->supp_flags, t->supp_flags + ns);
        const uint64_t n_groups = seg_group_off[n_seg];
        std::vector<uint64_t> so(seg_off, seg_off + n_seg + 1), sgo(seg_group_off, seg_group_off + n_seg + 1), go(group_off, group_off + n_groups + 1);
        std::vector<uint32_t> mem(members, members + go[n_groups]);
        std::vector<SplitFit> fits;
        splitFitsHost(T, so, sgo, go, mem, eps, min_pts, fits);
        if (!fits.empty()) memcpy(out, fits.data(), fits.size() * sizeof(SplitFit));
    })
}

}  // extern "C"
