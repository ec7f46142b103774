// merge.cpp — mergeSVs and friends on POD calls (the id rides in alt_allele: from_pod / to_pod)
#include "abi.hpp"
#include "../dbscan.h"

static std::vector<SVCall> from_pods(const csvhost_call *calls, uint64_t n)
{
    std::vector<SVCall> v; v.reserve(n);
    for (uint64_t i = 0; i < n; i++) v.push_back(from_pod(calls[i]));
    return v;
}

extern "C" {

// mergeSVs through the GPU (DBSCAN::fit -> csvgpu_dbscan_iv). out capacity >= n. *n_out = merged count.
int csvhost_merge_svs(const csvhost_call *calls, uint64_t n, double eps, int32_t min_pts, int keep_noise, csvhost_call *out, uint64_t *n_out)
{
    GUARD({
        std::vector<SVCall> v = from_pods(calls, n);
        mergeSVs(v, eps, min_pts, keep_noise != 0);
        for (size_t i = 0; i < v.size(); i++) out[i] = to_pod(v[i]);
        *n_out = v.size();
    })
}

// the representative choice alone, labels supplied (CPU-testable: no device involved)
int csvhost_merge_type_with_labels(const csvhost_call *calls, const int32_t *labels, uint64_t n, int keep_noise, csvhost_call *out, uint64_t *n_out)
{
    GUARD({
        std::vector<SVCall> v = from_pods(calls, n), merged;
        mergeTypeWithLabels(v, labels, keep_noise != 0, merged);
        for (size_t i = 0; i < merged.size(); i++) out[i] = to_pod(merged[i]);
        *n_out = merged.size();
    })
}

int csvhost_merge_duplicates(csvhost_call *calls, uint64_t n, uint64_t *n_out)
{
    GUARD({
        std::vector<SVCall> v = from_pods(calls, n);
        mergeDuplicateSVs(v);
        for (size_t i = 0; i < v.size(); i++) calls[i] = to_pod(v[i]);
        *n_out = v.size();
    })
}

// addSVCall order check: insert the calls one by one, return the resulting order of ids
int csvhost_add_sv_calls(const csvhost_call *calls, uint64_t n, int64_t *ids_out, uint64_t *n_out)
{
    GUARD({
        std::vector<SVCall> v;
        for (uint64_t i = 0; i < n; i++) { SVCall c = from_pod(calls[i]); addSVCall(v, c); }
        for (size_t i = 0; i < v.size(); i++) ids_out[i] = std::stoll(v[i].alt_allele);
        *n_out = v.size();
    })
}

// The host half alone (no device): ordered signatures + labels -> merged calls; `reps` timed repetitions, *ms = mean time of one.
int csvhost_merge_ordered(const csv_sig *sig, const int32_t *labels, uint64_t n_del, uint64_t n_ins, int reps, csvhost_call *out, uint64_t cap,
                          uint64_t *n_out, double *ms)
{
    GUARD({
        std::vector<SVCall> calls;
        const auto t0 = std::chrono::steady_clock::now();
        for (int r = 0; r < std::max(reps, 1); r++) SVCaller::mergeOrdered(sig, labels, n_del, n_ins, nullptr, calls);
        if (ms) *ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count() / std::max(reps, 1);
        for (size_t i = 0; i < calls.size() && i < cap; i++) out[i] = to_pod(calls[i]);
        *n_out = calls.size();
    })
}

}  // extern "C"
