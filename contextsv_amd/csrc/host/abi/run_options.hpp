// run_options.hpp — csvhost_run_options <-> RunParams, each direction written once. Inline and field-to-field only, so that
// tools/fuzz/run_options_check.cpp can hold the two together without linking the mirror.
#pragma once
#include <stdexcept>

#include "../sv_caller.h"
#include "csvhost_abi.h"

// X(field of csvhost_run_options, the RunParams member of the same name, its type there)
#define CSVHOST_RUN_OPTION_FIELDS(X) \
    X(dbscan_epsilon, dbscan_epsilon, double) X(dbscan_min_pts_pct, dbscan_min_pts_pct, double) \
    X(sample_size, sample_size, int) X(min_cnv_length, min_cnv_length, uint32_t) X(host_threads, host_threads, int) \
    X(cigar_cn, cigar_cn, bool) X(split_svs, split_svs, bool) X(merge_split_svs, merge_split_svs, bool) X(merge_final_svs, merge_final_svs, bool) \
    X(split_order_on_device, split_order_on_device, bool) X(overlap_split_prepare, overlap_split_prepare, bool) \
    X(split_groups_on_device, split_groups_on_device, bool) X(split_fits_on_device, split_fits_on_device, bool) \
    X(split_tables_on_device, split_tables_on_device, bool) X(cn_observations_on_device, cn_observations_on_device, bool) \
    X(inflate_on_device, inflate_on_device, bool) X(inflate_device, inflate_device, int) \
    X(unpack_on_device, unpack_on_device, bool) X(shard_on_device, shard_on_device, bool) X(save_cnv, save_cnv, bool) \
    X(early_batches, schedule.early_batches, RunSchedule::EarlyBatches) X(split_beside_pass, schedule.split_beside_pass, bool) \
    X(split_order_self, schedule.split_order_self, bool) X(prepare_delay_ms, schedule.prepare_delay_ms, int)

// the defaults are RunParams' own
inline void run_options_from(const RunParams &P, csvhost_run_options &o)
{
    o.size = (uint32_t)sizeof o;
#define X(field, member, type) o.field = (decltype(o.field))P.member;
    CSVHOST_RUN_OPTION_FIELDS(X)
#undef X
}

inline RunParams run_params_from(const csvhost_run_options &o)
{
    if (o.size != sizeof o) throw std::invalid_argument("csvhost_run_options: size " + std::to_string(o.size) + ", this library's is " + std::to_string(sizeof o));
    if (o.early_batches < 0 || o.early_batches > 3) throw std::invalid_argument("csvhost_run_options: early_batches must be 0-3, not " + std::to_string(o.early_batches));
    RunParams P;
#define X(field, member, type) P.member = (type)o.field;
    CSVHOST_RUN_OPTION_FIELDS(X)
#undef X
    return P;
}
