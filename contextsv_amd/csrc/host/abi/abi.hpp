// abi.hpp — what the files of host/abi/ share: extern "C" hooks over the C++ host mirror so the parity tests and bench.py (ctypes) can
// drive it. POD only (csvhost_abi.h); every function returns 0 or -1 (message via csvhost_last_error()) unless it says otherwise.
#pragma once
#include <algorithm>
#include <chrono>
#include <cstring>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

#include "../bam_io.h"
#include "../fasta_query.h"
#include "../sv_caller.h"
#include "../synth.h"
#include "csvhost_abi.h"
#include "run_options.hpp"

namespace csvhost_abi {
// the calling thread's last message (csvhost_last_error returns it: Python asks on the thread that failed)
inline std::string &last_error() { thread_local std::string e; return e; }
inline void set_error(const std::string &what) { last_error() = what; }
}
using csvhost_abi::set_error;
#define GUARD(...) try { __VA_ARGS__; return 0; } catch (const std::exception &e) { set_error(e.what()); return -1; }

// handles that more than one file takes
struct csvhost_synth { SynthShard sh; };
struct csvhost_fasta { ReferenceGenome g; };
struct csvhost_bam {
    BamReader r; std::vector<BamShard> shards; std::string names;
    csv_ctx *inflate_ctx = nullptr;          // csvhost_bam_set_device_inflate / _unpack: the reader's own context, one for both
    int ctx_device = -1;
    bool inflate_on = false, unpack_on = false, shard_on = false;
    void drop_residents() { for (BamShard &s : shards) s.resident.reset(); }      // (they are freed through inflate_ctx: before it goes)
    ~csvhost_bam() { drop_residents(); if (inflate_ctx) csvgpu_destroy(inflate_ctx); }
};

inline SVCall from_pod(const csvhost_call &c)
{
    SVCall s(c.start, c.end, (SVType)c.sv_type, std::to_string(c.id), SVEvidenceFlags(c.aln_flags), (Genotype)c.genotype,
             c.hmm_likelihood, c.cn_state, c.aln_offset, c.cluster_size);
    return s;   // the id rides in alt_allele so it survives every copy the merge makes
}
// every field but the string; id = -1 (alt_allele is not read)
inline csvhost_call flat_call(const SVCall &s)
{
    csvhost_call c;
    c.start = s.start; c.end = s.end; c.sv_type = (int32_t)s.sv_type; c.cluster_size = s.cluster_size; c.hmm_likelihood = s.hmm_likelihood;
    c.id = -1;
    c.aln_flags = (uint32_t)s.aln_type.to_ulong(); c.genotype = (int32_t)s.genotype; c.cn_state = s.cn_state; c.aln_offset = s.aln_offset;
    return c;
}
// flat_call + the id that from_pod put into alt_allele (-1 where the ALT was rewritten): the merge and copy-number hooks only
inline csvhost_call to_pod(const SVCall &s)
{
    csvhost_call c = flat_call(s);
    try { c.id = std::stoll(s.alt_allele); } catch (...) {}
    return c;
}
// 0 "<DEL>", 1 "<INS>", 2 literal sequence
inline uint8_t alt_tag(const SVCall &c) { return c.alt_allele == "<DEL>" ? 0 : (c.alt_allele == "<INS>" ? 1 : 2); }

inline void fill(csvhost_chr_stats &st, const ChrStats &cs, uint64_t n_calls)
{
    st.n_signatures = cs.n_signatures; st.n_del = cs.n_del; st.n_ins = cs.n_ins; st.depth_sum = cs.depth_sum;
    st.depth_nonzero = cs.depth_nonzero; st.min_pts = cs.dbscan_min_pts; st.mean_cov = cs.mean_chr_cov;
    st.ms_device = cs.ms_device; st.ms_host_merge = cs.ms_host_merge; st.n_calls = n_calls;
}

// at most cap bytes of t into buf; the full length through the return value
inline uint64_t copy_text(const std::string &t, char *buf, uint64_t cap)
{
    if (buf && cap) memcpy(buf, t.data(), (size_t)std::min<uint64_t>(cap, t.size()));
    return t.size();
}
// "<start>\t<end>\t<ALT>\n" per call (the string fields the POD view drops)
inline std::string alt_lines(const std::vector<SVCall> &calls)
{
    std::string t;
    for (const SVCall &c : calls) t += std::to_string(c.start) + "\t" + std::to_string(c.end) + "\t" + c.alt_allele + "\n";
    return t;
}
// '\n'-separated names; n < 0: as many as there are (null or empty: none)
inline std::vector<std::string> split_lines(const char *p, int64_t n = -1)
{
    std::vector<std::string> v;
    for (int64_t i = 0; n < 0 ? (p && *p) : i < n; i++) {
        const char *e = strchr(p, '\n');
        v.emplace_back(p, e ? (size_t)(e - p) : strlen(p));
        p = e ? e + 1 : p + strlen(p);
    }
    return v;
}

// with a genome and an output directory the run ends by writing <vcf_dir>/output.vcf
inline void set_vcf_output(RunParams &P, const csvhost_fasta *fasta, const char *vcf_dir, const char *gap_path, const char *file_date)
{
    if (!fasta || !vcf_dir) return;
    P.ref_genome = &fasta->g;
    P.vcf.output_dir = vcf_dir; P.vcf.assembly_gaps = gap_path ? gap_path : ""; P.vcf.file_date = file_date ? file_date : "";
}

CHMM chmm_from_pod(const csv_hmm *h);                                                                            // copynumber.cpp
SNPTable snp_table(const uint32_t *pos, const double *baf, const double *pfb, const uint8_t *has_pfb, uint64_t n);
