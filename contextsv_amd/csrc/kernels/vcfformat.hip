// vcfformat.hip — the VCF writer's record lines assembled in HBM (csvgpu_vcf_format; api/vcf_format.hip). The rules are vcf_format_core.hpp,
// shared with the host-side check; here is only how the lanes share the calls and the text.
//   vf_size                a lane per call: its contig by bisection of the contigs' first calls, the core's disposition and fields with the
//                          gap search, the depth at POS from the contig's resident map (csvgpu_depth_lookup_resident's value), the line's
//                          exact length (0 for a call without a line) and its status byte. The text's bytes are summed in a 64-bit word —
//                          the 32-bit lengths' exclusive sum of sort.hip then gives the lines' offsets, valid below 2^32 —; the first
//                          refused call, by call order, leaves its index and reason in the head.
//   vf_write               a lane owns an aligned 16-byte piece of the TEXT, not a line: the line of its first byte by bisection of the
//                          offsets, walking on where a piece holds a line's end. A piece wholly inside a REF run is one 16-byte load of the
//                          genome's array (five dwords shifted together where source and destination disagree mod 4 or 16), masked in
//                          registers, and one 16-byte store; every other piece runs the core's emission of its line through a window, which
//                          stores the piece's bytes only. The work is the same for one REF of 1 MB and for 1 MB of 150-byte lines.
// Nothing outside text[0, total) is written. Of the genome's array the REF cuts are read, and up to 3 bytes behind a cut's last base by the
// shifted loads: inside the array or the 16 spare bytes behind its last base.
#include "../common.hpp"
#include "../vcf_format_core.hpp"

namespace csv {

namespace {

using namespace vcffmt;

constexpr int VF_THREADS = 256;
constexpr unsigned VF_MAX_GRID_CALLS = 256;               // the per-call kernel strides over the calls beyond this many workgroups
constexpr unsigned VF_MAX_GRID_PIECES = 1024;             // the per-piece kernel strides over the text beyond 4 MiB a pass

// the last contig whose first call is at or in front of call i (contigs without calls in front of it are passed over); i < n_calls
__device__ inline VfContig vf_contig_of(const VfContig *__restrict__ ct, uint32_t n_contigs, uint64_t i)
{
    uint32_t lo = 0, hi = n_contigs;
    while (hi - lo > 1) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (ct[mid].call_first <= i) lo = mid; else hi = mid;
    }
    return ct[lo];
}

__global__ __launch_bounds__(VF_THREADS) void vf_size_kernel(const VfArgs a)
{
    const Call *__restrict__ calls = (const Call *)a.calls;
    const uint64_t t0 = (uint64_t)blockIdx.x * VF_THREADS + threadIdx.x;
    if (t0 == 0) a.len[a.n_calls] = 0;
    for (uint64_t i = t0; i < a.n_calls; i += (uint64_t)gridDim.x * VF_THREADS) {
        const VfContig ct = vf_contig_of(a.contig, a.n_contigs, i);
        const Call c = calls[i];
        const uint64_t ao = a.alt_off[i], alen = a.alt_off[i + 1] - ao;
        Line L = decide(c, ct.contig_len, a.gap_start + ct.gap_first, a.gap_end + ct.gap_first, ct.n_gaps, a.alts + ao, alen);
        uint32_t len = 0;
        int32_t d = 0;
        if (L.why) {
            atomicMin(&a.head->first_refused, (unsigned long long)(i << 8 | L.why));
        } else {
            const uint8_t disp = L.status & DISPOSITION;
            if (disp == SKIP_UNCLASSIFIED) atomicAdd(&a.head->unclassified, 1u); else atomicAdd(&a.head->total, 1u);
            if (L.gap_hit) atomicAdd(&a.head->gap_filtered, 1u);
            if (disp == WRITTEN) {
                d = ct.depth && L.pos < ct.depth_len ? (int32_t)ct.depth[L.pos] : -1;
                set_depth(L, d);
                const uint64_t ll = line_length(c, L, ct.name_len, alen, a.method_len);
                atomicAdd(&a.head->text_bytes, (unsigned long long)ll);
                atomicAdd(&a.head->n_lines, 1ull);
                len = ll > 0xffffffffull ? 0xffffffffu : (uint32_t)ll;      // (the batch is declined by its total then)
            }
        }
        a.len[i] = len;
        a.depth[i] = d;
        a.status[i] = L.status;
    }
}

__device__ inline uint32_t vf_mask4(uint32_t w)
{
    uint32_t r = 0;
#pragma unroll
    for (int b = 0; b < 4; b++) r |= (uint32_t)fastacore::mask_base((uint8_t)(w >> (8 * b))) << (8 * b);
    return r;
}

// 16 bytes from src at any alignment: aligned dwords shifted together (reads up to 3 bytes behind src + 15)
__device__ inline uint4 vf_load16(const uint8_t *src)
{
    if (((uintptr_t)src & 15) == 0) return *reinterpret_cast<const uint4 *>(src);
    const uint32_t *w = reinterpret_cast<const uint32_t *>((uintptr_t)src & ~(uintptr_t)3);
    const uint32_t sh = (uint32_t)((uintptr_t)src & 3) * 8;
    const uint32_t w0 = w[0], w1 = w[1], w2 = w[2], w3 = w[3];
    if (sh == 0) return make_uint4(w0, w1, w2, w3);
    const uint32_t w4 = w[4];
    return make_uint4(w0 >> sh | w1 << (32 - sh), w1 >> sh | w2 << (32 - sh), w2 >> sh | w3 << (32 - sh), w3 >> sh | w4 << (32 - sh));
}

__global__ __launch_bounds__(VF_THREADS) void vf_write_kernel(const VfArgs a, uint64_t total, uint8_t *__restrict__ out)
{
    const Call *__restrict__ calls = (const Call *)a.calls;
    const uint32_t *__restrict__ off = a.len;                 // [n_calls + 1] the lines' offsets; off[n_calls] = total
    const uint64_t n_pieces = (total + 15) / 16;
    for (uint64_t p = (uint64_t)blockIdx.x * VF_THREADS + threadIdx.x; p < n_pieces; p += (uint64_t)gridDim.x * VF_THREADS) {
        const uint64_t o0 = p * 16, o1 = o0 + 16 <= total ? o0 + 16 : total;
        uint64_t lo = 0, hi = a.n_calls;                      // the last call whose offset is at or in front of o0: the line that holds it
        while (hi - lo > 1) {
            const uint64_t mid = lo + (hi - lo) / 2;
            if (off[mid] <= o0) lo = mid; else hi = mid;
        }
        for (uint64_t i = lo; i < a.n_calls; i++) {
            const uint64_t b = off[i], e = off[i + 1];
            if (b >= o1) break;
            if (e <= b) continue;                             // a call without a line
            const VfContig ct = vf_contig_of(a.contig, a.n_contigs, i);
            const Call c = calls[i];
            const uint64_t ao = a.alt_off[i], alen = a.alt_off[i + 1] - ao;
            Line L = decide(c, ct.contig_len, nullptr, nullptr, 0, a.alts + ao, alen);      // (the gap search's answer is in the status byte)
            L.gap_hit = (a.status[i] & GAP_FILTERED) != 0;
            set_depth(L, a.depth[i]);
            const uint8_t *ref = L.ref_kind == REF_GENOME ? a.seq + ct.rec_start + L.ref_first : nullptr;
            if (ref && o1 - o0 == 16) {
                const uint64_t r0 = b + ref_offset(L, ct.name_len), r1 = r0 + L.ref_len;
                if (o0 >= r0 && o1 <= r1) {                   // wholly inside the REF run
                    uint4 v = vf_load16(ref + (o0 - r0));
                    v = make_uint4(vf_mask4(v.x), vf_mask4(v.y), vf_mask4(v.z), vf_mask4(v.w));
                    uint8_t *dst = out + o0;
                    if (((uintptr_t)dst & 15) == 0) *reinterpret_cast<uint4 *>(dst) = v;
                    else {
                        const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
                        for (int k = 0; k < 16; k++) dst[k] = (uint8_t)(w[k >> 2] >> (8 * (k & 3)));
                    }
                    break;
                }
            }
            WindowSink ws{out, b, o0, o1};
            emit_line(ws, c, L, a.names + ct.name_off, ct.name_len, ref, a.alts + ao, alen, a.method, a.method_len);
        }
    }
}

}  // namespace

void launch_vcf_format_size(hipStream_t s, const VfArgs &a)
{
    if (a.n_calls == 0) return;
    const unsigned grid = (unsigned)std::min<uint64_t>((a.n_calls + VF_THREADS - 1) / VF_THREADS, VF_MAX_GRID_CALLS);
    vf_size_kernel<<<grid, VF_THREADS, 0, s>>>(a);
    launch_exclusive_sum_u32(s, a.len, a.n_calls + 1, a.es_tmp);
}

void launch_vcf_format_write(hipStream_t s, const VfArgs &a, uint64_t total, uint8_t *text)
{
    if (a.n_calls == 0 || total == 0) return;
    const uint64_t pieces = (total + 15) / 16;
    const unsigned grid = (unsigned)std::min<uint64_t>((pieces + VF_THREADS - 1) / VF_THREADS, VF_MAX_GRID_PIECES);
    vf_write_kernel<<<grid, VF_THREADS, 0, s>>>(a, total, text);
}

}  // namespace csv
