// vcfparse.hip — VCF text lines parsed on the device (csvgpu_vcf_snp_parse / _af_parse / _dev; api/vcf.hip). The rules of one line are
// vcf_record_core.hpp, shared with the host-side check; here is only how the text is cut into lines and how the lanes share a line.
//   vp_count / vp_starts   every lane loads one aligned 16-byte piece (global_load_dwordx4) and marks its '\n': per-tile counts, their
//                          exclusive sum (sort.hip's), then every line's start written at its rank. Nothing walks the text byte by byte.
//   vp_parse<W>            a group of W lanes (8, 16 or 64, by the mean line length) per line: the tabs by ballot over the line's bytes,
//                          the short fields (REF .. the sample column) converted by the group's first lane with the core's functions, the
//                          INFO key (AF form) searched by the whole group over the field's 16-byte pieces. A line's length is bounded by
//                          nothing: every loop runs over the line, no buffer holds it.
//   vp_flags, vp_emit      a code per line -> flags (nothing at or behind the lowest STOP line counts) -> exclusive sums -> scatter: the
//                          outputs are in file order without an atomic append.
#include "../common.hpp"
#include "../vcf_record_core.hpp"

namespace csv {

namespace {

constexpr int VP_THREADS = 256;
static_assert(VP_THREADS * 16 == CSV_VCF_TILE_BYTES, "one 16-byte piece per lane and tile");
constexpr unsigned VP_MAX_GRID = 2048;                    // the per-line kernel strides over the lines beyond this many workgroups
constexpr uint8_t VP_EMPTY = 5;                           // a line slot without a line (empty, only '\r', or the slot behind the text's last '\n')

// bit j: byte j of the piece is `c`
__device__ inline uint32_t match16(const uint4 &v, uint8_t c)
{
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
    uint32_t m = 0;
#pragma unroll
    for (int k = 0; k < 4; k++)
#pragma unroll
        for (int b = 0; b < 4; b++) m |= (uint32_t)(((w[k] >> (8 * b)) & 0xff) == c) << (4 * k + b);
    return m;
}

// The line ends of this lane's piece of tile blockIdx.x, as a mask over the piece's bytes that lie in the text. `lead`: bytes of the first
// piece in front of the text (the text may start anywhere; the pieces are aligned). rel: the text offset of the piece's byte 0 (may be < 0).
__device__ inline uint32_t piece_newlines(const uint8_t *base, uint32_t lead, uint32_t len, int64_t &rel)
{
    const uint64_t at = (uint64_t)blockIdx.x * CSV_VCF_TILE_BYTES + (uint64_t)threadIdx.x * 16;       // from the aligned base
    rel = (int64_t)at - lead;
    if (at + 16 <= lead || at >= (uint64_t)lead + len) return 0;                                       // no byte of the text in this piece
    const uint4 v = *reinterpret_cast<const uint4 *>(base + at);
    uint32_t m = match16(v, '\n');
    if (rel < 0) m &= 0xffffu << (uint32_t)(-rel);
    const int64_t over = rel + 16 - (int64_t)len;
    if (over > 0) m &= 0xffffu >> (uint32_t)over;
    return m;
}

__global__ __launch_bounds__(VP_THREADS) void vp_count_kernel(const uint8_t *base, uint32_t lead, uint32_t len, uint32_t n_tiles, uint32_t *tile_cnt, VcfHead *head)
{
    __shared__ uint32_t s_wave[VP_THREADS / 64];
    int64_t rel;
    uint32_t c = __popc(piece_newlines(base, lead, len, rel));
    for (int d = 32; d; d >>= 1) c += __shfl_xor(c, d, 64);
    if ((threadIdx.x & 63) == 0) s_wave[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t t = 0;
        for (int k = 0; k < VP_THREADS / 64; k++) t += s_wave[k];
        tile_cnt[blockIdx.x] = t;
        if (blockIdx.x == 0) {
            tile_cnt[n_tiles] = 0;
            head->n_lines = 0; head->stop_off = 0xffffffffu; head->hash_off = ~0ull; head->n_kept = 0; head->n_defer = 0;
        }
    }
}

// tile_off: the exclusive sum of the tiles' counts. The line behind the text's k-th line end (k from 0) is slot k + 1; slot 0 starts at 0.
__global__ __launch_bounds__(VP_THREADS) void vp_starts_kernel(const uint8_t *base, uint32_t lead, uint32_t len, const uint32_t *tile_off, uint32_t *line_start)
{
    __shared__ uint32_t s_wave[VP_THREADS / 64];
    int64_t rel;
    uint32_t m = piece_newlines(base, lead, len, rel);
    const uint32_t c = __popc(m);
    uint32_t incl = c;                                    // inclusive sum over the wave
    const int lane = threadIdx.x & 63;
    for (int d = 1; d < 64; d <<= 1) { const uint32_t up = __shfl_up(incl, d, 64); if (lane >= d) incl += up; }
    if (lane == 63) s_wave[threadIdx.x >> 6] = incl;
    __syncthreads();
    uint32_t before = tile_off[blockIdx.x] + incl - c;
    for (int k = 0; k < (int)(threadIdx.x >> 6); k++) before += s_wave[k];
    if (blockIdx.x == 0 && threadIdx.x == 0) line_start[0] = 0;
    while (m) {
        const int j = __ffs(m) - 1;
        m &= m - 1;
        line_start[++before] = (uint32_t)(rel + j) + 1;   // (slot before + 1: one more line end in front of it)
    }
}

template <int W> __device__ inline uint32_t group_min(uint32_t v)
{
#pragma unroll
    for (int d = W / 2; d; d >>= 1) v = min(v, (uint32_t)__shfl_xor(v, d, W));
    return v;
}

template <int W, bool AF>
__global__ __launch_bounds__(VP_THREADS) void vp_parse_kernel(const uint8_t *__restrict__ text, uint32_t len, const uint32_t *__restrict__ line_start, uint32_t n_slots,
                                                              VcfParseArgs a, uint8_t *__restrict__ code, uint32_t *__restrict__ pos, uint32_t *__restrict__ chrom_len,
                                                              double *__restrict__ value, VcfHead *head)
{
    using namespace vcfcore;
    constexpr int GROUPS = VP_THREADS / W, NEED = AF ? kAfTabs : kSnpTabs;
    __shared__ uint32_t s_tab[GROUPS][kSnpTabs];          // the line's first tabs, written and read by the group's first lane alone
    const int g = threadIdx.x / W, gl = threadIdx.x % W;
    const int gshift = (threadIdx.x & 63) & ~(W - 1);     // the group's first lane in its wave
    const unsigned long long gmask = W == 64 ? ~0ull : ((1ull << W) - 1);
    for (uint64_t i = (uint64_t)blockIdx.x * GROUPS + g; i < n_slots; i += (uint64_t)gridDim.x * GROUPS) {     // (uniform in the group)
        const uint32_t start = line_start[i];
        uint32_t end = i + 1 < n_slots ? line_start[i + 1] - 1 : len;
        if (start < end && text[end - 1] == '\r') end--;
        if (start >= end) { if (gl == 0) code[i] = VP_EMPTY; continue; }
        if (text[start] == '#') {
            if (gl == 0) { code[i] = VCF_SKIP; atomicMin(&head->hash_off, (unsigned long long)start); }
            continue;
        }
        const uint8_t *p = text + start;
        const uint32_t n = end - start;
        int n_tab = 0;
        for (uint32_t o = 0; o < n && n_tab < NEED; o += W) {
            const uint32_t at = o + gl;
            const bool is_tab = at < n && p[at] == '\t';
            unsigned long long b = (__ballot(is_tab) >> gshift) & gmask;
            while (b && n_tab < NEED) {
                if (gl == 0) s_tab[g][n_tab] = o + (uint32_t)__builtin_ctzll(b);
                n_tab++;
                b &= b - 1;
            }
        }
        Rec r;
        int c = VCF_SKIP;
        if (!AF) {
            if (gl == 0) c = snp_line_tabs(p, n, s_tab[g], n_tab, a.dp_int, a.ad_int, r);
        } else {
            const uint32_t last_pos = a.n_sorted ? a.sorted_pos[a.n_sorted - 1] : 0;
            uint32_t info = 0;
            if (gl == 0) {
                c = af_line_head(p, n, s_tab[g], n_tab, a.contig, a.contig_len, a.sorted_pos, a.n_sorted, last_pos, r);
                if (c == VCF_MORE) info = s_tab[g][6] + 1;
            }
            c = __shfl(c, 0, W);
            if (c == VCF_MORE) {                          // the INFO field's end and the key, by the whole group over aligned 16-byte pieces
                info = __shfl(info, 0, W);
                const uintptr_t first = (uintptr_t)(p + info) & ~(uintptr_t)15;
                uint32_t tab_at = kNone, key_at = kNone;
                for (uintptr_t q = first; q < (uintptr_t)(p + n); q += (uintptr_t)W * 16) {
                    const uintptr_t mine = q + (uintptr_t)gl * 16;
                    if (mine < (uintptr_t)(p + n)) {
                        const uint4 v = *reinterpret_cast<const uint4 *>(mine);
                        const int64_t rel = (int64_t)(mine - (uintptr_t)p);           // the piece's byte 0 in the line (below info for the first piece)
                        uint32_t in = 0xffffu;
                        if (rel < (int64_t)info) in &= 0xffffu << (uint32_t)((int64_t)info - rel);
                        if (rel + 16 > (int64_t)n) in &= 0xffffu >> (uint32_t)(rel + 16 - (int64_t)n);
                        const uint32_t tabs = match16(v, '\t') & in;
                        if (tabs) tab_at = (uint32_t)(rel + __ffs(tabs) - 1);
                        uint32_t cand = match16(v, a.needle[0]) & in;
                        while (cand && key_at == kNone) {
                            const uint32_t k = (uint32_t)(rel + __ffs(cand) - 1);
                            cand &= cand - 1;
                            if (needle_at(p, info, n, k, a.needle, a.needle_len)) key_at = k;
                        }
                    }
                    tab_at = group_min<W>(tab_at);
                    key_at = group_min<W>(key_at);
                    if (tab_at != kNone || key_at != kNone) break;
                }
                if (gl == 0) {
                    // (the needle holds no tab: a match in front of every tab seen so far lies inside the field)
                    if (key_at != kNone && tab_at != kNone && key_at > tab_at) key_at = kNone;
                    uint32_t info_end = n;
                    if (key_at != kNone) {
                        info_end = key_at + a.needle_len;
                        while (info_end < n && p[info_end] != '\t' && p[info_end] != ';' && p[info_end] != ',') info_end++;
                    }
                    c = af_line_value(p, info_end, key_at, a.needle_len, r);
                }
            }
        }
        if (gl == 0) {
            code[i] = (uint8_t)c;
            if (c == VCF_KEEP) { pos[i] = r.pos; chrom_len[i] = r.chrom_len; value[i] = r.value; }
            if (c == VCF_STOP) atomicMin(&head->stop_off, start);
        }
    }
}

// flags of the lines in front of the lowest STOP line; slot n_slots: the sums' totals
__global__ __launch_bounds__(VP_THREADS) void vp_flags_kernel(const uint8_t *__restrict__ code, const uint32_t *__restrict__ line_start, uint32_t n_slots,
                                                              uint32_t *__restrict__ kept, uint32_t *__restrict__ defer, VcfHead *head)
{
    const uint64_t i = (uint64_t)blockIdx.x * VP_THREADS + threadIdx.x;
    if (i > n_slots) return;
    if (i == n_slots) { kept[i] = 0; defer[i] = 0; return; }
    const uint8_t c = code[i];
    const bool live = line_start[i] < head->stop_off;
    kept[i] = live && c == vcfcore::VCF_KEEP;
    defer[i] = live && c == vcfcore::VCF_DEFER;
    if (live && c != VP_EMPTY) atomicAdd(&head->n_lines, 1u);
}

__global__ void vp_totals_kernel(const uint32_t *kept, const uint32_t *defer, uint32_t n_slots, VcfHead *head)
{
    head->n_kept = kept[n_slots];
    head->n_defer = defer[n_slots];
}

__global__ __launch_bounds__(VP_THREADS) void vp_emit_kernel(uint32_t n_slots, bool af, const uint32_t *__restrict__ line_start, const uint32_t *__restrict__ kept,
                                                             const uint32_t *__restrict__ defer, const uint32_t *__restrict__ pos, const uint32_t *__restrict__ chrom_len,
                                                             const double *__restrict__ value, VcfOut out)
{
    const uint64_t i = (uint64_t)blockIdx.x * VP_THREADS + threadIdx.x;
    if (i >= n_slots) return;
    const uint32_t k = kept[i], d = defer[i];
    if (kept[i + 1] != k) {
        out.line_off[k] = line_start[i];
        out.pos[k] = pos[i];
        out.value[k] = value[i];
        if (!af) out.chrom_len[k] = chrom_len[i];
    }
    if (defer[i + 1] != d) out.defer_off[d] = line_start[i];
}

template <int W>
void parse_width(hipStream_t s, const uint8_t *text, uint32_t len, uint32_t n_slots, const VcfParseArgs &a, const VcfWs &w)
{
    const unsigned groups = VP_THREADS / W;
    const unsigned grid = (unsigned)std::min<uint64_t>(((uint64_t)n_slots + groups - 1) / groups, VP_MAX_GRID);
    if (a.af) vp_parse_kernel<W, true><<<grid, VP_THREADS, 0, s>>>(text, len, w.line_start, n_slots, a, w.code, w.pos, w.chrom_len, w.value, w.head);
    else vp_parse_kernel<W, false><<<grid, VP_THREADS, 0, s>>>(text, len, w.line_start, n_slots, a, w.code, w.pos, w.chrom_len, w.value, w.head);
}

}  // namespace

void launch_vcf_count(hipStream_t s, const uint8_t *text, uint32_t len, const VcfWs &w)
{
    const uint32_t lead = (uint32_t)((uintptr_t)text & 15), n_tiles = vcf_tiles(text, len);
    vp_count_kernel<<<n_tiles, VP_THREADS, 0, s>>>(text - lead, lead, len, n_tiles, w.tile_cnt, w.head);
    launch_exclusive_sum_u32(s, w.tile_cnt, (uint64_t)n_tiles + 1, w.es_tmp);
}

void launch_vcf_starts(hipStream_t s, const uint8_t *text, uint32_t len, const VcfWs &w)
{
    const uint32_t lead = (uint32_t)((uintptr_t)text & 15), n_tiles = vcf_tiles(text, len);
    vp_starts_kernel<<<n_tiles, VP_THREADS, 0, s>>>(text - lead, lead, len, w.tile_cnt, w.line_start);
}

void launch_vcf_parse(hipStream_t s, const uint8_t *text, uint32_t len, uint32_t n_slots, const VcfParseArgs &a, int width, const VcfWs &w)
{
    if (width == 0) {                                     // lanes per line from the mean line length: a lane's share is some tens of bytes
        const uint64_t mean = len / n_slots;
        width = mean <= 256 ? 8 : mean <= 1024 ? 16 : 64;
    }
    if (width == 8) parse_width<8>(s, text, len, n_slots, a, w);
    else if (width == 16) parse_width<16>(s, text, len, n_slots, a, w);
    else parse_width<64>(s, text, len, n_slots, a, w);
    const unsigned grid = (unsigned)(((uint64_t)n_slots + 1 + VP_THREADS - 1) / VP_THREADS);
    vp_flags_kernel<<<grid, VP_THREADS, 0, s>>>(w.code, w.line_start, n_slots, w.kept, w.defer, w.head);
    launch_exclusive_sum_u32(s, w.kept, (uint64_t)n_slots + 1, w.es_tmp2);
    launch_exclusive_sum_u32(s, w.defer, (uint64_t)n_slots + 1, w.es_tmp2);
    vp_totals_kernel<<<1, 1, 0, s>>>(w.kept, w.defer, n_slots, w.head);
}

void launch_vcf_emit(hipStream_t s, uint32_t n_slots, bool af, const VcfWs &w, const VcfOut &out)
{
    const unsigned grid = (unsigned)(((uint64_t)n_slots + VP_THREADS - 1) / VP_THREADS);
    vp_emit_kernel<<<grid, VP_THREADS, 0, s>>>(n_slots, af, w.line_start, w.kept, w.defer, w.pos, w.chrom_len, w.value, out);
}

}  // namespace csv
