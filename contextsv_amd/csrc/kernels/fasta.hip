// fasta.hip — a reference FASTA's text in HBM to the genome's base array, and cuts of that array (csvgpu_genome_builder_* / csvgpu_genome_fetch;
// api/fasta.hip). The rules are fasta_core.hpp, shared with the host-side check; here is only how the lanes share the text.
//   line starts            vcfparse.hip's launch_vcf_count / launch_vcf_starts, unchanged: aligned 16-byte loads, per-tile counts, the
//                          exclusive sum of sort.hip.
//   fa_lines               a lane per line: header or residues (the first line may continue the line the previous call left open: its kind
//                          comes with the call), the bytes it keeps, and for a header the span of its name. Then three exclusive sums: the
//                          kept bytes, the header lines, the name bytes. A call's text is below 2^32 bytes, so these sums fit 32 bits; the
//                          genome's 64-bit total is added where they are used.
//   fa_headers             a header line's event at its rank: the kept bytes in front of it, its name copied to the side buffer. The records
//                          follow from these on the host (fastacore::Assembler): owners are a sum and a compaction, nobody walks the lines.
//   fa_compact             a lane owns an aligned 16-byte piece of the TEXT, not a line: its first byte's line is the tile's line rank plus
//                          the line ends in front of it in the tile, and every further line end in the piece moves on by one. The work
//                          is the same for one 250 MB line and for 4e7 lines of 60 bytes.
//   fa_cut                 a lane owns an aligned 16-byte piece of the OUTPUT, finds the item of its first byte by bisection of out_off and
//                          walks on from there. A piece inside one item whose source is 16-byte aligned is one load and one store.
#include "../common.hpp"
#include "../fasta_core.hpp"

namespace csv {

namespace {

constexpr int FA_THREADS = 256;
static_assert(FA_THREADS * 16 == CSV_VCF_TILE_BYTES, "one 16-byte piece per lane and tile, as the line starts were found");
constexpr unsigned FA_MAX_GRID = 1024;                    // the per-line kernels stride over the lines beyond this many workgroups

// bit j: byte j of the piece is `c`
__device__ inline uint32_t fa_match16(const uint4 &v, uint8_t c)
{
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
    uint32_t m = 0;
#pragma unroll
    for (int k = 0; k < 4; k++)
#pragma unroll
        for (int b = 0; b < 4; b++) m |= (uint32_t)(((w[k] >> (8 * b)) & 0xff) == c) << (4 * k + b);
    return m;
}

__device__ inline uint8_t fa_byte(const uint4 &v, int j)
{
    const uint32_t w = j < 4 ? v.x : j < 8 ? v.y : j < 12 ? v.z : v.w;
    return (uint8_t)(w >> (8 * (j & 3)));
}

__global__ __launch_bounds__(FA_THREADS) void fa_lines_kernel(const uint8_t *__restrict__ text, uint32_t len, const uint32_t *__restrict__ line_start, uint32_t n_slots,
                                                              FastaCarry carry, uint32_t *__restrict__ kept, uint32_t *__restrict__ hdr, uint32_t *__restrict__ nlen,
                                                              uint8_t *__restrict__ blank, FastaHead *head)
{
    using namespace fastacore;
    for (uint64_t i = (uint64_t)blockIdx.x * FA_THREADS + threadIdx.x; i <= n_slots; i += (uint64_t)gridDim.x * FA_THREADS) {
        if (i == n_slots) { kept[i] = 0; hdr[i] = 0; nlen[i] = 0; continue; }                     // the sums' totals
        const uint32_t start = line_start[i];
        const uint32_t end = i + 1 < n_slots ? line_start[i + 1] - 1 : len;
        const uint32_t n = end - start;
        const bool cont = i == 0 && carry.mid_line;       // the line the previous call left open goes on
        const uint8_t kind = cont ? carry.kind : line_kind(text + start, n);
        uint32_t k = 0, h = 0, nl = 0;
        bool b = false;
        if (kind == LINE_HEADER) {
            h = 1;
            const uint32_t from = cont ? 0 : 1;           // behind the '>' of a line that starts here
            nl = name_span(text + start + from, n - from, b);
        } else {
            k = n;
        }
        kept[i] = k; hdr[i] = h; nlen[i] = nl; blank[i] = b;
        if (i + 1 == n_slots) { head->tail_len = n; head->tail_kind = kind; }
    }
}

__global__ void fa_totals_kernel(const uint32_t *kept, const uint32_t *hdr, const uint32_t *nlen, uint32_t n_slots, FastaHead *head)
{
    head->n_kept = kept[n_slots];
    head->n_hdr = hdr[n_slots];
    head->n_name = nlen[n_slots];
}

// kept / hdr / nlen: the exclusive sums now. ev_*[h]: the h-th header line of the text.
__global__ __launch_bounds__(FA_THREADS) void fa_headers_kernel(const uint8_t *__restrict__ text, const uint32_t *__restrict__ line_start, uint32_t n_slots, FastaCarry carry,
                                                                const uint32_t *__restrict__ kept, const uint32_t *__restrict__ hdr, const uint32_t *__restrict__ nlen,
                                                                const uint8_t *__restrict__ blank, FastaEvents ev)
{
    for (uint64_t i = (uint64_t)blockIdx.x * FA_THREADS + threadIdx.x; i < n_slots; i += (uint64_t)gridDim.x * FA_THREADS) {
        const uint32_t h = hdr[i];
        if (hdr[i + 1] == h) continue;
        const uint32_t off = nlen[i], n = nlen[i + 1] - off;
        ev.kept[h] = kept[i];
        ev.name_off[h] = off;
        ev.name_len[h] = n;
        ev.blank[h] = blank[i];
        const uint8_t *src = text + line_start[i] + (i == 0 && carry.mid_line ? 0 : 1);
        for (uint32_t k = 0; k < n; k++) ev.names[off + k] = src[k];
    }
}

// base / lead / len: as the line starts were found (the pieces are aligned, the text may start anywhere). dst: where this text's first
// kept byte goes.
__global__ __launch_bounds__(FA_THREADS) void fa_compact_kernel(const uint8_t *__restrict__ base, uint32_t lead, uint32_t len, const uint32_t *__restrict__ tile_off,
                                                                const uint32_t *__restrict__ line_start, const uint32_t *__restrict__ kept, uint8_t *__restrict__ dst)
{
    __shared__ uint32_t s_wave[FA_THREADS / 64];
    const uint64_t at = (uint64_t)blockIdx.x * CSV_VCF_TILE_BYTES + (uint64_t)threadIdx.x * 16;        // from the aligned base
    const int64_t rel = (int64_t)at - lead;                                                             // the text offset of the piece's byte 0
    const bool in_text = !(at + 16 <= lead || at >= (uint64_t)lead + len);
    uint4 v = make_uint4(0, 0, 0, 0);
    int j0 = 0, j1 = 0;                                   // the piece's bytes [j0, j1) lie in the text
    uint32_t m = 0;
    if (in_text) {
        v = *reinterpret_cast<const uint4 *>(base + at);
        j0 = rel < 0 ? (int)-rel : 0;
        j1 = rel + 16 > (int64_t)len ? (int)((int64_t)len - rel) : 16;
        m = fa_match16(v, '\n') & (0xffffu << j0) & (0xffffu >> (16 - j1));
    }
    const uint32_t c = __popc(m);
    uint32_t incl = c;                                    // inclusive sum of the line ends over the wave
    const int lane = threadIdx.x & 63;
    for (int d = 1; d < 64; d <<= 1) { const uint32_t up = __shfl_up(incl, d, 64); if (lane >= d) incl += up; }
    if (lane == 63) s_wave[threadIdx.x >> 6] = incl;
    __syncthreads();
    if (!in_text) return;
    uint32_t line = tile_off[blockIdx.x] + incl - c;      // the line of byte j0: as many line ends lie in front of it
    for (int k = 0; k < (int)(threadIdx.x >> 6); k++) line += s_wave[k];
    uint32_t ko = kept[line], ls = line_start[line];
    bool res = kept[line + 1] != ko;                      // a line that keeps bytes (a header and an empty line keep none)
    if (m == 0 && j0 == 0 && j1 == 16) {                  // the whole piece inside one line
        if (!res) return;
        uint8_t *d = dst + ko + ((uint32_t)rel - ls);
        if (((uintptr_t)d & 15) == 0) { *reinterpret_cast<uint4 *>(d) = v; return; }
        const uint32_t a = (uint32_t)((uintptr_t)d & 3);
        if (a == 0) {
            uint32_t *d4 = reinterpret_cast<uint32_t *>(d);
            d4[0] = v.x; d4[1] = v.y; d4[2] = v.z; d4[3] = v.w;
            return;
        }
        // 4 - a single bytes up to the next word, three words shifted together from the piece's four, a single bytes behind them
        const int s = 4 - (int)a;
        for (int j = 0; j < s; j++) d[j] = fa_byte(v, j);
        uint32_t *d4 = reinterpret_cast<uint32_t *>(d + s);
        const uint32_t sh = 8u * (uint32_t)s;
        d4[0] = (v.x >> sh) | (v.y << (32 - sh));
        d4[1] = (v.y >> sh) | (v.z << (32 - sh));
        d4[2] = (v.z >> sh) | (v.w << (32 - sh));
        for (int j = 12 + s; j < 16; j++) d[j] = fa_byte(v, j);
        return;
    }
    for (int j = j0; j < j1; j++) {
        if ((m >> j) & 1) {
            line++;
            ko = kept[line]; ls = line_start[line];
            res = kept[line + 1] != ko;
        } else if (res) {
            dst[ko + ((uint32_t)(rel + j) - ls)] = fa_byte(v, j);
        }
    }
}

// item i: out[out_off[i] .. out_off[i + 1]) = seq[src[i] ..), masked if asked. total = out_off[n]; out_off[0] = 0.
__global__ __launch_bounds__(FA_THREADS) void fa_cut_kernel(const uint8_t *__restrict__ seq, const uint64_t *__restrict__ src, const uint64_t *__restrict__ out_off, uint64_t n,
                                                            uint64_t total, int mask, uint8_t *__restrict__ out)
{
    const uint64_t o0 = ((uint64_t)blockIdx.x * FA_THREADS + threadIdx.x) * 16;
    if (o0 >= total) return;
    const uint64_t o1 = o0 + 16 <= total ? o0 + 16 : total;
    uint64_t lo = 0, hi = n;                              // the last item with out_off[item] <= o0 (empty items in front of it are passed over)
    while (hi - lo > 1) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (out_off[mid] <= o0) lo = mid; else hi = mid;
    }
    uint64_t item = lo, item_end = out_off[item + 1];
    const uint8_t *s = seq + src[item] - out_off[item];   // (the item's byte at output offset o is s[o])
    if (o1 - o0 == 16 && item_end >= o1 && ((uintptr_t)(s + o0) & 15) == 0) {
        uint4 v = *reinterpret_cast<const uint4 *>(s + o0);
        if (mask) {
            uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (int k = 0; k < 4; k++) {
                uint32_t r = 0;
#pragma unroll
                for (int b = 0; b < 4; b++) r |= (uint32_t)fastacore::mask_base((uint8_t)(w[k] >> (8 * b))) << (8 * b);
                w[k] = r;
            }
            v = make_uint4(w[0], w[1], w[2], w[3]);
        }
        *reinterpret_cast<uint4 *>(out + o0) = v;
        return;
    }
    for (uint64_t o = o0; o < o1; o++) {
        while (o >= item_end) {                           // (o < total = out_off[n]: an item that holds o exists)
            item++;
            item_end = out_off[item + 1];
            s = seq + src[item] - out_off[item];
        }
        const uint8_t c = s[o];
        out[o] = mask ? fastacore::mask_base(c) : c;
    }
}

unsigned line_grid(uint64_t n) { return (unsigned)std::min<uint64_t>((n + FA_THREADS - 1) / FA_THREADS, FA_MAX_GRID); }

}  // namespace

void launch_fasta_lines(hipStream_t s, const uint8_t *text, uint32_t len, uint32_t n_slots, const FastaCarry &carry, const FastaWs &w)
{
    fa_lines_kernel<<<line_grid((uint64_t)n_slots + 1), FA_THREADS, 0, s>>>(text, len, w.vcf.line_start, n_slots, carry, w.kept, w.hdr, w.nlen, w.blank, w.head);
    launch_exclusive_sum_u32(s, w.kept, (uint64_t)n_slots + 1, w.es_tmp);
    launch_exclusive_sum_u32(s, w.hdr, (uint64_t)n_slots + 1, w.es_tmp);
    launch_exclusive_sum_u32(s, w.nlen, (uint64_t)n_slots + 1, w.es_tmp);
    fa_totals_kernel<<<1, 1, 0, s>>>(w.kept, w.hdr, w.nlen, n_slots, w.head);
    fa_headers_kernel<<<line_grid(n_slots), FA_THREADS, 0, s>>>(text, w.vcf.line_start, n_slots, carry, w.kept, w.hdr, w.nlen, w.blank, w.ev);
}

void launch_fasta_compact(hipStream_t s, const uint8_t *text, uint32_t len, const FastaWs &w, uint8_t *dst)
{
    const uint32_t lead = (uint32_t)((uintptr_t)text & 15), n_tiles = vcf_tiles(text, len);
    fa_compact_kernel<<<n_tiles, FA_THREADS, 0, s>>>(text - lead, lead, len, w.vcf.tile_cnt, w.vcf.line_start, w.kept, dst);
}

void launch_fasta_cut(hipStream_t s, const uint8_t *seq, const uint64_t *src, const uint64_t *out_off, uint64_t n, uint64_t total, bool mask, uint8_t *out)
{
    if (n == 0 || total == 0) return;
    const uint64_t pieces = (total + 15) / 16;
    fa_cut_kernel<<<(unsigned)((pieces + FA_THREADS - 1) / FA_THREADS), FA_THREADS, 0, s>>>(seq, src, out_off, n, total, mask ? 1 : 0, out);
}

}  // namespace csv
