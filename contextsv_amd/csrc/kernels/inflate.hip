// inflate.hip — kernel #12: raw DEFLATE (RFC 1951) of BGZF members with the CRC-32 of what was decoded, one wave per member (gfx950).
//
// The device form of host/fast_inflate.cpp, under the same contract: a member either decodes to exactly out_len bytes, with the stream
// consumed to its last byte and the CRC-32 equal to the trailer's (status 0), or it is declined (status 1) and the caller decodes it on the
// host. Nothing depends on this kernel being right about a corner of the format.
//
// Huffman decoding is sequential, so the unit of parallelism is the member: a workgroup is ONE wave and owns one member at a time.
//   decode   every lane runs the sequential core (inflate_core.hpp: bit reader, table build, one symbol -> one token) on the same values:
//            uniform control flow, and every lane knows every token without a word exchanged. What comes out of LDS is read through
//            the first lane (IC_UNIFORM); the compiler nevertheless keeps the decoder's state in vector registers and builds the token
//            loop with exec-mask branches (249 VGPR, 44 SGPR spilled to lanes): a scalar decode loop is what comes next. The tables
//            (12.5 KiB: 10-bit literal/length root, 8-bit distance root, sub-tables for the longer codes) are built in LDS per DEFLATE block.
//   input    staged 1 KiB at a time into a 2 KiB LDS ring by aligned dword loads, four per lane (the edges byte by byte), never a byte
//            outside [in_off, in_off + in_len); the bit reader takes 32 bits from the ring at a time.
//   output   the whole member (<= 64 KiB) is assembled in LDS: a literal is one byte store of lane 0, a match is copied by all lanes
//            (i -> pos + i from pos - dist + i, or from pos - dist + i mod dist when the copy overlaps itself, so that no lane ever reads
//            a byte this copy produces), a stored block comes straight from global memory. Stores and the loads of a later match are
//            ordered by a barrier (one wave: a wait for the LDS counter) in front of every copy. No global memory is written while
//            decoding, so a damaged stream can at worst waste LDS traffic: positions are checked by the core before a token is handed out.
//   CRC      64 slices of whole words, an odd number of words each (consecutive lanes start on different banks), bitwise per byte; every
//            lane moves its register to the member's end by multiplying with x^(8 * bytes behind its slice) mod P; XOR across the wave.
//   write    only a member that passed all of it is written: LDS -> global in dwords aligned to the destination, the edges in bytes,
//            nothing outside [out_off, out_off + out_len).
// LDS: 64 KiB output + 2 KiB ring + 12.5 KiB tables = 80 400 B per workgroup: two members in flight per CU (160 KiB), 512 on the device.
// That occupancy is the price of keeping the output out of global memory until it has been checked.
#include <algorithm>

#include "../common.hpp"

#define IC_HD __host__ __device__
#define IC_UNIFORM(x) ((uint32_t)__builtin_amdgcn_readfirstlane((int)(x)))
#include "../inflate_core.hpp"

namespace csv {

namespace ic = inflate_core;

namespace {

constexpr uint32_t RING_WORDS = 512, HALF_WORDS = 256, HALF_BYTES = HALF_WORDS * 4;
constexpr uint32_t INFLATE_MAX_GRID = 4096;            // members beyond it are taken in strides

// The compressed bytes of one member behind a 2 KiB LDS ring of two halves. Positions are kept in q = pos + mis, mis = the stream's
// misalignment in global memory, so that an aligned word of the ring is an aligned word of global memory. [hi - 2 KiB, hi) is what the ring
// can hold, hi a multiple of 1 KiB; a half is staged when the reader first needs a word of it. All lanes call every member function together.
struct RingIn {
    const uint8_t *g;              // the stream's first byte
    uint32_t in_len, mis, hi;
    uint32_t *ring;
    uint32_t lane;

    __device__ RingIn(const uint8_t *g_, uint32_t in_len_, uint32_t *ring_, uint32_t lane_)
        : g(g_), in_len(in_len_), mis((uint32_t)((uintptr_t)g_ & 3)), hi(0), ring(ring_), lane(lane_) {}

    __device__ void stage_half()
    {
        __syncthreads();                               // the reads of the half that goes are done
        uint32_t *dst = ring + ((hi >> 10) & 1) * HALF_WORDS;
        const uint32_t lo_q = mis, hi_q = mis + in_len;               // the stream's bytes are q in [lo_q, hi_q)
        for (uint32_t j = 0; j < HALF_WORDS / WAVE; j++) {
            const uint32_t wi = j * WAVE + lane, q = hi + wi * 4;
            uint32_t v = 0;
            if (q >= lo_q && q + 4 <= hi_q) v = *(const uint32_t *)(g + (q - mis));          // g - mis is 4-byte aligned, and so is q
            else
                for (uint32_t b = 0; b < 4; b++) if (q + b >= lo_q && q + b < hi_q) v |= (uint32_t)g[q + b - mis] << (8 * b);
            dst[wi] = v;
        }
        hi += HALF_BYTES;
        __syncthreads();
    }
    __device__ uint32_t get32(uint32_t pos)
    {
        const uint32_t q = pos + mis;
        for (int k = 0; k < 3 && hi < (q & ~3u) + 8; k++) stage_half();      // sequential reads stage one half at a time; after a seek, two at most
        const uint32_t w0 = ring[(q >> 2) & (RING_WORDS - 1)], w1 = ring[((q >> 2) + 1) & (RING_WORDS - 1)];
        const uint32_t sh = (q & 3) * 8;
        return sh ? (w0 >> sh) | (w1 << (32 - sh)) : w0;
    }
    __device__ void seek(uint32_t pos)
    {
        const uint32_t q0 = (pos + mis) & ~(HALF_BYTES - 1);
        if (q0 > hi) hi = q0;                          // nothing of the ring is of use any more: start over at the half that holds pos
    }
};

__global__ __launch_bounds__(WAVE) void bgzf_inflate_kernel(const uint8_t *__restrict__ comp, const csv_bgzf_block *__restrict__ blocks, uint32_t n_blocks,
                                                            uint8_t *__restrict__ out, uint8_t *__restrict__ status, unsigned int *__restrict__ n_declined)
{
    __shared__ uint32_t s_out[ic::MAX_BLOCK / 4 + 4];          // + 4: the write pass reads one word past the last whole one
    __shared__ uint32_t s_ring[RING_WORDS];
    __shared__ ic::Work s_w;
    uint8_t *const o8 = (uint8_t *)s_out;
    const uint32_t lane = threadIdx.x;

    for (uint32_t blk = blockIdx.x; blk < n_blocks; blk += gridDim.x) {
        __syncthreads();                               // the last member's LDS is free
        const csv_bgzf_block b = blocks[blk];
        const uint32_t in_len = IC_UNIFORM(b.in_len), n = IC_UNIFORM(b.out_len);
        const uint8_t *const g = comp + b.in_off;
        bool ok = in_len <= ic::MAX_BLOCK && n <= ic::MAX_BLOCK;
        if (ok) {
            RingIn in(g, in_len, s_ring, lane);
            ic::Decoder<RingIn> dec(in, s_w, in_len, n);
            uint32_t pos = 0;
            uint32_t budget = in_len * 8 + 2;          // the core's own bound on its tokens, held against it
            for (;;) {
                const ic::Token t = dec.next();
                if (t.kind == ic::T_DONE) break;
                if (t.kind == ic::T_DECLINE || budget-- == 0) { ok = false; break; }
                if (t.kind == ic::T_LITERAL) {
                    if (lane == 0) o8[pos] = (uint8_t)t.a;
                    pos++;
                } else if (t.kind == ic::T_STORED) {                                   // t.b + t.a <= in_len, pos + t.a <= n: checked by the core
                    for (uint32_t i = lane; i < t.a; i += WAVE) o8[pos + i] = g[t.b + i];
                    pos += t.a;
                } else {                                                               // dist <= pos, pos + len <= n: checked by the core
                    const uint32_t len = t.a, dist = t.b, from = pos - dist;
                    __syncthreads();                   // every byte below pos is in LDS before a lane reads it
                    if (dist >= len) {
                        for (uint32_t i = lane; i < len; i += WAVE) o8[pos + i] = o8[from + i];
                    } else {
                        for (uint32_t i = lane; i < len; i += WAVE) o8[pos + i] = o8[from + i % dist];      // the pattern, never a byte of this copy
                    }
                    pos += len;
                }
            }
        }
        __syncthreads();
        if (ok) {
            const uint32_t L = ic::crc_slice_bytes(n);
            const uint32_t lo = min(lane * L, n), hi = min(lane * L + L, n);
            uint32_t c = lane == 0 ? 0xffffffffu : 0u;
            uint32_t i = lo;
            for (; i + 4 <= hi; i += 4) {
                const uint32_t v = s_out[i >> 2];
                c = ic::crc_byte(c, v & 0xff); c = ic::crc_byte(c, (v >> 8) & 0xff); c = ic::crc_byte(c, (v >> 16) & 0xff); c = ic::crc_byte(c, v >> 24);
            }
            for (; i < hi; i++) c = ic::crc_byte(c, o8[i]);
            c = ic::gf2_mulmod(c, ic::crc_x8n(n - hi));
            for (int off = WAVE / 2; off > 0; off >>= 1) c ^= __shfl_xor(c, off, WAVE);
            ok = ~c == b.crc32;
        }
        if (ok) {
            uint8_t *const a = out + b.out_off;
            const uint32_t head = min(n, (uint32_t)((4 - ((uintptr_t)a & 3)) & 3));
            const uint32_t body = (n - head) >> 2, tail = head + body * 4;
            if (lane < head) a[lane] = o8[lane];
            for (uint32_t wd = lane; wd < body; wd += WAVE) {
                const uint32_t at = head + wd * 4, sh = (at & 3) * 8;
                const uint32_t w0 = s_out[at >> 2], w1 = s_out[(at >> 2) + 1];
                *(uint32_t *)(a + at) = sh ? (w0 >> sh) | (w1 << (32 - sh)) : w0;
            }
            if (tail + lane < n) a[tail + lane] = o8[tail + lane];
        }
        if (lane == 0) {
            status[blk] = ok ? 0 : 1;
            if (!ok) atomicAdd(n_declined, 1u);
        }
    }
}

}  // namespace

void launch_bgzf_inflate(hipStream_t s, const uint8_t *comp, const csv_bgzf_block *blocks, uint32_t n_blocks, uint8_t *out, uint8_t *status, unsigned int *n_declined)
{
    if (n_blocks == 0) return;
    hipLaunchKernelGGL(bgzf_inflate_kernel, dim3(std::min(n_blocks, INFLATE_MAX_GRID)), dim3(WAVE), 0, s, comp, blocks, n_blocks, out, status, n_declined);
}

}  // namespace csv
