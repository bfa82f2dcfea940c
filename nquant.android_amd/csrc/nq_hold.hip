// nq_hold.hip -- temporal hold of palette indices over a frame sequence on gfx950 (include/nquant_abi.h, "temporal hold").
//
// A pixel whose SOURCE colour stays within `threshold` of its anchor keeps the palette index (and the ARGB output) it had in the frame
// before; the anchor moves only when the pixel is released.  Every pixel position is a chain over the frames, independent of every
// other position, so ONE launch covers the whole sequence: a thread owns G consecutive pixels, keeps their anchors and current indices
// (and outputs) in registers and walks frames 1 .. n - 1 through a table of frame pointers in device memory, loading frame i + 1 while
// it decides frame i.
//   hold_kernel<8, .>   the vector path: one 16-byte load / store of the index stream and two of each ARGB stream per thread and frame;
//                       needs every base pointer 16-byte aligned.  The last thread's group may be short (the tail): it alone reads and
//                       writes element by element.
//   hold_kernel<1, .>   the scalar path for any legal alignment (indices 2-byte, ARGB 4-byte): one pixel per thread.
// launch_hold picks the path on the host from the pointers; the kernels never test an address.
// held[i] (optional): the lanes' counts are summed over the wave with shuffles, the waves' sums over the block in LDS, and a block adds
// its sum of a frame with one 64-bit atomic; integer sums do not depend on the order.
#include "nq_kernels.h"

namespace nq {

namespace {

constexpr int HOLD_THREADS = 256;
constexpr int HOLD_SLOTS = 32;           // frames whose counts a block collects in LDS between two flushes

// A pointer read from the frame tables is generic to the compiler (flat_load / flat_store, which also count against the LDS wait
// counter): the frames are device memory, so the accesses name the global address space.
#define HOLD_G __attribute__((address_space(1)))
typedef unsigned hold_v4 __attribute__((ext_vector_type(4)));

// G pixels of one frame: source colours, palette indices, ARGB outputs (unused without an output stream)
template <int G> struct HoldGroup { unsigned src[G], idx[G], out[G]; };

// cnt = G: whole group (G = 8: 16-byte accesses, base is a multiple of 8 and the frames are 16-byte aligned); cnt < G: the first cnt elements
template <int G, bool OUT>
__device__ inline void hold_load(HoldGroup<G>& g, const unsigned* src_, const unsigned short* idx_, const unsigned* out_, long long base, int cnt) {
    const HOLD_G unsigned* src = (const HOLD_G unsigned*) src_;
    const HOLD_G unsigned short* idx = (const HOLD_G unsigned short*) idx_;
    const HOLD_G unsigned* out = (const HOLD_G unsigned*) out_;
    if constexpr (G == 8) {
        if (cnt == 8) {                             // (named components only: an indexable temporary would live in scratch memory)
            const hold_v4 a = *(const HOLD_G hold_v4*) (src + base), b = *(const HOLD_G hold_v4*) (src + base + 4);
            const hold_v4 k = *(const HOLD_G hold_v4*) (idx + base);
            g.src[0] = a.x; g.src[1] = a.y; g.src[2] = a.z; g.src[3] = a.w; g.src[4] = b.x; g.src[5] = b.y; g.src[6] = b.z; g.src[7] = b.w;
            g.idx[0] = k.x & 0xFFFFu; g.idx[1] = k.x >> 16; g.idx[2] = k.y & 0xFFFFu; g.idx[3] = k.y >> 16;
            g.idx[4] = k.z & 0xFFFFu; g.idx[5] = k.z >> 16; g.idx[6] = k.w & 0xFFFFu; g.idx[7] = k.w >> 16;
            if constexpr (OUT) {
                const hold_v4 c = *(const HOLD_G hold_v4*) (out + base), d = *(const HOLD_G hold_v4*) (out + base + 4);
                g.out[0] = c.x; g.out[1] = c.y; g.out[2] = c.z; g.out[3] = c.w; g.out[4] = d.x; g.out[5] = d.y; g.out[6] = d.z; g.out[7] = d.w;
            }
            return;
        }
    }
#pragma unroll
    for (int j = 0; j < G; ++j) {
        const bool in = j < cnt;
        g.src[j] = in ? src[base + j] : 0u;
        g.idx[j] = in ? (unsigned) idx[base + j] : 0u;
        if constexpr (OUT) g.out[j] = in ? out[base + j] : 0u;
    }
}

// writes the group back: whole (cnt = G = 8) with 16-byte stores, else only the held elements (bit j of mask), which lie below cnt
template <int G, bool OUT>
__device__ inline void hold_store(const HoldGroup<G>& g, unsigned short* idx_, unsigned* out_, long long base, int cnt, unsigned mask) {
    HOLD_G unsigned short* idx = (HOLD_G unsigned short*) idx_;
    HOLD_G unsigned* out = (HOLD_G unsigned*) out_;
    if constexpr (G == 8) {
        if (cnt == 8) {
            *(HOLD_G hold_v4*) (idx + base) = hold_v4{g.idx[0] | g.idx[1] << 16, g.idx[2] | g.idx[3] << 16, g.idx[4] | g.idx[5] << 16, g.idx[6] | g.idx[7] << 16};
            if constexpr (OUT) {
                *(HOLD_G hold_v4*) (out + base) = hold_v4{g.out[0], g.out[1], g.out[2], g.out[3]};
                *(HOLD_G hold_v4*) (out + base + 4) = hold_v4{g.out[4], g.out[5], g.out[6], g.out[7]};
            }
            return;
        }
    }
#pragma unroll
    for (int j = 0; j < G; ++j)
        if (j < cnt && (mask >> j & 1u)) {
            idx[base + j] = (unsigned short) g.idx[j];
            if constexpr (OUT) out[base + j] = g.out[j];
        }
}

// largest |difference| of the four 8-bit channels of two ARGB words
__device__ inline int hold_distance(unsigned c, unsigned a) {
    int d = 0;
#pragma unroll
    for (int s = 0; s < 32; s += 8) {
        const int e = (int) ((c >> s) & 255u) - (int) ((a >> s) & 255u);
        d = max(d, e < 0 ? -e : e);
    }
    return d;
}

// src / idx / out: n frame pointers each (out unused without OUT); held: n counters the caller zeroed, or null.  The grid covers
// ceil(npix / G) groups exactly; a thread behind the last group takes part in the reductions with nothing to add.
template <int G, bool OUT>
__global__ void __launch_bounds__(HOLD_THREADS) hold_kernel(const unsigned* const* __restrict__ src, unsigned short* const* __restrict__ idx,
                                                            unsigned* const* __restrict__ out, int n, long long npix, int threshold,
                                                            unsigned long long* __restrict__ held) {
    __shared__ unsigned s_cnt[HOLD_SLOTS];
    const long long base = ((long long) blockIdx.x * HOLD_THREADS + threadIdx.x) * G;
    const int cnt = base >= npix ? 0 : (npix - base >= G ? G : (int) (npix - base));
    if (held) {
        if (threadIdx.x < HOLD_SLOTS) s_cnt[threadIdx.x] = 0;
        __syncthreads();
    }
    HoldGroup<G> prev, cur = {}, nxt = {};
    unsigned anchor[G];
    hold_load<G, OUT>(prev, src[0], idx[0], OUT ? out[0] : nullptr, base, cnt);
#pragma unroll
    for (int j = 0; j < G; ++j) anchor[j] = prev.src[j];
    if (n > 1) hold_load<G, OUT>(cur, src[1], idx[1], OUT ? out[1] : nullptr, base, cnt);
    for (int i = 1; i < n; ++i) {
        if (i + 1 < n) hold_load<G, OUT>(nxt, src[i + 1], idx[i + 1], OUT ? out[i + 1] : nullptr, base, cnt);
        unsigned mask = 0;
#pragma unroll
        for (int j = 0; j < G; ++j) {
            if (j < cnt && hold_distance(cur.src[j], anchor[j]) <= threshold) {
                cur.idx[j] = prev.idx[j];
                if constexpr (OUT) cur.out[j] = prev.out[j];
                mask |= 1u << j;
            } else {
                anchor[j] = cur.src[j];
            }
        }
        if (mask) hold_store<G, OUT>(cur, idx[i], OUT ? out[i] : nullptr, base, cnt, mask);
        if (held) {                                 // (uniform: every thread of the block walks the same frames)
            unsigned c = (unsigned) __popc(mask);
#pragma unroll
            for (int d = 32; d >= 1; d >>= 1) c += __shfl_xor(c, d);
            const int slot = i % HOLD_SLOTS;
            if ((threadIdx.x & 63) == 0 && c) atomicAdd(&s_cnt[slot], c);
            if (slot == HOLD_SLOTS - 1 || i == n - 1) {
                __syncthreads();
                const int f = i - slot + (int) threadIdx.x;
                if (threadIdx.x < HOLD_SLOTS && f <= i) {
                    const unsigned v = s_cnt[threadIdx.x];
                    if (v) atomicAdd(held + f, (unsigned long long) v);
                    s_cnt[threadIdx.x] = 0;
                }
                __syncthreads();
            }
        }
#pragma unroll
        for (int j = 0; j < G; ++j) {
            prev.idx[j] = cur.idx[j];
            if constexpr (OUT) prev.out[j] = cur.out[j];
        }
        cur = nxt;
    }
}

template <int G>
void hold_launch(const unsigned* const* d_src, unsigned short* const* d_idx, unsigned* const* d_out, int n, long long npix, int threshold,
                 unsigned long long* d_held, hipStream_t s) {
    const long long groups = (npix + G - 1) / G;
    const unsigned grid = (unsigned) ((groups + HOLD_THREADS - 1) / HOLD_THREADS);      // npix < 2^31: at most 2^23 blocks
    if (d_out) hipLaunchKernelGGL((hold_kernel<G, true>), dim3(grid), dim3(HOLD_THREADS), 0, s, d_src, d_idx, d_out, n, npix, threshold, d_held);
    else hipLaunchKernelGGL((hold_kernel<G, false>), dim3(grid), dim3(HOLD_THREADS), 0, s, d_src, d_idx, d_out, n, npix, threshold, d_held);
}

} // namespace

void launch_hold(const unsigned* const* d_src, unsigned short* const* d_idx, unsigned* const* d_out, int n, long long npix, int threshold,
                 bool vec, unsigned long long* d_held, hipStream_t s) {
    if (vec) hold_launch<8>(d_src, d_idx, d_out, n, npix, threshold, d_held, s);
    else hold_launch<1>(d_src, d_idx, d_out, n, npix, threshold, d_held, s);
}

} // namespace nq
