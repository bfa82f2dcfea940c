// nq_ordered.hip -- ordered (positional) dither of a frame sequence on gfx950 (include/nquant_abi.h, "ordered dither").
//
// A counted pixel takes the nearest live palette entry i1 or, at a share of the mask positions that grows with how far it lies towards
// the second nearest entry i2, that one: its index depends on its colour, its coordinates and the palette only.  ONE launch covers the
// whole sequence: frame pointers and sizes come from a table in device memory, every workgroup strides over every frame.
//   ordered_kernel<4, ., .>   the vector path: one 16-byte load of four pixels, one 8-byte index store and (with an ARGB output) one
//                             16-byte store per lane and round; needs every source and ARGB output 16-byte and every index map 8-byte
//                             aligned.  The npix % 4 pixels behind the last whole group (the tail) go element by element.
//   ordered_kernel<1, ., .>   the scalar path for any legal alignment (indices 2-byte, ARGB 4-byte): one pixel per lane and round.
// launch_ordered picks the path on the host from the pointers; the kernels never test an address.
//
// Search.  As in nq_refine.hip the live entries sit in LDS as {packed colour, -(((|c|^2 + ORD_OFF) << 8) | index)}, so that
//     -key = (p.c << 9) + word,   key = ((|c|^2 - 2 p.c + ORD_OFF) << 8) | index = ((d(p, c) - |p|^2 + ORD_OFF) << 8) | index:
// the order of the keys is that of (d << 8) | index.  The two largest -key are kept with lo = max(lo, min(top, v)); top = max(top, v):
// one 4 x u8 dot product, one shift-add, one minimum and two maxima per entry and pixel.  |p|^2 is added back once for the two
// distances; the distance of the two entries comes from three more dot products of their colours (palette by index in LDS).
//
// Mask.  The 64 x 64 mask sits in LDS as 4096 bytes, raised by 128 when a workgroup copies it there.  A group of four consecutive
// pixels may straddle a row end: its first pixel's (x, y) comes from one unsigned division of the linear position by the width (both
// below 2^31: exact), the others' by increment-and-wrap.
//
// Statistics (optional).  A lane keeps the pixels that took i2 and the squared error of its pixels of the running frame in registers; at
// the end of a frame a wave that touched it sums them over its lanes with xor-shuffles and one lane adds them with two 64-bit atomics.
// Integer sums do not depend on the order: the result is deterministic.  Without statistics that code is compiled out.
//
// Loop bounds: the entry loop runs nlive <= 256 times; a workgroup walks the n frames once, and in a frame at most
// ceil(groups / (gridDim.x * ORD_THREADS)) rounds plus one for the tail; the reductions are 6 shuffle steps.
#include "nq_kernels.h"

namespace nq {

namespace {

constexpr int ORD_THREADS = 256;
constexpr int ORD_WAVES = ORD_THREADS / 64;
constexpr long long ORD_MAX_BLOCKS = 2048;           // the grid cap: 8 workgroups per compute unit of an unpartitioned MI355X
constexpr long long ORD_MIN_PIXELS = 1024;           // pixels a workgroup handles at least: one round of the vector path
constexpr unsigned ORD_OFF = 2u * 4u * 255u * 255u;  // 520 200 >= 2 p.c

#define ORD_G __attribute__((address_space(1)))
typedef unsigned ord_v4 __attribute__((ext_vector_type(4)));
typedef unsigned ord_v2 __attribute__((ext_vector_type(2)));

__device__ const int8_t g_ord_mask[4096] __attribute__((aligned(16))) = {
#include "../../include/nq_blue_noise_64x64.inc"
};

__device__ inline unsigned ord_dot(unsigned a, unsigned b) { return __builtin_amdgcn_udot4(a, b, 0u, false); }

// largest |difference| of the four 8-bit channels of two ARGB words
__device__ inline int ord_far(unsigned a, unsigned b) {
    int d = 0;
#pragma unroll
    for (int s = 0; s < 32; s += 8) {
        const int e = (int) ((a >> s) & 255u) - (int) ((b >> s) & 255u);
        d = max(d, e < 0 ? -e : e);
    }
    return d;
}

// G pixels p[] at the linear positions pos .. pos + G - 1 of a frame `width` wide: the entries taken in k[].  For the inside, counted
// pixels it adds the ones that took i2 to `mixed` and their squared error to `err` (STATS only).
template <int G, bool STATS>
__device__ inline void ord_pick(const uint2* ent, const unsigned* pal, const unsigned char* msk, int nlive, int T, int limit, unsigned width,
                                unsigned pos, const unsigned (&p)[G], const bool (&inside)[G], unsigned (&k)[G], unsigned& mixed,
                                unsigned long long& err) {
    int top[G], lo[G];                              // the largest and the second largest -key so far
#pragma unroll
    for (int i = 0; i < G; ++i) top[i] = lo[i] = (int) 0x80000000u;
#pragma unroll 4
    for (int j = 0; j < nlive; ++j) {
        const uint2 e = ent[j];                     // (the same address in every lane: one broadcast read)
#pragma unroll
        for (int i = 0; i < G; ++i) {
            const int v = (int) ((ord_dot(p[i], e.x) << 9) + e.y);
            lo[i] = max(lo[i], min(top[i], v));
            top[i] = max(top[i], v);
        }
    }
    unsigned y = pos / width, x = pos - y * width;  // (one exact unsigned division per group)
#pragma unroll
    for (int i = 0; i < G; ++i) {
        const int m = (int) msk[(y & 63u) * 64u + (x & 63u)];
        if (++x == width) { x = 0; ++y; }
        const bool counted = (p[i] >> 24) != 0 || T < 0;
        unsigned taken = (unsigned) (T < 0 ? 0 : T);           // a pixel that is not counted, and every pixel when no entry is live
        unsigned d = 0;
        if (nlive > 0) {                            // (uniform)
            const unsigned k1 = 0u - (unsigned) top[i], k2 = 0u - (unsigned) lo[i];
            const unsigned i1 = k1 & 255u, i2 = k2 & 255u;     // (nlive == 1: k2 = 2^31, i2 = 0, not used)
            const unsigned c1 = pal[i1], c2 = pal[i2];
            const int delta = (int) (k2 >> 8) - (int) (k1 >> 8);
            const int den = (int) (ord_dot(c1, c1) + ord_dot(c2, c2)) - 2 * (int) ord_dot(c1, c2);
            const bool mix = nlive > 1 && limit > 0 && ord_far(c1, c2) <= limit && (255 - 2 * m) * den > 256 * delta;
            if (counted) {
                taken = mix ? i2 : i1;
                if constexpr (STATS) {
                    d = (k1 >> 8) - ORD_OFF + ord_dot(p[i], p[i]) + (mix ? (unsigned) delta : 0u);
                    if (inside[i] && mix) mixed += 1;
                }
            }
        } else if constexpr (STATS) {
            if (counted) {
                const unsigned c = pal[0];
                d = ord_dot(p[i], p[i]) + ord_dot(c, c) - 2u * ord_dot(p[i], c);
            }
        }
        if constexpr (STATS) { if (inside[i] && counted) err += d; }
        k[i] = taken;
    }
}

// frames: n entries; the grid is B workgroups; of frame f, workgroup (blockIdx.x + f) % B takes the groups of G pixels
// (round * B + it) * ORD_THREADS + thread, and the one with number 0 the tail.  pal: the K palette entries.  stats: 2 n sums the caller
// zeroed (STATS only).
template <int G, bool OUT, bool STATS>
__global__ void __launch_bounds__(ORD_THREADS) ordered_kernel(const OrderedFrame* __restrict__ frames, int n, const unsigned* __restrict__ palette,
                                                              int K, int T, int limit, unsigned long long* __restrict__ stats) {
    __shared__ uint2 s_ent[256];
    __shared__ unsigned s_pal[256];
    __shared__ unsigned s_mask[4096 / 4];           // the mask, raised by 128, as 4096 bytes
    __shared__ int s_wn[ORD_WAVES];
    const int t = threadIdx.x, wave = t >> 6;
    // the live entries, in ascending order
    const unsigned c = t < K ? palette[t] : 0u;
    const bool live = (c >> 24) != 0;
    const unsigned long long lm = __ballot(live);
    if ((t & 63) == 0) s_wn[wave] = __popcll(lm);
    s_pal[t] = c;
    // (mask + 128 of a signed byte is the byte with its top bit flipped)
    for (int i = t; i < 4096 / 4; i += ORD_THREADS) s_mask[i] = reinterpret_cast<const unsigned*>(g_ord_mask)[i] ^ 0x80808080u;
    __syncthreads();
    int at = __popcll(lm & ((1ull << (t & 63)) - 1ull)), nlive = 0;
#pragma unroll
    for (int w = 0; w < ORD_WAVES; ++w) { if (w < wave) at += s_wn[w]; nlive += s_wn[w]; }
    if (live) s_ent[at] = make_uint2(c, 0u - (((ord_dot(c, c) + ORD_OFF) << 8) | (unsigned) t));
    __syncthreads();
    const long long B = gridDim.x;
    for (int f = 0; f < n; ++f) {
        const OrderedFrame fr = frames[f];
        const ORD_G unsigned* src = (const ORD_G unsigned*) fr.pixels;
        ORD_G unsigned short* idx = (ORD_G unsigned short*) fr.index;
        ORD_G unsigned* out = (ORD_G unsigned*) fr.argb;
        const long long npix = fr.npix;
        const unsigned width = (unsigned) fr.width;
        const long long groups = npix / G;          // whole groups
        const long long b = ((long long) blockIdx.x + f) % B;
        unsigned mixed = 0;
        unsigned long long err = 0;
        bool touched = false;
        for (long long g = b * ORD_THREADS + t; g < groups; g += B * ORD_THREADS) {
            unsigned p[G], k[G];
            bool inside[G];
            if constexpr (G == 4) {
                const ord_v4 v = *(const ORD_G ord_v4*) (src + g * 4);
                p[0] = v.x; p[1] = v.y; p[2] = v.z; p[3] = v.w;
            } else {
                p[0] = src[g];
            }
#pragma unroll
            for (int i = 0; i < G; ++i) inside[i] = true;
            ord_pick<G, STATS>(s_ent, s_pal, reinterpret_cast<const unsigned char*>(s_mask), nlive, T, limit, width, (unsigned) (g * G), p, inside, k, mixed, err);
            if constexpr (G == 4) {
                *(ORD_G ord_v2*) (idx + g * 4) = ord_v2{k[0] | k[1] << 16, k[2] | k[3] << 16};
                if constexpr (OUT) *(ORD_G ord_v4*) (out + g * 4) = ord_v4{s_pal[k[0]], s_pal[k[1]], s_pal[k[2]], s_pal[k[3]]};
            } else {
                idx[g] = (unsigned short) k[0];
                if constexpr (OUT) out[g] = s_pal[k[0]];
            }
            touched = true;
        }
        if constexpr (G > 1) {                      // the tail, element by element
            const long long at_tail = groups * G + t;
            if (b == 0 && at_tail < npix) {
                unsigned p[G], k[G];
                bool inside[G];
#pragma unroll
                for (int i = 0; i < G; ++i) { p[i] = 0u; inside[i] = false; }
                p[0] = src[at_tail];
                inside[0] = true;
                ord_pick<G, STATS>(s_ent, s_pal, reinterpret_cast<const unsigned char*>(s_mask), nlive, T, limit, width, (unsigned) at_tail, p, inside, k, mixed, err);
                idx[at_tail] = (unsigned short) k[0];
                if constexpr (OUT) out[at_tail] = s_pal[k[0]];
                touched = true;
            }
        }
        if constexpr (STATS) {
            if (__any(touched)) {                   // (wave-uniform: every lane of the wave takes part in the shuffles)
#pragma unroll
                for (int s = 32; s > 0; s >>= 1) {
                    mixed += (unsigned) __shfl_xor((int) mixed, s);
                    err += (unsigned long long) __shfl_xor((long long) err, s);
                }
                if ((t & 63) == 0) {
                    if (mixed) atomicAdd(stats + 2 * (long long) f, (unsigned long long) mixed);
                    if (err) atomicAdd(stats + 2 * (long long) f + 1, err);
                }
            }
        }
    }
}

template <int G, bool OUT>
void ordered_launch(const OrderedFrame* d_frames, int n, unsigned grid, const unsigned* d_palette, int K, int T, int limit,
                    unsigned long long* d_stats, hipStream_t s) {
    if (d_stats) hipLaunchKernelGGL((ordered_kernel<G, OUT, true>), dim3(grid), dim3(ORD_THREADS), 0, s, d_frames, n, d_palette, K, T, limit, d_stats);
    else hipLaunchKernelGGL((ordered_kernel<G, OUT, false>), dim3(grid), dim3(ORD_THREADS), 0, s, d_frames, n, d_palette, K, T, limit, d_stats);
}

} // namespace

void launch_ordered(const OrderedFrame* d_frames, int n, long long total, bool vec, bool out, const unsigned* d_palette, int K, int T, int limit,
                    unsigned long long* d_stats, hipStream_t s) {
    // workgroups: never so many that one handles fewer than ORD_MIN_PIXELS, at most ORD_MAX_BLOCKS, at least one
    long long B = total / ORD_MIN_PIXELS;
    if (B > ORD_MAX_BLOCKS) B = ORD_MAX_BLOCKS;
    if (B < 1) B = 1;
    if (vec) {
        if (out) ordered_launch<4, true>(d_frames, n, (unsigned) B, d_palette, K, T, limit, d_stats, s);
        else ordered_launch<4, false>(d_frames, n, (unsigned) B, d_palette, K, T, limit, d_stats, s);
    } else {
        if (out) ordered_launch<1, true>(d_frames, n, (unsigned) B, d_palette, K, T, limit, d_stats, s);
        else ordered_launch<1, false>(d_frames, n, (unsigned) B, d_palette, K, T, limit, d_stats, s);
    }
}

} // namespace nq
