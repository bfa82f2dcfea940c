// nq_refine.hip -- k-means (Lloyd) passes over a palette and its squared error on gfx950 (include/nquant_abi.h, "palette
// refinement").
//
// An assignment pass gives every counted pixel (alpha != 0) of the sequence to the live palette entry (alpha != 0) with the smallest
// d = da^2 + dr^2 + dg^2 + db^2, lowest index on a tie, and sums per entry {pixels, r, g, b} and over all pixels d.  ONE launch covers
// the whole sequence: frame pointers and sizes come from a table in device memory, every workgroup strides over every frame.
//   refine_pass_kernel<4>   the vector path: one 16-byte load of four pixels per lane and round; needs every frame 16-byte aligned.
//                           The npix % 4 pixels behind the last whole group (the tail) are read element by element.
//   refine_pass_kernel<1>   the scalar path for 4-byte aligned frames: one pixel per lane and round.
// launch_refine picks the path on the host from the pointers; the kernels never test an address.
//
// Inner loop.  |p|^2 does not change the argmin, so a pixel's order of the entries is that of
//     key = ((|c|^2 - 2 p.c + REF_OFF) << 8) | index,   REF_OFF = 2 * 4 * 255^2 keeps it non-negative, key < 2^28:
// the smallest key is the smallest distance and, among equal distances, the lowest index.  The live entries sit in LDS as {packed
// colour, -(((|c|^2 + REF_OFF) << 8) | index)}, so that -key = (p.c << 9) + word: an entry costs one 4 x u8 dot product
// (v_dot4_u32_u8), one shift-add (v_lshl_add_u32) and half a three-way signed maximum (v_max3_i32) per pixel.  |p|^2 is added back
// once for the error.
//
// Accumulation.  One sub-table [256][4] of 32-bit LDS counters per wave (waves never meet on a counter).  A lane merges equal
// neighbouring entries of its four pixels before the atomics; when every counted pixel of the wave's round has one entry, the wave sums
// over its lanes and ONE lane adds (flat content would otherwise send 64 lanes to four counters).  A workgroup flushes its counters to
// the 64-bit global sums before it has counted more than REF_FLUSH_PIXELS = 2^24 pixels since the last flush: a counter is at most
// 255 * 2^24 < 2^32.  The flush adds the non-zero counters with 64-bit global atomics; the error is kept in a 64-bit register per lane
// and added once per wave.  Integer sums do not depend on the order: the result is deterministic.
//
// refine_update_kernel (K threads) turns the sums into the next palette (rounded mean of r, g, b; alpha, empty and pinned entries
// stay), records the pass's error and counts, clears the sums and raises `done` when nothing changed.  All passes of a call are
// enqueued up front; a pass that finds `done` set returns at once, so the host waits once per call.
#include "nq_kernels.h"

namespace nq {

namespace {

constexpr int REF_THREADS = 256;
constexpr int REF_WAVES = REF_THREADS / 64;
constexpr long long REF_MIN_PIXELS = 16384;          // pixels a workgroup reads at least (64 KB) for the atomics of its flush
#ifndef NQ_REFINE_FLUSH_PIXELS                        // (build.py NQ_BUILD_DEFS: a small value runs the tests through the flush inside the loop)
#define NQ_REFINE_FLUSH_PIXELS (1 << 24)
#endif
constexpr unsigned REF_FLUSH_PIXELS = NQ_REFINE_FLUSH_PIXELS;   // 255 * 2^24 < 2^32: what a 32-bit LDS counter holds
constexpr unsigned REF_OFF = 2u * 4u * 255u * 255u;  // 520 200 >= 2 p.c

#define REF_G __attribute__((address_space(1)))
typedef unsigned ref_v4 __attribute__((ext_vector_type(4)));

__device__ inline unsigned ref_dot(unsigned a, unsigned b) { return __builtin_amdgcn_udot4(a, b, 0u, false); }

// one run of a lane's pixels into the sub-table h
__device__ inline void ref_add(unsigned* h, unsigned k, unsigned cnt, unsigned r, unsigned g, unsigned b) {
    atomicAdd(&h[k * 4 + 0], cnt);
    atomicAdd(&h[k * 4 + 1], r);
    atomicAdd(&h[k * 4 + 2], g);
    atomicAdd(&h[k * 4 + 3], b);
}

// The G pixels p[] of every lane of the wave (inside: the pixel exists) against the nlive entries ent[]; counts into h, returns the
// lane's squared error.  Called by all lanes of the wave together.
template <int G>
__device__ inline unsigned ref_count(const uint2* ent, int nlive, unsigned* h, const unsigned (&p)[G], const bool (&inside)[G]) {
    int top[G];                                     // the largest -key so far
#pragma unroll
    for (int i = 0; i < G; ++i) top[i] = (int) 0x80000000u;
#pragma unroll 4
    for (int j = 0; j < nlive; ++j) {
        const uint2 e = ent[j];                     // (the same address in every lane: one broadcast read)
#pragma unroll
        for (int i = 0; i < G; ++i) top[i] = max(top[i], (int) ((ref_dot(p[i], e.x) << 9) + e.y));
    }
    unsigned err = 0, best[G];
    bool counted[G];
    unsigned k[G];
    int lk = -1;                                    // the entry of this lane's first counted pixel
    bool uni = true;                                // ... and whether all its counted pixels have it
#pragma unroll
    for (int i = 0; i < G; ++i) {
        counted[i] = inside[i] && (p[i] >> 24) != 0;
        best[i] = (unsigned) -top[i];
        k[i] = best[i] & 255u;
        if (counted[i]) {
            err += (best[i] >> 8) - REF_OFF + ref_dot(p[i], p[i]);
            if (lk < 0) lk = (int) k[i];
            else uni = uni && (int) k[i] == lk;
        }
    }
    const unsigned long long any = __ballot(lk >= 0);
    if (any == 0) return 0;                         // (wave-uniform)
    const int first = __shfl(lk, (int) __ffsll(any) - 1);
    if (__all(lk < 0 || (uni && lk == first))) {    // (wave-uniform) one entry for the whole round: sum over the lanes, one lane adds
        unsigned cr = 0, gb = 0;                    // {count, r} and {g, b} in 16-bit halves: at most 256 pixels, sums <= 65 280
#pragma unroll
        for (int i = 0; i < G; ++i)
            if (counted[i]) {
                cr += (1u << 16) + ((p[i] >> 16) & 255u);
                gb += (((p[i] >> 8) & 255u) << 16) + (p[i] & 255u);
            }
#pragma unroll
        for (int s = 32; s > 0; s >>= 1) {
            cr += (unsigned) __shfl_xor((int) cr, s);
            gb += (unsigned) __shfl_xor((int) gb, s);
        }
        if ((threadIdx.x & 63) == 0) ref_add(h, (unsigned) first, cr >> 16, cr & 0xFFFFu, gb >> 16, gb & 0xFFFFu);
        return err;
    }
    int run = -1;
    unsigned c = 0, r = 0, g = 0, b = 0;
#pragma unroll
    for (int i = 0; i < G; ++i) {
        if (!counted[i]) continue;
        if ((int) k[i] != run) {
            if (run >= 0) ref_add(h, (unsigned) run, c, r, g, b);
            run = (int) k[i]; c = r = g = b = 0;
        }
        c += 1; r += (p[i] >> 16) & 255u; g += (p[i] >> 8) & 255u; b += p[i] & 255u;
    }
    if (run >= 0) ref_add(h, (unsigned) run, c, r, g, b);
    return err;
}

// the workgroup's counters into the global sums, and cleared
__device__ inline void ref_flush(unsigned (*s_h)[256 * 4], int K, unsigned long long* acc) {
    // Every wave's LDS adds must have landed before another wave reads the counters.  The wait is spelled out (lgkmcnt(0); vmcnt and
    // expcnt left alone): for the flush at the top of the round loop the compiler emitted the barrier without it, and the last add of
    // a round (the b sums) was lost.
    __builtin_amdgcn_s_waitcnt(0xC07F);
    __syncthreads();
    for (int i = threadIdx.x; i < K * 4; i += REF_THREADS) {
        unsigned long long v = 0;
#pragma unroll
        for (int w = 0; w < REF_WAVES; ++w) { v += s_h[w][i]; s_h[w][i] = 0; }
        if (v) atomicAdd(acc + i, v);
    }
    __syncthreads();
}

// frames: n entries; the grid is B workgroups, workgroup b takes of every frame the groups of G pixels (round * B + b) * REF_THREADS +
// thread.  st: the call's state (RefineState layout, nq_kernels.h).
template <int G>
__global__ void __launch_bounds__(REF_THREADS) refine_pass_kernel(const RefineFrame* __restrict__ frames, int n, int K,
                                                                  unsigned long long* __restrict__ st) {
    __shared__ uint2 s_ent[256];
    __shared__ unsigned s_h[REF_WAVES][256 * 4];
    __shared__ int s_wn[REF_WAVES];
    if (st[REFINE_DONE]) return;                    // (uniform over the grid: written by the update kernel of an earlier pass)
    const unsigned* pal = reinterpret_cast<const unsigned*>(st + REFINE_PALETTE);
    const int t = threadIdx.x, wave = t >> 6;
    // the live entries, in ascending order
    const unsigned c = t < K ? pal[t] : 0u;
    const bool live = (c >> 24) != 0;
    const unsigned long long mask = __ballot(live);
    if ((t & 63) == 0) s_wn[wave] = __popcll(mask);
    for (int i = t; i < REF_WAVES * 256 * 4; i += REF_THREADS) (&s_h[0][0])[i] = 0;
    __syncthreads();
    int at = __popcll(mask & ((1ull << (t & 63)) - 1ull)), nlive = 0;
#pragma unroll
    for (int w = 0; w < REF_WAVES; ++w) { if (w < wave) at += s_wn[w]; nlive += s_wn[w]; }
    if (live) s_ent[at] = make_uint2(c, 0u - (((ref_dot(c, c) + REF_OFF) << 8) | (unsigned) t));
    __syncthreads();
    if (nlive == 0) return;                         // no live entry: no pixel is counted
    unsigned* h = s_h[wave];
    const long long B = gridDim.x, b = blockIdx.x;
    unsigned long long err = 0;
    unsigned seen = 0;                              // pixels this workgroup may have counted since its last flush (uniform)
    for (int f = 0; f < n; ++f) {
        const REF_G unsigned* src = (const REF_G unsigned*) frames[f].pixels;
        const long long npix = frames[f].npix;
        const long long groups = npix / G;          // whole groups
        const long long per_round = B * REF_THREADS;
        const long long rounds = (groups + per_round - 1) / per_round;   // the same for every workgroup: the wave-level steps need all lanes
        for (long long r = 0; r < rounds; ++r) {
            if (seen + REF_THREADS * G > REF_FLUSH_PIXELS) { ref_flush(s_h, K, st + REFINE_ACC); seen = 0; }
            seen += REF_THREADS * G;
            const long long g = (r * B + b) * REF_THREADS + t;
            const bool valid = g < groups;
            unsigned p[G];
            bool inside[G];
            if constexpr (G == 4) {
                ref_v4 v = {0u, 0u, 0u, 0u};
                if (valid) v = *(const REF_G ref_v4*) (src + g * 4);
                p[0] = v.x; p[1] = v.y; p[2] = v.z; p[3] = v.w;
            } else {
                p[0] = valid ? src[g] : 0u;
            }
#pragma unroll
            for (int i = 0; i < G; ++i) inside[i] = valid;
            err += ref_count<G>(s_ent, nlive, h, p, inside);
        }
        if constexpr (G > 1) {                      // the tail, element by element
            if (b == 0 && npix != groups * G) {     // (uniform over the workgroup)
                if (seen + REF_THREADS * G > REF_FLUSH_PIXELS) { ref_flush(s_h, K, st + REFINE_ACC); seen = 0; }
                seen += REF_THREADS * G;
                unsigned p[G];
                bool inside[G];
#pragma unroll
                for (int i = 0; i < G; ++i) { p[i] = 0u; inside[i] = false; }
                inside[0] = (long long) t < npix - groups * G;
                if (inside[0]) p[0] = src[groups * G + t];
                err += ref_count<G>(s_ent, nlive, h, p, inside);
            }
        }
    }
    ref_flush(s_h, K, st + REFINE_ACC);
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) err += (unsigned long long) __shfl_xor((long long) err, s);
    if ((t & 63) == 0 && err) atomicAdd(st + REFINE_SSE_ACC, err);
}

// After assignment pass j (one workgroup of REF_THREADS >= K threads): sse[j] and the counts recorded; unless j is the last pass the
// next palette, `done` raised and the remaining sse[] filled when nothing changed; the sums cleared.
__global__ void __launch_bounds__(REF_THREADS) refine_update_kernel(int K, int j, int iterations, unsigned long long* __restrict__ st) {
    if (st[REFINE_DONE]) return;
    unsigned* pal = reinterpret_cast<unsigned*>(st + REFINE_PALETTE);
    const int k = threadIdx.x;
    const unsigned long long sse = st[REFINE_SSE_ACC];
    int changed = 0;
    if (k < K) {
        unsigned long long* a = st + REFINE_ACC + k * 4;
        const unsigned long long cnt = a[0];
        st[REFINE_COUNTS + k] = cnt;
        if (j < iterations && cnt > 0) {            // (cnt > 0 only for a live entry)
            const unsigned old = pal[k];
            unsigned nw = old & 0xFF000000u;
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) nw |= (unsigned) ((2 * a[1 + ch] + cnt) / (2 * cnt)) << (16 - 8 * ch);    // mean, half rounds up
            if (nw != old) { pal[k] = nw; changed = 1; }
        }
        a[0] = a[1] = a[2] = a[3] = 0;
    }
    changed = __syncthreads_or(changed);
    if (k == 0) {
        st[REFINE_SSE_OUT + j] = sse;
        st[REFINE_PASSES] = (unsigned long long) (j + 1);
        st[REFINE_SSE_ACC] = 0;
        if (j < iterations && !changed) st[REFINE_DONE] = 1;
    }
    if (j < iterations && !changed)
        for (int i = j + 1 + k; i <= iterations; i += REF_THREADS) st[REFINE_SSE_OUT + i] = sse;
}

} // namespace

void launch_refine(const RefineFrame* d_frames, int n, long long total, bool vec, int cus, int K, int iterations, unsigned long long* d_state,
                   hipStream_t s) {
    // workgroups: enough to fill the device (8 per CU), never so many that one reads fewer than REF_MIN_PIXELS, at least one
    long long B = total / REF_MIN_PIXELS;
    const long long cap = 8ll * (cus > 0 ? cus : 256);
    if (B > cap) B = cap;
    if (B < 1) B = 1;
    for (int j = 0; j <= iterations; ++j) {
        if (vec) hipLaunchKernelGGL((refine_pass_kernel<4>), dim3((unsigned) B), dim3(REF_THREADS), 0, s, d_frames, n, K, d_state);
        else hipLaunchKernelGGL((refine_pass_kernel<1>), dim3((unsigned) B), dim3(REF_THREADS), 0, s, d_frames, n, K, d_state);
        hipLaunchKernelGGL(refine_update_kernel, dim3(1), dim3(REF_THREADS), 0, s, K, j, iterations, d_state);
    }
}

} // namespace nq
