// nq_shots.hip -- per-frame colour signatures for shot detection on gfx950 (include/nquant_abi.h, "shot detection").
//
// sig[frame][c][v] = pixels of the frame whose channel c (a, r, g, b: shifts 24, 16, 8, 0) has the value v: four 256-bin histograms,
// NQ_SIG_WORDS = 1024 counters per frame.  ONE launch covers the whole sequence: the grid is bpf workgroups per frame (launch_signatures
// bounds it), frame pointers come from a table in device memory, and a workgroup grid-strides over its frame's pixels, counts in LDS
// with integer atomics and at its end adds its non-zero counters to sig[frame] with one 32-bit global atomic each.  Integer sums do
// not depend on the order: the result is deterministic.
//   signature_kernel<4>   the vector path: one 16-byte load of four pixels per lane and round; needs every frame 16-byte aligned.
//                         The npix % 4 pixels behind the last whole group (the tail) are read element by element.
//   signature_kernel<1>   the scalar path for 4-byte aligned frames: one pixel per lane and round.
// launch_signatures picks the path on the host from the pointers; the kernels never test an address.
//
// Same-address contention (a flat frame sends every lane's four channels to four counters; opaque footage sends every alpha there)
// is met in three steps (timed one by one, DESIGN.md 5b "Shot detection"):
//   one sub-histogram per wave (SIG_WAVES x 4 KB of LDS), so that waves never meet on a counter;
//   a lane merges equal neighbouring values of its four pixels before the atomic (one add of the run length);
//   wave-level match: a channel in which every pixel of the wave's round has the first lane's value costs ONE add of the pixel
//   count by one lane.  The test is an XOR/OR over the lane's words and one ballot per channel.
// LDS counters are 32 bits wide: a workgroup sees fewer than 2^31 pixels.
#include "nq_kernels.h"

namespace nq {

namespace {

constexpr int SIG_THREADS = 256;
constexpr int SIG_WAVES = SIG_THREADS / 64;
constexpr int SIG_WORDS = 1024;
constexpr long long SIG_MIN_PIXELS = 16384;      // pixels a workgroup reads at least (64 KB) for the 1024 atomics of its flush

// A pointer read from the frame table is generic to the compiler (flat_load, which also counts against the LDS wait counter): the
// frames are device memory, so the loads name the global address space.
#define SIG_G __attribute__((address_space(1)))
typedef unsigned sig_v4 __attribute__((ext_vector_type(4)));

// one pixel into the sub-histogram h
__device__ inline void sig_count_one(unsigned* h, unsigned p) {
#pragma unroll
    for (int c = 0; c < 4; ++c) atomicAdd(&h[c * 256 + ((p >> (24 - 8 * c)) & 255u)], 1u);
}

// The G pixels p[] of every lane of the wave (valid: this lane has pixels; the lanes without are the wave's last) into h.  Called by
// all lanes of the wave together.
template <int G>
__device__ inline void sig_count(unsigned* h, const unsigned (&p)[G], bool valid) {
    // bits in which any pixel of this lane differs from the first lane's first pixel
    const unsigned first = (unsigned) __builtin_amdgcn_readfirstlane((int) p[0]);
    unsigned d = p[0] ^ first;
#pragma unroll
    for (int j = 1; j < G; ++j) d |= p[0] ^ p[j];
    if (!valid) d = 0;
    const unsigned total = (unsigned) G * (unsigned) __popcll(__ballot(valid));
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const int s = 24 - 8 * c;
        if (__all(((d >> s) & 255u) == 0)) {                       // (wave-uniform branch)
            if ((threadIdx.x & 63) == 0 && total) atomicAdd(&h[c * 256 + ((first >> s) & 255u)], total);
        } else if (valid) {
            unsigned run = 1;
#pragma unroll
            for (int j = 0; j + 1 < G; ++j) {
                const unsigned x = (p[j] >> s) & 255u;
                if (x == ((p[j + 1] >> s) & 255u)) ++run;
                else { atomicAdd(&h[c * 256 + x], run); run = 1; }
            }
            atomicAdd(&h[c * 256 + ((p[G - 1] >> s) & 255u)], run);
        }
    }
}

// frames: n frame pointers (npix pixels each); the grid is n * bpf workgroups, workgroup b of a frame takes the groups of G pixels
// (round * bpf + b) * SIG_THREADS + thread; sig: n * SIG_WORDS counters the caller zeroed.
template <int G>
__global__ void __launch_bounds__(SIG_THREADS) signature_kernel(const unsigned* const* __restrict__ frames, int bpf, long long npix,
                                                                unsigned* __restrict__ sig) {
    __shared__ unsigned s_h[SIG_WAVES][SIG_WORDS];
    const long long frame = blockIdx.x / (unsigned) bpf;
    const int b = (int) (blockIdx.x % (unsigned) bpf);
    for (int i = threadIdx.x; i < SIG_WAVES * SIG_WORDS; i += SIG_THREADS) (&s_h[0][0])[i] = 0;
    __syncthreads();
    const SIG_G unsigned* src = (const SIG_G unsigned*) frames[frame];
    unsigned* h = s_h[threadIdx.x >> 6];
    const long long groups = npix / G;              // whole groups
    const long long per_round = (long long) bpf * SIG_THREADS;
    const long long rounds = (groups + per_round - 1) / per_round;      // the same for every workgroup: the wave-level steps need all lanes
    for (long long r = 0; r < rounds; ++r) {
        const long long g = (r * bpf + b) * SIG_THREADS + threadIdx.x;
        const bool valid = g < groups;
        unsigned p[G];
        if constexpr (G == 4) {
            sig_v4 v = {0u, 0u, 0u, 0u};
            if (valid) v = *(const SIG_G sig_v4*) (src + g * 4);
            p[0] = v.x; p[1] = v.y; p[2] = v.z; p[3] = v.w;
        } else {
            p[0] = valid ? src[g] : 0u;
        }
        sig_count<G>(h, p, valid);
    }
    if constexpr (G > 1) {                          // the tail, element by element
        if (b == 0 && (long long) threadIdx.x < npix - groups * G) sig_count_one(h, src[groups * G + threadIdx.x]);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < SIG_WORDS; i += SIG_THREADS) {
        unsigned v = 0;
#pragma unroll
        for (int w = 0; w < SIG_WAVES; ++w) v += s_h[w][i];
        if (v) atomicAdd(sig + frame * SIG_WORDS + i, v);
    }
}

} // namespace

void launch_signatures(const unsigned* const* d_frames, int n, long long npix, bool vec, int cus, unsigned* d_sig, hipStream_t s) {
    // workgroups per frame: enough to fill the device (8 per CU over the sequence), never so many that one reads fewer than
    // SIG_MIN_PIXELS, at least one.  n * bpf <= max(n, 8 * cus): n * npix < 2^31 bounds the grid.
    long long bpf = npix / SIG_MIN_PIXELS;
    const long long cap = (8ll * (cus > 0 ? cus : 256) + n - 1) / n;
    if (bpf > cap) bpf = cap;
    if (bpf < 1) bpf = 1;
    const unsigned grid = (unsigned) (bpf * n);
    if (vec) hipLaunchKernelGGL((signature_kernel<4>), dim3(grid), dim3(SIG_THREADS), 0, s, d_frames, (int) bpf, npix, d_sig);
    else hipLaunchKernelGGL((signature_kernel<1>), dim3(grid), dim3(SIG_THREADS), 0, s, d_frames, (int) bpf, npix, d_sig);
}

} // namespace nq
