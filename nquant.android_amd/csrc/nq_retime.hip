// nq_retime.hip -- retime a sequence of ARGB frames: every output frame is the weighted mean of a window of source frames, on gfx950
// (include/nquant_abi.h "retiming").
//
// Output pixel p of output j is the footprint sum of nq_resample.hip with time in place of x and y: over the window's (source, weight)
// pairs S_a = sum w a and S_c = sum w a T[c] in unsigned 64-bit (w a T[c] is ONE 32 x 32 -> 64 multiply of w by a T[c] < 2^24; the sums
// stay below 2^31 255 65535 < 2^55), then A = floor((2 S_a + W) / (2 W)) and rs_encode per channel, once.  The outputs of a launch and
// their windows travel in the kernel arguments (RetimeLaunch): nothing is read from a table in device memory.
//   * A work item is (output of the launch, block of RT_BLOCK pixels); a workgroup takes the items blockIdx.x, + gridDim.x, ...
//   * A thread owns four pixels and walks the window RT_DEPTH sources at a time: their loads are issued before the first is used;
//     behind the window's last pair that pair's frame is read again, with weight 0.
//   retime_kernel<true>   the vector path: the thread's pixels are adjacent and come with one 16-byte load per source; needs every
//                         frame of the launch 16-byte aligned.  The px mod 4 pixels behind the last whole group are taken by the
//                         thread behind that group, one pixel per access.
//   retime_kernel<false>  any 4-byte aligned frames: the thread's pixels lie RT_THREADS apart, one pixel per access.
// launch_retime takes the path from the host; the kernels never test an address.  Every loop is bounded by the pairs of a window
// (<= 64) or the item count; workgroups do not wait for each other.
#include "nq_kernels.h"

namespace nq {

namespace {

constexpr int RT_THREADS = 256;
constexpr int RT_BLOCK = 4 * RT_THREADS;     // pixels of a work item: four per thread
constexpr int RT_DEPTH = 4;                  // sources a thread has in flight
constexpr long long RT_MAX_BLOCKS = 8192;    // grid cap: a workgroup walks the items blockIdx.x + k * gridDim.x

#include "nq_resample.inc"                     // RS_G, rs_v4, rs_u64, RS_LINEAR, rs_encode

// items = a.count * bpf, bpf = blocks per frame; item -> (output, block) with the block fastest.  px < 2^31.
template <bool VEC>
__global__ void __launch_bounds__(RT_THREADS) retime_kernel(RetimeLaunch a, int items, int bpf, unsigned px, int linear) {
    __shared__ unsigned short s_T[256];
    const int t = threadIdx.x;
    s_T[t] = linear ? RS_LINEAR[t] : (unsigned short) (257 * t);
    __syncthreads();
    for (int item = blockIdx.x; item < items; item += gridDim.x) {
        const int o = item / bpf;
        const unsigned base = (unsigned) (item - o * bpf) * (unsigned) RT_BLOCK;        // < px <= 2^31 - 1
        // the thread's pixels: pix[e] for e < count.  Vector path: a whole group (wide), or the tail behind the last whole group.
        unsigned pix[4];
        int count = 0;
        bool wide = false;
        if constexpr (VEC) {
            const unsigned p0 = base + 4u * (unsigned) t;
            wide = p0 + 4u <= px;
            count = wide ? 4 : (p0 < px ? (int) (px - p0) : 0);
#pragma unroll
            for (int e = 0; e < 4; ++e) pix[e] = p0 + (unsigned) e;
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                pix[e] = base + (unsigned) (t + e * RT_THREADS);
                if (pix[e] < px) count = e + 1;
            }
        }
        if (count == 0) continue;
        rs_u64 S[4][4];
#pragma unroll
        for (int e = 0; e < 4; ++e) S[e][0] = S[e][1] = S[e][2] = S[e][3] = 0;
        const int k0 = a.first[o], k1 = a.first[o + 1] - 1;       // the window's pairs k0 .. k1
        for (int kb = k0; kb <= k1; kb += RT_DEPTH) {
            unsigned p[RT_DEPTH][4], w[RT_DEPTH];
#pragma unroll
            for (int r = 0; r < RT_DEPTH; ++r) {
                const int k = min(kb + r, k1);
                const RS_G unsigned* frame = (const RS_G unsigned*) a.src[k];
                w[r] = kb + r <= k1 ? a.weight[k] : 0u;
                p[r][0] = p[r][1] = p[r][2] = p[r][3] = 0u;
                if (VEC && wide) {
                    const rs_v4 v = *(const RS_G rs_v4*) (frame + pix[0]);
                    p[r][0] = v.x; p[r][1] = v.y; p[r][2] = v.z; p[r][3] = v.w;
                } else {
#pragma unroll
                    for (int e = 0; e < 4; ++e)
                        if (e < count) p[r][e] = frame[pix[e]];
                }
            }
#pragma unroll
            for (int r = 0; r < RT_DEPTH; ++r) {
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const unsigned al = p[r][e] >> 24;
                    S[e][0] += (rs_u64) w[r] * al;
                    S[e][1] += (rs_u64) w[r] * (al * s_T[(p[r][e] >> 16) & 255u]);     // a T[c] <= 255 * 65535 < 2^24
                    S[e][2] += (rs_u64) w[r] * (al * s_T[(p[r][e] >> 8) & 255u]);
                    S[e][3] += (rs_u64) w[r] * (al * s_T[p[r][e] & 255u]);
                }
            }
        }
        const rs_u64 W = a.W[o];
        unsigned out[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            out[e] = 0u;
            if (S[e][0]) {
                const unsigned A = (unsigned) ((2 * S[e][0] + W) / (2 * W));
                out[e] = A << 24 | rs_encode(s_T, S[e][1], S[e][0]) << 16 | rs_encode(s_T, S[e][2], S[e][0]) << 8 | rs_encode(s_T, S[e][3], S[e][0]);
            }
        }
        RS_G unsigned* dst = (RS_G unsigned*) a.dst[o];
        if (VEC && wide) {
            rs_v4 v;
            v.x = out[0]; v.y = out[1]; v.z = out[2]; v.w = out[3];
            *(RS_G rs_v4*) (dst + pix[0]) = v;
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (e < count) dst[pix[e]] = out[e];
        }
    }
}

} // namespace

void launch_retime(const RetimeLaunch& a, long long px, bool linear, bool vec, hipStream_t s) {
    const int bpf = (int) ((px + RT_BLOCK - 1) / RT_BLOCK);               // <= 2^21
    const int items = a.count * bpf;                                      // <= 2^25
    const unsigned grid = (unsigned) (items < RT_MAX_BLOCKS ? items : RT_MAX_BLOCKS);
    if (vec)
        hipLaunchKernelGGL((retime_kernel<true>), dim3(grid), dim3(RT_THREADS), 0, s, a, items, bpf, (unsigned) px, linear ? 1 : 0);
    else
        hipLaunchKernelGGL((retime_kernel<false>), dim3(grid), dim3(RT_THREADS), 0, s, a, items, bpf, (unsigned) px, linear ? 1 : 0);
}

} // namespace nq
