// nq_compare.hip -- the quality of a conversion on gfx950: per-pixel squared error, error of the 8 x 8 block means and block SSIM of
// pairs of resident frames (include/nquant_abi.h, "quality measurement").
//
// A streaming reduction: every pixel of both frames is read once (8 bytes per pixel, 6 in the indexed form), nothing but the 16
// result slots of a frame is written.  All arithmetic is integer; there is no floating point in this file.
//   compare_kernel<true,  I>   the vector path: one 16-byte load of four pixels per lane, row and image (8 bytes of an index map);
//                              needs every pointer of the launch 16-byte aligned (index maps: 8-byte) and the width a multiple of 4.
//   compare_kernel<false, I>   one pixel per access: 4-byte aligned frames, 2-byte aligned index maps, any width.
//   I = true                   `out` is an index map; the palette comes by value and sits in LDS; an index >= K reads as word 0.
// launch_compare picks the path on the host; the kernels never test an address.  The frames of a launch come BY VALUE in the kernel
// arguments (COMPARE_FRAMES_PER_LAUNCH of them): no table in device memory exists, so the call allocates and uploads nothing.
//
// Work.  A frame is cut into strips of 8 rows x CMP_STRIP_WIDTH columns, in row-major order.  A wave takes a strip, a lane 4 columns x 8
// rows of it: a wave's read of one row is 1 KB, contiguous.  Lanes 2k and 2k + 1 hold the two halves of one 8 x 8 block; they exchange
// their 13 block sums with one __shfl_xor(.., 1) each.  Every sum of a block fits 32 bits (64 * 65535 < 2^23, 64 * 255^2 < 2^23).
// The pair then shares the divisions: the even lane forms the block means of a and r and the luminance quotient l, the odd lane those
// of g and b and the contrast-structure quotient cs, and one more exchange gives the even lane q.  No divisor is a run-time value of
// a division instruction sequence (hipcc lowers those through a floating-point reciprocal): the means go through a table of
// reciprocals of 2 N and a high multiply, the quotients, which have 16 bits, through a restoring division on 32-bit words.  blockIdx.y is the frame of the launch; blockIdx.x strides over its strips, four at a time
// (one per wave), and the grid is capped at CMP_GRID_CAP workgroups per frame.
//
// Accumulation.  Per strip in 32-bit registers (32 pixels of a lane: 32 * 255^2 < 2^21), per lane across strips in 64-bit registers,
// then over the wave by shuffles, over the four waves through LDS, and ONE 64-bit atomic per non-zero slot and workgroup: adds for the
// sums, atomicMax for slots 6 and 12, whose identity is the zero the caller's memset left.  Integer sums do not depend on the order
// of arrival: the result is deterministic.
#include "nq_kernels.h"

namespace nq {

namespace {

constexpr int CMP_THREADS = 256;
constexpr int CMP_WAVES = CMP_THREADS / 64;
constexpr int CMP_STRIP_WIDTH = 256;                  // columns of a wave's strip: 64 lanes x 4 pixels
constexpr int CMP_GRID_CAP = 512;                     // workgroups per frame: 2048 strips in flight, the rest by the strip loop
constexpr int CMP_ONE = 32768;

#define CMP_G __attribute__((address_space(1)))
typedef unsigned cmp_v4 __attribute__((ext_vector_type(4)));
typedef unsigned cmp_v2 __attribute__((ext_vector_type(2)));
typedef long long cmp_i64;
typedef unsigned long long cmp_u64;

__constant__ unsigned short CMP_LINEAR[256] = {
#include "../../include/nq_srgb_linear_16.inc"
};

struct ComparePalette { unsigned c[256]; };

// slots of the workgroup's partial result, in the order of the frame's slots from 2 on: sse a r g b, maxdiff, lf a r g b, ssim, deficit
constexpr int CMP_PARTS = 11;

// floor(32768 num / den) for 0 < den < 2^30 and |num| <= den (so the quotient has 16 bits): a restoring division of 15 steps on 32-bit
// words -- the remainder stays below den, twice it below 2^31 -- instead of a 64-bit division
__device__ inline int cmp_quotient(int num, unsigned den) {
    const unsigned an = (unsigned) (num < 0 ? -num : num);
    unsigned q = an >= den ? 1u : 0u, r = an - (q ? den : 0u);
#pragma unroll
    for (int k = 0; k < 15; ++k) {
        r <<= 1; q <<= 1;
        if (r >= den) { r -= den; q |= 1u; }
    }
    return num < 0 ? -(int) q - (r != 0u ? 1 : 0) : (int) q;
}

// floor(2^32 / (2 N)) + 1 for N = 1..64: x / (2 N) = mulhi(x, CMP_RECIP[N]) exactly for x < 2^24 (the error x (2 N - 2^32 mod 2 N) / 2^32
// stays below 1 / (2 N))
struct CmpRecip { unsigned v[65]; };
constexpr CmpRecip cmp_recip() {
    CmpRecip t = {};
    for (unsigned N = 1; N <= 64; ++N) t.v[N] = (unsigned) ((1ull << 32) / (2 * N)) + 1u;
    return t;
}
__constant__ CmpRecip CMP_RECIP = cmp_recip();

// the rounded mean floor((2 S + N) / (2 N)), rcp = CMP_RECIP[N]; 2 S + N <= 2 * 64 * 65535 + 64 < 2^24
__device__ inline unsigned cmp_mean(unsigned S, unsigned N, unsigned rcp) { return __umulhi(2u * S + N, rcp); }

__device__ inline cmp_i64 cmp_wave_sum(cmp_i64 v, int from) {
#pragma unroll
    for (int s = 32; s >= from; s >>= 1) v += __shfl_xor(v, s);
    return v;
}

template <bool VEC, bool IDX>
__global__ void __launch_bounds__(CMP_THREADS) compare_kernel(CompareLaunch a, ComparePalette pal, int K, int* __restrict__ d_bad) {
    __shared__ unsigned short s_T[256];
    __shared__ unsigned s_pal[IDX ? 256 : 1];
    __shared__ unsigned s_rcp[65];
    __shared__ cmp_i64 s_part[CMP_WAVES][CMP_PARTS];
    const int t = threadIdx.x, wave = t >> 6, lane = t & 63, odd = lane & 1;
    s_T[t] = a.linear ? CMP_LINEAR[t] : (unsigned short) (257 * t);
    if constexpr (IDX) s_pal[t] = t < K ? pal.c[t] : 0u;
    if (t <= 64) s_rcp[t] = CMP_RECIP.v[t];
    __syncthreads();
    const CompareFrame fr = a.frame[blockIdx.y];
    const int W = fr.width, H = fr.height;
    const int strips_x = (W + CMP_STRIP_WIDTH - 1) / CMP_STRIP_WIDTH, strips_y = (H + 7) >> 3;
    const int nstrips = strips_x * strips_y;          // <= 256 * 8192
    const CMP_G unsigned* src = (const CMP_G unsigned*) fr.src;
    const CMP_G unsigned* outw = (const CMP_G unsigned*) fr.out;
    const CMP_G unsigned short* outi = (const CMP_G unsigned short*) fr.out;

    cmp_u64 sse[4] = {0, 0, 0, 0}, lf[2] = {0, 0};
    cmp_i64 ssim = 0;
    unsigned maxsq = 0;                               // the largest squared channel difference
    int deficit = 0;
    bool bad = false;

    for (int s = (int) blockIdx.x * CMP_WAVES + wave; s < nstrips; s += (int) gridDim.x * CMP_WAVES) {
        const int sy = strips_x == 1 ? s : (int) __umulhi((unsigned) s, fr.strips_x_rcp), sx = s - sy * strips_x;   // s / strips_x
        const int x0 = sx * CMP_STRIP_WIDTH + lane * 4, y0 = sy * 8;
        const int ny = min(8, H - y0);
        unsigned e[4] = {0, 0, 0, 0};                 // squared error of the lane's 32 pixels per channel
        unsigned S[2][4] = {{0, 0, 0, 0}, {0, 0, 0, 0}};   // block sums of a (unscaled) and P_r, P_g, P_b: src, out
        unsigned Sx = 0, Sy = 0, Sxx = 0, Syy = 0, Sxy = 0;
        // (two halves of four rows: eight 16-byte loads in flight per lane, and registers for two workgroups per compute unit)
#pragma unroll 1
        for (int r0 = 0; r0 < 8; r0 += 4)
#pragma unroll
        for (int r4 = 0; r4 < 4; ++r4) {
            const int r = r0 + r4;
            unsigned p[2][4] = {{0, 0, 0, 0}, {0, 0, 0, 0}};
            if (r < ny) {
                const long long at = (long long) (y0 + r) * W + x0;
                if constexpr (VEC) {
                    if (x0 < W) {                     // W is a multiple of 4: all four pixels exist
                        const cmp_v4 v = *(const CMP_G cmp_v4*) (src + at);
                        p[0][0] = v.x; p[0][1] = v.y; p[0][2] = v.z; p[0][3] = v.w;
                        if constexpr (IDX) {
                            const cmp_v2 iv = *(const CMP_G cmp_v2*) (outi + at);
                            const unsigned i0 = iv.x & 0xFFFFu, i1 = iv.x >> 16, i2 = iv.y & 0xFFFFu, i3 = iv.y >> 16;
                            bad = bad || max(max(i0, i1), max(i2, i3)) >= (unsigned) K;
                            p[1][0] = s_pal[min(i0, 255u)] & (i0 < 256u ? ~0u : 0u);
                            p[1][1] = s_pal[min(i1, 255u)] & (i1 < 256u ? ~0u : 0u);
                            p[1][2] = s_pal[min(i2, 255u)] & (i2 < 256u ? ~0u : 0u);
                            p[1][3] = s_pal[min(i3, 255u)] & (i3 < 256u ? ~0u : 0u);
                        } else {
                            const cmp_v4 o = *(const CMP_G cmp_v4*) (outw + at);
                            p[1][0] = o.x; p[1][1] = o.y; p[1][2] = o.z; p[1][3] = o.w;
                        }
                    }
                } else {
#pragma unroll
                    for (int i = 0; i < 4; ++i)
                        if (x0 + i < W) {
                            p[0][i] = src[at + i];
                            if constexpr (IDX) {
                                const unsigned ix = outi[at + i];
                                bad = bad || ix >= (unsigned) K;
                                p[1][i] = s_pal[min(ix, 255u)] & (ix < 256u ? ~0u : 0u);
                            } else {
                                p[1][i] = outw[at + i];
                            }
                        }
                }
            }
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                unsigned ch[2][4], y[2];
#pragma unroll
                for (int m = 0; m < 2; ++m) {
                    const unsigned al = p[m][i] >> 24;
                    const unsigned w = al ? p[m][i] : 0u;              // the seen colour
                    ch[m][0] = al; ch[m][1] = (w >> 16) & 255u; ch[m][2] = (w >> 8) & 255u; ch[m][3] = w & 255u;
                    S[m][0] += al;
#pragma unroll
                    for (int c = 1; c < 4; ++c) S[m][c] += ((unsigned) s_T[ch[m][c]] * al + 127u) / 255u;
                    const unsigned lum = __builtin_amdgcn_udot4(w, 0x004D961Du, 128u, false) >> 8;   // (77 r + 150 g + 29 b + 128) >> 8
                    y[m] = (lum * al + 127u) / 255u;
                }
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    const int d = (int) ch[0][c] - (int) ch[1][c];
                    const unsigned dd = (unsigned) (d * d);
                    e[c] += dd;
                    maxsq = max(maxsq, dd);
                }
                Sx += y[0]; Sy += y[1]; Sxx += y[0] * y[0]; Syy += y[1] * y[1]; Sxy += y[0] * y[1];
            }
        }
#pragma unroll
        for (int c = 0; c < 4; ++c) sse[c] += e[c];
        // the other half of the block
#pragma unroll
        for (int m = 0; m < 2; ++m)
#pragma unroll
            for (int c = 0; c < 4; ++c) S[m][c] += (unsigned) __shfl_xor((int) S[m][c], 1);
        Sx += (unsigned) __shfl_xor((int) Sx, 1); Sy += (unsigned) __shfl_xor((int) Sy, 1);
        Sxx += (unsigned) __shfl_xor((int) Sxx, 1); Syy += (unsigned) __shfl_xor((int) Syy, 1);
        Sxy += (unsigned) __shfl_xor((int) Sxy, 1);
        const int bx = sx * CMP_STRIP_WIDTH + (lane >> 1) * 8;        // the block's first column
        const bool valid = bx < W;
        const unsigned N = valid ? (unsigned) (min(8, W - bx) * ny) : 1u;
        // block means: a and r on the even lane, g and b on the odd one (P_a = 257 a, so its sum is 257 times the sum of a)
        const unsigned u0 = odd ? S[0][2] : 257u * S[0][0], u1 = odd ? S[0][3] : S[0][1];
        const unsigned v0 = odd ? S[1][2] : 257u * S[1][0], v1 = odd ? S[1][3] : S[1][1];
        const unsigned rcp = s_rcp[N];
        const unsigned d0 = cmp_mean(u0, N, rcp) - cmp_mean(v0, N, rcp), d1 = cmp_mean(u1, N, rcp) - cmp_mean(v1, N, rcp);   // (mod 2^32: the squares are right)
        lf[0] += d0 * d0;                             // |difference| <= 65535: the square fits 32 bits, whatever the sign was
        lf[1] += d1 * d1;
        // SSIM: l on the even lane, cs on the odd one.  Every term is below 2^30.
        const unsigned C1 = (65025u * N * N + 5000u) / 10000u, C2 = (585225u * N * N + 5000u) / 10000u;   // N <= 64: below 2^32
        const int num = odd ? 2 * (int) (N * Sxy - Sx * Sy) + (int) C2 : (int) (2u * Sx * Sy + C1);
        const unsigned den = odd ? N * (Sxx + Syy) - Sx * Sx - Sy * Sy + C2 : Sx * Sx + Sy * Sy + C1;
        const int mine = cmp_quotient(num, den);
        const int other = __shfl_xor(mine, 1);
        if (valid && !odd) {
            const int q = (mine * other) >> 15;       // floor(l cs / 32768): an arithmetic shift rounds toward minus infinity
            ssim += q;
            deficit = max(deficit, CMP_ONE - q);
        }
    }

    if constexpr (IDX) {
        if (__any(bad) && lane == 0 && d_bad) atomicMin(d_bad, a.first + (int) blockIdx.y);
    }
    // over the wave: the sums of every lane, lf per parity (lanes 0 and 1 end up with a, r and g, b)
    cmp_i64 part[CMP_PARTS];
#pragma unroll
    for (int c = 0; c < 4; ++c) part[c] = cmp_wave_sum((cmp_i64) sse[c], 1);
    const cmp_i64 l0 = cmp_wave_sum((cmp_i64) lf[0], 2), l1 = cmp_wave_sum((cmp_i64) lf[1], 2);
    const cmp_i64 m0 = __shfl_xor(l0, 1), m1 = __shfl_xor(l1, 1);     // the other parity's pair
    part[5] = odd ? m0 : l0; part[6] = odd ? m1 : l1; part[7] = odd ? l0 : m0; part[8] = odd ? l1 : m1;
    part[9] = cmp_wave_sum(ssim, 1);
    int mx = (int) maxsq, df = deficit;
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) { mx = max(mx, __shfl_xor(mx, s)); df = max(df, __shfl_xor(df, s)); }
    part[4] = mx; part[10] = df;
    if (lane == 0) {
#pragma unroll
        for (int i = 0; i < CMP_PARTS; ++i) s_part[wave][i] = part[i];
    }
    __syncthreads();
    cmp_i64* res = a.result + 16ll * blockIdx.y;
    if (t < CMP_PARTS) {
        const bool is_max = t == 4 || t == 10;
        cmp_i64 v = s_part[0][t];
#pragma unroll
        for (int w = 1; w < CMP_WAVES; ++w) v = is_max ? max(v, s_part[w][t]) : v + s_part[w][t];
        if (t == 4) {                                 // the largest |difference| from its square (<= 255^2)
            int root = 0;
#pragma unroll
            for (int bit = 128; bit > 0; bit >>= 1) if ((cmp_i64) (root + bit) * (root + bit) <= v) root += bit;
            v = root;
        }
        if (v != 0) {
            if (is_max) atomicMax(res + 2 + t, v);
            else atomicAdd((cmp_u64*) (res + 2 + t), (cmp_u64) v);
        }
    }
    if (blockIdx.x == 0 && t == 0) {
        res[0] = (cmp_i64) W * H;
        res[1] = (cmp_i64) ((W + 7) >> 3) * strips_y;
    }
}

} // namespace

int compare_grid(int width, int height) {
    const long long strips = (long long) ((width + CMP_STRIP_WIDTH - 1) / CMP_STRIP_WIDTH) * ((height + 7) / 8);
    const long long groups = (strips + CMP_WAVES - 1) / CMP_WAVES;
    return (int) (groups < CMP_GRID_CAP ? groups : CMP_GRID_CAP);
}

void launch_compare(const CompareLaunch& launch, int count, bool vec, bool indexed, const unsigned* palette, int K, int* d_bad, hipStream_t s) {
    CompareLaunch a = launch;
    int gx = 1;
    for (int i = 0; i < count; ++i) {
        const int g = compare_grid(a.frame[i].width, a.frame[i].height);
        gx = gx > g ? gx : g;
        // floor(2^32 / strips_x) + 1: strip / strips_x = mulhi(strip, this) exactly for strip * strips_x < 2^32 (unused at strips_x = 1)
        const unsigned strips_x = (unsigned) ((a.frame[i].width + CMP_STRIP_WIDTH - 1) / CMP_STRIP_WIDTH);
        a.frame[i].strips_x_rcp = strips_x > 1 ? (unsigned) ((1ull << 32) / strips_x) + 1u : 0u;
    }
    const dim3 grid((unsigned) gx, (unsigned) count), block(CMP_THREADS);
    ComparePalette pal;
    for (int i = 0; i < 256; ++i) pal.c[i] = indexed && i < K ? palette[i] : 0u;
    if (indexed) {
        if (vec) hipLaunchKernelGGL((compare_kernel<true, true>), grid, block, 0, s, a, pal, K, d_bad);
        else hipLaunchKernelGGL((compare_kernel<false, true>), grid, block, 0, s, a, pal, K, d_bad);
    } else {
        if (vec) hipLaunchKernelGGL((compare_kernel<true, false>), grid, block, 0, s, a, pal, K, d_bad);
        else hipLaunchKernelGGL((compare_kernel<false, false>), grid, block, 0, s, a, pal, K, d_bad);
    }
}

} // namespace nq
