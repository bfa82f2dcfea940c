// nq_yuv16.hip -- 10-bit YUV 4:2:0 frames (P010, I010 and their chroma-swapped forms; SDR, PQ, HLG) in front of the frame path on gfx950
// (include/nquant_abi.h "10-bit YUV input").
//
// A frame is three pointers to 16-bit words y, u, v with a luma row stride, a chroma row stride and a chroma element step, all in
// samples; the sample is the high or the low ten bits of its word.  The conversion is the header's: the 2^14 fixed-point matrix to
// R'G'B' on a 12-bit scale, then either the scaling to 8 bits (SDR) or E[] -> the 2^12 gamut matrix -> the logarithmic index -> O[]
// (PQ, HLG), exact in signed 32-bit integers.  The frames of a launch travel in the kernel arguments (Yuv16Launch).
//   yuv16_argb_kernel<HDR, PATH>      the 1:1 conversion to ARGB words.  A frame's items are cut into strips of Y16_STRIP; a workgroup
//                                     takes the strips blockIdx.x, + gridDim.x, ... of the launch (a strip lies in one frame, so the
//                                     frame's pointers are uniform), its threads the items t, t + Y16_THREADS, ... of the strip.
//       wide paths                    an item is a block of 4 columns x 2 rows: two 8-byte luma loads, the chroma of its two sample
//                                     pairs (one 8-byte load when interleaved, two 4-byte loads when planar), two 16-byte stores; an
//                                     odd last row is a block of one row
//       one-pixel path                an item is a pixel: three 2-byte loads, one store; any pointers and strides
//   resample_yuv16_kernel<HDR, PATH>  resample_yuv_kernel of nq_yuv.hip with 16-bit loads and this conversion in front of the table
//                                     lookup: work items, chunks, YR16_ROWS rows in flight, LDS column sums and rs_encode as there.
// HDR kernels stage the transfer's E (8 KiB) and O (1.25 KiB) in LDS once per workgroup, before the strip / item loop; the SDR
// kernels of the 1:1 conversion use no LDS.  The launch functions take the path from the host (nq_abi.cpp: yuv16_launches), which
// derives it from pointers and strides; the kernels never test an address.  Every loop is bounded by a side length, the chunk count
// of a span or the strip / item count; workgroups do not wait for each other.
#include "nq_kernels.h"

namespace nq {

namespace {

constexpr int Y16_THREADS = 256;
constexpr int Y16_STRIP = 4 * Y16_THREADS;   // items of a strip: four per thread
constexpr long long Y16_MAX_BLOCKS = 2048;   // grid cap of the 1:1 kernel: 8 workgroups per compute unit
constexpr int YR16_THREADS = 256;
constexpr int YR16_CHUNK = 4 * YR16_THREADS; // source columns whose sums a workgroup stages in LDS at once (3 x 8 bytes each: 24 KiB)
constexpr int YR16_ROWS = 4;                 // source rows a thread has in flight: their loads are issued together
constexpr long long YR16_MAX_BLOCKS = 8192;  // grid cap of the fused kernel: a workgroup walks the items blockIdx.x + k * gridDim.x

#include "nq_resample.inc"                    // RS_G, rs_v4, rs_u64, RS_LINEAR, rs_overlap, rs_encode

#include "nq_yuv.inc"                         // yuv_u16, yuv_chroma

typedef unsigned y16_v2 __attribute__((ext_vector_type(2)));

#define NQ_HDR_LUT(type, name, entries) __device__ const type name[entries] __attribute__((aligned(16)))
#include "../../include/nq_hdr_luts.inc"
#undef NQ_HDR_LUT

constexpr int Y16_E = 4096, Y16_O = 1280;

// the transfer's tables into LDS: 512 + 80 16-byte pieces, every thread of the workgroup takes part (the caller synchronises)
__device__ inline void y16_stage(int transfer, unsigned short* s_E, unsigned char* s_O, int t, int threads) {
    const rs_v4* gE = (const rs_v4*) (transfer == YUV16_HLG ? NQ_HDR_E_HLG : NQ_HDR_E_PQ);
    const rs_v4* gO = (const rs_v4*) (transfer == YUV16_HLG ? NQ_HDR_O_HLG : NQ_HDR_O_PQ);
    for (int i = t; i < Y16_E * 2 / 16; i += threads) ((rs_v4*) s_E)[i] = gE[i];
    for (int i = t; i < Y16_O / 16; i += threads) ((rs_v4*) s_O)[i] = gO[i];
}

__device__ inline unsigned y16_sample(unsigned word, int shift) { return (word >> shift) & 1023u; }

// what a chroma sample adds to the three channels of the (up to four) pixels that share it
__device__ inline yuv_chroma y16_terms(const YuvCoef& k, unsigned U, unsigned V) {
    const int u = (int) U - 512, v = (int) V - 512;
    yuv_chroma c;
    c.r = k.crv * v;
    c.g = -(k.cgu * u) - k.cgv * v;
    c.b = k.cbu * u;
    return c;
}

__device__ inline int y16_clamp(int v, int hi) { return min(max(v, 0), hi); }

// the index of O for linear light l (0..65535): l itself below 256, then 128 buckets per power of two
__device__ inline unsigned y16_index(unsigned l) {
    const unsigned e = 31u - (unsigned) __clz((int) (l | 256u));       // 8..15 where it is used
    return l < 256u ? l : 128u * (e - 6u) + ((l >> (e - 7u)) & 127u);
}

// 0x00RRGGBB of a luma sample and its chroma terms.  Every intermediate of the matrix is below 1.6e8 in magnitude, every term of the
// gamut rows below 4.5e8; >> is the arithmetic shift.
template <bool HDR>
__device__ inline unsigned y16_rgb(const YuvCoef& k, unsigned Y, const yuv_chroma& c, const unsigned short* E, const unsigned char* O) {
    const int l = k.cy * ((int) Y - k.yo) + 8192;
    const int r = y16_clamp((l + c.r) >> 14, 4095), g = y16_clamp((l + c.g) >> 14, 4095), b = y16_clamp((l + c.b) >> 14, 4095);
    if constexpr (!HDR) {
        return ((unsigned) (r * 255 + 2047) / 4095u) << 16 | ((unsigned) (g * 255 + 2047) / 4095u) << 8 | ((unsigned) (b * 255 + 2047) / 4095u);
    } else {
        const int er = E[r], eg = E[g], eb = E[b];
        const unsigned lr = (unsigned) y16_clamp((6801 * er - 2407 * eg - 298 * eb + 2048) >> 12, 65535);
        const unsigned lg = (unsigned) y16_clamp((-510 * er + 4640 * eg - 34 * eb + 2048) >> 12, 65535);
        const unsigned lb = (unsigned) y16_clamp((-75 * er - 412 * eg + 4583 * eb + 2048) >> 12, 65535);
        return (unsigned) O[y16_index(lr)] << 16 | (unsigned) O[y16_index(lg)] << 8 | (unsigned) O[y16_index(lb)];
    }
}

// the raw words of the two sample pairs under four adjacent columns (the first, `col`, a multiple of 4) of a chroma row that begins
// `crow_off` samples into the plane.  Interleaved: `lo` is the lower of the two chroma pointers, one 8-byte load; planar: two 4-byte
// loads.
template <int PATH>
__device__ inline void y16_load_pairs(const RS_G yuv_u16* lo, const RS_G yuv_u16* hi, size_t crow_off, int col, unsigned raw[2]) {
    if constexpr (PATH == YUV_WIDE_INTERLEAVED) {
        const y16_v2 w = *(const RS_G y16_v2*) (lo + crow_off + col);
        raw[0] = w.x; raw[1] = w.y;
    } else {
        raw[0] = *(const RS_G unsigned*) (lo + crow_off + (col >> 1));
        raw[1] = *(const RS_G unsigned*) (hi + crow_off + (col >> 1));
    }
}
// interleaved: raw[p] holds pair p, the lower pointer's sample in the low half (swap: that one is v's); planar: raw[0] holds u's two
// samples, raw[1] v's
template <int PATH>
__device__ inline void y16_pairs(const YuvCoef& k, const unsigned raw[2], int shift, int swap, yuv_chroma out[2]) {
    if constexpr (PATH == YUV_WIDE_INTERLEAVED) {
        const unsigned a0 = y16_sample(raw[0], shift), b0 = y16_sample(raw[0] >> 16, shift);
        const unsigned a1 = y16_sample(raw[1], shift), b1 = y16_sample(raw[1] >> 16, shift);
        out[0] = swap ? y16_terms(k, b0, a0) : y16_terms(k, a0, b0);
        out[1] = swap ? y16_terms(k, b1, a1) : y16_terms(k, a1, b1);
    } else {
        out[0] = y16_terms(k, y16_sample(raw[0], shift), y16_sample(raw[1], shift));
        out[1] = y16_terms(k, y16_sample(raw[0] >> 16, shift), y16_sample(raw[1] >> 16, shift));
    }
}

// the four pixels of two luma words (columns 0, 1 in w.x, 2, 3 in w.y) under the chroma terms of their two pairs
template <bool HDR>
__device__ inline void y16_four(const YuvCoef& k, y16_v2 w, int shift, const yuv_chroma c[2], const unsigned short* E, const unsigned char* O,
                                unsigned p[4]) {
    p[0] = y16_rgb<HDR>(k, y16_sample(w.x, shift), c[0], E, O); p[1] = y16_rgb<HDR>(k, y16_sample(w.x >> 16, shift), c[0], E, O);
    p[2] = y16_rgb<HDR>(k, y16_sample(w.y, shift), c[1], E, O); p[3] = y16_rgb<HDR>(k, y16_sample(w.y >> 16, shift), c[1], E, O);
}

// strips = a.count * spf, spf = strips per frame.  Wide paths: a frame has ceil(height / 2) * (width / 4) items; one-pixel path:
// height * width.  The column (block) runs fastest.
template <bool HDR, int PATH>
__global__ void __launch_bounds__(Y16_THREADS) yuv16_argb_kernel(Yuv16Launch a, int strips, int spf, int width, int height) {
    __shared__ __attribute__((aligned(16))) unsigned short s_E[HDR ? Y16_E : 8];
    __shared__ __attribute__((aligned(16))) unsigned char s_O[HDR ? Y16_O : 16];
    const int t = threadIdx.x;
    if constexpr (HDR) {
        y16_stage(a.transfer, s_E, s_O, t, Y16_THREADS);
        __syncthreads();
    }
    const YuvCoef k = a.k;
    const int shift = a.shift;
    const int bw = width >> 2, bh = (height + 1) >> 1;
    const unsigned items = PATH == YUV_BYTE ? (unsigned) width * (unsigned) height : (unsigned) bw * (unsigned) bh;    // of a frame: < 2^31
    for (int strip = blockIdx.x; strip < strips; strip += gridDim.x) {
        const int f = strip / spf;
        const unsigned first = (unsigned) (strip - f * spf) * (unsigned) Y16_STRIP;
        const Yuv16Frame fr = a.frame[f];
        const RS_G yuv_u16* yp = (const RS_G yuv_u16*) fr.y;
        const RS_G yuv_u16* up = (const RS_G yuv_u16*) fr.u;
        const RS_G yuv_u16* vp = (const RS_G yuv_u16*) fr.v;
        RS_G unsigned* dst = (RS_G unsigned*) fr.dst;
#pragma unroll
        for (int j = 0; j < Y16_STRIP / Y16_THREADS; ++j) {
            const unsigned item = first + (unsigned) (t + j * Y16_THREADS);
            if (item >= items) continue;
            if constexpr (PATH == YUV_BYTE) {
                const int x = (int) (item % (unsigned) width), y = (int) (item / (unsigned) width);
                const size_t coff = (size_t) (y >> 1) * (size_t) a.c_stride + (size_t) (x >> 1) * (size_t) a.c_step;
                const unsigned Y = y16_sample(yp[(size_t) y * (size_t) a.y_stride + x], shift);
                const unsigned U = y16_sample(up[coff], shift), V = y16_sample(vp[coff], shift);
                dst[(size_t) y * width + x] = 0xFF000000u | y16_rgb<HDR>(k, Y, y16_terms(k, U, V), s_E, s_O);
            } else {
                const int col = 4 * (int) (item % (unsigned) bw), ry = (int) (item / (unsigned) bw);
                const bool two = 2 * ry + 1 < height;                        // (an odd last row stands alone)
                const RS_G yuv_u16* row0 = yp + (size_t) (2 * ry) * (size_t) a.y_stride + col;
                const y16_v2 l0 = *(const RS_G y16_v2*) row0;
                y16_v2 l1 = {0u, 0u};
                if (two) l1 = *(const RS_G y16_v2*) (row0 + a.y_stride);
                unsigned raw[2];
                y16_load_pairs<PATH>(up, PATH == YUV_WIDE_PLANAR ? vp : nullptr, (size_t) ry * (size_t) a.c_stride, col, raw);
                yuv_chroma c[2];
                y16_pairs<PATH>(k, raw, shift, a.swap, c);
                RS_G unsigned* out = dst + (size_t) (2 * ry) * width + col;
                unsigned p[4];
                y16_four<HDR>(k, l0, shift, c, s_E, s_O, p);
                rs_v4 w;
                w.x = 0xFF000000u | p[0]; w.y = 0xFF000000u | p[1]; w.z = 0xFF000000u | p[2]; w.w = 0xFF000000u | p[3];
                *(RS_G rs_v4*) out = w;
                if (two) {
                    y16_four<HDR>(k, l1, shift, c, s_E, s_O, p);
                    w.x = 0xFF000000u | p[0]; w.y = 0xFF000000u | p[1]; w.z = 0xFF000000u | p[2]; w.w = 0xFF000000u | p[3];
                    *(RS_G rs_v4*) (out + width) = w;
                }
            }
        }
    }
}

// items = a.count * dh * colblocks; item -> (frame, y, column block) with the column block fastest (as resample_yuv_kernel).
template <bool HDR, int PATH>
__global__ void __launch_bounds__(YR16_THREADS) resample_yuv16_kernel(Yuv16Launch a, long long items, int colblocks, int oc, int crop_x,
                                                                      int crop_y, unsigned cw, unsigned ch, unsigned dw, unsigned dh,
                                                                      int linear) {
    constexpr bool VEC = PATH != YUV_BYTE;
    __shared__ rs_u64 s_sum[3][YR16_CHUNK];          // r, g, b column sums of the current chunk (of wy T[c]: alpha is 255 everywhere)
    __shared__ unsigned short s_T[256];
    __shared__ __attribute__((aligned(16))) unsigned short s_E[HDR ? Y16_E : 8];
    __shared__ __attribute__((aligned(16))) unsigned char s_O[HDR ? Y16_O : 16];
    const int t = threadIdx.x;
    s_T[t] = linear ? RS_LINEAR[t] : (unsigned short) (257 * t);
    if constexpr (HDR) y16_stage(a.transfer, s_E, s_O, t, YR16_THREADS);
    __syncthreads();
    const YuvCoef k = a.k;
    const int shift = a.shift, swap = a.swap, y_stride = a.y_stride, c_stride = a.c_stride, c_step = a.c_step;
    const rs_u64 W = (rs_u64) cw * ch;
    for (long long item = blockIdx.x; item < items; item += gridDim.x) {
        const int cb = (int) (item % colblocks);
        const long long fy = item / colblocks;
        const unsigned y = (unsigned) (fy % dh);
        const int f = (int) (fy / dh);
        const Yuv16Frame fr = a.frame[f];
        const RS_G yuv_u16* luma = (const RS_G yuv_u16*) fr.y;
        const RS_G yuv_u16* fu = (const RS_G yuv_u16*) fr.u;
        const RS_G yuv_u16* fv = PATH == YUV_WIDE_INTERLEAVED ? nullptr : (const RS_G yuv_u16*) fr.v;
        // outputs [x0, x1) of row y; their source columns J0 .. J1 and rows i0 .. i1 (of the crop)
        const unsigned x0 = (unsigned) cb * (unsigned) oc, x1 = min(x0 + (unsigned) oc, dw);
        const unsigned J0 = x0 * cw / dw, J1 = (x1 * cw - 1u) / dw;
        const unsigned i0 = y * ch / dh, i1 = ((y + 1u) * ch - 1u) / dh;
        const unsigned x = x0 + (unsigned) t;
        const bool owner = x < x1;
        // this thread's output: its footprint in columns of the FRAME
        const int fa = owner ? crop_x + (int) (x * cw / dw) : 0, fb = owner ? crop_x + (int) (((x + 1u) * cw - 1u) / dw) : -1;
        rs_u64 S[3] = {0, 0, 0};
        const int cend = crop_x + (int) J1;           // last column of the frame the item reads
        int c = crop_x + (int) J0;
        if (VEC) c &= ~3;
        for (; c <= cend; c += YR16_CHUNK) {
            // the thread's four columns of the chunk: kk in the chunk, c + kk in the frame
            rs_u64 acc[4][3];
#pragma unroll
            for (int e = 0; e < 4; ++e) acc[e][0] = acc[e][1] = acc[e][2] = 0;
            for (unsigned ib = i0; ib <= i1; ib += YR16_ROWS) {
                // YR16_ROWS rows are loaded before the first is used; behind the footprint's last row that row is read again, with
                // weight 0.  A column that is not loaded keeps 0x000000, and T[0] = 0 in both tables.
                unsigned p[YR16_ROWS][4];
                size_t yoff[YR16_ROWS], coff[YR16_ROWS];
#pragma unroll
                for (int r = 0; r < YR16_ROWS; ++r) {
                    const int row = crop_y + (int) min(ib + r, i1);
                    yoff[r] = (size_t) row * (size_t) y_stride;
                    coff[r] = (size_t) (row >> 1) * (size_t) c_stride;
                    p[r][0] = p[r][1] = p[r][2] = p[r][3] = 0u;
                }
                if constexpr (VEC) {                    // (width is a multiple of 4 and c + 4 t <= cend < width: the loads stay in the row)
                    if (c + 4 * t <= cend) {
                        y16_v2 l[YR16_ROWS];
                        unsigned raw[YR16_ROWS][2];
#pragma unroll
                        for (int r = 0; r < YR16_ROWS; ++r) {
                            l[r] = *(const RS_G y16_v2*) (luma + yoff[r] + c + 4 * t);
                            y16_load_pairs<PATH>(fu, fv, coff[r], c + 4 * t, raw[r]);
                        }
#pragma unroll
                        for (int r = 0; r < YR16_ROWS; ++r) {
                            yuv_chroma q[2];
                            y16_pairs<PATH>(k, raw[r], shift, swap, q);
                            y16_four<HDR>(k, l[r], shift, q, s_E, s_O, p[r]);
                        }
                    }
                } else {
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const int col = c + t + e * YR16_THREADS;
                        if (col <= cend) {
                            unsigned Y[YR16_ROWS], U[YR16_ROWS], V[YR16_ROWS];
                            const size_t cx = (size_t) (col >> 1) * (size_t) c_step;
#pragma unroll
                            for (int r = 0; r < YR16_ROWS; ++r) {
                                Y[r] = luma[yoff[r] + col];
                                U[r] = fu[coff[r] + cx];
                                V[r] = fv[coff[r] + cx];
                            }
#pragma unroll
                            for (int r = 0; r < YR16_ROWS; ++r)
                                p[r][e] = y16_rgb<HDR>(k, y16_sample(Y[r], shift), y16_terms(k, y16_sample(U[r], shift), y16_sample(V[r], shift)),
                                                       s_E, s_O);
                        }
                    }
                }
#pragma unroll
                for (int r = 0; r < YR16_ROWS; ++r) {
                    const unsigned wy = ib + r <= i1 ? rs_overlap(ib + r, dh, y * ch, ch) : 0u;      // <= 65535
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        acc[e][0] += (rs_u64) wy * s_T[(p[r][e] >> 16) & 255u];
                        acc[e][1] += (rs_u64) wy * s_T[(p[r][e] >> 8) & 255u];
                        acc[e][2] += (rs_u64) wy * s_T[p[r][e] & 255u];
                    }
                }
            }
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int kk = VEC ? 4 * t + e : t + e * YR16_THREADS;
#pragma unroll
                for (int q = 0; q < 3; ++q) s_sum[q][kk] = acc[e][q];
            }
            __syncthreads();
            const int lo = max(fa, c), hi = min(fb, c + YR16_CHUNK - 1);
            for (int ja = lo; ja <= hi; ++ja) {
                const rs_u64 wx = rs_overlap((unsigned) (ja - crop_x), dw, x * cw, cw);
#pragma unroll
                for (int q = 0; q < 3; ++q) S[q] += wx * s_sum[q][ja - c];
            }
            __syncthreads();                            // the next chunk (or item) overwrites the sums
        }
        if (owner)
            ((RS_G unsigned*) fr.dst)[(size_t) y * dw + x] =
                0xFF000000u | rs_encode(s_T, S[0], W) << 16 | rs_encode(s_T, S[1], W) << 8 | rs_encode(s_T, S[2], W);
    }
}

} // namespace

#define NQ_YUV16_PATHS(LAUNCH, HDR)                                      \
    do {                                                                 \
        if (a.path == YUV_WIDE_INTERLEAVED) LAUNCH(HDR, YUV_WIDE_INTERLEAVED); \
        else if (a.path == YUV_WIDE_PLANAR) LAUNCH(HDR, YUV_WIDE_PLANAR); \
        else LAUNCH(HDR, YUV_BYTE);                                      \
    } while (0)

void launch_yuv16_argb(const Yuv16Launch& a, int width, int height, hipStream_t s) {
    const long long items = a.path == YUV_BYTE ? (long long) width * height : (long long) ((height + 1) / 2) * (width / 4);
    const int spf = (int) ((items + Y16_STRIP - 1) / Y16_STRIP);          // <= 2^21
    const int strips = a.count * spf;                                     // <= 2^25
    const unsigned grid = (unsigned) (strips < Y16_MAX_BLOCKS ? strips : Y16_MAX_BLOCKS);
#define NQ_YUV16_LAUNCH(H, P) hipLaunchKernelGGL((yuv16_argb_kernel<H, P>), dim3(grid), dim3(Y16_THREADS), 0, s, a, strips, spf, width, height)
    if (a.transfer == YUV16_SDR) NQ_YUV16_PATHS(NQ_YUV16_LAUNCH, false);
    else NQ_YUV16_PATHS(NQ_YUV16_LAUNCH, true);
#undef NQ_YUV16_LAUNCH
}

void launch_resample_yuv16(const Yuv16Launch& a, int crop_x, int crop_y, int crop_w, int crop_h, int dst_width, int dst_height, bool linear,
                           hipStream_t s) {
    // output columns per item: as launch_resample
    long long oc = (long long) (YR16_CHUNK - 4) * dst_width / crop_w;
    oc = oc < 1 ? 1 : (oc > YR16_THREADS ? YR16_THREADS : oc);
    const int colblocks = (int) ((dst_width + oc - 1) / oc);
    const long long items = (long long) a.count * dst_height * colblocks;  // <= count * crop_w * crop_h < 2^31
    const unsigned grid = (unsigned) (items < YR16_MAX_BLOCKS ? items : YR16_MAX_BLOCKS);
#define NQ_YUV16_LAUNCH(H, P) hipLaunchKernelGGL((resample_yuv16_kernel<H, P>), dim3(grid), dim3(YR16_THREADS), 0, s, a, items, colblocks, (int) oc, \
                                                 crop_x, crop_y, (unsigned) crop_w, (unsigned) crop_h, (unsigned) dst_width, (unsigned) dst_height,   \
                                                 linear ? 1 : 0)
    if (a.transfer == YUV16_SDR) NQ_YUV16_PATHS(NQ_YUV16_LAUNCH, false);
    else NQ_YUV16_PATHS(NQ_YUV16_LAUNCH, true);
#undef NQ_YUV16_LAUNCH
}

#undef NQ_YUV16_PATHS

} // namespace nq
