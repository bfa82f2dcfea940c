// nq_yuv.hip -- YUV 4:2:0 frames (NV12 / NV21 / I420 / YV12, 8 bit) in front of the frame path on gfx950 (include/nquant_abi.h, "YUV
// input").
//
// A frame is three byte pointers y, u, v with a luma row stride, a chroma row stride and a chroma element step (1: planar, 2: the
// two chroma planes interleaved, or any two planes of step 2).  The chroma sample of pixel (x, y) is (x >> 1, y >> 1) (replication);
// the conversion is the fixed-point matrix of the header, exact in signed 32-bit integers.
//   yuv_argb_kernel<PATH>      the 1:1 conversion to ARGB words.  ONE launch covers the sequence; a workgroup takes the items
//                              blockIdx.x * YUV_THREADS + threadIdx.x, + gridDim.x * YUV_THREADS, ...
//       wide paths             an item is a block of 4 columns x 2 rows: two 4-byte luma loads, the chroma of its two sample pairs
//                              (one 4-byte load when interleaved, two 2-byte loads when planar), two 16-byte stores; an odd last row
//                              is a block of one row
//       byte path              an item is a pixel: three byte loads, one store; any pointers and strides
//   resample_yuv_kernel<PATH>  the reducer of nq_resample.hip with the source load replaced by luma + chroma loads and the conversion
//                              in front of the table lookup: work items, chunks, RS_ROWS rows in flight, LDS column sums and
//                              rs_encode as there.  Every converted pixel has alpha 255, so S_a = 255 W is known, the alpha sums
//                              are not formed, and the common factor 255 is left out of the colour sums:
//                              floor((2 * 255 S' + 255 W) / (2 * 255 W)) = floor((2 S' + W) / (2 W)) with S' = sum of wx wy T[c].
//       wide paths             a thread's four columns are adjacent: one 4-byte luma load and one 4-byte (interleaved) or two 2-byte
//                              (planar) chroma loads per row
//       byte path              a thread's columns lie YR_THREADS apart, three byte loads per pixel
// The launch functions take the path from the host (nq_abi.cpp: yuv_path), which derives it from pointers and strides; the kernels
// never test an address.  Every loop is bounded by a side length, the chunk count of a span or the item count; workgroups do not
// wait for each other.
#include "nq_kernels.h"

namespace nq {

namespace {

constexpr int YUV_THREADS = 256;
constexpr long long YUV_MAX_BLOCKS = 2048;   // grid cap of the 1:1 kernel: 8 workgroups per compute unit
constexpr int YR_THREADS = 256;
constexpr int YR_CHUNK = 4 * YR_THREADS;     // source columns whose sums a workgroup stages in LDS at once (3 x 8 bytes each: 24 KiB)
constexpr int YR_ROWS = 4;                   // source rows a thread has in flight: their loads are issued together
constexpr long long YR_MAX_BLOCKS = 8192;    // grid cap of the fused kernel: a workgroup walks the items blockIdx.x + k * gridDim.x

#include "nq_resample.inc"                    // RS_G, rs_v4, rs_u64, RS_LINEAR, rs_overlap, rs_encode

#include "nq_yuv.inc"                         // yuv_u8, yuv_chroma, yuv_terms, yuv_rgb, yuv_load_pairs, yuv_pairs

// yp / up / vp / dst: n frame pointers each (interleaved wide path: up holds the lower chroma pointer of every frame, vp is not read).
// Wide paths: items = n * ceil(height / 2) * (width / 4); byte path: items = n * height * width.  The column (block) runs fastest.
template <int PATH>
__global__ void __launch_bounds__(YUV_THREADS) yuv_argb_kernel(const yuv_u8* const* __restrict__ yp, const yuv_u8* const* __restrict__ up,
                                                               const yuv_u8* const* __restrict__ vp, unsigned* const* __restrict__ dst,
                                                               long long items, int width, int height, int y_stride, int c_stride,
                                                               int c_step, int swap, YuvCoef k) {
    const long long step = (long long) gridDim.x * YUV_THREADS;
    if constexpr (PATH == YUV_BYTE) {
        for (long long item = (long long) blockIdx.x * YUV_THREADS + threadIdx.x; item < items; item += step) {
            const int x = (int) (item % width);
            const long long fy = item / width;
            const int y = (int) (fy % height);
            const long long f = fy / height;
            const size_t coff = (size_t) (y >> 1) * (size_t) c_stride + (size_t) (x >> 1) * (size_t) c_step;
            const unsigned Y = ((const RS_G yuv_u8*) yp[f])[(size_t) y * (size_t) y_stride + x];
            const unsigned U = ((const RS_G yuv_u8*) up[f])[coff];
            const unsigned V = ((const RS_G yuv_u8*) vp[f])[coff];
            ((RS_G unsigned*) dst[f])[(size_t) y * width + x] = 0xFF000000u | yuv_rgb(k, Y, yuv_terms(k, U, V));
        }
    } else {
        const int bw = width >> 2, bh = (height + 1) >> 1;
        for (long long item = (long long) blockIdx.x * YUV_THREADS + threadIdx.x; item < items; item += step) {
            const int col = 4 * (int) (item % bw);
            const long long fr = item / bw;
            const int ry = (int) (fr % bh);
            const long long f = fr / bh;
            const bool two = 2 * ry + 1 < height;                        // (an odd last row stands alone)
            const RS_G yuv_u8* row0 = (const RS_G yuv_u8*) yp[f] + (size_t) (2 * ry) * (size_t) y_stride + col;
            const unsigned l0 = *(const RS_G unsigned*) row0;
            const unsigned l1 = two ? *(const RS_G unsigned*) (row0 + y_stride) : 0u;
            unsigned raw[2];
            yuv_load_pairs<PATH>((const RS_G yuv_u8*) up[f], PATH == YUV_WIDE_PLANAR ? (const RS_G yuv_u8*) vp[f] : nullptr,
                                 (size_t) ry * (size_t) c_stride, col, raw);
            yuv_chroma c[2];
            yuv_pairs<PATH>(k, raw, swap, c);
            RS_G unsigned* out = (RS_G unsigned*) dst[f] + (size_t) (2 * ry) * width + col;
            rs_v4 w;
            w.x = 0xFF000000u | yuv_rgb(k, l0 & 255u, c[0]); w.y = 0xFF000000u | yuv_rgb(k, (l0 >> 8) & 255u, c[0]);
            w.z = 0xFF000000u | yuv_rgb(k, (l0 >> 16) & 255u, c[1]); w.w = 0xFF000000u | yuv_rgb(k, l0 >> 24, c[1]);
            *(RS_G rs_v4*) out = w;
            if (two) {
                w.x = 0xFF000000u | yuv_rgb(k, l1 & 255u, c[0]); w.y = 0xFF000000u | yuv_rgb(k, (l1 >> 8) & 255u, c[0]);
                w.z = 0xFF000000u | yuv_rgb(k, (l1 >> 16) & 255u, c[1]); w.w = 0xFF000000u | yuv_rgb(k, l1 >> 24, c[1]);
                *(RS_G rs_v4*) (out + width) = w;
            }
        }
    }
}

// items = n * dh * colblocks; item -> (frame, y, column block) with the column block fastest (as resample_kernel).
template <int PATH>
__global__ void __launch_bounds__(YR_THREADS) resample_yuv_kernel(const yuv_u8* const* __restrict__ yp, const yuv_u8* const* __restrict__ up,
                                                                  const yuv_u8* const* __restrict__ vp, unsigned* const* __restrict__ dst,
                                                                  long long items, int colblocks, int oc, int y_stride, int c_stride,
                                                                  int c_step, int swap, YuvCoef k, int crop_x, int crop_y, unsigned cw,
                                                                  unsigned ch, unsigned dw, unsigned dh, int linear) {
    constexpr bool VEC = PATH != YUV_BYTE;
    __shared__ rs_u64 s_sum[3][YR_CHUNK];            // r, g, b column sums of the current chunk (of wy T[c]: alpha is 255 everywhere)
    __shared__ unsigned short s_T[256];
    const int t = threadIdx.x;
    s_T[t] = linear ? RS_LINEAR[t] : (unsigned short) (257 * t);
    __syncthreads();
    const rs_u64 W = (rs_u64) cw * ch;
    for (long long item = blockIdx.x; item < items; item += gridDim.x) {
        const int cb = (int) (item % colblocks);
        const long long fy = item / colblocks;
        const unsigned y = (unsigned) (fy % dh);
        const long long f = fy / dh;
        const RS_G yuv_u8* luma = (const RS_G yuv_u8*) yp[f];
        const RS_G yuv_u8* fu = (const RS_G yuv_u8*) up[f];
        const RS_G yuv_u8* fv = PATH == YUV_WIDE_INTERLEAVED ? nullptr : (const RS_G yuv_u8*) vp[f];
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
        for (; c <= cend; c += YR_CHUNK) {
            // the thread's four columns of the chunk: k[e] in the chunk, c + k[e] in the frame
            rs_u64 acc[4][3];
#pragma unroll
            for (int e = 0; e < 4; ++e) acc[e][0] = acc[e][1] = acc[e][2] = 0;
            for (unsigned ib = i0; ib <= i1; ib += YR_ROWS) {
                // YR_ROWS rows are loaded before the first is used; behind the footprint's last row that row is read again, with weight 0.
                // A column that is not loaded keeps 0x000000, and T[0] = 0 in both tables.
                unsigned p[YR_ROWS][4];
                size_t yoff[YR_ROWS], coff[YR_ROWS];
#pragma unroll
                for (int r = 0; r < YR_ROWS; ++r) {
                    const int row = crop_y + (int) min(ib + r, i1);
                    yoff[r] = (size_t) row * (size_t) y_stride;
                    coff[r] = (size_t) (row >> 1) * (size_t) c_stride;
                    p[r][0] = p[r][1] = p[r][2] = p[r][3] = 0u;
                }
                if constexpr (VEC) {                    // (width is a multiple of 4 and c + 4 t <= cend < width: the loads stay in the row)
                    if (c + 4 * t <= cend) {
                        unsigned l[YR_ROWS], raw[YR_ROWS][2];
#pragma unroll
                        for (int r = 0; r < YR_ROWS; ++r) {
                            l[r] = *(const RS_G unsigned*) (luma + yoff[r] + c + 4 * t);
                            yuv_load_pairs<PATH>(fu, fv, coff[r], c + 4 * t, raw[r]);
                        }
#pragma unroll
                        for (int r = 0; r < YR_ROWS; ++r) {
                            yuv_chroma q[2];
                            yuv_pairs<PATH>(k, raw[r], swap, q);
                            p[r][0] = yuv_rgb(k, l[r] & 255u, q[0]); p[r][1] = yuv_rgb(k, (l[r] >> 8) & 255u, q[0]);
                            p[r][2] = yuv_rgb(k, (l[r] >> 16) & 255u, q[1]); p[r][3] = yuv_rgb(k, l[r] >> 24, q[1]);
                        }
                    }
                } else {
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const int col = c + t + e * YR_THREADS;
                        if (col <= cend) {
                            unsigned Y[YR_ROWS], U[YR_ROWS], V[YR_ROWS];
                            const size_t cx = (size_t) (col >> 1) * (size_t) c_step;
#pragma unroll
                            for (int r = 0; r < YR_ROWS; ++r) {
                                Y[r] = luma[yoff[r] + col];
                                U[r] = fu[coff[r] + cx];
                                V[r] = fv[coff[r] + cx];
                            }
#pragma unroll
                            for (int r = 0; r < YR_ROWS; ++r) p[r][e] = yuv_rgb(k, Y[r], yuv_terms(k, U[r], V[r]));
                        }
                    }
                }
#pragma unroll
                for (int r = 0; r < YR_ROWS; ++r) {
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
                const int kk = VEC ? 4 * t + e : t + e * YR_THREADS;
#pragma unroll
                for (int q = 0; q < 3; ++q) s_sum[q][kk] = acc[e][q];
            }
            __syncthreads();
            const int lo = max(fa, c), hi = min(fb, c + YR_CHUNK - 1);
            for (int ja = lo; ja <= hi; ++ja) {
                const rs_u64 wx = rs_overlap((unsigned) (ja - crop_x), dw, x * cw, cw);
#pragma unroll
                for (int q = 0; q < 3; ++q) S[q] += wx * s_sum[q][ja - c];
            }
            __syncthreads();                            // the next chunk (or item) overwrites the sums
        }
        if (owner)
            ((RS_G unsigned*) dst[f])[(size_t) y * dw + x] =
                0xFF000000u | rs_encode(s_T, S[0], W) << 16 | rs_encode(s_T, S[1], W) << 8 | rs_encode(s_T, S[2], W);
    }
}

} // namespace

void launch_yuv_argb(const void* const* d_tab, int n, int width, int height, int y_stride, int c_stride, int c_step, int path, bool swap,
                     const YuvCoef& k, hipStream_t s) {
    const yuv_u8* const* yp = reinterpret_cast<const yuv_u8* const*>(d_tab);
    unsigned* const* dst = reinterpret_cast<unsigned* const*>(const_cast<void* const*>(d_tab + 3 * (size_t) n));
    const long long items = path == YUV_BYTE ? (long long) n * height * width : (long long) n * ((height + 1) / 2) * (width / 4);
    const long long blocks = (items + YUV_THREADS - 1) / YUV_THREADS;
    const unsigned grid = (unsigned) (blocks < YUV_MAX_BLOCKS ? blocks : YUV_MAX_BLOCKS);
#define NQ_YUV_LAUNCH(P) hipLaunchKernelGGL((yuv_argb_kernel<P>), dim3(grid), dim3(YUV_THREADS), 0, s, yp, yp + n, yp + 2 * (size_t) n, dst, \
                                            items, width, height, y_stride, c_stride, c_step, swap ? 1 : 0, k)
    if (path == YUV_WIDE_INTERLEAVED) NQ_YUV_LAUNCH(YUV_WIDE_INTERLEAVED);
    else if (path == YUV_WIDE_PLANAR) NQ_YUV_LAUNCH(YUV_WIDE_PLANAR);
    else NQ_YUV_LAUNCH(YUV_BYTE);
#undef NQ_YUV_LAUNCH
}

void launch_resample_yuv(const void* const* d_tab, int n, int y_stride, int c_stride, int c_step, int path, bool swap, const YuvCoef& k,
                         int crop_x, int crop_y, int crop_w, int crop_h, int dst_width, int dst_height, bool linear, hipStream_t s) {
    const yuv_u8* const* yp = reinterpret_cast<const yuv_u8* const*>(d_tab);
    unsigned* const* dst = reinterpret_cast<unsigned* const*>(const_cast<void* const*>(d_tab + 3 * (size_t) n));
    // output columns per item: as launch_resample
    long long oc = (long long) (YR_CHUNK - 4) * dst_width / crop_w;
    oc = oc < 1 ? 1 : (oc > YR_THREADS ? YR_THREADS : oc);
    const int colblocks = (int) ((dst_width + oc - 1) / oc);
    const long long items = (long long) n * dst_height * colblocks;       // <= n * crop_w * crop_h < 2^31
    const unsigned grid = (unsigned) (items < YR_MAX_BLOCKS ? items : YR_MAX_BLOCKS);
#define NQ_YUV_LAUNCH(P) hipLaunchKernelGGL((resample_yuv_kernel<P>), dim3(grid), dim3(YR_THREADS), 0, s, yp, yp + n, yp + 2 * (size_t) n, dst, \
                                            items, colblocks, (int) oc, y_stride, c_stride, c_step, swap ? 1 : 0, k, crop_x, crop_y,          \
                                            (unsigned) crop_w, (unsigned) crop_h, (unsigned) dst_width, (unsigned) dst_height, linear ? 1 : 0)
    if (path == YUV_WIDE_INTERLEAVED) NQ_YUV_LAUNCH(YUV_WIDE_INTERLEAVED);
    else if (path == YUV_WIDE_PLANAR) NQ_YUV_LAUNCH(YUV_WIDE_PLANAR);
    else NQ_YUV_LAUNCH(YUV_BYTE);
#undef NQ_YUV_LAUNCH
}

} // namespace nq
