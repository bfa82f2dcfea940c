// nq_resample.hip -- crop and area-average a sequence of ARGB frames down to a target size on gfx950 (include/nquant_abi.h, "frame
// reduction").
//
// Output pixel (x, y) of a frame is a weighted mean over its footprint in the crop: weights wx(x, j) * wy(y, i) are overlap lengths on
// axes scaled by the other side, colour is looked up in a 256 x u16 table T (sRGB -> linear light, or 257 v) and premultiplied by alpha,
// all in exact integers, so the result is the one the header states, bit for bit.  ONE launch covers the sequence.  There is no
// intermediate image in global memory:
//   * A work item is (frame, output row y, block of `oc` output columns); a workgroup takes items blockIdx.x, + gridDim.x, ...
//   * The item's source columns are taken in chunks of RS_CHUNK.  Per chunk a thread owns four source columns and walks the footprint's
//     source rows, RS_ROWS at a time (their loads are in flight together), accumulating wy * a and wy * a * T[c] per column in 64-bit
//     registers (<= ch * 255 * 65535 < 2^40); the column sums go to LDS; then thread o < oc folds the columns of output x0 + o that
//     lie in the chunk with wx into its own four 64-bit sums (< 2^56), which it keeps across the chunks.
//   * After the last chunk the output threads do the two kinds of division and the table search, once per output pixel.
//   resample_kernel<true>   the vector path: a thread's four columns are adjacent and come with one 16-byte load; needs every frame
//                           16-byte aligned and src_width a multiple of 4 (a chunk then starts at a multiple of 4 columns of the frame,
//                           up to 3 columns left of the span: those sums are staged and never folded)
//   resample_kernel<false>  any 4-byte aligned frames: a thread's columns lie RS_THREADS apart, one pixel per load
// launch_resample picks the path on the host; the kernels never test an address.  Every loop is bounded by a side length (rows and
// columns of a footprint), the chunk count of a span or the item count; workgroups do not wait for each other.
#include "nq_kernels.h"

namespace nq {

namespace {

constexpr int RS_THREADS = 256;
constexpr int RS_CHUNK = 4 * RS_THREADS;     // source columns whose sums a workgroup stages in LDS at once (4 x 8 bytes each: 32 KiB)
constexpr int RS_ROWS = 4;                   // source rows a thread has in flight: their loads are issued together
constexpr long long RS_MAX_BLOCKS = 8192;    // grid cap: a workgroup walks the items blockIdx.x + k * gridDim.x

#include "nq_resample.inc"                     // RS_G, rs_v4, rs_u64, RS_LINEAR, rs_overlap, rs_encode (shared with nq_yuv.hip)

// src / dst: n frame pointers each.  items = n * dh * colblocks; item -> (frame, y, column block) with the column block fastest.
template <bool VEC>
__global__ void __launch_bounds__(RS_THREADS) resample_kernel(const unsigned* const* __restrict__ src, unsigned* const* __restrict__ dst,
                                                              long long items, int colblocks, int oc, int src_width, int crop_x, int crop_y,
                                                              unsigned cw, unsigned ch, unsigned dw, unsigned dh, int linear) {
    __shared__ rs_u64 s_sum[4][RS_CHUNK];            // a, r, g, b column sums of the current chunk
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
        const RS_G unsigned* frame = (const RS_G unsigned*) src[f];
        // outputs [x0, x1) of row y; their source columns J0 .. J1 and rows i0 .. i1 (of the crop)
        const unsigned x0 = (unsigned) cb * (unsigned) oc, x1 = min(x0 + (unsigned) oc, dw);
        const unsigned J0 = x0 * cw / dw, J1 = (x1 * cw - 1u) / dw;
        const unsigned i0 = y * ch / dh, i1 = ((y + 1u) * ch - 1u) / dh;
        const unsigned x = x0 + (unsigned) t;
        const bool owner = x < x1;
        // this thread's output: its footprint in columns of the FRAME
        const int fa = owner ? crop_x + (int) (x * cw / dw) : 0, fb = owner ? crop_x + (int) (((x + 1u) * cw - 1u) / dw) : -1;
        rs_u64 S[4] = {0, 0, 0, 0};
        const int cend = crop_x + (int) J1;           // last column of the frame the item reads
        int c = crop_x + (int) J0;
        if (VEC) c &= ~3;
        for (; c <= cend; c += RS_CHUNK) {
            // the thread's four columns of the chunk: k[e] in the chunk, c + k[e] in the frame
            rs_u64 acc[4][4];
#pragma unroll
            for (int e = 0; e < 4; ++e) acc[e][0] = acc[e][1] = acc[e][2] = acc[e][3] = 0;
            for (unsigned ib = i0; ib <= i1; ib += RS_ROWS) {
                // RS_ROWS rows are loaded before the first is used; behind the footprint's last row that row is read again, with weight 0
                unsigned p[RS_ROWS][4];
                const RS_G unsigned* row[RS_ROWS];
#pragma unroll
                for (int r = 0; r < RS_ROWS; ++r) {
                    row[r] = frame + (size_t) (crop_y + (int) min(ib + r, i1)) * (size_t) src_width + c;
                    p[r][0] = p[r][1] = p[r][2] = p[r][3] = 0u;
                }
                if constexpr (VEC) {                    // (src_width is a multiple of 4 and c + 4 t <= cend < src_width: the load stays in the row)
                    if (c + 4 * t <= cend) {
#pragma unroll
                        for (int r = 0; r < RS_ROWS; ++r) {
                            const rs_v4 v = *(const RS_G rs_v4*) (row[r] + 4 * t);
                            p[r][0] = v.x; p[r][1] = v.y; p[r][2] = v.z; p[r][3] = v.w;
                        }
                    }
                } else {
#pragma unroll
                    for (int e = 0; e < 4; ++e)
                        if (c + t + e * RS_THREADS <= cend) {
#pragma unroll
                            for (int r = 0; r < RS_ROWS; ++r) p[r][e] = row[r][t + e * RS_THREADS];
                        }
                }
#pragma unroll
                for (int r = 0; r < RS_ROWS; ++r) {
                    const unsigned wy = ib + r <= i1 ? rs_overlap(ib + r, dh, y * ch, ch) : 0u;
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const unsigned wa = wy * (p[r][e] >> 24);               // <= 65535 * 255
                        acc[e][0] += wa;
                        acc[e][1] += (rs_u64) wa * s_T[(p[r][e] >> 16) & 255u];
                        acc[e][2] += (rs_u64) wa * s_T[(p[r][e] >> 8) & 255u];
                        acc[e][3] += (rs_u64) wa * s_T[p[r][e] & 255u];
                    }
                }
            }
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int k = VEC ? 4 * t + e : t + e * RS_THREADS;
#pragma unroll
                for (int q = 0; q < 4; ++q) s_sum[q][k] = acc[e][q];
            }
            __syncthreads();
            const int lo = max(fa, c), hi = min(fb, c + RS_CHUNK - 1);
            for (int ja = lo; ja <= hi; ++ja) {
                const rs_u64 wx = rs_overlap((unsigned) (ja - crop_x), dw, x * cw, cw);
#pragma unroll
                for (int q = 0; q < 4; ++q) S[q] += wx * s_sum[q][ja - c];
            }
            __syncthreads();                            // the next chunk (or item) overwrites the sums
        }
        if (owner) {
            unsigned out = 0;
            if (S[0]) {
                const unsigned A = (unsigned) ((2 * S[0] + W) / (2 * W));
                out = A << 24 | rs_encode(s_T, S[1], S[0]) << 16 | rs_encode(s_T, S[2], S[0]) << 8 | rs_encode(s_T, S[3], S[0]);
            }
            ((RS_G unsigned*) dst[f])[(size_t) y * dw + x] = out;
        }
    }
}

} // namespace

void launch_resample(const unsigned* const* d_src, unsigned* const* d_dst, int n, int src_width, int crop_x, int crop_y, int crop_w,
                     int crop_h, int dst_width, int dst_height, bool linear, bool vec, hipStream_t s) {
    // output columns per item: as many as have their source span in one chunk (span < oc * cw / dw + 2 columns, and the vector path
    // may start 3 columns early); one output whose span is longer takes several chunks
    long long oc = (long long) (RS_CHUNK - 4) * dst_width / crop_w;
    oc = oc < 1 ? 1 : (oc > RS_THREADS ? RS_THREADS : oc);
    const int colblocks = (int) ((dst_width + oc - 1) / oc);
    const long long items = (long long) n * dst_height * colblocks;       // <= n * crop_w * crop_h < 2^31
    const unsigned grid = (unsigned) (items < RS_MAX_BLOCKS ? items : RS_MAX_BLOCKS);
    if (vec)
        hipLaunchKernelGGL((resample_kernel<true>), dim3(grid), dim3(RS_THREADS), 0, s, d_src, d_dst, items, colblocks, (int) oc, src_width,
                           crop_x, crop_y, (unsigned) crop_w, (unsigned) crop_h, (unsigned) dst_width, (unsigned) dst_height, linear ? 1 : 0);
    else
        hipLaunchKernelGGL((resample_kernel<false>), dim3(grid), dim3(RS_THREADS), 0, s, d_src, d_dst, items, colblocks, (int) oc, src_width,
                           crop_x, crop_y, (unsigned) crop_w, (unsigned) crop_h, (unsigned) dst_width, (unsigned) dst_height, linear ? 1 : 0);
}

} // namespace nq
