// nq_orient.hip -- turn and mirror frame sequences on gfx950 (include/nquant_abi.h, "orientation").
//
// orientation is 1..8 with EXIF's meaning; for a source of W x H pixels:
//   1  out(x, y) = src(x, y)              W x H        5  out(x, y) = src(y, x)              H x W
//   2  out(x, y) = src(W-1-x, y)          W x H        6  out(x, y) = src(y, H-1-x)          H x W
//   3  out(x, y) = src(W-1-x, H-1-y)      W x H        7  out(x, y) = src(W-1-y, H-1-x)      H x W
//   4  out(x, y) = src(x, H-1-y)          W x H        8  out(x, y) = src(W-1-y, x)          H x W
// In every code the source column either runs with or against one output axis (FX: against) and the source row with or against
// the other (FY: against); codes 5..8 also swap the axes (T).
//
//   orient_argb_kernel<ORIENT, PATH>   ARGB words to ARGB words
//   yuv_orient_kernel<ORIENT, PATH>    the 1:1 YUV 4:2:0 conversion of nq_yuv.hip with the oriented store: the unrotated ARGB frame
//                                      never exists
// ONE launch covers the sequence.  An item is (frame, tile): a tile is ORIENT_TILE x ORIENT_TILE SOURCE pixels (less at the right and
// bottom edges), the tile column runs fastest; a workgroup of ORIENT_THREADS takes the items blockIdx.x, + gridDim.x, ...
//   codes 1..4   source rows become output rows: every thread stores what it loaded, no LDS
//   codes 5..8   the tile goes through LDS, in source order with a row pitch of ORIENT_TILE + 1 words.  Loading, a wave writes (parts
//                of) rows: word path bank = column, conflict-free; wide path 16 quads x 2 rows (or row pairs) per 32 lanes, 2-way,
//                which a 4-byte LDS store hides.  Storing, a lane reads down a column: word path 32 consecutive rows of one
//                column, banks (row + column) mod 32 all different; wide path 8 quads of rows x 4 columns per 32 lanes, banks
//                (4 q + e + column) mod 32 all different for each of the four reads e.  Global reads and writes of a tile row
//                are contiguous runs (256 bytes of a full tile, 128 per half wave on the wide store).  One barrier after the
//                loads, one after the stores (the next item overwrites the tile).
// The wide paths move 16 bytes per access where the host has checked what they need (nq_abi.cpp: orient_device, yuv_orient_device);
// the kernels never test an address.  Every loop is bounded by the tile side or the item count; workgroups do not wait for each other.
#include "nq_kernels.h"

namespace nq {

namespace {

constexpr int ORIENT_TILE = 64;
constexpr int ORIENT_PITCH = ORIENT_TILE + 1;
constexpr int ORIENT_THREADS = 256;
constexpr long long ORIENT_MAX_BLOCKS = 2048;   // grid cap of both kernels: 8 workgroups per compute unit (17 KiB of LDS each)

// A pointer read from the frame tables is generic to the compiler: the frames are device memory (as in nq_resample.inc).
#define RS_G __attribute__((address_space(1)))
typedef unsigned or_v4 __attribute__((ext_vector_type(4)));

#include "nq_yuv.inc"                           // yuv_u8, yuv_chroma, yuv_terms, yuv_rgb, yuv_load_pairs, yuv_pairs

template <int ORIENT> struct or_code {
    static_assert(ORIENT >= 1 && ORIENT <= 8, "orientation");
    static constexpr bool T = ORIENT >= 5;
    static constexpr bool FX = ORIENT == 2 || ORIENT == 3 || ORIENT == 7 || ORIENT == 8;
    static constexpr bool FY = ORIENT == 3 || ORIENT == 4 || ORIENT == 6 || ORIENT == 7;
};

// the tile of an item: its first source column and row, its sides and its frame
struct or_tile { int x0, y0, tw, th; long long f; };

__device__ inline or_tile or_item(long long item, int tiles_x, int tiles_y, int width, int height) {
    or_tile t;
    const int tx = (int) (item % tiles_x);
    const long long fr = item / tiles_x;
    const int ty = (int) (fr % tiles_y);
    t.f = fr / tiles_y;
    t.x0 = tx * ORIENT_TILE; t.y0 = ty * ORIENT_TILE;
    t.tw = min(ORIENT_TILE, width - t.x0); t.th = min(ORIENT_TILE, height - t.y0);
    return t;
}

__device__ inline or_v4 or_reverse(or_v4 v) { or_v4 r; r.x = v.w; r.y = v.z; r.z = v.y; r.w = v.x; return r; }

// codes 1..4: the word of source pixel (sx, sy) / the four words of source columns sx .. sx + 3 (sx, width multiples of 4) to their place
template <int ORIENT>
__device__ inline void or_put(RS_G unsigned* out, int width, int height, int sx, int sy, unsigned w) {
    typedef or_code<ORIENT> C;
    out[(size_t) (C::FY ? height - 1 - sy : sy) * width + (C::FX ? width - 1 - sx : sx)] = w;
}
template <int ORIENT>
__device__ inline void or_put4(RS_G unsigned* out, int width, int height, int sx, int sy, or_v4 w) {
    typedef or_code<ORIENT> C;
    *(RS_G or_v4*) (out + (size_t) (C::FY ? height - 1 - sy : sy) * width + (C::FX ? width - 4 - sx : sx)) = C::FX ? or_reverse(w) : w;
}

// codes 5..8: the tile in LDS (source order) to the output frame, which is `height` words wide and `width` rows tall.  Output row j
// of the tile is its source column j (FX: tw - 1 - j), output column i its source row i (FY: th - 1 - i).  WIDE: height, and so th and
// the tile's first output column, are multiples of 4 and the output is 16-byte aligned.
template <int ORIENT, bool WIDE>
__device__ inline void or_store_tile(const unsigned (*tile)[ORIENT_PITCH], RS_G unsigned* out, int width, int height, const or_tile& t) {
    typedef or_code<ORIENT> C;
    const int ox0 = C::FY ? height - t.y0 - t.th : t.y0, oy0 = C::FX ? width - t.x0 - t.tw : t.x0;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if constexpr (WIDE) {
        const int i = 4 * ((lane & 7) + 8 * (wave & 1)), jb = (lane >> 3) + 8 * (wave >> 1);
        if (i < t.th) {
#pragma unroll
            for (int k = 0; k < ORIENT_TILE / 16; ++k) {
                const int j = jb + 16 * k;
                if (j < t.tw) {
                    const int sc = C::FX ? t.tw - 1 - j : j;
                    or_v4 v;
                    v.x = tile[C::FY ? t.th - 1 - i : i][sc]; v.y = tile[C::FY ? t.th - 2 - i : i + 1][sc];
                    v.z = tile[C::FY ? t.th - 3 - i : i + 2][sc]; v.w = tile[C::FY ? t.th - 4 - i : i + 3][sc];
                    *(RS_G or_v4*) (out + (size_t) (oy0 + j) * height + ox0 + i) = v;
                }
            }
        }
    } else {
        if (lane < t.th) {
            const int sr = C::FY ? t.th - 1 - lane : lane;
#pragma unroll
            for (int k = 0; k < ORIENT_TILE / 4; ++k) {
                const int j = wave + 4 * k;
                if (j < t.tw) out[(size_t) (oy0 + j) * height + ox0 + lane] = tile[sr][C::FX ? t.tw - 1 - j : j];
            }
        }
    }
}

// src / dst: n frame pointers each; items = n * tiles_x * tiles_y.  WIDE: every pointer is 16-byte aligned, width is a multiple of 4
// and, for codes 5..8, so is height.
template <int ORIENT, bool WIDE>
__global__ void __launch_bounds__(ORIENT_THREADS) orient_argb_kernel(const unsigned* const* __restrict__ src, unsigned* const* __restrict__ dst,
                                                                     long long items, int tiles_x, int tiles_y, int width, int height) {
    typedef or_code<ORIENT> C;
    __shared__ unsigned s_tile[C::T ? ORIENT_TILE : 1][ORIENT_PITCH];
    const int t = threadIdx.x;
    for (long long item = blockIdx.x; item < items; item += gridDim.x) {
        const or_tile tl = or_item(item, tiles_x, tiles_y, width, height);
        const RS_G unsigned* in = (const RS_G unsigned*) src[tl.f];
        RS_G unsigned* out = (RS_G unsigned*) dst[tl.f];
        if constexpr (WIDE) {
            const int c = 4 * (t & 15), rb = t >> 4;
            if (c < tl.tw) {
#pragma unroll
                for (int k = 0; k < ORIENT_TILE / 16; ++k) {
                    const int r = rb + 16 * k;
                    if (r < tl.th) {
                        const or_v4 v = *(const RS_G or_v4*) (in + (size_t) (tl.y0 + r) * width + tl.x0 + c);
                        if constexpr (C::T) { s_tile[r][c] = v.x; s_tile[r][c + 1] = v.y; s_tile[r][c + 2] = v.z; s_tile[r][c + 3] = v.w; }
                        else or_put4<ORIENT>(out, width, height, tl.x0 + c, tl.y0 + r, v);
                    }
                }
            }
        } else {
            const int c = t & 63, rb = t >> 6;
            if (c < tl.tw) {
#pragma unroll
                for (int k = 0; k < ORIENT_TILE / 4; ++k) {
                    const int r = rb + 4 * k;
                    if (r < tl.th) {
                        const unsigned v = in[(size_t) (tl.y0 + r) * width + tl.x0 + c];
                        if constexpr (C::T) s_tile[r][c] = v;
                        else or_put<ORIENT>(out, width, height, tl.x0 + c, tl.y0 + r, v);
                    }
                }
            }
        }
        if constexpr (C::T) {
            __syncthreads();
            or_store_tile<ORIENT, WIDE>(s_tile, out, width, height, tl);
            __syncthreads();                            // the next item overwrites the tile
        }
    }
}

// yp / up / vp / dst: n frame pointers each, as for yuv_argb_kernel (interleaved wide path: up holds the lower chroma pointer of every
// frame, vp is not read); items = n * tiles_x * tiles_y.  The wide paths need what yuv_argb_kernel's need and, for codes 5..8, height
// a multiple of 4.  A tile starts at an even column and row, so the chroma pairing of (x >> 1, y >> 1) is that of the frame.
template <int ORIENT, int PATH>
__global__ void __launch_bounds__(ORIENT_THREADS) yuv_orient_kernel(const yuv_u8* const* __restrict__ yp, const yuv_u8* const* __restrict__ up,
                                                                    const yuv_u8* const* __restrict__ vp, unsigned* const* __restrict__ dst,
                                                                    long long items, int tiles_x, int tiles_y, int width, int height,
                                                                    int y_stride, int c_stride, int c_step, int swap, YuvCoef k) {
    typedef or_code<ORIENT> C;
    __shared__ unsigned s_tile[C::T ? ORIENT_TILE : 1][ORIENT_PITCH];
    const int t = threadIdx.x;
    for (long long item = blockIdx.x; item < items; item += gridDim.x) {
        const or_tile tl = or_item(item, tiles_x, tiles_y, width, height);
        RS_G unsigned* out = (RS_G unsigned*) dst[tl.f];
        if constexpr (PATH == YUV_BYTE) {
            const int c = t & 63, rb = t >> 6;
            if (c < tl.tw) {
                const int x = tl.x0 + c;
                const size_t cx = (size_t) (x >> 1) * (size_t) c_step;
#pragma unroll
                for (int kk = 0; kk < ORIENT_TILE / 4; ++kk) {
                    const int r = rb + 4 * kk;
                    if (r < tl.th) {
                        const int y = tl.y0 + r;
                        const size_t coff = (size_t) (y >> 1) * (size_t) c_stride + cx;
                        const unsigned Y = ((const RS_G yuv_u8*) yp[tl.f])[(size_t) y * (size_t) y_stride + x];
                        const unsigned U = ((const RS_G yuv_u8*) up[tl.f])[coff];
                        const unsigned V = ((const RS_G yuv_u8*) vp[tl.f])[coff];
                        const unsigned w = 0xFF000000u | yuv_rgb(k, Y, yuv_terms(k, U, V));
                        if constexpr (C::T) s_tile[r][c] = w;
                        else or_put<ORIENT>(out, width, height, x, y, w);
                    }
                }
            }
        } else {
            // a block of 4 columns x 2 rows per thread and step, as in yuv_argb_kernel; an odd last row is a block of one row
            const int c = 4 * (t & 15), pb = t >> 4;
            if (c < tl.tw) {
                const int col = tl.x0 + c;
#pragma unroll
                for (int kk = 0; kk < ORIENT_TILE / 32; ++kk) {
                    const int r = 2 * (pb + 16 * kk);
                    if (r < tl.th) {
                        const int y = tl.y0 + r;
                        const bool two = r + 1 < tl.th;
                        const RS_G yuv_u8* row0 = (const RS_G yuv_u8*) yp[tl.f] + (size_t) y * (size_t) y_stride + col;
                        const unsigned l0 = *(const RS_G unsigned*) row0;
                        const unsigned l1 = two ? *(const RS_G unsigned*) (row0 + y_stride) : 0u;
                        unsigned raw[2];
                        yuv_load_pairs<PATH>((const RS_G yuv_u8*) up[tl.f], PATH == YUV_WIDE_PLANAR ? (const RS_G yuv_u8*) vp[tl.f] : nullptr,
                                             (size_t) (y >> 1) * (size_t) c_stride, col, raw);
                        yuv_chroma q[2];
                        yuv_pairs<PATH>(k, raw, swap, q);
                        or_v4 w0, w1;
                        w0.x = 0xFF000000u | yuv_rgb(k, l0 & 255u, q[0]); w0.y = 0xFF000000u | yuv_rgb(k, (l0 >> 8) & 255u, q[0]);
                        w0.z = 0xFF000000u | yuv_rgb(k, (l0 >> 16) & 255u, q[1]); w0.w = 0xFF000000u | yuv_rgb(k, l0 >> 24, q[1]);
                        w1.x = 0xFF000000u | yuv_rgb(k, l1 & 255u, q[0]); w1.y = 0xFF000000u | yuv_rgb(k, (l1 >> 8) & 255u, q[0]);
                        w1.z = 0xFF000000u | yuv_rgb(k, (l1 >> 16) & 255u, q[1]); w1.w = 0xFF000000u | yuv_rgb(k, l1 >> 24, q[1]);
                        if constexpr (C::T) {
                            s_tile[r][c] = w0.x; s_tile[r][c + 1] = w0.y; s_tile[r][c + 2] = w0.z; s_tile[r][c + 3] = w0.w;
                            if (two) { s_tile[r + 1][c] = w1.x; s_tile[r + 1][c + 1] = w1.y; s_tile[r + 1][c + 2] = w1.z; s_tile[r + 1][c + 3] = w1.w; }
                        } else {
                            or_put4<ORIENT>(out, width, height, col, y, w0);
                            if (two) or_put4<ORIENT>(out, width, height, col, y + 1, w1);
                        }
                    }
                }
            }
        }
        if constexpr (C::T) {
            __syncthreads();
            or_store_tile<ORIENT, PATH != YUV_BYTE>(s_tile, out, width, height, tl);
            __syncthreads();                            // the next item overwrites the tile
        }
    }
}

// tiles per frame side, items and grid of a launch
struct or_grid { int tiles_x, tiles_y; long long items; unsigned blocks; };

or_grid or_plan(int n, int width, int height) {
    or_grid g;
    g.tiles_x = (width + ORIENT_TILE - 1) / ORIENT_TILE;
    g.tiles_y = (height + ORIENT_TILE - 1) / ORIENT_TILE;
    g.items = (long long) n * g.tiles_x * g.tiles_y;                      // <= n * width * height < 2^31
    g.blocks = (unsigned) (g.items < ORIENT_MAX_BLOCKS ? g.items : ORIENT_MAX_BLOCKS);
    return g;
}

} // namespace

#define NQ_ORIENT_CODES(LAUNCH) \
    switch (orientation) {      \
    case 1: LAUNCH(1); break; case 2: LAUNCH(2); break; case 3: LAUNCH(3); break; case 4: LAUNCH(4); break; \
    case 5: LAUNCH(5); break; case 6: LAUNCH(6); break; case 7: LAUNCH(7); break; default: LAUNCH(8); break; \
    }

void launch_orient(const unsigned* const* d_src, unsigned* const* d_dst, int n, int width, int height, int orientation, bool wide,
                   hipStream_t s) {
    const or_grid g = or_plan(n, width, height);
#define NQ_ORIENT_LAUNCH(O) do {                                                                                                       \
        if (wide) hipLaunchKernelGGL((orient_argb_kernel<O, true>), dim3(g.blocks), dim3(ORIENT_THREADS), 0, s, d_src, d_dst, g.items,  \
                                     g.tiles_x, g.tiles_y, width, height);                                                            \
        else hipLaunchKernelGGL((orient_argb_kernel<O, false>), dim3(g.blocks), dim3(ORIENT_THREADS), 0, s, d_src, d_dst, g.items,      \
                                g.tiles_x, g.tiles_y, width, height);                                                                 \
    } while (0)
    NQ_ORIENT_CODES(NQ_ORIENT_LAUNCH)
#undef NQ_ORIENT_LAUNCH
}

void launch_yuv_orient(const void* const* d_tab, int n, int width, int height, int y_stride, int c_stride, int c_step, int path, bool swap,
                       const YuvCoef& k, int orientation, hipStream_t s) {
    const yuv_u8* const* yp = reinterpret_cast<const yuv_u8* const*>(d_tab);
    unsigned* const* dst = reinterpret_cast<unsigned* const*>(const_cast<void* const*>(d_tab + 3 * (size_t) n));
    const or_grid g = or_plan(n, width, height);
#define NQ_ORIENT_KERNEL(O, P) hipLaunchKernelGGL((yuv_orient_kernel<O, P>), dim3(g.blocks), dim3(ORIENT_THREADS), 0, s, yp, yp + n,            \
                                                  yp + 2 * (size_t) n, dst, g.items, g.tiles_x, g.tiles_y, width, height, y_stride, c_stride, \
                                                  c_step, swap ? 1 : 0, k)
#define NQ_ORIENT_LAUNCH(O) do {                                                        \
        if (path == YUV_WIDE_INTERLEAVED) NQ_ORIENT_KERNEL(O, YUV_WIDE_INTERLEAVED);    \
        else if (path == YUV_WIDE_PLANAR) NQ_ORIENT_KERNEL(O, YUV_WIDE_PLANAR);         \
        else NQ_ORIENT_KERNEL(O, YUV_BYTE);                                             \
    } while (0)
    NQ_ORIENT_CODES(NQ_ORIENT_LAUNCH)
#undef NQ_ORIENT_LAUNCH
#undef NQ_ORIENT_KERNEL
}

#undef NQ_ORIENT_CODES

} // namespace nq
