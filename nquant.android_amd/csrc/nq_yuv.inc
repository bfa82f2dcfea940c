// nq_yuv.inc -- the YUV 4:2:0 conversion the kernels share (nq_yuv.hip: 1:1 and fused with the reducer; nq_orient.hip: 1:1 with the
// oriented store).  Included inside namespace nq { namespace { ... } } of each translation unit, after RS_G (the global address
// space of a pointer read from a frame table: nq_resample.inc) and YuvCoef (nq_kernels.h).

typedef unsigned char yuv_u8;
typedef unsigned short yuv_u16;

// what a chroma sample adds to the three channels of the (up to four) pixels that share it
struct yuv_chroma { int r, g, b; };

__device__ inline yuv_chroma yuv_terms(const YuvCoef& k, unsigned U, unsigned V) {
    const int u = (int) U - 128, v = (int) V - 128;
    yuv_chroma c;
    c.r = k.crv * v;
    c.g = -(k.cgu * u) - k.cgv * v;
    c.b = k.cbu * u;
    return c;
}

__device__ inline unsigned yuv_clamp(int v) { return (unsigned) min(max(v, 0), 255); }

// 0x00RRGGBB of a luma value and its chroma terms: every intermediate is below 3.6e7 in magnitude, >> is the arithmetic shift
__device__ inline unsigned yuv_rgb(const YuvCoef& k, unsigned Y, const yuv_chroma& c) {
    const int l = k.cy * ((int) Y - k.yo) + 32768;
    return yuv_clamp((l + c.r) >> 16) << 16 | yuv_clamp((l + c.g) >> 16) << 8 | yuv_clamp((l + c.b) >> 16);
}

// the chroma terms of the two sample pairs under four adjacent columns (the first a multiple of 4) of chroma row `crow`.  `col` is
// that first column.  Interleaved: `lo` is the lower of the two chroma pointers, swap says that it is v's.
template <int PATH>
__device__ inline void yuv_load_pairs(const RS_G yuv_u8* lo, const RS_G yuv_u8* hi, size_t crow_off, int col, unsigned raw[2]) {
    if constexpr (PATH == YUV_WIDE_INTERLEAVED) {
        raw[0] = *(const RS_G unsigned*) (lo + crow_off + col);
        raw[1] = 0u;
    } else {
        raw[0] = *(const RS_G yuv_u16*) (lo + crow_off + (col >> 1));
        raw[1] = *(const RS_G yuv_u16*) (hi + crow_off + (col >> 1));
    }
}
template <int PATH>
__device__ inline void yuv_pairs(const YuvCoef& k, const unsigned raw[2], int swap, yuv_chroma out[2]) {
    if constexpr (PATH == YUV_WIDE_INTERLEAVED) {
        const unsigned a0 = raw[0] & 255u, b0 = (raw[0] >> 8) & 255u, a1 = (raw[0] >> 16) & 255u, b1 = raw[0] >> 24;
        out[0] = swap ? yuv_terms(k, b0, a0) : yuv_terms(k, a0, b0);
        out[1] = swap ? yuv_terms(k, b1, a1) : yuv_terms(k, a1, b1);
    } else {
        out[0] = yuv_terms(k, raw[0] & 255u, raw[1] & 255u);
        out[1] = yuv_terms(k, raw[0] >> 8, raw[1] >> 8);
    }
}
