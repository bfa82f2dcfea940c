// nq_resample.inc -- the arithmetic the frame reducers share (nq_resample.hip: ARGB sources; nq_yuv.hip: YUV 4:2:0 sources).  Included
// inside namespace nq { namespace { ... } } of each translation unit.

// A pointer read from the frame tables is generic to the compiler: the frames are device memory, so the accesses name the global
// address space (as HOLD_G in nq_hold.hip).
#define RS_G __attribute__((address_space(1)))
typedef unsigned rs_v4 __attribute__((ext_vector_type(4)));
typedef unsigned long long rs_u64;

__constant__ unsigned short RS_LINEAR[256] = {
#include "../../include/nq_srgb_linear_16.inc"
};

// length of the overlap of cell k of an axis of cells `cell` long with [lo, lo + len): every product is <= 65535^2 < 2^32
__device__ inline unsigned rs_overlap(unsigned k, unsigned cell, unsigned lo, unsigned len) {
    return min((k + 1u) * cell, lo + len) - max(k * cell, lo);
}

// the stored value nearest to t = floor((2 S_c + S_a) / (2 S_a)) in the table, ties to the smaller: the smallest v with
// 2 t <= T[v] + T[v + 1], 255 if there is none (T is strictly increasing, so the condition is monotone in v)
__device__ inline unsigned rs_encode(const unsigned short* T, rs_u64 sc, rs_u64 sa) {
    const unsigned t2 = 2u * (unsigned) ((2 * sc + sa) / (2 * sa));
    unsigned lo = 0, hi = 255;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const unsigned mid = (lo + hi) >> 1;             // < 255 while lo < hi
        const bool ok = t2 <= (unsigned) T[mid] + (unsigned) T[min(mid + 1u, 255u)];
        if (lo < hi) { if (ok) hi = mid; else lo = mid + 1; }
    }
    return lo;
}
