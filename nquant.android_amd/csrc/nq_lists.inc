// nq_lists.inc -- exact acceleration of the per-pixel palette scans: candidate lists per colour cell.
// Included by nq_kernels.hip before nq_dither.inc.
//
// closestColorIndex (RGB NQ/PnnQuantizer.java:329-357, LAB NQ/PnnLABQuantizer.java:418-458) keeps, over the palette in index
// order, the two candidates with the smallest err; because every comparison is `err < (int)`, the outcome is exactly the two
// lexicographically smallest (floor(err_k), k) -- the gates only skip candidates that cannot enter.  nearestColorIndex for
// K > 32 (NQ/PnnLABQuantizer.java:369-375) is an argmin of |dL| + sqrt(dA^2 + dB^2) with ties to the highest index.
// For all colours of one 5-6-5 RGB cell (8 x 4 x 8 colours) a palette entry whose SMALLEST possible error over the cell
// exceeds the second smallest (closest) / smallest (nearest) LARGEST possible error (+1 for the floor, + margins) can never be
// chosen, so scanning only the remaining entries, in index order with the unchanged arithmetic, returns the same result.
// Cells whose list would not fit (or K > 256) fall back to the full scan.

namespace nq {

// Two levels (both list builders below).  A wavefront handles a CUBE of 4 x 4 x 4 cells (32 x 16 x 32 colours, lane = cell).  First the
// 64 lanes share the palette (four entries each) and list the entries that can be chosen for SOME colour of the cube -- the same
// criterion on the bigger box --, 256 bits of ballot masks; then every lane runs its own cell's two scans over those entries only
// (~30 of 256).  Exact: an entry's smallest error over the cube is <= its smallest error over the cell and every entry's largest error
// over the cube is >= the one over the cell (integer distances, the same float operations on non-negative operands: rounding is
// monotone), so the cube's threshold is >= the cell's and every entry a cell would list survives the cube's test; the two entries
// that define the cell's threshold are themselves listed entries, so the threshold computed over the survivors is the cell's own.
__device__ __forceinline__ int cube_cell_of_lane(int wave_global, int lane) {
    const int r5 = ((wave_global >> 7) << 2) + (lane >> 4), g6 = (((wave_global >> 3) & 15) << 2) + ((lane >> 2) & 3), b5 = ((wave_global & 7) << 2) + (lane & 3);
    return (r5 << 11) | (g6 << 5) | b5;
}
// a cell's list is collected in registers (32 bytes) and leaves as two 16-byte stores (the cells of a cube lie far apart in memory)
static_assert(NQ_LIST_CAP == 32, "list_append / list_store hold exactly 32 entries");
__device__ __forceinline__ void list_append(unsigned long long (&acc)[4], int n, int k) {
    const unsigned long long v = (unsigned long long) (unsigned) k << ((n & 7) * 8);
    const int w = n >> 3;
    if (w == 0) acc[0] |= v; else if (w == 1) acc[1] |= v; else if (w == 2) acc[2] |= v; else if (w == 3) acc[3] |= v;
}
__device__ __forceinline__ void list_store(unsigned char* out, const unsigned long long (&acc)[4]) {
    ulonglong2* o = reinterpret_cast<ulonglong2*>(out);
    o[0] = make_ulonglong2(acc[0], acc[1]); o[1] = make_ulonglong2(acc[2], acc[3]);
}
// The cell's half of the 32-byte record the specialised kernels read (half 0: closest, 1: nearest) and its continuation entry, in the layout of
// pack_lists_kernel (nq_dither_fast.hip): bytes 0..14 the first candidates, byte 15 their number, candidates 15..30 in cont[half][cell]; a
// cell whose count is above 31 (32 entries, or NQ_LIST_FULLSCAN) gets 255 and zeros.  acc holds zeros behind the list's last entry, so the
// zero padding is the accumulator's own.  packed: [65536][2] records followed by the [2][65536] continuation entries (16 bytes each).
__device__ __forceinline__ void list_store_packed(void* packed, int half, int cell, const unsigned long long (&acc)[4], int count) {
    ulonglong2* rec = reinterpret_cast<ulonglong2*>(packed);
    const bool ok = count <= 31;
    const unsigned long long top = (unsigned long long) (ok ? count : 255) << 56;
    rec[2 * cell + half] = ok ? make_ulonglong2(acc[0], (acc[1] & 0x00FFFFFFFFFFFFFFULL) | top) : make_ulonglong2(0ULL, top);
    rec[2 * 65536 + half * 65536 + cell] = ok ? make_ulonglong2((acc[1] >> 56) | (acc[2] << 8), (acc[2] >> 56) | (acc[3] << 8)) : make_ulonglong2(0ULL, 0ULL);
}
__device__ __forceinline__ float rl_f(float x, int l) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(x), l)); }
// the two smallest values of the wavefront's (m1 <= m2) pairs, in every lane
__device__ __forceinline__ void wave_two_smallest(float& m1, float& m2) {
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const float o1 = __shfl_xor(m1, off, 64), o2 = __shfl_xor(m2, off, 64);
        const float n1 = fminf(m1, o1), n2 = fminf(fmaxf(m1, o1), fminf(m2, o2));
        m1 = n1; m2 = n2;
    }
}

// closest-error lists.  weights W[4] = total weight of da^2, dr^2, dg^2, db^2 in err
__device__ __forceinline__ void closest_lists_body(const DevParams& P, const int* __restrict__ g_palette, double wA, double wR,
                                                   double wG, double wB, unsigned char* __restrict__ lists,
                                                   unsigned char* __restrict__ counts, int block, void* packed = nullptr) {
    // in the per-cell scans the palette index k is uniform over the wavefront: g_palette[k] is a scalar load and its channels are
    // unpacked on the scalar unit -- the vector ALUs only see the per-cell arithmetic
    const int* __restrict__ pal = g_palette;
    const int lane = threadIdx.x & 63;
    const int wave_global = (block * (int) blockDim.x + (int) threadIdx.x) >> 6;
    if (wave_global >= 1024) return;
    const int cell = cube_cell_of_lane(wave_global, lane);
    const int r_lo = (cell >> 8) & 0xF8, g_lo = (cell >> 3) & 0xFC, b_lo = (cell << 3) & 0xF8;
    const int r_hi = r_lo + 7, g_hi = g_lo + 3, b_hi = b_lo + 7;
    const int K = P.K;
    // float32 arithmetic with margins that cover it: every quantity below is a sum of four non-negative products of numbers < 2^17,
    // relative error < 1e-6; a list only has to be a SUPERSET of the entries that can win, so the upper bound is raised and the lower
    // bounds are lowered by 1e-5 (ten times the arithmetic error) on top of the margins of the f64 formulation
    const float fA = (float) wA, fR = (float) wR, fG = (float) wG, fB = (float) wB;
    // ---- the cube ----
    unsigned long long cand[4];
    int pal4[4];                // palette entries lane + 64 j: the per-cell scans fetch entry k with v_readlane (no memory access in the loops)
    {
        const int R_lo = (wave_global >> 7) << 5, G_lo = ((wave_global >> 3) & 15) << 4, B_lo = (wave_global & 7) << 5;
        const int R_hi = R_lo + 31, G_hi = G_lo + 15, B_hi = B_lo + 31;
        float c1 = 3.0e38f, c2m = 3.0e38f, emin4[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int k = lane + 64 * j;
            emin4[j] = 3.0e38f;
            pal4[j] = 0;
            if (k < K) {
                const int c2 = pal4[j] = pal[k];
                const int pr = c_red(c2), pg = c_green(c2), pb = c_blue(c2), pa = c_alpha(c2);
                const float xr = (float) max(abs(pr - R_lo), abs(pr - R_hi)), xg = (float) max(abs(pg - G_lo), abs(pg - G_hi)),
                            xb = (float) max(abs(pb - B_lo), abs(pb - B_hi)), xa = (float) max(pa, 255 - pa);
                const float emax = fA * xa * xa + fR * xr * xr + fG * xg * xg + fB * xb * xb;
                if (emax < c1) { c2m = c1; c1 = emax; } else if (emax < c2m) c2m = emax;
                const float nr = (float) max(0, max(R_lo - pr, pr - R_hi)), ng = (float) max(0, max(G_lo - pg, pg - G_hi)),
                            nb = (float) max(0, max(B_lo - pb, pb - B_hi));
                emin4[j] = (fR * nr * nr + fG * ng * ng + fB * nb * nb) * (1.0f - 1.2e-5f);
            }
        }
        wave_two_smallest(c1, c2m);
        const float UC = c2m * (1.0f + 1.2e-5f) + 1.0f + 1e-5f;
#pragma unroll
        for (int j = 0; j < 4; ++j) cand[j] = __ballot(emin4[j] <= UC);
    }
    // ---- the cell: second smallest of the per-entry maximum error over the cell ----
    float m1 = 3.0e38f, m2 = 3.0e38f;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        unsigned long long m = cand[j];
        while (m) {
            const int bit = __ffsll((long long) m) - 1;
            m &= m - 1;
            const int c2 = __builtin_amdgcn_readlane(pal4[j], bit);
            const int pr = c_red(c2), pg = c_green(c2), pb = c_blue(c2), pa = c_alpha(c2);
            const float dr = (float) max(abs(pr - r_lo), abs(pr - r_hi)), dg = (float) max(abs(pg - g_lo), abs(pg - g_hi)),
                        db = (float) max(abs(pb - b_lo), abs(pb - b_hi)), da = (float) max(pa, 255 - pa);
            const float emax = fA * da * da + fR * dr * dr + fG * dg * dg + fB * db * db;
            if (emax < m1) { m2 = m1; m1 = emax; } else if (emax < m2) m2 = emax;
        }
    }
    const float U = m2 * (1.0f + 1.2e-5f) + 1.0f + 1e-5f;   // +1: floor(); 1e-6: the reference rounds coeffs*d to float; 1e-5: float32 here
    int n = 0;
    unsigned char* out = lists + (size_t) cell * NQ_LIST_CAP;
    unsigned long long acc[4] = {0ULL, 0ULL, 0ULL, 0ULL};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        unsigned long long m = cand[j];
        while (m) {
            const int bit = __ffsll((long long) m) - 1;
            const int k = 64 * j + bit;
            m &= m - 1;
            const int c2 = __builtin_amdgcn_readlane(pal4[j], bit);
            const int pr = c_red(c2), pg = c_green(c2), pb = c_blue(c2);
            const float dr = (float) max(0, max(r_lo - pr, pr - r_hi)), dg = (float) max(0, max(g_lo - pg, pg - g_hi)),
                        db = (float) max(0, max(b_lo - pb, pb - b_hi));
            const float emin = (fR * dr * dr + fG * dg * dg + fB * db * db) * (1.0f - 1.2e-5f);   // alpha of the colour is unknown: da_min = 0
            if (emin <= U) { list_append(acc, n, k); ++n; }
        }
    }
    list_store(out, acc);
    const int count = (K > 256 || n > NQ_LIST_CAP) ? NQ_LIST_FULLSCAN : n;
    counts[cell] = (unsigned char) count;
    if (packed) list_store_packed(packed, 0, cell, acc, count);
}
__global__ void __launch_bounds__(256) build_closest_lists_kernel(DevParams P, const int* __restrict__ g_palette, double wA, double wR,
                                                                  double wG, double wB, unsigned char* __restrict__ lists,
                                                                  unsigned char* __restrict__ counts) {
    closest_lists_body(P, g_palette, wA, wR, wG, wB, lists, counts, (int) blockIdx.x);
}

// one thread per cell: nearest lists for the RGB metric pa da^2 + pr dr^2 + pg dg^2 + pb db^2 (NQ/PnnQuantizer.java:276-310), for
// OPAQUE query colours (alpha 255: the alpha term of an entry is then the same for every colour of the cell) and images without
// a transparent colour (the scan starts at index 0).  Ties go to the highest index in the reference; every entry that can reach
// the minimum for some colour of the cell is listed (smallest possible value <= smallest largest possible value), so ties survive.
__global__ void __launch_bounds__(256) build_nearest_rgb_lists_kernel(DevParams P, const int* __restrict__ g_palette, double wA, double wR,
                                                                      double wG, double wB, unsigned char* __restrict__ lists,
                                                                      unsigned char* __restrict__ counts) {
    extern __shared__ __align__(16) unsigned char smem[];
    int* pal = (int*) smem;
    for (int i = threadIdx.x; i < P.K; i += blockDim.x) pal[i] = g_palette[i];
    __syncthreads();
    const int cell = blockIdx.x * blockDim.x + threadIdx.x;
    if (cell >= 65536) return;
    const int r_lo = (cell >> 8) & 0xF8, g_lo = (cell >> 3) & 0xFC, b_lo = (cell << 3) & 0xF8;
    const int r_hi = r_lo + 7, g_hi = g_lo + 3, b_hi = b_lo + 7;
    const int K = P.K;
    double m1 = 1e300;
    for (int k = 0; k < K; ++k) {
        const int c2 = pal[k];
        const int pr = c_red(c2), pg = c_green(c2), pb = c_blue(c2);
        const double dr = (double) max(abs(pr - r_lo), abs(pr - r_hi)), dg = (double) max(abs(pg - g_lo), abs(pg - g_hi)),
                     db = (double) max(abs(pb - b_lo), abs(pb - b_hi)), da = (double) (255 - c_alpha(c2));
        m1 = fmin(m1, wA * da * da + wR * dr * dr + wG * dg * dg + wB * db * db);
    }
    const double U = m1 * (1.0 + 1e-9) + 1e-9;
    int n = 0;
    unsigned char* out = lists + (size_t) cell * NQ_LIST_CAP;
    for (int k = 0; k < K; ++k) {
        const int c2 = pal[k];
        const int pr = c_red(c2), pg = c_green(c2), pb = c_blue(c2);
        const double dr = (double) max(0, max(r_lo - pr, pr - r_hi)), dg = (double) max(0, max(g_lo - pg, pg - g_hi)),
                     db = (double) max(0, max(b_lo - pb, pb - b_hi)), da = (double) (255 - c_alpha(c2));
        const double emin = (wA * da * da + wR * dr * dr + wG * dg * dg + wB * db * db) * (1.0 - 1e-9);
        if (emin <= U) {
            if (n < NQ_LIST_CAP) out[n] = (unsigned char) k;
            ++n;
        }
    }
    counts[cell] = (K > 256 || n > NQ_LIST_CAP) ? NQ_LIST_FULLSCAN : (unsigned char) n;
}

// Lab bounding box of every 5-6-5 cell over its 256 lattice colours (the only colours a lookup can see), computed with the
// same conversion the nearest scan uses; palette independent, built once per handle.  box[cell] = {Lmin,Lmax,Amin,Amax,Bmin,Bmax}
__global__ void __launch_bounds__(256) cell_lab_box_kernel(float* __restrict__ box) {
    const int cell = blockIdx.x * blockDim.x + threadIdx.x;
    if (cell >= 65536) return;
    const int r_lo = (cell >> 8) & 0xF8, g_lo = (cell >> 3) & 0xFC, b_lo = (cell << 3) & 0xF8;
    float l0 = 1e30f, l1 = -1e30f, a0 = 1e30f, a1 = -1e30f, b0 = 1e30f, b1 = -1e30f;
    for (int r = r_lo; r < r_lo + 8; ++r)
        for (int g = g_lo; g < g_lo + 4; ++g)
            for (int b = b_lo; b < b_lo + 8; ++b) {
                const Lab lab = RGB2LAB_fast(c_argb(255, r, g, b), g_tab.gamma);
                l0 = fminf(l0, lab.L); l1 = fmaxf(l1, lab.L);
                a0 = fminf(a0, lab.A); a1 = fmaxf(a1, lab.A);
                b0 = fminf(b0, lab.B); b1 = fmaxf(b1, lab.B);
            }
    float* o = box + (size_t) cell * 6;
    o[0] = l0; o[1] = l1; o[2] = a0; o[3] = a1; o[4] = b0; o[5] = b1;
}

// nearest lists for the LAB K > 32 metric, two levels as above (the cube's Lab box = the union of its cells' boxes).  `kstart` = 1 when
// palette[0] is the transparent colour and is skipped for visible pixels (NQ/PnnLABQuantizer.java:340-341); pixels that take the other
// start index use the full scan.
__device__ __forceinline__ void nearest_lists_body(const DevParams& P, const int* __restrict__ g_palette, int kstart,
                                                   const float* __restrict__ box,
                                                   unsigned char* __restrict__ lists, unsigned char* __restrict__ counts, int block, unsigned char* smem,
                                                   void* packed = nullptr) {
    PalView pal = stage_palette(P, g_palette, smem);
    const int lane = threadIdx.x & 63;
    const int wave_global = (block * (int) blockDim.x + (int) threadIdx.x) >> 6;
    if (wave_global >= 1024) return;
    const int cell = cube_cell_of_lane(wave_global, lane);
    const float* bx = box + (size_t) cell * 6;
    // float32 with margins that cover it: distances are sums of an absolute difference and a square root of two squares, all < 600,
    // float32 error < 2e-4 absolute; the box is widened by `slack` (a flip of the last float bit of a query's L, A or B moves it by
    // < 2e-5) and the comparison by another 1e-3: a superset of the entries that can be nearest for some colour of the cell
    const float slack = 1e-3f;
    const float L0 = bx[0] - slack, L1 = bx[1] + slack, A0 = bx[2] - slack, A1 = bx[3] + slack, B0 = bx[4] - slack, B1 = bx[5] + slack;
    const int K = P.K;
    // ---- the cube ----
    unsigned long long cand[4];
    float l4[4], a4[4], b4[4];  // Lab of the palette entries lane + 64 j (fetched with v_readlane in the per-cell scans)
    {
        float cL0 = L0, cL1 = L1, cA0 = A0, cA1 = A1, cB0 = B0, cB1 = B1;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            cL0 = fminf(cL0, __shfl_xor(cL0, off, 64)); cL1 = fmaxf(cL1, __shfl_xor(cL1, off, 64));
            cA0 = fminf(cA0, __shfl_xor(cA0, off, 64)); cA1 = fmaxf(cA1, __shfl_xor(cA1, off, 64));
            cB0 = fminf(cB0, __shfl_xor(cB0, off, 64)); cB1 = fmaxf(cB1, __shfl_xor(cB1, off, 64));
        }
        float c1 = 3.0e38f, dmin4[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int k = lane + 64 * j;
            dmin4[j] = 3.0e38f;
            l4[j] = a4[j] = b4[j] = 0.f;
            if (k >= kstart && k < K) {
                const float l = l4[j] = pal.L[k], a = a4[j] = pal.A[k], b = b4[j] = pal.B[k];
                const float xl = fmaxf(fabsf(l - cL0), fabsf(l - cL1)), xa = fmaxf(fabsf(a - cA0), fabsf(a - cA1)), xb = fmaxf(fabsf(b - cB0), fabsf(b - cB1));
                c1 = fminf(c1, xl + __builtin_amdgcn_sqrtf(xa * xa + xb * xb));
                const float nl = fmaxf(0.0f, fmaxf(cL0 - l, l - cL1)), na = fmaxf(0.0f, fmaxf(cA0 - a, a - cA1)), nb = fmaxf(0.0f, fmaxf(cB0 - b, b - cB1));
                dmin4[j] = (nl + __builtin_amdgcn_sqrtf(na * na + nb * nb)) * (1.0f - 1e-5f);
            }
        }
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) c1 = fminf(c1, __shfl_xor(c1, off, 64));
        const float UC = c1 * (1.0f + 1e-5f) + 1e-3f;
#pragma unroll
        for (int j = 0; j < 4; ++j) cand[j] = __ballot(dmin4[j] <= UC);
    }
    // ---- the cell ----
    float m1 = 3.0e38f;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        unsigned long long m = cand[j];
        while (m) {
            const int bit = __ffsll((long long) m) - 1;
            m &= m - 1;
            const float l = rl_f(l4[j], bit), a = rl_f(a4[j], bit), b = rl_f(b4[j], bit);
            const float dl = fmaxf(fabsf(l - L0), fabsf(l - L1)), da = fmaxf(fabsf(a - A0), fabsf(a - A1)), db = fmaxf(fabsf(b - B0), fabsf(b - B1));
            const float dmax = dl + __builtin_amdgcn_sqrtf(da * da + db * db);
            if (dmax < m1) m1 = dmax;
        }
    }
    const float U = m1 * (1.0f + 1e-5f) + 1e-3f;
    int n = 0;
    unsigned char* out = lists + (size_t) cell * NQ_LIST_CAP;
    unsigned long long acc[4] = {0ULL, 0ULL, 0ULL, 0ULL};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        unsigned long long m = cand[j];
        while (m) {
            const int bit = __ffsll((long long) m) - 1;
            const int k = 64 * j + bit;
            m &= m - 1;
            const float l = rl_f(l4[j], bit), a = rl_f(a4[j], bit), b = rl_f(b4[j], bit);
            const float dl = fmaxf(0.0f, fmaxf(L0 - l, l - L1)), da = fmaxf(0.0f, fmaxf(A0 - a, a - A1)), db = fmaxf(0.0f, fmaxf(B0 - b, b - B1));
            const float dmin = (dl + __builtin_amdgcn_sqrtf(da * da + db * db)) * (1.0f - 1e-5f);
            if (dmin <= U) { list_append(acc, n, k); ++n; }
        }
    }
    list_store(out, acc);
    const int count = (K > 256 || n > NQ_LIST_CAP) ? NQ_LIST_FULLSCAN : n;
    counts[cell] = (unsigned char) count;
    if (packed) list_store_packed(packed, 1, cell, acc, count);
}
__global__ void __launch_bounds__(256) build_nearest_lists_kernel(DevParams P, const int* __restrict__ g_palette, int kstart,
                                                                  const float* __restrict__ box,
                                                                  unsigned char* __restrict__ lists, unsigned char* __restrict__ counts) {
    extern __shared__ __align__(16) unsigned char smem[];
    nearest_lists_body(P, g_palette, kstart, box, lists, counts, (int) blockIdx.x, smem);
}
} // namespace nq
