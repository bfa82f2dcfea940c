// nq_dither.inc -- per-pixel lookup kernels, the gilbert error-diffusion kernel and the blue-noise pass.
// Included by nq_kernels.hip (single translation unit).
//
// Parallel decomposition (DESIGN.md "dither pass"): the reference diffuses the error along ONE gilbert curve
// over the whole image (NQ/GilbertCurve.java:194-204,276) -- a strict N-step recurrence.  Here the image is cut
// into tiles; every tile owns an independent curve, error queue and java.util.Random stream and is walked by ONE
// lane, so a wavefront advances 64 tiles in lock step and a launch carries tiles_x*tiles_y chains.  With one tile
// (REFERENCE_SEQUENTIAL) the kernel is the reference algorithm itself, executed by a single lane.

namespace nq {

// the pixel as convert() leaves it in `pixels` (NQ/PnnQuantizer.java:417-425)
__device__ __forceinline__ int load_pixel(const DevParams& P, const int* __restrict__ pixels, long long i) {
    int c = pixels[i];
    if (P.rewriteA0 && c_alpha(c) == 0) c = P.transparentColor;
    return c;
}

// ------------------------------------------------------------------------------------------------
// pure lookups
// ------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) nearest_index_kernel(DevParams P, const int* __restrict__ g_palette, CellLists lists,
                                                            const int* __restrict__ colors, long long M, short* __restrict__ out) {
    extern __shared__ __align__(16) unsigned char smem[];
    PalView pal = stage_palette(P, g_palette, smem);
    for (long long i = (long long) blockIdx.x * blockDim.x + threadIdx.x; i < M; i += (long long) gridDim.x * blockDim.x)
        out[i] = (short) nearest_any(P, pal, colors[i], &lists);
}

__global__ void __launch_bounds__(256) closest_tuple_kernel(DevParams P, const int* __restrict__ g_palette, CellLists lists,
                                                            const int* __restrict__ colors, long long M, int* __restrict__ out4) {
    extern __shared__ __align__(16) unsigned char smem[];
    PalView pal = stage_palette(P, g_palette, smem);
    for (long long i = (long long) blockIdx.x * blockDim.x + threadIdx.x; i < M; i += (long long) gridDim.x * blockDim.x) {
        int c = colors[i];
        int closest[4];
        if (c_alpha(c) <= 0xF) closest[0] = closest[1] = closest[2] = closest[3] = -1;
        else if (P.kind == 0) closest_tuple_rgb(P, pal, c, closest, &lists);
        else closest_tuple_lab(P, pal, c, closest, &lists);
        reinterpret_cast<int4*>(out4)[i] = make_int4(closest[0], closest[1], closest[2], closest[3]);
    }
}

__global__ void __launch_bounds__(256) lookup_only_kernel(DevParams P, const int* __restrict__ g_palette, CellLists lists,
                                                          const int* __restrict__ pixels, long long N,
                                                          unsigned short* __restrict__ out_index, int* __restrict__ out_argb) {
    extern __shared__ __align__(16) unsigned char smem[];
    PalView pal = stage_palette(P, g_palette, smem);
    for (long long i = (long long) blockIdx.x * blockDim.x + threadIdx.x; i < N; i += (long long) gridDim.x * blockDim.x) {
        int k = nearest_any(P, pal, load_pixel(P, pixels, i), &lists);
        if (out_index) out_index[i] = (unsigned short) k;
        if (out_argb) out_argb[i] = pal.argb[k];
    }
}

// ------------------------------------------------------------------------------------------------
// GilbertCurve (NQ/GilbertCurve.java)
// ------------------------------------------------------------------------------------------------
#define NQ_QCAP 32          // sorted queue: grows 1 -> 3 -> 7 -> 15 (DITHER_MAX 9) -> 31 (DITHER_MAX 25, only with weight > .99: NQ/GilbertCurve.java:80-83)

// ErrorBox queue of one chain (:16-32,:45): p in r,g,b,a order.  Only the sorted-by-yDiff mode uses it (the ArrayDeque of the other
// modes is a register shift register, see diffusePixel).  Two storages behind one set of accessors:
//  * LDSQ = false: per-lane arrays -- dynamically indexed, so they live in scratch memory (every access a device-memory round trip);
//  * LDSQ = true: a column of the workgroup's LDS, word (6 t + f) of box t at lds[(6 t + f) * 64] (f = 0..3 the errors, 4..5 the
//    two halves of yDiff): lane-interleaved, bank-conflict free, 30 ns per access.  64 lanes x 32 boxes x 24 bytes = 48 KB per
//    workgroup; launch_gilbert_t uses it whenever that fits next to the staged palette.
template <bool LDSQ> struct ErrQueueT;
template <> struct ErrQueueT<false> {
    float p_[NQ_QCAP][4];
    double y_[NQ_QCAP];
    int head, size;
    __device__ __forceinline__ void bind(unsigned*) {}
    __device__ __forceinline__ float p(int t, int j) const { return p_[t][j]; }
    __device__ __forceinline__ double y(int t) const { return y_[t]; }
    __device__ __forceinline__ void set(int t, const float e[4], double yy) { for (int j = 0; j < 4; ++j) p_[t][j] = e[j]; y_[t] = yy; }
    __device__ __forceinline__ void move(int dst, int src) { for (int j = 0; j < 4; ++j) p_[dst][j] = p_[src][j]; y_[dst] = y_[src]; }
};
template <> struct ErrQueueT<true> {
    unsigned* lds;          // this lane's column
    int head, size;
    __device__ __forceinline__ void bind(unsigned* column) { lds = column; }
    __device__ __forceinline__ float p(int t, int j) const { return __uint_as_float(lds[(6 * t + j) * 64]); }
    __device__ __forceinline__ double y(int t) const {
        const unsigned lo = lds[(6 * t + 4) * 64], hi = lds[(6 * t + 5) * 64];
        return __longlong_as_double((long long) (((unsigned long long) hi << 32) | lo));
    }
    __device__ __forceinline__ void set(int t, const float e[4], double yy) {
        for (int j = 0; j < 4; ++j) lds[(6 * t + j) * 64] = __float_as_uint(e[j]);
        const unsigned long long b = (unsigned long long) __double_as_longlong(yy);
        lds[(6 * t + 4) * 64] = (unsigned) b; lds[(6 * t + 5) * 64] = (unsigned) (b >> 32);
    }
    __device__ __forceinline__ void move(int dst, int src) { for (int f = 0; f < 6; ++f) lds[(6 * dst + f) * 64] = lds[(6 * src + f) * 64]; }
};
#define NQ_QLDS_BYTES ((size_t) 64 * NQ_QCAP * 6 * 4)

// Double.compare(o2.yDiff, o1.yDiff) (:87-94)
__device__ __forceinline__ int dcompare(double a, double b) {
    if (a < b) return -1;
    if (a > b) return 1;
    long long ab = __double_as_longlong(a), bb = __double_as_longlong(b);
    return ab == bb ? 0 : (ab < bb ? -1 : 1);
}

// java.util.PriorityQueue offer/poll on the per-lane array (sorted mode only)
template <class Q>
__device__ __forceinline__ void pq_offer(Q& q, const float e[4], double y) {
    int k = q.size++;
    while (k > 0) {
        int parent = (k - 1) >> 1;
        if (dcompare(q.y(parent), y) >= 0) break;               // cmp(x, parent) = compare(parent.y, x.y)
        q.move(k, parent);
        k = parent;
    }
    q.set(k, e, y);
}
template <class Q>
__device__ __forceinline__ void pq_poll(Q& q) {
    int n = --q.size;
    float x[4]; for (int j = 0; j < 4; ++j) x[j] = q.p(n, j);
    double xy = q.y(n);
    if (n > 0) {
        int k = 0, half = n >> 1;
        while (k < half) {
            int child = 2 * k + 1, right = child + 1;
            // cmp(c, r) = compare(r.y, c.y) > 0  -> take right
            if (right < n && dcompare(q.y(right), q.y(child)) > 0) child = right;
            if (dcompare(q.y(child), xy) <= 0) break;           // cmp(x, c) = compare(c.y, x.y) <= 0
            q.move(k, child);
            k = child;
        }
        q.set(k, x, xy);
    }
}

struct ChainCtx {
    const DevParams* P;
    const GilbertConsts* G;
    LookupCtx lk;
    const int* pixels;
    const float* saliency;  // saliency map (NQ/PnnLABQuantizer.java:156 / :506), or nullptr
    int width;
    int gofs;               // y_origin * width: band-local pixel index -> pixel index in the whole image
    int yorg;               // y_origin
    const float* weights;   // current weights array (sorted mode)
    int nweights;
};

// the saliency map (a throughput kernel: the dither chains are latency bound): four pixels per thread and step as one 16-byte load and
// one 16-byte store, the gamma table in LDS (three dependent look-ups per pixel); `vec4` = N / 4 when the buffers allow it, else 0
__device__ __forceinline__ float saliency_lds(int c, const double* __restrict__ gam) {
    const double Y = 100 * (gam[c_red(c)] * 0.2126 + gam[c_green(c)] * 0.7152 + gam[c_blue(c)] * 0.0722);      // RGB2L (nq_device.h), table in LDS
    const float L = (float) fmax(0.0, 116 * pivot_xyz_fast(Y / 100.0) - 16);
    return .1f + (1 - .1f) * L / 100.0f * (float) c_alpha(c) / 255.0f;                                       // saliency_of
}
// (block / nblocks: this workgroup's index among the workgroups that share the map -- the kernel below, or a role of build_lab_lists_kernel)
__device__ __forceinline__ void saliency_body(const DevParams& P, int salSubst, const int* __restrict__ pixels, long long N,
                                              float* __restrict__ out, long long vec4, int block, int nblocks, double* gam /* LDS, 256 */) {
    gam[threadIdx.x] = g_tab.gamma[threadIdx.x];
    __syncthreads();
    auto fix = [&](int pixel) -> int {
        if (P.rewriteA0 && c_alpha(pixel) == 0) pixel = P.transparentColor;         // load_pixel
        if (salSubst && c_alpha(pixel) <= 0xF) pixel = P.transparentColor;         // NQ/PnnLABQuantizer.java:141-145,156
        return pixel;
    };
    const long long stride = (long long) nblocks * blockDim.x, t0 = (long long) block * blockDim.x + threadIdx.x;
    for (long long g = t0; g < vec4; g += stride) {
        const int4 p = reinterpret_cast<const int4*>(pixels)[g];
        float4 r;
        r.x = saliency_lds(fix(p.x), gam); r.y = saliency_lds(fix(p.y), gam); r.z = saliency_lds(fix(p.z), gam); r.w = saliency_lds(fix(p.w), gam);
        reinterpret_cast<float4*>(out)[g] = r;
    }
    for (long long i = 4 * vec4 + t0; i < N; i += stride) out[i] = saliency_lds(fix(pixels[i]), gam);
}
__global__ void __launch_bounds__(256) saliency_kernel(DevParams P, int salSubst, const int* __restrict__ pixels, long long N,
                                                       float* __restrict__ out, long long vec4) {
    __shared__ double gam[256];
    saliency_body(P, salSubst, pixels, N, out, vec4, (int) blockIdx.x, (int) gridDim.x, gam);
}

// Both LAB builders -- and, when the caller has one to build, the saliency map of the image -- in ONE launch (round 4).  Each builder is
// 1024 wavefronts of dependent scans, one per SIMD, vector ALUs busy 11 / 16 % of the time (PMC); the saliency map is the opposite, a
// throughput pass with the vector ALUs busy 76 %; none of the three depends on another (the lists need the palette, the map the pixels).
// Side by side -- workgroups [0, 256) closest, [256, 512) nearest, [512, 512 + sal_blocks) saliency -- they overlap instead of following
// each other on the stream (38 + 28 + 47 us).
__global__ void __launch_bounds__(256) build_lab_lists_kernel(DevParams P, const int* __restrict__ g_palette, double wA, double wR, double wG,
                                                              double wB, int kstart, const float* __restrict__ box,
                                                              unsigned char* __restrict__ closest, unsigned char* __restrict__ closestCount,
                                                              unsigned char* __restrict__ nearest, unsigned char* __restrict__ nearestCount, SalJob sal,
                                                              void* packed, int* failed, float4* lab_table) {
    extern __shared__ __align__(16) unsigned char smem[];
    // packed (nullable): each builder also writes its half of the specialised kernels' records; failed (nullable): the hand-back count of
    // the dither kernel that follows on the stream starts at zero (one fill per image less), and the need count of its split form, the
    // word in front of it (launch_gilbert_fast, nq_kernels.h)
    if (failed && blockIdx.x == 0 && threadIdx.x == 0) { failed[-1] = 0; failed[0] = 0; }
    // lab_table (nullable): the palette's Lab as the dither kernels stage it -- getLab(palette[i]) (NQ/PnnLABQuantizer.java:352), zero from
    // entry K on -- once per image; the pixel-form light pass loads it instead of converting the palette in every workgroup (one closest-list
    // workgroup takes it: 256 threads, one entry each)
    if (lab_table && blockIdx.x == 255) {
        const Lab l2 = RGB2LAB((int) threadIdx.x < P.K ? g_palette[threadIdx.x] : 0);
        lab_table[threadIdx.x] = make_float4(l2.L, l2.A, l2.B, 0.f);
    }
    if (blockIdx.x < 256) closest_lists_body(P, g_palette, wA, wR, wG, wB, closest, closestCount, (int) blockIdx.x, packed);
    else if (blockIdx.x < 512) nearest_lists_body(P, g_palette, kstart, box, nearest, nearestCount, (int) blockIdx.x - 256, smem, packed);
    else saliency_body(P, sal.salSubst, sal.pixels, sal.N, sal.out, sal.vec4, (int) blockIdx.x - 512, sal.blocks, reinterpret_cast<double*>(smem));
}


// ditherPixel :125-185 up to (not including) its final `ditherable.nearestColorIndex(palette, c2, bidx)`: returns that c2, so that
// the caller has ONE inlined lookup site on its hot path (every inlined copy of the lookup is ~15 000 instructions).
// qcur = palette[qPixels[bidx]] as the reference reads it at this point.
__device__ __forceinline__ int ditherPixelColor(ChainCtx& cx, int x, int y, int c2, float beta, int pixel, float sal, int qcurIdx) {
    const DevParams& P = *cx.P;
    const GilbertConsts& G = *cx.G;
    const int K = P.K;
    const int bidx = x + y * cx.width;
    const double* __restrict__ gam = cx.lk.pal.gamma;
    const signed char* __restrict__ blue = cx.lk.pal.blue;
    const int qcur = cx.lk.pal.argb[qcurIdx];
    const int r_pix = c_red(c2), g_pix = c_green(c2), b_pix = c_blue(c2), a_pix = c_alpha(c2);
    const double weight = G.weightAbs;
    const float strength = 1 / 3.0f;
    const int acceptedDiff = max(2, K - G.margin);
    const double yPixel = color2Y_t(pixel, gam);                       // Y of `pixel`, shared by the Y_Diff(pixel, .) calls
    if (K <= 4 && sal > .2f && sal < .25f)
        c2 = blue_diffuse_t(pixel, qcur, beta * 2 / sal, strength, x, y, blue);
    else if (K <= 4 || Y_Diff_y(yPixel, color2Y_t(c2, gam)) < (2 * acceptedDiff)) {
        if (K > 64) {
            float kappa = sal < .6f ? beta * .15f / sal : beta * .4f / sal;
            c2 = blue_diffuse_t(pixel, qcur, kappa, strength, x, y, blue);
        }
        else if (K > 16 && weight < .005)
            c2 = blue_diffuse_t(pixel, qcur, beta * normalDistribution(sal, .5f) + beta, strength, x, y, blue);
        else
            c2 = blue_diffuse_t(pixel, qcur, beta * .5f / sal, strength, x, y, blue);
    }
    double gamma = (K <= 32 && weight < .01 && weight > .007) ? 1 - beta : beta;
    if (K > 4 && Y_Diff_y(yPixel, color2Y_t(c2, gam)) > (gamma * acceptedDiff)) {
        if (G.margin > 6 || gamma > beta) {
            float kappa = sal < .4f ? beta * .4f * sal : beta * .4f / sal;
            int c1 = c_argb(a_pix, r_pix, g_pix, b_pix);
            if (K > 32 && sal < .9)
                kappa = beta * normalDistribution(sal, 2.0f);
            else {
                if (weight >= .0015 && sal < .6) c1 = pixel;
                if (weight >= .005 && sal < .6)
                    kappa = beta * normalDistribution(sal, weight < .0008 ? 2.5f : 1.75f);
                else if (K >= 32 || Y_Diff_y(color2Y_t(c1, gam), color2Y_t(c2, gam)) > (gamma * NQ_PI * acceptedDiff)) {
                    double ub = 1 - K / 320.0;
                    if (sal > .15 && sal < ub)
                        kappa = beta * (!G.sortedByYDiff && weight < .0025 ? .55f : .5f) / sal;
                    else
                        kappa = beta * normalDistribution(sal, weight < .0025 ? 1.82f : 2.0f);
                }
            }
            c2 = blue_diffuse_t(c1, qcur, kappa, strength, x, y, blue);
        }
        else if (K <= 32 && weight >= .004)
            c2 = blue_diffuse_t(c2, qcur, beta * normalDistribution(sal, .25f), strength, x, y, blue);
        else
            c2 = c_argb(a_pix, r_pix, g_pix, b_pix);
    }
    if (G.DITHER_MAX < 16 && K > 4 && sal < .6f && Y_Diff_y(yPixel, color2Y_t(c2, gam)) > G.margin - 1)
        c2 = c_argb(a_pix, r_pix, g_pix, b_pix);
    if (K > 32 && sal > .95) {
        float kappa = beta * fmaxf(.05f, .75f - K / 128.0f) * sal;
        c2 = blue_diffuse_t(pixel, qcur, kappa, strength, x, y, blue);
    }
    (void) bidx;
    return c2;
}

// DM = DITHER_MAX of the non-sorted mode (9, 16 or 25): the ArrayDeque always holds exactly DM boxes (run() pre-fills it,
// every pixel polls one and adds one), kept in registers as a shift register rq[0] (oldest) .. rq[DM-1] (newest).
template <bool SORTED, int DM, class Q>
__device__ __forceinline__ int diffusePixel(ChainCtx& cx, Q& q, float (&rq)[DM][4], int x, int y) {
    const DevParams& P = *cx.P;
    const GilbertConsts& G = *cx.G;
    const int K = P.K;
    const int lidx = x + y * cx.width;                 // band-local: where the pixel and its saliency live
    const int bidx = lidx + cx.gofs;                   // bidx of the reference: position in the whole image
    const int pixel = load_pixel(P, cx.pixels, lidx);
    const bool hasSal = G.hasSaliencies != 0;
    const float sal = hasSal ? cx.saliency[lidx] : 0.0f;
    const int yg = y + cx.yorg;                        // image row (blue-noise phase)

    float e[4] = {(float) c_red(pixel), (float) c_green(pixel), (float) c_blue(pixel), (float) c_alpha(pixel)};
    float maxErr = (float) (G.DITHER_MAX - 1);
    if (!SORTED) {
        // ArrayDeque iteration oldest -> newest, weights[0..DM)
        // two channels per packed multiply / add (same two roundings per channel as `error.p[j] += eb.p[j] * weights[c]`); the
        // running maximum over all partial sums is order independent
        typedef float v2f __attribute__((ext_vector_type(2)));
        v2f e01 = {e[0], e[1]}, e23 = {e[2], e[3]};
#pragma unroll
        for (int t = 0; t < DM; ++t) {
            const float w = G.weights[t];
            const v2f p01 = (v2f){rq[t][0], rq[t][1]} * w, p23 = (v2f){rq[t][2], rq[t][3]} * w;
            e01 = e01 + p01; e23 = e23 + p23;
            maxErr = fmaxf(fmaxf(maxErr, e01.x), e01.y);
            maxErr = fmaxf(fmaxf(maxErr, e23.x), e23.y);
        }
        e[0] = e01.x; e[1] = e01.y; e[2] = e23.x; e[3] = e23.y;
    } else {
        // PriorityQueue iteration = array order, weights from the last one downwards
        int i = cx.nweights - 1;
        for (int t = 0; t < q.size; ++t) {
            if (i < 0 || i >= cx.nweights) break;
            const float w = cx.weights[i];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                e[j] += q.p(t, j) * w;
                if (e[j] > maxErr) maxErr = e[j];
            }
            --i;
        }
    }

    // (int) Math.min(BYTE_MAX, Math.max(error.p[j], 0.0)): the float clamp is identical (float -> double is exact, no NaN)
    const int r_pix = (int) fminf(255.0f, fmaxf(e[0], 0.0f));
    const int g_pix = (int) fminf(255.0f, fmaxf(e[1], 0.0f));
    const int b_pix = (int) fminf(255.0f, fmaxf(e[2], 0.0f));
    const int a_pix = (int) fminf(255.0f, fmaxf(e[3], 0.0f));

    int c2 = c_argb(a_pix, r_pix, g_pix, b_pix);
    int qidx = 0;                                   // qPixels[bidx] of the fresh array (:369)
    // :212-229: every branch starts with exactly one lookup; only the colour handed to it differs
    const bool branchA = hasSal && G.dither && !SORTED && (!G.hasAlphaW || c_alpha(pixel) < a_pix);
    const bool branchB = !branchA && K <= 32 && a_pix > 0xF0;
    int c_look = c2;
    if (branchA) {
        const bool direct = (K >= 256 && sal > .99f) || (G.hasAlphaW && (c_alpha(pixel) - a_pix) < (.5 * G.margin));
        if (!direct) c_look = ditherPixelColor(cx, x, yg, c2, G.beta, pixel, sal, qidx);
    }
    qidx = ditherable_lookup(cx.lk, c_look, bidx);
    if (branchB) {
        const int acceptedDiff = max(2, K - G.margin);
        if (hasSal && (Y_Diff_y(color2Y_t(pixel, cx.lk.pal.gamma), color2Y_t(c2, cx.lk.pal.gamma)) > acceptedDiff || U_Diff(pixel, c2) > (2 * acceptedDiff))) {
            const float strength = 1 / 3.0f;
            c2 = blue_diffuse_t(pixel, cx.lk.pal.argb[qidx], 1 / sal, strength, x, yg, cx.lk.pal.blue);
            qidx = ditherable_lookup(cx.lk, c2, bidx);
        }
    }

    // :231-234
    if (!SORTED) {
        // errorq.poll(): done together with errorq.add() below (shift register)
    } else {
        if (q.size >= G.DITHER_MAX) pq_poll(q);
        else if (q.size != 0) {
            // initWeights(size): size is 1, 3, 7 (growth 1 -> 3 -> 7 -> 15 >= DITHER_MAX = 9) or 15 (-> 31 >= DITHER_MAX = 25)
            const int size = q.size;
            cx.nweights = size;
            cx.weights = size == 1 ? G.w1 : size == 3 ? G.w3 : size == 7 ? G.w7 : G.w15;
            const float z[4] = {0.f, 0.f, 0.f, 0.f};
            for (int c = 0; c < size; ++c) pq_offer(q, z, 0.0);
        }
    }

    c2 = cx.lk.pal.argb[qidx];
    e[0] = (float) (r_pix - c_red(c2));
    e[1] = (float) (g_pix - c_green(c2));
    e[2] = (float) (b_pix - c_blue(c2));
    e[3] = (float) (a_pix - c_alpha(c2));

    const bool denoise = K > 2;
    const bool diffuse = cx.lk.pal.blue[bidx & 4095] > G.thresold;
    const double yDiff = SORTED ? Y_Diff_y(color2Y_t(pixel, cx.lk.pal.gamma), color2Y_t(c2, cx.lk.pal.gamma)) : 1;
    const bool illusion = !diffuse && cx.lk.pal.blue[j_d2i(yDiff * 4096) & 4095] > G.thresold;

    bool unaccepted = false;
    const int errLength = denoise ? 3 : 0;
    for (int j = 0; j < 3; ++j) {
        if (j >= errLength) break;
        if (fabsf(e[j]) >= G.ditherMax) {
            if (SORTED && hasSal) unaccepted = true;
            if (diffuse)
                e[j] = (float) tanh((double) (e[j] / maxErr * 20)) * (G.ditherMax - 1);
            else if (illusion)
                e[j] = (float) ((double) (e[j] / maxErr) * yDiff) * (G.ditherMax - 1);
            else
                e[j] /= (float) (1 + sqrt((double) G.ditherMax));
        }
        if (SORTED && !hasSal && fabsf(e[j]) >= G.DITHER_MAX) unaccepted = true;
    }

    if (unaccepted) {
        if (hasSal) qidx = ditherable_lookup(cx.lk, ditherPixelColor(cx, x, yg, c2, G.beta, pixel, sal, qidx), bidx);
        else if (Y_Diff_y(color2Y_t(pixel, cx.lk.pal.gamma), color2Y_t(c2, cx.lk.pal.gamma)) > 3 && U_Diff(pixel, c2) > 3) {
            const float strength = 1 / 3.0f;
            c2 = blue_diffuse_t(pixel, cx.lk.pal.argb[qidx], strength, strength, x, yg, cx.lk.pal.blue);
            qidx = ditherable_lookup(cx.lk, c2, bidx);
        }
    }

    // errorq.add(error) :276
    if (!SORTED) {
#pragma unroll
        for (int t = 0; t + 1 < DM; ++t) {
#pragma unroll
            for (int j = 0; j < 4; ++j) rq[t][j] = rq[t + 1][j];
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) rq[DM - 1][j] = e[j];
    } else {
        pq_offer(q, e, yDiff);
    }
    return qidx;
}

// STAGE: the tile's palette indices are kept in LDS ([position in tile][lane], one byte each) while the chain runs and the
// tile is written out row by row at the end -- per-step 4-byte stores scattered over 64 tiles left L2 as partial lines
// (measured: 640 MB written for 96 MB of output).  Needs K <= 256 and <= 256 pixels per tile.
template <bool SORTED, int DM, bool STAGE, bool LDSQ = false>
__global__ void __launch_bounds__(64) gilbert_kernel(DevParams P, GilbertConsts G, TileGeom T, CellLists lists,
                                                     const int* __restrict__ pixels, const float* __restrict__ saliency,
                                                     const int* __restrict__ g_palette,
                                                     short* binCache, long long seed, int sequential, long long* rng_out,
                                                     unsigned short* __restrict__ out_index, int* __restrict__ out_argb, SeqLog slog,
                                                     const int* __restrict__ tile_list) {
    extern __shared__ __align__(16) unsigned char smem[];
    if (tile_list && tile_list[0] <= 0) return;       // the specialised kernel handed nothing back (the usual case): no tables to stage
    PalView pal = stage_palette_tables(P, g_palette, smem);

    // tile_list (nullable): {count, tile indices...} written by gilbert_fast_kernel -- only those tiles are walked (grid-stride)
    const int ntiles = T.tiles_x * T.tiles_y;
    const int nwork = tile_list ? min(tile_list[0], ntiles) : ntiles;
    for (int work = blockIdx.x * blockDim.x + threadIdx.x; work < nwork; work += gridDim.x * blockDim.x) {
    const int tile = tile_list ? tile_list[1 + work] : work;
    const int ty = tile / T.tiles_x, tx = tile - ty * T.tiles_x;
    const int shape = (tx == T.tiles_x - 1 ? 1 : 0) | (ty == T.tiles_y - 1 ? 2 : 0);   // host fills all four tables
    const uint32_t* __restrict__ path = T.path[shape];
    const int steps = T.path_len[shape];
    const int x0 = tx * T.tile_w, y0 = ty * T.tile_h;

    ChainCtx cx;
    cx.P = &P; cx.G = &G;
    cx.lk.P = &P; cx.lk.pal = pal; cx.lk.binCache = sequential ? binCache : nullptr; cx.lk.dither = G.dither;
    cx.lk.lists = (lists.closest || lists.nearest) ? &lists : nullptr;
    cx.lk.slog = (!STAGE && sequential && slog.colors) ? &slog : nullptr;      // (never in the staged, tiled instantiations)
    // one java.util.Random per chain: Random(seed) for the single sequential chain, Random(mix64(seed + tile)) per tile
    cx.lk.rng = sequential ? jr_seed(seed) : jr_seed((long long) mix64((unsigned long long) seed + (unsigned long long) (T.tile_base + tile)));
    cx.pixels = pixels; cx.saliency = saliency; cx.width = T.width; cx.gofs = T.y_origin * T.width; cx.yorg = T.y_origin;

    ErrQueueT<LDSQ> q;
    q.head = 0; q.size = 0;
    // (LDSQ: the queue area lies behind the palette tables and the index staging; one column per lane)
    q.bind(reinterpret_cast<unsigned*>(smem + ((palette_tables_smem_bytes(P.kind, P.K) + (STAGE ? (size_t) 64 * T.tile_w * T.tile_h : 0) + 15) & ~(size_t) 15)) + threadIdx.x);
    float rq[DM][4];
#pragma unroll
    for (int t = 0; t < DM; ++t) { rq[t][0] = rq[t][1] = rq[t][2] = rq[t][3] = 0.f; }   // run(): initWeights(DITHER_MAX) zero boxes
    cx.weights = G.w1; cx.nweights = 0;
    if (SORTED && !sequential) {
        // A TILE chain of the sorted-by-yDiff mode starts with its queue in the steady state: the growth 1 -> 3 -> 7 -> 15 (-> 31) of
        // NQ/GilbertCurve.java:231-234 run with zero boxes in place of the first pixels' errors.  The reference grows the queue once per
        // image; restarting the growth at every tile put its erratic first steps (one or three weights) at every tile start -- pixels
        // with deltaE > 40 on few-colour noise images, which is why round 2 kept 64x64 tiles for this mode.  With the steady-state start
        // they are gone at every tile size (oracle: gilbert_run, tile_chain) and the mode takes the ordinary tile rule.
        const float z[4] = {0.f, 0.f, 0.f, 0.f};
        pq_offer(q, z, 0.0);
        while (q.size < G.DITHER_MAX) {
            const int size = q.size;
            cx.nweights = size;
            cx.weights = size == 1 ? G.w1 : size == 3 ? G.w3 : size == 7 ? G.w7 : G.w15;
            for (int c = 0; c < size; ++c) pq_offer(q, z, 0.0);
            pq_offer(q, z, 0.0);
        }
    }

    unsigned char* stage = smem + palette_tables_smem_bytes(P.kind, P.K);
    for (int s = 0; s < steps; ++s) {
        const uint32_t d = path[s];
        const int dx = (int) (d & 0xFFFFu), dy = (int) (d >> 16);
        const int x = x0 + dx, y = y0 + dy;
        const int k = diffusePixel<SORTED, DM>(cx, q, rq, x, y);      // (Q deduced)
        if (STAGE) stage[(dy * T.tile_w + dx) * 64 + threadIdx.x] = (unsigned char) k;
        else {
            const int bidx = x + y * T.width;
            out_index[bidx] = (unsigned short) k;
            if (out_argb) out_argb[bidx] = pal.argb[k];
        }
    }
    if (STAGE) {
        // row-major write-out: at every iteration the 64 lanes (64 horizontally adjacent tiles) write one 4-byte word each of the
        // same image row, tile_w*4 bytes apart, and the next iteration fills the neighbouring word
        const int tw = T.shape_w[shape], th = T.shape_h[shape];
        for (int r = 0; r < T.tile_h; ++r) {
            for (int c = 0; c < T.tile_w; ++c) {
                if (r < th && c < tw) {
                    const int k = stage[(r * T.tile_w + c) * 64 + threadIdx.x];
                    const int bidx = (x0 + c) + (y0 + r) * T.width;
                    out_index[bidx] = (unsigned short) k;
                    if (out_argb) out_argb[bidx] = pal.argb[k];
                }
            }
        }
    }
    if (sequential && rng_out) *rng_out = cx.lk.rng;
    }
}

// ------------------------------------------------------------------------------------------------
// BlueNoise.dither (NQ/BlueNoise.java:207-222)
// ------------------------------------------------------------------------------------------------
// parallel form: every pixel is independent apart from the RNG stream -> one Random(mix64(seed ^ tag + bidx)) each
__global__ void __launch_bounds__(256) bluenoise_kernel(DevParams P, const int* __restrict__ g_palette, CellLists lists,
                                                        const int* __restrict__ pixels, int width, int height, int y_origin, float weight,
                                                        long long seed, unsigned short* __restrict__ io_index,
                                                        int* __restrict__ out_argb) {
    extern __shared__ __align__(16) unsigned char smem[];
    PalView pal = stage_palette_tables(P, g_palette, smem);
    const long long N = (long long) width * height;
    const float strength = 1 / 3.0f;
    LookupCtx lk; lk.P = &P; lk.pal = pal; lk.binCache = nullptr; lk.dither = 0;
    lk.lists = (lists.closest || lists.nearest) ? &lists : nullptr;
    for (long long i = (long long) blockIdx.x * blockDim.x + threadIdx.x; i < N; i += (long long) gridDim.x * blockDim.x) {
        const int y = (int) (i / width), x = (int) (i - (long long) y * width);
        const long long gi = i + (long long) y_origin * width;          // position in the whole image (band runs: SURVEY 8e)
        const int pixel = load_pixel(P, pixels, i);
        const int qPixel = pal.argb[io_index[i]];
        const int c1 = blue_diffuse_t(pixel, qPixel, weight, strength, x, y + y_origin, pal.blue);
        lk.rng = jr_seed((long long) mix64(((unsigned long long) seed ^ 0xB10E5EEDULL) + (unsigned long long) gi));
        const int k = ditherable_lookup(lk, c1, (int) gi);
        io_index[i] = (unsigned short) k;
        out_argb[i] = pal.argb[k];
    }
}
// sequential form (REFERENCE_SEQUENTIAL): one lane, row-major, continuing the chain's Random and bin cache
__global__ void __launch_bounds__(64) bluenoise_seq_kernel(DevParams P, const int* __restrict__ g_palette, CellLists lists,
                                                           const int* __restrict__ pixels, int width, int height, float weight,
                                                           short* binCache, long long* rng_io,
                                                           unsigned short* __restrict__ io_index, int* __restrict__ out_argb) {
    extern __shared__ __align__(16) unsigned char smem[];
    PalView pal = stage_palette(P, g_palette, smem);
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    const float strength = 1 / 3.0f;
    LookupCtx lk; lk.P = &P; lk.pal = pal; lk.binCache = binCache; lk.dither = 0; lk.rng = *rng_io;
    lk.lists = (lists.closest || lists.nearest) ? &lists : nullptr;
    for (int y = 0; y < height; ++y)
        for (int x = 0; x < width; ++x) {
            const int bidx = x + y * width;
            const int c1 = blue_diffuse(load_pixel(P, pixels, bidx), pal.argb[io_index[bidx]], weight, strength, x, y);
            const int k = ditherable_lookup(lk, c1, bidx);
            io_index[bidx] = (unsigned short) k;
            out_argb[bidx] = pal.argb[k];
        }
    *rng_io = lk.rng;
}

} // namespace nq
