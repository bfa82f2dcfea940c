// nq_palette.inc -- pnnquan on the GPU: alpha pre-scan, 65536-bin histogram, find_nn, heap-driven merge loop,
// palette fill.  Included by nq_kernels.hip (single translation unit).
//
// Exactness notes (DESIGN.md "palette build"):
//  * LAB bin sums are float32 running sums in pixel order (NQ/PnnLABQuantizer.java:150-154) -> the pixels are
//    stably sorted by bin (rocPRIM radix sort, plumbing) and each bin is summed in order by one wavefront.
//  * find_nn's early-outs are semantics, not optimisation (R_T can be negative, NQ/CIELABConvertor.java:192-193):
//    a wavefront evaluates 64 candidates at once against the running error and then resolves accept/reject in
//    candidate order with ballots -- identical to the sequential scan.
//  * the merge loop is one persistent workgroup: lane 0 owns the heap, all 16 wavefronts scan for find_nn.

namespace nq {

// ------------------------------------------------------------------------------------------------
// S1: alpha pre-scan (NQ/PnnQuantizer.java:410-431)
// scan3 = {max global index with alpha == 0 (init -1), colour at that index (filled by a second tiny kernel), count of
//          pixels with 0xF < alpha < 0xE0}
// ------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) prescan_kernel(const int* __restrict__ pixels, long long n, long long index_offset,
                                                      long long* __restrict__ scan3) {
    long long maxIdx = -1, semi = 0;
    for (long long i = (long long) blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long) gridDim.x * blockDim.x) {
        const int alfa = c_alpha(pixels[i]);
        if (alfa < 0xE0) {
            if (alfa == 0) maxIdx = i + index_offset;       // ascending i per thread: the last one wins
            else if (alfa > 0xF) ++semi;
        }
    }
    // wavefront reduction, then one atomic per wavefront
    for (int off = 32; off > 0; off >>= 1) {
        long long o = __shfl_down(maxIdx, off, 64); if (o > maxIdx) maxIdx = o;
        semi += __shfl_down(semi, off, 64);
    }
    if ((threadIdx.x & 63) == 0) {
        if (maxIdx >= 0) atomicMax((long long*) &scan3[0], maxIdx);
        if (semi) atomicAdd((unsigned long long*) &scan3[2], (unsigned long long) semi);
    }
}
__device__ __forceinline__ unsigned pack_bin_pixel(int c, int keyfmt);         // (defined with the histogram below)
// The pre-scan and the histogram's sort words in ONE read of the image, for the common configuration (no alpha == 0 pixel, nothing
// semi-transparent, nMaxColors >= 64: 5-6-5 keys, pixels with alpha <= 15 read as the default m_transparentColor).  Which configuration
// the image has is only known once the scan is complete, so the words are written speculatively: the caller uses them when scan3 says
// the image is of that kind and runs bin_keys_kernel otherwise.  Four pixels per lane (16-byte accesses).
// occ_zero (nullable): the two counters occupied_bins_kernel adds to later on this stream are cleared here (one fill per image less).
__global__ void __launch_bounds__(256) front_kernel(const int4* __restrict__ pixels4, long long n4, long long index_offset,
                                                    long long* __restrict__ scan3, uint4* __restrict__ packed4, int defaultTransparent,
                                                    unsigned* __restrict__ occ_zero) {
    if (occ_zero && blockIdx.x == 0 && threadIdx.x == 0) { occ_zero[0] = 0u; occ_zero[1] = 0u; }
    long long maxIdx = -1, semi = 0;
    for (long long i = (long long) blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (long long) gridDim.x * blockDim.x) {
        const int4 v = pixels4[i];
        const int px[4] = {v.x, v.y, v.z, v.w};
        unsigned w[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int alfa = c_alpha(px[k]);
            if (alfa < 0xE0) {
                if (alfa == 0) maxIdx = 4 * i + k + index_offset;
                else if (alfa > 0xF) ++semi;
            }
            w[k] = pack_bin_pixel(alfa <= 0xF ? defaultTransparent : px[k], 0);
        }
        packed4[i] = make_uint4(w[0], w[1], w[2], w[3]);
    }
    for (int off = 32; off > 0; off >>= 1) {
        long long o = __shfl_down(maxIdx, off, 64); if (o > maxIdx) maxIdx = o;
        semi += __shfl_down(semi, off, 64);
    }
    if ((threadIdx.x & 63) == 0) {
        if (maxIdx >= 0) atomicMax((long long*) &scan3[0], maxIdx);
        if (semi) atomicAdd((unsigned long long*) &scan3[2], (unsigned long long) semi);
    }
}
// (runs behind the scan kernel; the scan's three words start as ONE fill with 0xFF -- {-1, -1, -1} -- so the count of [2], which the
// scan only ever adds to, is put right here: one buffer fill per image instead of two)
__global__ void prescan_color_kernel(const int* __restrict__ pixels, long long n, long long index_offset, long long* scan3) {
    const long long idx = scan3[0] - index_offset;
    scan3[1] = (idx >= 0 && idx < n) ? (long long) (unsigned) pixels[idx] : -1;
    scan3[2] += 1;
}

// ------------------------------------------------------------------------------------------------
// P1-P3: histogram
// ------------------------------------------------------------------------------------------------
// HistParams (nq_kernels.h): hasSemi = hasSemiTransparency; hasTransp = nMaxColors < 64 || m_transparentPixelIndex >= 0
// (:144); transparentColor = m_transparentColor

// One 32-bit word per pixel: the histogram bin in the upper half, the pixel's remaining 16 bits in the lower half -- getColorIndex
// takes 16 of the pixel's 32 bits, so (bin, rest) is a bijection of the pixel as the histogram sees it (alpha <= alphaThreshold ->
// m_transparentColor, :141-142).  A keys-only radix sort over bits [16, 32) then moves 4 bytes per pixel instead of a 2-byte key and a
// 4-byte value, and stays stable (pixel order inside a bin).  keyfmt: 0 = 5-6-5, 1 = 1-5-5-5, 2 = 4-4-4-4 (getColorIndex's three forms).
__device__ __forceinline__ unsigned pack_bin_pixel(int c, int keyfmt) {
    const unsigned a = (unsigned) c_alpha(c), r = (unsigned) c_red(c), g = (unsigned) c_green(c), b = (unsigned) c_blue(c);
    if (keyfmt == 2)
        return ((a & 0xF0) << 24) | ((r & 0xF0) << 20) | ((g & 0xF0) << 16) | ((b >> 4) << 16) | ((a & 0xF) << 12) | ((r & 0xF) << 8) | ((g & 0xF) << 4) | (b & 0xF);
    if (keyfmt == 1)
        return ((a & 0x80) << 24) | ((r & 0xF8) << 23) | ((g & 0xF8) << 18) | ((b >> 3) << 16) | ((a & 0x7F) << 9) | ((r & 7) << 6) | ((g & 7) << 3) | (b & 7);
    return ((r & 0xF8) << 24) | ((g & 0xFC) << 19) | ((b >> 3) << 16) | (a << 8) | ((r & 7) << 5) | ((g & 3) << 3) | (b & 7);
}
__device__ __forceinline__ int unpack_bin_pixel(unsigned w, int keyfmt) {
    unsigned a, r, g, b;
    if (keyfmt == 2) {
        a = ((w >> 24) & 0xF0) | ((w >> 12) & 0xF); r = ((w >> 20) & 0xF0) | ((w >> 8) & 0xF);
        g = ((w >> 16) & 0xF0) | ((w >> 4) & 0xF); b = ((w >> 12) & 0xF0) | (w & 0xF);
    } else if (keyfmt == 1) {
        a = ((w >> 24) & 0x80) | ((w >> 9) & 0x7F); r = ((w >> 23) & 0xF8) | ((w >> 6) & 7);
        g = ((w >> 18) & 0xF8) | ((w >> 3) & 7); b = ((w >> 13) & 0xF8) | (w & 7);
    } else {
        a = (w >> 8) & 0xFF; r = ((w >> 24) & 0xF8) | ((w >> 5) & 7);
        g = ((w >> 19) & 0xFC) | ((w >> 3) & 3); b = ((w >> 13) & 0xF8) | (w & 7);
    }
    return c_argb((int) a, (int) r, (int) g, (int) b);
}
__global__ void __launch_bounds__(256) bin_keys_kernel(const int* __restrict__ pixels, long long n, HistParams hp, unsigned* __restrict__ packed,
                                                       unsigned* __restrict__ occ_zero /* occupied_bins_kernel's two counters: cleared here */) {
    if (blockIdx.x == 0 && threadIdx.x == 0) { occ_zero[0] = 0u; occ_zero[1] = 0u; }
    const int keyfmt = hp.hasSemi ? 2 : hp.hasTransp ? 1 : 0;
    for (long long i = (long long) blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long) gridDim.x * blockDim.x) {
        int pixel = pixels[i];
        if (c_alpha(pixel) <= 0xF) pixel = hp.transparentColor;
        packed[i] = pack_bin_pixel(pixel, keyfmt);
    }
}

// ---- distinct colours of the image as the histogram sees it = keys of the reference's pixelMap right after the histogram
// (NQ/PnnLABQuantizer.java:145,193): colours are radix-sorted (stable, value = pixel index), run heads counted / collected ----
__global__ void __launch_bounds__(256) subst_colors_kernel(const int* __restrict__ pixels, long long n, int transparentColor,
                                                           unsigned* __restrict__ keys, unsigned* __restrict__ idx) {
    for (long long i = (long long) blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long) gridDim.x * blockDim.x) {
        int pixel = pixels[i];
        if (c_alpha(pixel) <= 0xF) pixel = transparentColor;
        keys[i] = (unsigned) pixel;
        if (idx) idx[i] = (unsigned) i;
    }
}
// ---- the same per-pixel passes over a SEQUENCE of frames read in place (nq_pnnquan_frames_device): pixel i of frame f has the global
// index frames[f].offset + i, the index of that pixel in the concatenation of the frames, and every output word sits at that global
// index -- what the single-image kernels above compute for a concatenated copy, without the copy.  The work list holds (frame, chunk)
// items of at most NQ_FRAME_CHUNK pixels that never cross a frame boundary; one workgroup takes an item at a time.  Frames may have odd
// pixel counts and 4-byte-aligned pointers: an item reads its pixels as 16-byte loads from the first 16-byte boundary of the SOURCE on
// (head and tail pixels one by one), and stores a group of four words as one 16-byte store only where the destination is aligned too.
// OP: FRAMES_SCAN = pre-scan (prescan_kernel), FRAMES_FRONT = pre-scan + speculative 5-6-5 words (front_kernel), FRAMES_KEYS = sort
// words with the histogram's keys (bin_keys_kernel), FRAMES_SUBST = substituted colours + global index (subst_colors_kernel).
template <int OP>
__global__ void __launch_bounds__(256) frames_kernel(const FrameDesc* __restrict__ frames, const FrameChunk* __restrict__ items, int n_items,
                                                     long long* __restrict__ scan3, unsigned* __restrict__ words, unsigned* __restrict__ idx,
                                                     int color, int keyfmt) {
    constexpr bool SCAN = OP == FRAMES_SCAN || OP == FRAMES_FRONT, STORE = OP != FRAMES_SCAN;
    long long maxIdx = -1, semi = 0;
    // one pixel at global index g: the scan's counters, the word written at g
    auto word_of = [&](int px, long long g) -> unsigned {
        const int alfa = c_alpha(px);
        if (SCAN && alfa < 0xE0) {
            if (alfa == 0) maxIdx = max(maxIdx, g);
            else if (alfa > 0xF) ++semi;
        }
        if (OP == FRAMES_SCAN) return 0u;
        if (OP == FRAMES_SUBST) return (unsigned) (alfa <= 0xF ? color : px);
        return pack_bin_pixel(alfa <= 0xF ? color : px, OP == FRAMES_FRONT ? 0 : keyfmt);
    };
    auto put = [&](long long g, unsigned w) {
        if (!STORE) return;
        words[g] = w;
        if (OP == FRAMES_SUBST && idx) idx[g] = (unsigned) g;
    };
    for (int it = blockIdx.x; it < n_items; it += gridDim.x) {
        const FrameChunk c = items[it];
        const int* __restrict__ p = frames[c.frame].pixels + c.begin;
        const long long g0 = frames[c.frame].offset + c.begin;
        const int count = c.count;
        int head = count;                              // (a pointer that is not 4-byte aligned: every pixel one by one)
        if (!((uintptr_t) p & 3)) head = min(count, (int) (((16u - ((unsigned) (uintptr_t) p & 15u)) & 15u) >> 2));
        const int body4 = (count - head) >> 2, tail0 = head + 4 * body4;
        const bool vstore = STORE && !(((uintptr_t) (words + g0 + head)) & 15) && (OP != FRAMES_SUBST || !idx || !(((uintptr_t) (idx + g0 + head)) & 15));
        for (int t = threadIdx.x; t < head; t += blockDim.x) put(g0 + t, word_of(p[t], g0 + t));
        const int4* __restrict__ p4 = reinterpret_cast<const int4*>(p + head);
        for (int j = threadIdx.x; j < body4; j += blockDim.x) {
            const int4 v = p4[j];
            const long long g = g0 + head + 4LL * j;
            const unsigned w0 = word_of(v.x, g), w1 = word_of(v.y, g + 1), w2 = word_of(v.z, g + 2), w3 = word_of(v.w, g + 3);
            if (!STORE) continue;
            if (vstore) {
                reinterpret_cast<uint4*>(words + g)[0] = make_uint4(w0, w1, w2, w3);
                if (OP == FRAMES_SUBST && idx)
                    reinterpret_cast<uint4*>(idx + g)[0] = make_uint4((unsigned) g, (unsigned) g + 1u, (unsigned) g + 2u, (unsigned) g + 3u);
            } else {
                put(g, w0); put(g + 1, w1); put(g + 2, w2); put(g + 3, w3);
            }
        }
        for (int t = tail0 + threadIdx.x; t < count; t += blockDim.x) put(g0 + t, word_of(p[t], g0 + t));
    }
    if (!SCAN) return;
    for (int off = 32; off > 0; off >>= 1) {
        long long o = __shfl_down(maxIdx, off, 64); if (o > maxIdx) maxIdx = o;
        semi += __shfl_down(semi, off, 64);
    }
    if ((threadIdx.x & 63) == 0) {
        if (maxIdx >= 0) atomicMax((long long*) &scan3[0], maxIdx);
        if (semi) atomicAdd((unsigned long long*) &scan3[2], (unsigned long long) semi);
    }
}
// prescan_color_kernel of a frame sequence: the colour at the winning GLOBAL index, read from the frame that holds it
__global__ void frames_prescan_color_kernel(const FrameDesc* __restrict__ frames, int n_frames, long long* scan3) {
    const long long idx = scan3[0];
    long long c = -1;
    if (idx >= 0) {
        int lo = 0, hi = n_frames - 1;                 // last frame whose offset <= idx
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (frames[mid].offset <= idx) lo = mid; else hi = mid - 1;
        }
        const long long i = idx - frames[lo].offset;
        if (i >= 0 && i < frames[lo].n) c = (long long) (unsigned) frames[lo].pixels[i];
    }
    scan3[1] = c;
    scan3[2] += 1;
}

// Which colours does a band hold (after the histogram's alpha substitution)?  Opaque colours set their byte of a 2^24-byte table
// (bands of one image combine by byte-wise MAX, SURVEY 8e item 3), the others go into an open-addressing set of `slots` words
// (0xFFFFFFFF = empty: no non-opaque colour has that value); counters[0] = set entries, counters[1] = 1 when the set overflowed.
__global__ void __launch_bounds__(256) color_presence_kernel(const int* __restrict__ pixels, long long n, int transparentColor,
                                                             unsigned char* __restrict__ bytes, unsigned* __restrict__ set, unsigned slots,
                                                             unsigned* __restrict__ counters) {
    for (long long i = (long long) blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long) gridDim.x * blockDim.x) {
        int pixel = pixels[i];
        if (c_alpha(pixel) <= 0xF) pixel = transparentColor;
        const unsigned c = (unsigned) pixel;
        if ((c >> 24) == 0xFFu) { if (!bytes[c & 0xFFFFFFu]) bytes[c & 0xFFFFFFu] = 1; continue; }
        unsigned hsh = (c * 0x9E3779B1u) >> 8;
        bool done = false;
        for (unsigned probe = 0; probe < 64 && !done; ++probe) {
            const unsigned slot = (hsh + probe) & (slots - 1);
            const unsigned old = atomicCAS(&set[slot], 0xFFFFFFFFu, c);
            if (old == 0xFFFFFFFFu) { atomicAdd(&counters[0], 1u); done = true; }
            else if (old == c) done = true;
        }
        if (!done) counters[1] = 1;
    }
}
// out[0] = number of runs; when `heads` != nullptr the first `cap` run heads are stored as {colour, first pixel index}
__global__ void __launch_bounds__(256) count_runs_kernel(const unsigned* __restrict__ keys, const unsigned* __restrict__ idx, long long n,
                                                         unsigned long long* __restrict__ out, uint2* __restrict__ heads, unsigned cap) {
    unsigned long long local = 0;
    for (long long i = (long long) blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long) gridDim.x * blockDim.x) {
        if (i == 0 || keys[i - 1] != keys[i]) {
            if (heads) {
                const unsigned long long slot = atomicAdd(out + 1, 1ULL);
                if (slot < cap) heads[slot] = make_uint2(keys[i], idx ? idx[i] : 0u);
            }
            ++local;
        }
    }
    for (int off = 32; off > 0; off >>= 1) local += __shfl_down(local, off, 64);
    if ((threadIdx.x & 63) == 0 && local) atomicAdd(out, local);
}

// Segment [start, end) of every bin in the bin-sorted words (bin = upper half) and the list of the occupied bins (order: by 1024-bin
// group as the groups' atomics land, ascending inside a group): the histogram kernel visits only those -- a third of the 65 536 on the
// bench image -- so that every resident workgroup has four busy wavefronts.  64 workgroups x 1024 bins, one thread per bin: its segment
// starts at the first word whose bin is not smaller (a binary search over the sorted words: 24 dependent loads, all bins side by side
// -- the pass over all n words that used to mark the run boundaries, and the clear of the two arrays in front of it, are gone) and
// ends where the next bin's starts.  ONE atomic per workgroup.  The histogram records of the EMPTY bins are zeroed here (the histogram
// kernel never sees them): no 2.6 MB clear per image.
__device__ __forceinline__ unsigned first_word_of_bin(const unsigned* __restrict__ packed, unsigned n, unsigned bin) {
    unsigned lo = 0, hi = n;                        // first i in [0, n] with (packed[i] >> 16) >= bin
    while (lo < hi) {
        const unsigned mid = lo + ((hi - lo) >> 1);
        if ((packed[mid] >> 16) < bin) lo = mid + 1; else hi = mid;
    }
    return lo;
}
// Bins of fat_min pixels and more ("fat": a flat area of a photograph, a 2^24-pixel test image) are listed a second time, behind
// occ_count[1] in fat_list: the RGB histogram gives each of them a whole workgroup (below).  fat_min > n / NQ_FAT_CAP, so the list
// cannot overflow; 0xFFFFFFFF (the LAB kind): no such bin.
#define NQ_FAT_WGS 64
#define NQ_FAT_CAP 1024
__global__ void __launch_bounds__(1024) occupied_bins_kernel(const unsigned* __restrict__ packed, unsigned n,
                                                             unsigned* __restrict__ seg_start, unsigned* __restrict__ seg_end,
                                                             unsigned* __restrict__ occ_count, unsigned* __restrict__ occ_list,
                                                             double* __restrict__ hist, unsigned fat_min, unsigned* __restrict__ fat_list) {
    __shared__ unsigned wcount[16];
    __shared__ unsigned base;
    __shared__ unsigned first[1025];
    const int bin = blockIdx.x * 1024 + threadIdx.x, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    first[threadIdx.x] = first_word_of_bin(packed, n, (unsigned) bin);
    if (threadIdx.x == 0) first[1024] = bin + 1024 >= 65536 ? n : first_word_of_bin(packed, n, (unsigned) bin + 1024u);
    __syncthreads();
    const unsigned s0 = first[threadIdx.x], e0 = first[threadIdx.x + 1];
    seg_start[bin] = s0; seg_end[bin] = e0;
    const bool occ = e0 > s0;
    const unsigned long long m = __ballot(occ);
    if (lane == 0) wcount[wave] = (unsigned) __popcll(m);
    __syncthreads();
    unsigned before = 0, total = 0;
    for (int w = 0; w < 16; ++w) { const unsigned c = wcount[w]; total += c; if (w < wave) before += c; }
    if (threadIdx.x == 0) base = total ? atomicAdd(occ_count, total) : 0u;
    __syncthreads();
    if (occ) occ_list[base + before + (unsigned) __popcll(m & ((1ULL << lane) - 1ULL))] = (unsigned) bin;
    else for (int k = 0; k < 5; ++k) hist[(size_t) bin * 5 + k] = 0.0;
    if (occ && e0 - s0 >= fat_min) {
        const unsigned slot = atomicAdd(occ_count + 1, 1u);
        if (slot < NQ_FAT_CAP) fat_list[slot] = (unsigned) bin;
    }
}

// one wavefront per bin; hist[bin][5] = {count, sum0..sum3}
// LAB: float32 running sums of alpha, L, A, B in pixel order (sequential adds; 64 Lab conversions in parallel)
// RGB: exact integer sums of a, r, g, b
// LAB, keyfmt 0 (5-6-5 keys) / 1 (1-5-5-5 keys): a bin holds at most 256 / 512 distinct opaque colours, so a bin with many pixels
// converts each possible colour ONCE into a per-wavefront table (dynamic LDS: 4 x entries float4) and its opaque pixels look their
// Lab up (same function, same argument: same floats); keyfmt 2 (4-4-4-4 keys) converts every pixel.
// Fat bins of the RGB kind (>= fat_min pixels; hist_fat_rgb_kernel, NQ_FAT_WGS workgroups that take them from fat_list, in front of
// hist_segments_kernel): exact integer sums, so all 256 threads of a workgroup stride over the bin (one wavefront per bin needed 4.5 ms
// for the 1.7 M pixels of a photograph's fullest bin, this 1.5 with everything else).
// The LAB kind has no such kernel, on purpose.  Built and measured: a workgroup per fat bin whose wavefronts 1..3 convert and park chunk
// after chunk into an LDS ring while wavefront 0 does nothing but read its rows and add in pixel order -- 7.56 ms for the same bin, exactly
// what the one-wavefront form needs: the chain is 1.7 M DEPENDENT float32 adds per channel at ~10 cycles each (the issue-to-result latency
// of v_add_f32 with a single wavefront on the SIMD), i.e. ~640 cycles per 64-pixel chunk whatever happens around them; conversion and
// parking were already hidden.  Only a different summation order could be faster, and the order is the reference's (SURVEY fact 5).
__global__ void __launch_bounds__(256) hist_fat_rgb_kernel(const unsigned* __restrict__ vals, const unsigned* __restrict__ seg_start,
                                                           const unsigned* __restrict__ seg_end, double* __restrict__ hist, int keyfmt,
                                                           const unsigned* __restrict__ occ_count, const unsigned* __restrict__ fat_list) {
    __shared__ unsigned long long part[4][4];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const unsigned nfat = min(occ_count[1], (unsigned) NQ_FAT_CAP);
    for (unsigned f = blockIdx.x; f < nfat; f += NQ_FAT_WGS) {          // (uniform over the workgroup; usually no fat bin at all)
        const int bin = (int) fat_list[f];
        const unsigned s = seg_start[bin], e = seg_end[bin];
        unsigned long long sa = 0, sr = 0, sg = 0, sb = 0;
        for (unsigned long long i = (unsigned long long) s + tid; i < e; i += 256) {
            const int c = unpack_bin_pixel(vals[i], keyfmt);
            sa += c_alpha(c); sr += c_red(c); sg += c_green(c); sb += c_blue(c);
        }
        for (int off = 32; off > 0; off >>= 1) {
            sa += __shfl_down(sa, off, 64); sr += __shfl_down(sr, off, 64);
            sg += __shfl_down(sg, off, 64); sb += __shfl_down(sb, off, 64);
        }
        __syncthreads();                               // (the bin before this one has been read out of `part`)
        if (lane == 0) { part[wave][0] = sa; part[wave][1] = sr; part[wave][2] = sg; part[wave][3] = sb; }
        __syncthreads();
        if (tid == 0) {
            double* out = hist + (size_t) bin * 5;
            out[0] = (double) (e - s);
            for (int k = 0; k < 4; ++k) out[1 + k] = (double) (part[0][k] + part[1][k] + part[2][k] + part[3][k]);
        }
    }
}
template <int KIND>
__global__ void __launch_bounds__(256) hist_segments_kernel(const unsigned* __restrict__ vals, const unsigned* __restrict__ seg_start,
                                                            const unsigned* __restrict__ seg_end, double* __restrict__ hist, int keyfmt,
                                                            const unsigned* __restrict__ occ_count, const unsigned* __restrict__ occ_list,
                                                            unsigned fat_min) {
    extern __shared__ __align__(16) unsigned char hist_dyn[];
    __shared__ double gamma[256];
    if (KIND == 1) {
        gamma[threadIdx.x] = g_tab.gamma[threadIdx.x];
        __syncthreads();                               // (before any wavefront can leave)
    }
    const unsigned slot = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (slot >= *occ_count) return;                    // (the empty bins were zeroed by occupied_bins_kernel)
    const int bin = (int) occ_list[slot];
    const unsigned s = seg_start[bin], e = seg_end[bin];
    double* out = hist + (size_t) bin * 5;
    if (s >= e || e - s >= fat_min) return;            // (fat, RGB kind only: hist_fat_rgb_kernel has it; LAB passes no limit)
    if (KIND == 1) {
        // 64 Lab conversions in parallel, parked in LDS; then lane c (c < 4) alone runs channel c's chain
        // tb.ac += lab1.alpha; ... in pixel order (a float32 running sum is order dependent, SURVEY fact 5): 64 dependent adds
        // per chunk instead of 64 x 4 broadcast+add steps executed by the whole wavefront
        // (channel-major, rows padded to 68 floats: lane c reads its 64 values as 16 conflict-free 16-byte loads -- the chain of the
        // fullest bin is this kernel's tail, and its speed is instructions per pixel of the four working lanes)
        __shared__ __align__(16) float park[4][4][68];
        float (*mine)[68] = park[threadIdx.x >> 6];
        float acc = 0.f;
        const int entries = keyfmt == 0 ? 256 : 512;
        float4* table = reinterpret_cast<float4*>(hist_dyn) + (size_t) (threadIdx.x >> 6) * entries;
        const bool tabled = keyfmt < 2 && (e - s) >= 2u * (unsigned) entries;
        if (tabled) {
            for (int t = lane; t < entries; t += 64) {
                int c;
                if (keyfmt == 0) c = c_argb(255, ((bin >> 11) << 3) | (t >> 5), (((bin >> 5) & 63) << 2) | ((t >> 3) & 3), ((bin & 31) << 3) | (t & 7));
                else c = c_argb(255, (((bin >> 10) & 31) << 3) | (t >> 6), (((bin >> 5) & 31) << 3) | ((t >> 3) & 7), ((bin & 31) << 3) | (t & 7));
                const Lab l = RGB2LAB_fast(c, gamma);
                table[t] = make_float4(l.alpha, l.L, l.A, l.B);
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        }
        // The chain of the fullest bin is this kernel's tail, so nothing may wait inside it: the sort words are requested 256 pixels
        // (four chunks) ahead, in two register sets that take turns (no copies: a copy of a word still in flight would wait for it).
        auto chunk = [&](unsigned word, unsigned base) {
            const unsigned i = base + lane;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (i < e) {
                const int c = unpack_bin_pixel(word, keyfmt);
                if (tabled && c_alpha(c) == 255) {
                    const int t = keyfmt == 0 ? ((c_red(c) & 7) << 5) | ((c_green(c) & 3) << 3) | (c_blue(c) & 7)
                                              : ((c_red(c) & 7) << 6) | ((c_green(c) & 7) << 3) | (c_blue(c) & 7);
                    v = table[t];
                } else {
                    const Lab lab = RGB2LAB_fast(c, gamma);     // cube root <= 0.72 ulp in f64, narrowed to float (nq_device.h)
                    v = make_float4(lab.alpha, lab.L, lab.A, lab.B);
                }
            }
            mine[0][lane] = v.x; mine[1][lane] = v.y; mine[2][lane] = v.z; mine[3][lane] = v.w;
            asm volatile("" ::: "memory");         // (LDS operations of one wavefront execute in order: no wait is needed, only the compiler's order)
            __builtin_amdgcn_wave_barrier();
            const int n = (int) min(64u, e - base);
            if (lane < 4) {
                const float* col = mine[lane];
                if (n == 64) {
                    const float4* col4 = reinterpret_cast<const float4*>(col);
#pragma unroll
                    for (int q = 0; q < 16; ++q) {
                        const float4 t = col4[q];
                        acc += t.x; acc += t.y; acc += t.z; acc += t.w;
                    }
                } else {
                    for (int l = 0; l < n; ++l) acc += col[l];
                }
            }
            asm volatile("" ::: "memory");
            __builtin_amdgcn_wave_barrier();       // the next chunk overwrites the park
        };
        auto load4 = [&](unsigned base, unsigned (&w)[4]) {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const unsigned long long i = (unsigned long long) base + 64u * k + lane;
                w[k] = vals[i < e ? i : (unsigned long long) e - 1];        // (unconditional: the wait counters stay exact)
            }
        };
        unsigned wa[4], wb[4];
        load4(s, wa);
        for (unsigned base = s; base < e; base += 512) {       // (base + 512 cannot wrap: e <= 2^31)
            load4(base + 256, wb);
#pragma unroll
            for (int k = 0; k < 4; ++k) if (base + 64u * k < e) chunk(wa[k], base + 64u * k);
            load4(base + 512, wa);
#pragma unroll
            for (int k = 0; k < 4; ++k) if (base + 256u + 64u * k < e) chunk(wb[k], base + 256u + 64u * k);
        }
        if (lane == 0) out[0] = (double) (e - s);
        if (lane < 4) out[1 + lane] = (double) acc;
    } else {
        unsigned long long sa = 0, sr = 0, sg = 0, sb = 0;
        for (unsigned i = s + lane; i < e; i += 64) {
            const int c = unpack_bin_pixel(vals[i], keyfmt);
            sa += c_alpha(c); sr += c_red(c); sg += c_green(c); sb += c_blue(c);
        }
        for (int off = 32; off > 0; off >>= 1) {
            sa += __shfl_down(sa, off, 64); sr += __shfl_down(sr, off, 64);
            sg += __shfl_down(sg, off, 64); sb += __shfl_down(sb, off, 64);
        }
        if (lane == 0) {
            out[0] = (double) (e - s); out[1] = (double) sa; out[2] = (double) sr; out[3] = (double) sg; out[4] = (double) sb;
        }
    }
}

// ------------------------------------------------------------------------------------------------
// bins (compacted, structure of arrays).  LAB uses f[0..3] = ac,Lc,Ac,Bc; RGB uses d[0..3] = ac,rc,gc,bc.
// ------------------------------------------------------------------------------------------------
// struct Bins: nq_kernels.h

// P4: compaction + means (RGB NQ/PnnQuantizer.java:159-170, LAB NQ/PnnLABQuantizer.java:162-173); band partials are
// combined first (n_bands == 1 on a single GPU).  64 workgroups x 1024 threads, one histogram slot per thread: the first kernel
// counts the occupied slots of every 1024-slot slice, the second turns the counts into offsets and writes the bins in order;
// *out_maxbins = number of bins.
__device__ __forceinline__ double slot_total(const double* __restrict__ hists, int n_bands, int bin) {
    double c = 0;
    for (int b = 0; b < n_bands; ++b) c += hists[((size_t) b * 65536 + bin) * 5];
    return c;
}
__global__ void __launch_bounds__(1024) compact_count_kernel(const double* __restrict__ hists, int n_bands, int* __restrict__ blockcnt) {
    __shared__ int s_w[16];
    const int tid = threadIdx.x, bin = blockIdx.x * 1024 + tid;
    const unsigned long long m = __ballot(slot_total(hists, n_bands, bin) > 0);
    if ((tid & 63) == 0) s_w[tid >> 6] = __popcll(m);
    __syncthreads();
    if (tid == 0) { int t = 0; for (int w = 0; w < 16; ++w) t += s_w[w]; blockcnt[blockIdx.x] = t; }
}
template <int KIND>
__global__ void __launch_bounds__(1024) compact_means_kernel(const double* __restrict__ hists, int n_bands, Bins B,
                                                             const int* __restrict__ blockcnt, int* __restrict__ out_maxbins) {
    __shared__ int s_w[16];
    __shared__ int s_base;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, bin = blockIdx.x * 1024 + tid;
    const double total = slot_total(hists, n_bands, bin);
    const bool present = total > 0;
    const unsigned long long m = __ballot(present);
    if (lane == 0) s_w[wave] = __popcll(m);
    if (tid == 0) {
        int before = 0, all = 0;
        for (int g = 0; g < 64; ++g) { const int c = blockcnt[g]; all += c; if (g < (int) blockIdx.x) before += c; }
        s_base = before;
        if (blockIdx.x == 0) *out_maxbins = all;
    }
    __syncthreads();
    if (!present) return;
    int pos = s_base + __popcll(m & ((1ULL << lane) - 1ULL));
    for (int w = 0; w < wave; ++w) pos += s_w[w];
    // float cnt: "+= 1.0f" per pixel saturates at 2^24
    const float cnt = (float) (total > 16777216.0 ? 16777216.0 : total);
    const float dd = 1.0f / cnt;
    if (KIND == 1) {
        for (int ch = 0; ch < 4; ++ch) {
            float acc = (float) hists[((size_t) 0 * 65536 + bin) * 5 + 1 + ch];
            for (int b = 1; b < n_bands; ++b) acc += (float) hists[((size_t) b * 65536 + bin) * 5 + 1 + ch];
            acc *= dd;
            B.f[ch][pos] = acc;
        }
    } else {
        for (int ch = 0; ch < 4; ++ch) {
            double acc = 0;
            for (int b = 0; b < n_bands; ++b) acc += hists[((size_t) b * 65536 + bin) * 5 + 1 + ch];
            acc *= dd;                      // double *= float
            B.d[ch][pos] = acc;
        }
    }
    B.cnt[pos] = cnt;
    B.err[pos] = 0.f; B.nn[pos] = 0; B.tm[pos] = 0; B.mtm[pos] = 0;
}

// P6: getQuanFn (RGB NQ/PnnQuantizer.java:123-132, LAB NQ/PnnLABQuantizer.java:117-128), applied while linking (:184-191 / :210-217)
// fn: 0 identity, 1 (float)sqrt, 2 (float)(int)sqrt, 3 (float)(int)cbrt, 4 (float)pow(cnt,.75)
__global__ void __launch_bounds__(256) quanfn_kernel(float* __restrict__ cnt, int maxbins, int fn) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= maxbins) return;
    const float c = cnt[i];
    float r = c;
    if (fn == 1) r = (float) sqrt((double) c);
    else if (fn == 2) r = (float) j_d2i(sqrt((double) c));
    else if (fn == 3) {
        // (int) Math.cbrt(cnt) for an integer-valued cnt: exact integer cube root (cbrt of a perfect cube is exact in
        // fdlibm/glibc; for other integers <= 2^24 cbrt is never within an ulp of an integer)
        int q = j_d2i(cbrt((double) c));
        while ((double) (q + 1) * (q + 1) * (q + 1) <= (double) c) ++q;
        while (q > 0 && (double) q * q * q > (double) c) --q;
        r = (float) q;
    }
    else if (fn == 4) r = (float) pow((double) c, 0.75);
    cnt[i] = r;
}

// ------------------------------------------------------------------------------------------------
// find_nn
// ------------------------------------------------------------------------------------------------
// struct NNParams: nq_kernels.h; pgLessThanCoeff = (PG < coeffs[0][1]) for the RGB `start` selection (:69-71)

// candidate of the LAB scan, evaluated against an upper bound `e` of the running error.
// Returns alive=false as soon as a gate would `continue` against e (any later running error is <= e).
// M = last partial behind a `>=` gate, N = max of the partials behind `>` gates, F = final value.
struct CandLab { double M, N, F; };
// QUAD: the four lanes of a quad hold the same candidate and share the CIEDE2000 pass (ciede_terms_fast_quad, nq_device.h); every
// lane of the quad returns the same result.  r = lane & 3.
template <bool QUAD = false>
__device__ __forceinline__ bool eval_cand_lab(const NNParams& np, const Lab& lab1, float n1, const Lab& lab2, float n2,
                                              double e, bool valid, CandLab& out, int r = 0) {
    const double ratio = np.ratio;
    bool alive = valid;
    double nerr2 = (double) ((n1 * n2) / (n1 + n2));
    alive = alive && !(nerr2 >= e);
    double alphaDiff = np.hasSemi ? sqr((double) (lab2.alpha - lab1.alpha)) / g_tab.exp1_75 : 0;
    double nerr = nerr2 * alphaDiff;
    alive = alive && !(nerr >= e);
    double M;
    if (!np.texicab) {
        nerr += (1 - ratio) * nerr2 * sqr((double) (lab2.L - lab1.L));
        alive = alive && !(nerr >= e);
        nerr += (1 - ratio) * nerr2 * sqr((double) (lab2.A - lab1.A));
        alive = alive && !(nerr >= e);
        M = nerr > nerr2 ? nerr : nerr2;     // nerr2 is gated on its own (:57); the sum restarts at nerr2*alphaDiff (:63)
        nerr += (1 - ratio) * nerr2 * sqr((double) (lab2.B - lab1.B));
    } else {
        nerr += (1 - ratio) * nerr2 * (double) fabsf(lab2.L - lab1.L);
        alive = alive && !(nerr >= e);
        M = nerr > nerr2 ? nerr : nerr2;
        nerr += (1 - ratio) * nerr2 * sqrt(sqr((double) (lab2.A - lab1.A)) + sqr((double) (lab2.B - lab1.B)));
    }
    alive = alive && !(nerr > e);
    double N = nerr, F = nerr;           // N = max of the partials behind `>` gates (ratio may be negative: they can fall)
    if (alive) {
        // the four CIEDE2000 terms in one branch-free pass; the literal functions decide where a narrowing is too close to call
        float deltaL, deltaC, deltaH, rtf;
        const bool decided = QUAD ? ciede_terms_fast_quad(lab1, lab2, r, deltaL, deltaC, deltaH, rtf) : ciede_terms_fast(lab1, lab2, deltaL, deltaC, deltaH, rtf);
        if (!decided) {          // (alpha is not an input of the four terms)
            const CiedeTerms t = ciede_terms_literal_ool(lab1.L, lab1.A, lab1.B, lab2.L, lab2.A, lab2.B);
            deltaL = t.dL; deltaC = t.dC; deltaH = t.dH; rtf = t.rt;
        }
        nerr += ratio * nerr2 * sqr((double) deltaL);
        alive = !(nerr > e);
        N = fmax(N, nerr);
        if (alive) {
            nerr += ratio * nerr2 * sqr((double) deltaC);
            alive = !(nerr > e);
            N = fmax(N, nerr);
            if (alive) {
                nerr += ratio * nerr2 * sqr((double) deltaH);
                alive = !(nerr > e);
                N = fmax(N, nerr);
                if (alive) {
                    nerr += ratio * nerr2 * (double) rtf;
                    alive = !(nerr > e);
                    F = nerr;
                    N = fmax(N, F);
                }
            }
        }
    }
    out.M = M; out.N = N; out.F = F;
    return alive;
}

// value held by lane l (wavefront-uniform l): v_readlane_b32 instead of the ds_bpermute_b32 that __shfl compiles to
__device__ __forceinline__ int readlane_i(int x, int l) { return __builtin_amdgcn_readlane(x, __builtin_amdgcn_readfirstlane(l)); }
__device__ __forceinline__ float readlane_f(float x, int l) { return __int_as_float(readlane_i(__float_as_int(x), l)); }
__device__ __forceinline__ double readlane_d(double x, int l) {
    const long long b = __double_as_longlong(x);
    const unsigned lo = (unsigned) readlane_i((int) (unsigned) b, l), hi = (unsigned) readlane_i((int) (unsigned) (b >> 32), l);
    return __longlong_as_double((long long) (((unsigned long long) hi << 32) | lo));
}

// in-order resolution of one 64-candidate chunk (LAB): candidates that survived every gate against the chunk's
// starting error are accepted exactly when the sequential scan would accept them.
__device__ __forceinline__ void resolve_chunk_lab(bool alive, const CandLab& c, int j, double& e, int& nn) {
    const int lane = threadIdx.x & 63;
    bool cand = alive;
    for (;;) {
        const bool ok = cand && (c.M < e) && (c.N <= e);
        const unsigned long long mask = __ballot(ok);
        if (!mask) break;
        const int l = __ffsll((long long) mask) - 1;
        e = readlane_d(c.F, l);
        nn = readlane_i(j, l);
        cand = cand && lane > l;
    }
}

// candidate of the RGB scan (NQ/PnnQuantizer.java:73-113): pB = partial behind the last pre-YUV gate, s[] = the YUV
// prefix sums behind it (from row `start`)
struct CandRgb { double pB; double s[9]; int t0; };     // s[t], t >= t0 = 3 x start: the partial sums of the rows that are walked (slots
                                                        // below t0 repeat the pre-YUV sum; fixed slots keep the record in registers)
__device__ __forceinline__ void eval_cand_rgb(const NNParams& np, const double w[4], float n1, const double c[4], float n2f,
                                              int start, CandRgb& out) {
    const double ratio = np.ratio;
    double n2 = n2f, nerr2 = (n1 * n2) / (n1 + n2);
    double nerr = 0.0;
    // the pre-gates test monotone non-decreasing partials, the first of them nerr2 itself: keep the maximum
    double gate = nerr2;
    if (np.hasSemi) { nerr += nerr2 * np.PA * sqr(c[0] - w[0]); if (nerr > gate) gate = nerr; }
    nerr += nerr2 * (1 - ratio) * np.PR * sqr(c[1] - w[1]); if (nerr > gate) gate = nerr;
    nerr += nerr2 * (1 - ratio) * np.PG * sqr(c[2] - w[2]); if (nerr > gate) gate = nerr;
    nerr += nerr2 * (1 - ratio) * np.PB * sqr(c[3] - w[3]); if (nerr > gate) gate = nerr;
    out.pB = gate;
    double run = nerr;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const bool on = j >= start;
        const double r0 = run + nerr2 * ratio * sqr(k_coeffs[j][0] * (c[1] - w[1])); run = on ? r0 : run; out.s[3 * j] = run;
        const double r1 = run + nerr2 * ratio * sqr(k_coeffs[j][1] * (c[2] - w[2])); run = on ? r1 : run; out.s[3 * j + 1] = run;
        const double r2 = run + nerr2 * ratio * sqr(k_coeffs[j][2] * (c[3] - w[3])); run = on ? r2 : run; out.s[3 * j + 2] = run;
    }
    out.t0 = 3 * start;                      // start == 3: every slot holds the pre-YUV sum, which then is err
}
// the gate value alone (what decides whether a candidate is accepted at all): pB of eval_cand_rgb without the nine YUV partial sums
__device__ __forceinline__ double gate_only_rgb(const NNParams& np, const double w[4], float n1, const double c[4], float n2f) {
    const double ratio = np.ratio;
    double n2 = n2f, nerr2 = (n1 * n2) / (n1 + n2);
    double nerr = 0.0, gate = nerr2;
    if (np.hasSemi) { nerr += nerr2 * np.PA * sqr(c[0] - w[0]); if (nerr > gate) gate = nerr; }
    nerr += nerr2 * (1 - ratio) * np.PR * sqr(c[1] - w[1]); if (nerr > gate) gate = nerr;
    nerr += nerr2 * (1 - ratio) * np.PG * sqr(c[2] - w[2]); if (nerr > gate) gate = nerr;
    nerr += nerr2 * (1 - ratio) * np.PB * sqr(c[3] - w[3]); if (nerr > gate) gate = nerr;
    return gate;
}
// float32 LOWER bound of that gate value (needs 0 <= ratio <= 1 and P >= 0: every term >= 0, the alpha term is left out): the real
// value is nerr2 max(1, S), S >= (1 - ratio)(PR dr^2 + PG dg^2 + PB db^2); a dozen float32 roundings stay below 2e-6 relative
__device__ __forceinline__ float gate_lb32_rgb(float omr_pr, float omr_pg, float omr_pb, const float w[3], float n1, float r, float g, float b, float n2) {
    const float nerr2 = (n1 * n2) / (n1 + n2);
    const float dr = r - w[0], dg = g - w[1], db = b - w[2];
    const float q = __builtin_fmaf(omr_pb, db * db, __builtin_fmaf(omr_pg, dg * dg, omr_pr * (dr * dr)));
    return nerr2 * fmaxf(1.0f, q) * 0.99999f;
}
// value assigned to err when the candidate is accepted with running error e: first YUV partial >= e, else the full sum
__device__ __forceinline__ double accept_value_rgb(const CandRgb& c, double e) {
    double v = c.s[8];
#pragma unroll
    for (int t = 8; t >= 0; --t) if (t >= c.t0 && c.s[t] >= e) v = c.s[t];
    return v;
}
__device__ __forceinline__ void resolve_chunk_rgb(bool valid, const CandRgb& c, int j, double& e, int& nn) {
    const int lane = threadIdx.x & 63;
    bool cand = valid;
    for (;;) {
        const bool ok = cand && (c.pB < e);
        const unsigned long long mask = __ballot(ok);
        if (!mask) break;
        const int l = __ffsll((long long) mask) - 1;
        const double v = accept_value_rgb(c, e);
        e = readlane_d(v, l);
        nn = readlane_i(j, l);
        cand = cand && lane > l;
    }
}

// one wavefront scans candidate positions p = first .. end-1 in order; the candidate bin is live[p] (merge loop: the
// ascending list of bins that were alive at the last rebuild; entries that died since are skipped) or p itself
// (initial pass, live == nullptr).
template <int KIND>
__device__ __forceinline__ void find_nn_wave(const NNParams& np, const Bins& B, int idx, int first, int end,
                                             const int* __restrict__ live, double& e_out, int& nn_out) {
    const int lane = threadIdx.x & 63;
    double e = 1e100;
    int nn = 0;
    const float n1 = B.cnt[idx];
    if (KIND == 1) {
        Lab lab1; lab1.alpha = B.f[0][idx]; lab1.L = B.f[1][idx]; lab1.A = B.f[2][idx]; lab1.B = B.f[3][idx];
        for (int base = first; base < end; base += 64) {
            const int p = base + lane;
            bool valid = p < end;
            int j = p;
            if (live) { j = valid ? live[p] : 0; if (valid) valid = B.mtm[j] != 0xFFFF; }
            Lab lab2; float n2 = 1.f;
            lab2.alpha = lab2.L = lab2.A = lab2.B = 0.f;
            if (valid) { lab2.alpha = B.f[0][j]; lab2.L = B.f[1][j]; lab2.A = B.f[2][j]; lab2.B = B.f[3][j]; n2 = B.cnt[j]; }
            CandLab c;
            const bool alive = eval_cand_lab(np, lab1, n1, lab2, n2, e, valid, c);
            resolve_chunk_lab(alive, c, j, e, nn);
        }
    } else {
        const double w[4] = {B.d[0][idx], B.d[1][idx], B.d[2][idx], B.d[3][idx]};
        int start = 0;
        if (g_tab.blue[idx & 4095] > 0) start = np.pgLessThanCoeff ? 3 : 1;
        for (int base = first; base < end; base += 64) {
            const int p = base + lane;
            bool valid = p < end;
            int j = p;
            if (live) { j = valid ? live[p] : 0; if (valid) valid = B.mtm[j] != 0xFFFF; }
            double c4[4] = {0, 0, 0, 0}; float n2 = 1.f;
            if (valid) { c4[0] = B.d[0][j]; c4[1] = B.d[1][j]; c4[2] = B.d[2][j]; c4[3] = B.d[3][j]; n2 = B.cnt[j]; }
            CandRgb c;
            eval_cand_rgb(np, w, n1, c4, n2, start, c);
            resolve_chunk_rgb(valid, c, j, e, nn);
        }
    }
    e_out = e; nn_out = nn;
}

// initial pass (RGB :196-198, LAB :246-247): one wavefront per bin, find_nn_init_rgb_kernel / find_nn_init_lab_*_kernel below

// RGB initial pass with block pruning (the scheme of find_nn_block_rgb_boxes, nq_merge.inc, for one wavefront per bin): boxes of
// the initial bins per 64 consecutive bins, two float4 each {rmin, rmax, gmin, gmax}, {bmin, bmax, nmin, -}
__global__ void __launch_bounds__(256) init_boxes_rgb_kernel(Bins B, int maxbins, float* __restrict__ box) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= (maxbins + 63) / 64) return;
    float v0[4] = {3.0e38f, -3.0e38f, 3.0e38f, -3.0e38f}, v1[4] = {3.0e38f, -3.0e38f, 3.0e38f, 0.0f};
    const int hi = min(maxbins, (c + 1) * 64);
    for (int j = c * 64; j < hi; ++j) {
        const double r = B.d[1][j], g = B.d[2][j], b = B.d[3][j];
        v0[0] = fminf(v0[0], __double2float_rd(r)); v0[1] = fmaxf(v0[1], __double2float_ru(r));
        v0[2] = fminf(v0[2], __double2float_rd(g)); v0[3] = fmaxf(v0[3], __double2float_ru(g));
        v1[0] = fminf(v1[0], __double2float_rd(b)); v1[1] = fmaxf(v1[1], __double2float_ru(b));
        v1[2] = fminf(v1[2], B.cnt[j]);
    }
    for (int k = 0; k < 4; ++k) { box[8 * c + k] = v0[k]; box[8 * c + 4 + k] = v1[k]; }
}
__global__ void __launch_bounds__(256) find_nn_init_rgb_kernel(NNParams np, Bins B, int maxbins, const float* __restrict__ box) {
    const int lane = threadIdx.x & 63;
    const int idx = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (idx >= maxbins) return;
    double e = 1e100; int nn = 0;
    const bool bounds_ok = np.ratio >= 0.0 && np.ratio <= 1.0 && np.PR >= 0.0 && np.PG >= 0.0 && np.PB >= 0.0 && np.PA >= 0.0;
    bool exact = !bounds_ok;
    if (!exact) {
        const double w[4] = {B.d[0][idx], B.d[1][idx], B.d[2][idx], B.d[3][idx]};
        const float n1 = B.cnt[idx];
        int start = 0;
        if (g_tab.blue[idx & 4095] > 0) start = np.pgLessThanCoeff ? 3 : 1;
        const int first = idx + 1;
        const int cA = first >> 6, nblk = (maxbins + 63) >> 6;
        auto resolve_block = [&](int c) {
            const int j = (c << 6) + lane;
            const bool valid = j >= first && j < maxbins;
            double c4[4] = {0, 0, 0, 0}; float n2 = 1.f;
            if (valid) { c4[0] = np.hasSemi ? B.d[0][j] : 0.0; c4[1] = B.d[1][j]; c4[2] = B.d[2][j]; c4[3] = B.d[3][j]; n2 = B.cnt[j]; }
            CandRgb cand;
            eval_cand_rgb(np, w, n1, c4, n2, start, cand);
            resolve_chunk_rgb(valid, cand, j, e, nn);
        };
        const int cS = min(nblk, cA + 2);                  // seed: the block holding `first` and the one behind it
        for (int c = cA; c < cS; ++c) resolve_block(c);
        const double theta = e * np.rgbTheta;
        double emax = e;
        const double omr = 1.0 - np.ratio;
        // (float32 means rounded to nearest: the 0.99999 factor of gate_lb32_rgb covers that too -- differences of means up to 255 with
        // an absolute error of 3e-5 matter only where d^2 is tiny, and there the max(1, .) takes over)
        const float w32[3] = {(float) w[1], (float) w[2], (float) w[3]};
        const float oq[3] = {(float) (omr * np.PR) * 0.9999f, (float) (omr * np.PG) * 0.9999f, (float) (omr * np.PB) * 0.9999f};
        for (int cbase = cS; cbase < nblk; cbase += 64) {
            const int c = min(cbase + lane, nblk - 1);
            const float4 ba = *reinterpret_cast<const float4*>(box + 8 * c), bb = *reinterpret_cast<const float4*>(box + 8 * c + 4);
            const double dr = fmax(0.0, fmax((double) ba.x - w[1], w[1] - (double) ba.y)), dg = fmax(0.0, fmax((double) ba.z - w[2], w[2] - (double) ba.w)),
                         db = fmax(0.0, fmax((double) bb.x - w[3], w[3] - (double) bb.y));
            const double nmin = bb.z;
            const double nu = ((double) n1 * nmin) / ((double) n1 + nmin);
            const double lb = nu * fmax(1.0, omr * (np.PR * dr * dr + np.PG * dg * dg + np.PB * db * db)) * (1.0 - 1e-12);
            unsigned long long keep = __ballot((cbase + lane) < nblk && lb < theta);
            // the surviving blocks four at a time: their records are requested together (each block used to be a dependent round
            // trip of its own: 1.2 - 2.6 ms per image for ~20 blocks per bin), then evaluated and resolved in order
            while (keep) {
                int cb[4]; double c4[4][4]; float n2[4]; bool valid[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    cb[u] = -1;
                    if (keep) { cb[u] = cbase + __ffsll((long long) keep) - 1; keep &= keep - 1; }
                    const int j = ((cb[u] < 0 ? 0 : cb[u]) << 6) + lane;
                    valid[u] = cb[u] >= 0 && j >= first && j < maxbins;
                    c4[u][0] = c4[u][1] = c4[u][2] = c4[u][3] = 0.0; n2[u] = 1.f;
                    if (valid[u]) { c4[u][0] = np.hasSemi ? B.d[0][j] : 0.0; c4[u][1] = B.d[1][j]; c4[u][2] = B.d[2][j]; c4[u][3] = B.d[3][j]; n2[u] = B.cnt[j]; }
                }
#pragma unroll
                for (int u = 0; u < 4; ++u)
                    if (cb[u] >= 0) {
                        // a block in which no record's float32 lower bound of the gate is below the running error cannot change it (the
                        // boxes keep most blocks alive: their bound rests on the SMALLEST count of the block, often 1)
                        const float glb = valid[u] ? gate_lb32_rgb(oq[0], oq[1], oq[2], w32, n1, (float) c4[u][1], (float) c4[u][2], (float) c4[u][3], n2[u])
                                                   : 3.0e38f;
                        if (!__ballot((double) glb < e)) continue;
                        CandRgb cand;
                        eval_cand_rgb(np, w, n1, c4[u], n2[u], start, cand);
                        resolve_chunk_rgb(valid[u], cand, (cb[u] << 6) + lane, e, nn);
                        emax = fmax(emax, e);
                    }
            }
        }
        exact = emax > theta;                              // the assumed cap did not hold (uniform): unpruned scan
    }
    if (exact) find_nn_wave<0>(np, B, idx, idx + 1, maxbins, nullptr, e, nn);
    if (lane == 0) { B.err[idx] = (float) e; B.nn[idx] = nn; }
}

// ------------------------------------------------------------------------------------------------
// P9: heap build + merge loop, one persistent workgroup per image (nq_merge.inc); shared helpers first
// (RGB NQ/PnnQuantizer.java:193-255, LAB NQ/PnnLABQuantizer.java:243-312)
// ------------------------------------------------------------------------------------------------
#define NQ_INF_F 3.0e38f

// Pointers read from a job record are generic to the compiler (flat_load / flat_store, which also count against the LDS wait
// counter); the merge loop therefore keeps its device-memory pointers in the global address space explicitly.
#define NQ_G __attribute__((address_space(1)))
typedef int v2i __attribute__((ext_vector_type(2)));
typedef int v4i __attribute__((ext_vector_type(4)));
typedef float v4f __attribute__((ext_vector_type(4)));
struct GBins {
    NQ_G float* f[4]; NQ_G double* d[4]; NQ_G float* cnt; NQ_G float* err; NQ_G int* nn; NQ_G int* tm; NQ_G int* mtm;
    __device__ explicit GBins(const Bins& b) {
        for (int c = 0; c < 4; ++c) { f[c] = (NQ_G float*) b.f[c]; d[c] = (NQ_G double*) b.d[c]; }
        cnt = (NQ_G float*) b.cnt; err = (NQ_G float*) b.err; nn = (NQ_G int*) b.nn; tm = (NQ_G int*) b.tm; mtm = (NQ_G int*) b.mtm;
    }
};
struct HeapNode { int id; float err; };
// relaxed workgroup-scope accesses to LDS flags that other wavefronts poll (volatile would keep the generic address space)
__device__ __forceinline__ float lds_peek(const float* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
__device__ __forceinline__ void lds_poke(float* p, float v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }

// Scan arrays of the LAB merge loop, indexed by POSITION in the live list (ascending bin id), so that a scan reads
// contiguous memory: id (bin, -1 once the bin is deleted), q = {L, A, B, n} (the bin's Lab mean and count in one 16-byte record; a
// deleted bin carries a negative count), alpha mean.  A scan may read up to 63 records past the live list: the buffers
// are padded.
struct ScanArrays { NQ_G int* id; NQ_G v4f* q; NQ_G float* al; };
// Accessors of device arrays that another workgroup of the same launch may rewrite (merge teams, nq_merge.inc): COH = true reads
// with sc1 loads -- served by L2, never by this CU's vector L1, which no other CU's store refreshes (MI355X guide, "inter-workgroup
// visibility") -- and writes with sc1 (write-through) stores; COH = false is the plain access.
typedef unsigned long long nq_u64;
template <bool COH> struct CohV4 {
    const NQ_G v4f* p; __amdgpu_buffer_rsrc_t r;
    __device__ __forceinline__ explicit CohV4(const NQ_G v4f* base) : p(base) {
        if (COH) r = __builtin_amdgcn_make_buffer_rsrc((void*) base, 0, 0x7FFFFFFF, 0x00020000);
    }
    __device__ __forceinline__ v4f operator[](int i) const {
        if (COH) return __builtin_bit_cast(v4f, __builtin_amdgcn_raw_buffer_load_b128(r, i * 16, 0, 16));     // aux 16 = sc1
        return p[i];
    }
    __device__ __forceinline__ void store(int i, v4f v) const {
        if (COH) __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(v4i, v), r, i * 16, 0, 16);
        else ((NQ_G v4f*) p)[i] = v;
    }
};
template <bool COH> struct CohF32 {
    const NQ_G float* p;
    __device__ __forceinline__ explicit CohF32(const NQ_G float* base) : p(base) {}
    __device__ __forceinline__ float operator[](int i) const {
        return COH ? __hip_atomic_load(p + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : p[i];
    }
    __device__ __forceinline__ void store(int i, float v) const {
        if (COH) __hip_atomic_store((NQ_G float*) p + i, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        else ((NQ_G float*) p)[i] = v;
    }
};
template <bool COH> struct CohI32 {
    const NQ_G int* p;
    __device__ __forceinline__ explicit CohI32(const NQ_G int* base) : p(base) {}
    __device__ __forceinline__ int operator[](int i) const {
        return COH ? __hip_atomic_load(p + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : p[i];
    }
    __device__ __forceinline__ void store(int i, int v) const {
        if (COH) __hip_atomic_store((NQ_G int*) p + i, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        else ((NQ_G int*) p)[i] = v;
    }
};
template <bool COH> struct CohF64 {
    const NQ_G double* p;
    __device__ __forceinline__ explicit CohF64(const NQ_G double* base) : p(base) {}
    __device__ __forceinline__ double operator[](int i) const {
        if (COH) return __longlong_as_double((long long) __hip_atomic_load((const NQ_G nq_u64*) p + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
        return p[i];
    }
    __device__ __forceinline__ void store(int i, double v) const {
        if (COH) __hip_atomic_store((NQ_G nq_u64*) p + i, (nq_u64) __double_as_longlong(v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        else ((NQ_G double*) p)[i] = v;
    }
};
// 8-byte {tag, value} granules of the team protocol: ONE aligned sc1 store / load each (the data is its own flag)
__device__ __forceinline__ nq_u64 gran_load(const NQ_G nq_u64* g) { return __hip_atomic_load(g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void gran_store(NQ_G nq_u64* g, unsigned tag, unsigned value) {
    __hip_atomic_store(g, ((nq_u64) tag << 32) | value, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// upper bound of the chroma sqrt(A^2 + B^2) from the record itself (hardware square root, 1 ulp): the bounds only need C2 <= this
__device__ __forceinline__ float chroma_ub(float A, float B) { return __builtin_amdgcn_sqrtf(A * A + B * B) * 1.000001f; }
// Bounding boxes of the records of every 64-position block (absolute: block c = positions [64 c, 64 c + 64)), two v4f each:
// {Lmin, Lmax, Amin, Amax}, {Bmin, Bmax, nmin, Cmax}.  Conservative: a merge only widens the box of the surviving bin's block
// (the merged count only grows, a deleted record keeps its share of the box); rebuilt with the live list.
__device__ __forceinline__ void build_boxes(const ScanArrays& S, int nlive, NQ_G v4f* __restrict__ box) {
    const int nblk = (nlive + 63) >> 6;
    for (int c = threadIdx.x; c < nblk; c += blockDim.x) {
        v4f a = {3.0e38f, -3.0e38f, 3.0e38f, -3.0e38f}, b = {3.0e38f, -3.0e38f, 3.0e38f, 0.0f};
        const int hi = min(nlive, (c + 1) << 6);
        for (int p = c << 6; p < hi; ++p) {
            const v4f q = S.q[p];
            if (q.w < 0.0f) continue;
            a.x = fminf(a.x, q.x); a.y = fmaxf(a.y, q.x); a.z = fminf(a.z, q.y); a.w = fmaxf(a.w, q.y);
            b.x = fminf(b.x, q.z); b.y = fmaxf(b.y, q.z); b.z = fminf(b.z, q.w); b.w = fmaxf(b.w, chroma_ub(q.y, q.z));
        }
        box[2 * c] = a; box[2 * c + 1] = b;
    }
}

// Interval bounds, in float32, on the acceptance threshold T_j of a LAB candidate: the sequential scan accepts candidate j
// exactly when the running error e satisfies e >= T_j, T_j = max(nerr2+, partials behind the `>=`/`>` gates, final value)
// (NQ/PnnLABQuantizer.java:57-108).  Two facts make bounds useful:
//   (a) after candidate i has been visited the running error is <= T_i (accepted: e = F_i <= T_i; rejected: e < T_i), so the
//       running error at candidate j is <= min over earlier i of any UPPER bound of T_i;
//   (b) a candidate whose LOWER bound of T_j exceeds that minimum is rejected by the sequential scan.
// Everything else is evaluated exactly in f64.  Bounds use only: every term of the sum is >= 0 except the R_T term,
// |R_T| <= 2 sin(60 deg), S_H >= 1, S_C >= S_H, dC'^2 + dH'^2 = da'^2 + db^2 (exact identity of the hue difference), with a
// relative slack of 1e-4 (float32 rounding of these few operations and of the reference's own float narrowing is < 1e-5)
// and an absolute slack where the chroma difference cancels.
// wavefront-wide inclusive minimum scan and shift by one lane with DPP modifiers (GFX9 row_shr / row_bcast / wave_shr): six + one
// VALU instructions; `__shfl_up` compiles to ds_bpermute_b32, seven dependent LDS-crossbar round trips per scan
template <int CTRL, int ROWMASK>
__device__ __forceinline__ float dpp_min_step(float x) {
    const int y = __builtin_amdgcn_update_dpp(__float_as_int(NQ_INF_F), __float_as_int(x), CTRL, ROWMASK, 0xF, false);
    return fminf(x, __int_as_float(y));
}
__device__ __forceinline__ float wave_incl_min_scan(float x) {
    x = dpp_min_step<0x111, 0xF>(x);        // row_shr:1
    x = dpp_min_step<0x112, 0xF>(x);        // row_shr:2
    x = dpp_min_step<0x114, 0xF>(x);        // row_shr:4
    x = dpp_min_step<0x118, 0xF>(x);        // row_shr:8   -> inclusive scan inside every row of 16 lanes
    x = dpp_min_step<0x142, 0xA>(x);        // row_bcast:15 into rows 1 and 3
    x = dpp_min_step<0x143, 0xC>(x);        // row_bcast:31 into rows 2 and 3
    return x;
}
// value of lane - 1 (lane 0: +inf)
__device__ __forceinline__ float wave_prev_lane_or_inf(float x) {
    return __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(NQ_INF_F), __float_as_int(x), 0x138, 0xF, 0xF, false));   // wave_shr:1
}
struct PreLab { float L, A, B, alpha, C, n1; };
// hardware reciprocal / square root (v_rcp_f32, v_sqrt_f32: 1 ulp), used ONLY inside the bounds, whose 1e-4 margins dwarf it
__device__ __forceinline__ float frcp(float x) { return __builtin_amdgcn_rcpf(x); }
__device__ __forceinline__ float fsqrt(float x) { return __builtin_amdgcn_sqrtf(x); }
struct BoundTmp { float nerr2, base, dLq2, a1p, a2p, C1p, C2p, S_C, ab2; };

// cheap lower bound of T_j (about 40 float32 operations): (dC/S_C)^2 + (dH/S_H)^2 >= (dC^2 + dH^2)/S_C^2 (S_C >= S_H >= 1)
__device__ __forceinline__ float cheap_lb_lab(const NNParams& np, const PreLab& a, float L2, float A2, float B2, float al2, float n2,
                                              float C2, float ratio_f, float omr_f, float inv_e175, BoundTmp& t) {
    const float nerr2 = (a.n1 * n2) / (a.n1 + n2);                  // same float ops as the reference (:55-56), IEEE division
    const float dL = fabsf(L2 - a.L), dA = A2 - a.A, dB = B2 - a.B;
    float base = 0.f;                                                // alpha + "texicab" terms, all >= 0
    if (np.hasSemi) { const float da = al2 - a.alpha; base += da * da * inv_e175; }
    if (np.texicab) base += omr_f * (dL + fsqrt(dA * dA + dB * dB));
    else base += omr_f * (dL * dL + dA * dA + dB * dB);
    const float barL = (a.L + L2) * 0.5f - 50.0f;
    const float pp = barL * barL;
    const float S_L = 1.0f + 0.015f * pp * frcp(fsqrt(20.0f + pp));
    const float dLq = dL * frcp(S_L);
    const float barC = (a.C + C2) * 0.5f;
    const float b2 = barC * barC, b4 = b2 * b2, b7 = b4 * b2 * barC;
    const float G = 0.5f * (1.0f - fsqrt(b7 * frcp(b7 + 6103515625.0f)));
    t.a1p = (1.0f + G) * a.A; t.a2p = (1.0f + G) * A2;
    t.C1p = fsqrt(t.a1p * t.a1p + a.B * a.B); t.C2p = fsqrt(t.a2p * t.a2p + B2 * B2);
    t.S_C = 1.0f + 0.045f * ((t.C1p + t.C2p) * 0.5f);
    const float dap = t.a2p - t.a1p;
    t.ab2 = dap * dap + dB * dB;                                     // = dC'^2 + dH'^2
    t.nerr2 = nerr2; t.base = base; t.dLq2 = dLq * dLq;
    const float low = base + ratio_f * (t.dLq2 + t.ab2 * frcp(t.S_C * t.S_C));
    return fmaxf(nerr2, nerr2 * low * 0.9999f - 1e-30f);
}

// atan2 by octant reduction + Hastings' degree-11 odd polynomial: |error| < 1.2e-5 rad (the margin on T below allows 1e-4)
__device__ __forceinline__ float fast_atan2f(float y, float x) {
    const float ax = fabsf(x), ay = fabsf(y);
    const float a = fminf(ax, ay) * frcp(fmaxf(ax, ay));
    const float s = a * a;
    float r = -0.0117212f;
    r = r * s + 0.05265332f; r = r * s - 0.11643287f; r = r * s + 0.19354346f; r = r * s - 0.33262347f; r = r * s + 0.99997726f;
    r = r * a;
    if (ay > ax) r = 1.57079637f - r;
    if (x < 0.0f) r = 3.14159274f - r;
    return y < 0.0f ? -r : r;
}

// tight interval [lb, ub] of T_j (about 150 float32 operations, evaluated only for candidates that pass the cheap bound):
// S_H from the mean hue angle, |R_T| from its closed form; when the mean hue is ill-defined (a chroma of zero, or the two
// hues within 2e-3 rad of opposite) the loose facts S_H in [1, 1 + 0.015 barC' 1.93], |R_T| <= 1.7321 are used instead.
__device__ __forceinline__ void tight_bounds_lab(const PreLab& a, float B2, float ratio_f, const BoundTmp& t, float& lb, float& ub) {
    const float PI_F = 3.14159265f, TWO_PI_F = 6.28318531f;
    const float sumC = t.C1p + t.C2p, barCp = sumC * 0.5f;
    const float dC = t.C2p - t.C1p;
    const float slackC = 4e-6f * sumC + 1e-6f;
    const float dClo = fmaxf(0.0f, fabsf(dC) - slackC), dChi = fabsf(dC) + slackC;
    const float dCq_lo = dClo * frcp(t.S_C * 1.00001f), dCq_hi = dChi * frcp(t.S_C * 0.99999f);
    const float slackH = 1e-5f * t.ab2 + 1e-9f;
    const float dH2_lo = fmaxf(0.0f, (t.ab2 - dChi * dChi) * 0.9999f - slackH);
    const float dH2_hi = fmaxf(0.0f, t.ab2 - dClo * dClo) * 1.0001f + slackH;
    float T_lo = 0.07f, T_hi = 1.93f, RT_hi = 1.7321f;
    const bool zero1 = (t.a1p == 0.0f && a.B == 0.0f), zero2 = (t.a2p == 0.0f && B2 == 0.0f);
    if (!zero1 && !zero2) {
        float h1 = fast_atan2f(a.B, t.a1p); if (h1 < 0.0f) h1 += TWO_PI_F;
        float h2 = fast_atan2f(B2, t.a2p); if (h2 < 0.0f) h2 += TWO_PI_F;
        const float dh = fabsf(h1 - h2), hs = h1 + h2;
        if (fabsf(dh - PI_F) > 2e-3f) {
            float bh;
            if (dh <= PI_F) bh = hs * 0.5f;
            else bh = hs < TWO_PI_F ? (hs + TWO_PI_F) * 0.5f : (hs - TWO_PI_F) * 0.5f;
            // hardware cosine (v_cos_f32, abs. error ~1e-6 for these |x| < 30) -- the margin on T is 3e-4
            const float T = 1.0f - 0.17f * __cosf(bh - 0.523598776f) + 0.24f * __cosf(2.0f * bh) + 0.32f * __cosf(3.0f * bh + 0.104719755f)
                            - 0.20f * __cosf(4.0f * bh - 1.09955743f);
            T_lo = T - 3e-4f; T_hi = T + 3e-4f;
            const float z = (bh - 4.79965544f) * 2.29183118f;                 // (barh - 275 deg) / 25 deg
            const float dTheta = 0.523598776f * __expf(-z * z);
            const float c2 = barCp * barCp, c4 = c2 * c2, c7 = c4 * c2 * barCp;
            const float R_C = 2.0f * fsqrt(c7 * frcp(c7 + 6103515625.0f));
            RT_hi = __sinf(2.0f * dTheta) * R_C * 1.001f + 1e-4f;
        }
    }
    const float S_H_lo = 1.0f + 0.015f * barCp * T_lo * 0.9999f, S_H_hi = 1.0f + 0.015f * barCp * T_hi * 1.0001f;
    const float dHq2_lo = dH2_lo * frcp(S_H_hi * S_H_hi), dHq2_hi = dH2_hi * frcp(S_H_lo * S_H_lo);
    const float low = t.base + ratio_f * (t.dLq2 + dCq_lo * dCq_lo + dHq2_lo);
    const float high = t.base + ratio_f * (t.dLq2 + dCq_hi * dCq_hi + dHq2_hi + RT_hi * dCq_hi * fsqrt(dHq2_hi));
    lb = fmaxf(t.nerr2, t.nerr2 * low * 0.9999f - 1e-30f);
    ub = fmaxf(t.nerr2 * 1.000001f, t.nerr2 * high * 1.0001f + 1e-30f);
}

// Initial pass for LAB (NQ/PnnLABQuantizer.java:246-247) with the same interval bounds as the merge loop, one wavefront per bin:
// the candidates behind `idx` are visited in order, 64 per step, against the running minimum of the upper bounds (level 0 ->
// S_C bound -> tight bound); the few that may be accepted are evaluated exactly in f64 and replayed in order.
// bounding boxes of the initial bins, one thread per block of 64 consecutive bins (layout as in build_boxes)
__global__ void __launch_bounds__(256) init_boxes_kernel(Bins B, int maxbins, float* __restrict__ box) {
    // one wavefront per block of 64 bins: lane = bin, butterfly min / max
    const int c = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (c >= (maxbins + 63) / 64) return;
    const int j = c * 64 + lane;
    float v[8] = {3.0e38f, -3.0e38f, 3.0e38f, -3.0e38f, 3.0e38f, -3.0e38f, 3.0e38f, 0.0f};
    if (j < maxbins) {
        const float L = B.f[1][j], A = B.f[2][j], Bv = B.f[3][j], n = B.cnt[j];
        const float C = sqrtf(A * A + Bv * Bv) * 1.000001f;
        v[0] = v[1] = L; v[2] = v[3] = A; v[4] = v[5] = Bv; v[6] = n; v[7] = C;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const float o = __shfl_xor(v[k], off, 64);
            v[k] = (k == 0 || k == 2 || k == 4 || k == 6) ? fminf(v[k], o) : fmaxf(v[k], o);
        }
    }
    if (lane < 8) {
        float r = v[0];
#pragma unroll
        for (int k = 1; k < 8; ++k) if (lane == k) r = v[k];
        box[8 * c + lane] = r;
    }
}
// Two kernels: the bound phase needs ~70 registers and is a chain of dependent block loads (latency bound: it wants many wavefronts
// per SIMD), the exact phase needs the 200+ registers of the f64 CIEDE2000 code for a handful of candidates per bin.  The lists go
// through device memory: cand[idx][NQ_INIT_LIST] = {bin j, bound U_j of the running error at j}, ncand[idx] (> NQ_INIT_LIST: overflow,
// the exact kernel scans that bin literally).
#define NQ_INIT_LIST 128
__global__ void __launch_bounds__(256) find_nn_init_lab_bounds_kernel(NNParams np, Bins B, int maxbins, const float* __restrict__ box,
                                                                      int2* __restrict__ cand, int* __restrict__ ncand_out) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int idx = blockIdx.x * 4 + wave;
    if (idx >= maxbins) return;
    // (the bounds need 0 <= ratio <= 1, see find_nn_block_lab: otherwise this kernel is not launched and the exact kernel scans)
    const float n1 = B.cnt[idx];
    Lab lab1; lab1.alpha = B.f[0][idx]; lab1.L = B.f[1][idx]; lab1.A = B.f[2][idx]; lab1.B = B.f[3][idx];
    PreLab pa; pa.L = lab1.L; pa.A = lab1.A; pa.B = lab1.B; pa.alpha = lab1.alpha; pa.n1 = n1;
    pa.C = sqrtf(lab1.A * lab1.A + lab1.B * lab1.B);
    const float ratio_f = (float) np.ratio, omr_f = (float) (1.0 - np.ratio);
    const float inv_e175 = (float) (1.0 / g_tab.exp1_75);
    const float k0 = pa.n1 * ratio_f * 0.999f;
    float runmin = NQ_INF_F;
    int ncand = 0;
    // blocks of 64 consecutive bins, aligned to absolute indices; the block of idx + 1 and the next one first (the seed), then
    // only the blocks whose bounding box passes the level-0 inequality against the running minimum
    const int first = idx + 1, cA = first >> 6, nblk = (maxbins + 63) >> 6;
    auto do_block = [&](int c) {
        const int j = (c << 6) + lane;
        const bool valid = j >= first && j < maxbins;
        const int jc = min(j, maxbins - 1);
        const float n2 = B.cnt[jc], L2 = B.f[1][jc], A2 = B.f[2][jc], B2 = B.f[3][jc];
        const float al2 = np.hasSemi ? B.f[0][jc] : 0.f;
        const float C2 = fsqrt(A2 * A2 + B2 * B2) * 1.000001f;          // (an upper bound of the chroma is what the bounds need)
        float lb = NQ_INF_F, ub = NQ_INF_F;
        BoundTmp bt;
        bool pass0 = false;
        if (valid) {                                                     // level 0: see find_nn_block_lab
            const float dL0 = L2 - pa.L, dA0 = A2 - pa.A, dB0 = B2 - pa.B;
            const float scm = __builtin_fmaf(0.03375f, pa.C + C2, 1.0f);
            const float scm2 = scm * scm;
            const float t = __builtin_fmaf(0.3265f * dL0 * dL0, scm2, __builtin_fmaf(dA0, dA0, dB0 * dB0));
            pass0 = (k0 * n2) * t <= runmin * ((pa.n1 + n2) * scm2);
        }
        if (!__ballot(pass0)) return;
        if (pass0) {
            lb = cheap_lb_lab(np, pa, L2, A2, B2, al2, n2, C2, ratio_f, omr_f, inv_e175, bt);
            pass0 = lb <= runmin;
        }
        if (!__ballot(pass0)) return;
        if (pass0) { tight_bounds_lab(pa, B2, ratio_f, bt, lb, ub); pass0 = lb <= runmin; }
        if (!__ballot(pass0)) return;
        float x = pass0 ? ub : NQ_INF_F;                                 // exclusive prefix minimum of the upper bounds
        x = wave_incl_min_scan(x);
        const float excl = wave_prev_lane_or_inf(x);
        const float Uj = fminf(runmin, excl);
        const bool pass = pass0 && lb <= Uj;
        const unsigned long long mask = __ballot(pass);
        const int pos = ncand + __popcll(mask & ((1ULL << lane) - 1ULL));
        if (pass && pos < NQ_INIT_LIST) cand[(size_t) idx * NQ_INIT_LIST + pos] = make_int2(j, __float_as_int(Uj));
        ncand += __popcll(mask);
        runmin = fminf(runmin, readlane_f(x, 63));
    };
    if (cA < nblk) do_block(cA);
    if (cA + 1 < nblk) do_block(cA + 1);
    for (int cbase = cA + 2; cbase < nblk; cbase += 64) {
        const int c = min(cbase + lane, nblk - 1);
        const float4 ba = *reinterpret_cast<const float4*>(box + 8 * c), bb = *reinterpret_cast<const float4*>(box + 8 * c + 4);
        const float dL = fmaxf(0.0f, fmaxf(ba.x - pa.L, pa.L - ba.y)), dA = fmaxf(0.0f, fmaxf(ba.z - pa.A, pa.A - ba.w)),
                    dB = fmaxf(0.0f, fmaxf(bb.x - pa.B, pa.B - bb.y));
        const float scm = __builtin_fmaf(0.03375f, pa.C + bb.w, 1.0f), scm2 = scm * scm;
        const float t = __builtin_fmaf(0.3265f * dL * dL, scm2, __builtin_fmaf(dA, dA, dB * dB));
        unsigned long long todo = __ballot((cbase + lane) < nblk && (k0 * bb.z) * t <= runmin * ((pa.n1 + bb.z) * scm2));
        while (todo) {
            const int cb = cbase + __ffsll((long long) todo) - 1;
            todo &= todo - 1;
            do_block(cb);
        }
    }
    if (lane == 0) ncand_out[idx] = ncand;
}

__global__ void __launch_bounds__(256) find_nn_init_lab_exact_kernel(NNParams np, Bins B, int maxbins, const int2* __restrict__ cand,
                                                                     const int* __restrict__ ncand_in) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int idx = blockIdx.x * 4 + wave;
    if (idx >= maxbins) return;
    (void) wave;
    const bool bounded = np.ratio >= 0.0 && np.ratio <= 1.0;
    const int ncand = bounded ? ncand_in[idx] : NQ_INIT_LIST + 1;
    const float n1 = B.cnt[idx];
    Lab lab1; lab1.alpha = B.f[0][idx]; lab1.L = B.f[1][idx]; lab1.A = B.f[2][idx]; lab1.B = B.f[3][idx];
    double e = 1e100; int nn = 0;
    if (ncand > NQ_INIT_LIST) {
        find_nn_wave<1>(np, B, idx, idx + 1, maxbins, nullptr, e, nn);   // list overflow / no bounds: the exact wavefront scan
    } else {
        // each listed candidate against ITS bound U of the running error (a gate that fails against U fails against the true running
        // error <= U); the survivors are accepted or not in order, against the true running error.  More than 16 candidates left:
        // one per lane (one pass of the f64 chain serves 64); up to 16: one QUAD per candidate, the four lanes share the CIEDE2000 pass
        int r = 0;
        while (r < ncand) {
            const bool quads = ncand - r <= 16;
            const int t = quads ? r + (lane >> 2) : r + lane;
            const bool have = t < ncand;
            CandLab c; c.M = c.N = c.F = 0; int j = 0;
            bool keep = false;
            double U = 0.0; Lab lab2; lab2.alpha = lab2.L = lab2.A = lab2.B = 0.f; float n2 = 1.f;
            if (have) {
                const int2 cu = cand[(size_t) idx * NQ_INIT_LIST + t];
                j = cu.x;
                U = (double) __int_as_float(cu.y);
                lab2.alpha = B.f[0][j]; lab2.L = B.f[1][j]; lab2.A = B.f[2][j]; lab2.B = B.f[3][j]; n2 = B.cnt[j];
            }
            if (quads) {
                if (have) {
                    const bool alive = eval_cand_lab<true>(np, lab1, n1, lab2, n2, U, true, c, lane & 3);
                    keep = alive && (c.M < U) && (c.N <= U) && (lane & 3) == 0;   // (lane 0 of the quad stands for the candidate)
                }
                r += 16;
            } else {
                if (have) {
                    const bool alive = eval_cand_lab<false>(np, lab1, n1, lab2, n2, U, true, c);
                    keep = alive && (c.M < U) && (c.N <= U);
                }
                r += 64;
            }
            resolve_chunk_lab(keep, c, j, e, nn);
        }
    }
    if (lane == 0) { B.err[idx] = (float) e; B.nn[idx] = nn; }
}

// the merge loop, compiled for three workgroup sizes (nq_merge.inc)
#define NQ_MERGE_THREADS 512
namespace m512 {
#include "nq_merge.inc"
}
#undef NQ_MERGE_THREADS
#define NQ_MERGE_THREADS 256
namespace m256 {
#include "nq_merge.inc"
}
#undef NQ_MERGE_THREADS
#define NQ_MERGE_THREADS 128
namespace m128 {
#include "nq_merge.inc"
}
#undef NQ_MERGE_DENSE
#define NQ_MERGE_DENSE 1
namespace m128d {
#include "nq_merge.inc"
}
#undef NQ_MERGE_DENSE
#undef NQ_MERGE_THREADS


// self-test of ciede_terms_fast (nq_selftest_ciede): per pair {L1,A1,B1,L2,A2,B2} -> the four floats of the fast pass (when it
// decided), the four floats of the literal functions, and the decided flag, as bit patterns
__global__ void __launch_bounds__(256) ciede_selftest_kernel(const float* __restrict__ pairs, long long n, unsigned* __restrict__ out) {
    // one QUAD per pair (n rounded up so that whole quads stay active): lane 0 of the quad also runs the one-lane pass and the literal
    // functions; word 8 of the record = decided | (quad pass identical to the one-lane pass, flags included) << 1
    const long long nq4 = 4 * n;
    for (long long t = (long long) blockIdx.x * blockDim.x + threadIdx.x; t < nq4; t += (long long) gridDim.x * blockDim.x) {
        const long long i = t >> 2;
        const int r = (int) (t & 3);
        Lab a, b;
        a.alpha = b.alpha = 255.f;
        a.L = pairs[6 * i]; a.A = pairs[6 * i + 1]; a.B = pairs[6 * i + 2];
        b.L = pairs[6 * i + 3]; b.A = pairs[6 * i + 4]; b.B = pairs[6 * i + 5];
        float f[4] = {0, 0, 0, 0}, l[4], q[4] = {0, 0, 0, 0};
        const bool okq = ciede_terms_fast_quad(a, b, r, q[0], q[1], q[2], q[3]);
        const bool ok = ciede_terms_fast(a, b, f[0], f[1], f[2], f[3]);
        if (r == 0) {
            ciede_terms_literal(a, b, l[0], l[1], l[2], l[3]);
            bool same = ok == okq;
            for (int j = 0; j < 4; ++j) same = same && __float_as_uint(f[j]) == __float_as_uint(q[j]);
            for (int j = 0; j < 4; ++j) { out[9 * i + j] = __float_as_uint(f[j]); out[9 * i + 4 + j] = __float_as_uint(l[j]); }
            out[9 * i + 8] = (ok ? 1u : 0u) | (same ? 2u : 0u);
        }
    }
}

} // namespace nq
