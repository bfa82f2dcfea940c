// nq_gif.hip -- GIF encoding of palette index maps on gfx950 (include/nquant_abi.h, "GIF encoding"; DESIGN.md "GIF encoder").
//
// A frame's indices are cut into segments of S pixels.  Every segment is one LZW chain with a dictionary of its own, so the
// chains run in parallel; a frame's data is the chains' bit strings one after another (GIF allows a Clear code anywhere).
//   gif_lzw_kernel     one wave per chain, four chains per workgroup; the dictionary lives in LDS and the indices are staged into
//                      LDS by the whole wave, 1 KiB ahead of the chain.  <true> is the lossy mode ("GIF encoding, lossy mode"): on a
//                      miss the 64 lanes try the near colours that would continue the string, four candidates each
//   gif_scan_kernel    per frame: exclusive scan of the segments' bit lengths, the frame's bit length
//   gif_gather_kernel  one thread per byte of the file: header bytes from the host's blob, sub-block length bytes, and the data
//                      bytes ORed together from the <= 3 segments each one overlaps
// Delta mode (nq_encode_gif_delta_device) puts two passes in front: the frames after the first become cropped bodies in scratch, and
// the three kernels above run on those as on any index map.
//   gif_diff_kernel    frame f against frame f - 1: bounding box of the changed pixels (and the index >= K check of all frames)
//   gif_body_kernel    the box's pixels, row-major, the unchanged ones replaced by the transparent index
// Local colour tables (nq_encode_gif_local*): one GifLocal record per frame (K, Kt, m, T and the written table) replaces the per-call
// values.  gif_lzw_kernel<.., true> takes them per chain; gif_diff_local_kernel and gif_body_local_kernel are the two delta passes with
// "differs" judged on the colours the two frames' tables give the indices (the tables sit in LDS).  Scan and gather are shared.
#include "nq_kernels.h"

#include <type_traits>

namespace nq {

namespace {

constexpr int GIF_CHAINS = 4;            // chains (waves) per workgroup
constexpr int GIF_SLOTS = 8192;          // open-addressing slots per chain: {key = pre << 8 | c : 20, code : 12}, 0 = empty
constexpr int GIF_STAGE = 512;           // indices per staging block: 64 lanes x 16 bytes

// every lane's LDS accesses so far are done and visible to the whole wave, and no access moves across this point
__device__ inline void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

// 16 bytes of index map at byte address a (16-byte aligned); the u16 elements outside [lo, hi) read as 0 and are never loaded
__device__ inline uint4 load_chunk(uintptr_t a, uintptr_t lo, uintptr_t hi) {
    if (a >= lo && a + 16 <= hi) return *reinterpret_cast<const uint4*>(a);
    unsigned v[4] = {0, 0, 0, 0};
    for (int j = 0; j < 8; ++j) {
        const uintptr_t e = a + 2 * j;
        if (e >= lo && e < hi) v[j >> 1] |= (unsigned) *reinterpret_cast<const unsigned short*>(e) << (16 * (j & 1));
    }
    return make_uint4(v[0], v[1], v[2], v[3]);
}

__device__ inline void clear_table(unsigned* tab, int lane) {
    uint4* t4 = reinterpret_cast<uint4*>(tab);
    for (int i = lane; i < GIF_SLOTS / 4; i += 64) t4[i] = make_uint4(0, 0, 0, 0);
    wave_sync();
}

// the code of `key` (pre << 8 | c) in a chain's dictionary, 0 when it is not there; *slot: where it is, or the empty slot it would take
__device__ inline unsigned find_code(const unsigned* tab, unsigned key, unsigned* slot) {
    unsigned h = (key * 0x9E3779B1u) >> 19;
    unsigned code = 0;
    for (int probe = 0; probe < GIF_SLOTS; ++probe) {
        const unsigned ent = tab[h];
        if (ent == 0) break;
        if ((ent >> 12) == key) { code = ent & 4095u; break; }
        h = (h + 1) & (GIF_SLOTS - 1);
    }
    *slot = h;
    return code;
}

// largest channel difference (.x) and squared distance (.y) of two packed 0x00RRGGBB colours
__device__ inline uint2 rgb_apart(unsigned a, unsigned b) {
    const int dr = (int) (a >> 16 & 255u) - (int) (b >> 16 & 255u), dg = (int) (a >> 8 & 255u) - (int) (b >> 8 & 255u),
              db = (int) (a & 255u) - (int) (b & 255u);
    return make_uint2((unsigned) max(max(abs(dr), abs(dg)), abs(db)), (unsigned) (dr * dr + dg * dg + db * db));
}

// All 64 lanes of a wave run the chain in lockstep on the same values (the LDS reads broadcast); lane 0 alone stores to the
// dictionary and to global memory.  Every loop is bounded by the segment length or the table size.
// LOSSY: `rgb` is the file's colour table (256 entries 0x00RRGGBB, zeros from entry K on; here K is the table's Kt), T its transparent
// index (-1: none), lossy the threshold 1..255.  Where the exact index misses, lane l looks up (pre, c') for c' = l, l + 64, l + 128,
// l + 192, a wave minimum over d^2 << 8 | c' picks the winner, and its code is handed to every lane: all lanes hold the same `pre` again.
// LOCAL ("GIF encoding, local colour tables"): `rgb` is the per-frame records instead, and K, m, T and the colour table are those of
// the chain's frame, rgb[frame] (the arguments K, m and T are not read).  The four chains of a workgroup may sit in four frames, so
// every wave has an LDS palette of its own and fills it, and `mine`, when its frame changes from one chain to the next.  *bad is
// lowered to the frame's number.  The parameter list is the same for both forms: the code of <.., false> is what it was without LOCAL.
template <bool LOSSY, bool LOCAL>
__global__ void __launch_bounds__(64 * GIF_CHAINS) gif_lzw_kernel(const GifFrame* __restrict__ frames, int n_frames, long long n_segs,
                                                                   int K, int m, unsigned* __restrict__ words,
                                                                   unsigned long long* __restrict__ seg_bits, unsigned long long* __restrict__ bad,
                                                                   std::conditional_t<LOCAL, const GifLocal*, const unsigned*> __restrict__ rgb,
                                                                   int T, int lossy) {
    __shared__ unsigned table[GIF_CHAINS][GIF_SLOTS];
    __shared__ uint4 stage[GIF_CHAINS][2][GIF_STAGE / 8];
    __shared__ unsigned pal[LOSSY ? (LOCAL ? 256 * GIF_CHAINS : 256) : 1];     // the colour of the index at hand is read from here (a broadcast)
    const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
    unsigned* tab = table[wv];
    unsigned* wpal = pal + (LOSSY && LOCAL ? 256 * wv : 0);                      // LOCAL: this wave's palette
    unsigned mine[4] = {0, 0, 0, 0};               // this lane's four candidates' colours
    if constexpr (LOSSY && !LOCAL) {
        static_assert(64 * GIF_CHAINS == 256, "one thread per colour table entry");
        pal[threadIdx.x] = rgb[threadIdx.x];
        for (int j = 0; j < 4; ++j) mine[j] = rgb[lane + 64 * j];
        __syncthreads();
    }
    unsigned CLEAR = 1u << m, EOI = CLEAR + 1;
    int held = -1;                                 // LOCAL: the frame whose K, m, T and colours this wave holds
    for (long long g = (long long) blockIdx.x * GIF_CHAINS + wv; g < n_segs; g += (long long) gridDim.x * GIF_CHAINS) {
        int lo = 0, hi = n_frames - 1;                 // frame of segment g: the last one whose first segment is <= g
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (frames[mid].seg_base <= g) lo = mid; else hi = mid - 1;
        }
        if constexpr (LOCAL) {
            if (lo != held) {                          // (g is the same in every lane of the wave, so is this branch)
                const GifLocal& P = rgb[lo];
                K = P.Kt; m = P.m; T = P.T;
                CLEAR = 1u << m; EOI = CLEAR + 1;
                if constexpr (LOSSY) {
                    wave_sync();                       // the chain before has read this wave's palette for the last time
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        mine[j] = P.rgb[lane + 64 * j];
                        wpal[lane + 64 * j] = mine[j];
                    }
                    wave_sync();
                }
                held = lo;
            }
        }
        const GifFrame& F = frames[lo];
        const long long s = g - F.seg_base;
        const long long b = s * F.seg_len;
        const long long L = min((long long) F.seg_len, F.npix - b);
        const uintptr_t flo = reinterpret_cast<uintptr_t>(F.index), fhi = flo + 2 * (uintptr_t) F.npix;
        const uintptr_t a0 = (flo + 2 * (uintptr_t) b) & ~(uintptr_t) 15;        // staging window: 16-byte aligned
        const long long q0 = (long long) (((flo + 2 * (uintptr_t) b) & 15) >> 1), qend = q0 + L;
        const long long nblk = (qend + GIF_STAGE - 1) / GIF_STAGE;
        unsigned* __restrict__ out = words + F.word_base + s * F.seg_words;
        unsigned long long acc = 0;
        int nb = 0;
        long long wpos = 0;
        auto emit = [&](unsigned code, unsigned w) {
            acc |= (unsigned long long) code << nb;
            nb += (int) w;
            if (nb >= 32) {
                if (lane == 0) out[wpos] = (unsigned) acc;
                ++wpos; acc >>= 32; nb -= 32;
            }
        };
        bool badc = false;
        auto index_at = [&](long long q) -> unsigned {
            unsigned c = reinterpret_cast<const unsigned short*>(stage[wv][(q / GIF_STAGE) & 1])[q & (GIF_STAGE - 1)];
            if (c >= (unsigned) K) { badc = true; c &= 255u; }
            return c;
        };
        clear_table(tab, lane);
        stage[wv][0][lane] = load_chunk(a0 + 16 * (uintptr_t) lane, flo, fhi);
        wave_sync();
        unsigned w = m + 1, next = EOI + 1;
        if (s == 0) emit(CLEAR, w);
        unsigned pre = index_at(q0);
        long long q = q0 + 1;
        for (long long k = 0; k < nblk; ++k) {
            // the next block's indices are in flight while this block is encoded
            const uint4 nv = k + 1 < nblk ? load_chunk(a0 + (uintptr_t) (k + 1) * 1024 + 16 * (uintptr_t) lane, flo, fhi) : make_uint4(0, 0, 0, 0);
            const long long e = min(qend, (k + 1) * GIF_STAGE);
            for (; q < e; ++q) {
                const unsigned c = index_at(q);
                const unsigned key = pre << 8 | c;
                unsigned h;
                unsigned code = find_code(tab, key, &h);
                if (code) { pre = code; continue; }
                if constexpr (LOSSY) {
                    if (c != (unsigned) T) {
                        wave_sync();                                            // lane 0's dictionary stores, read by every lane below
                        const unsigned want = wpal[c];
                        unsigned best = ~0u, best_code = 0;                     // this lane's smallest d^2 << 8 | c' and its code
#pragma unroll
                        for (int j = 0; j < 4; ++j) {
                            const unsigned cc = (unsigned) lane + 64u * j;
                            const uint2 d = rgb_apart(mine[j], want);
                            if (cc < (unsigned) K && cc != c && cc != (unsigned) T && d.x <= (unsigned) lossy) {
                                unsigned at;
                                const unsigned cd = find_code(tab, pre << 8 | cc, &at);
                                const unsigned v = d.y << 8 | cc;
                                if (cd && v < best) { best = v; best_code = cd; }
                            }
                        }
                        unsigned win = best;
#pragma unroll
                        for (int d = 32; d >= 1; d >>= 1) win = min(win, (unsigned) __shfl_xor((int) win, d));
                        if (win != ~0u) {
                            // the winner's lane is the only one whose `best` names that c'
                            pre = (unsigned) __shfl((int) best_code, (int) (win & 63u));
                            continue;
                        }
                    }
                }
                emit(pre, w);
                if (next == 4096) {
                    emit(CLEAR, w);
                    wave_sync();
                    clear_table(tab, lane);
                    next = EOI + 1; w = m + 1;
                } else {
                    if (lane == 0) tab[h] = key << 12 | next;
                    if (next == (1u << w) && w < 12) ++w;
                    ++next;
                }
                pre = c;
            }
            wave_sync();
            stage[wv][(k + 1) & 1][lane] = nv;
            wave_sync();
        }
        emit(pre, w);
        if (next == (1u << w) && w < 12) ++w;       // the decoder adds its last entry on reading `pre`
        emit(s == F.nseg - 1 ? EOI : CLEAR, w);
        if (lane == 0) {
            if (nb > 0) out[wpos] = (unsigned) acc;
            seg_bits[g] = (unsigned long long) wpos * 32 + nb;
            if constexpr (LOCAL) {
                if (badc) atomicMin(bad, (unsigned long long) lo);
            } else {
                if (badc) *bad = 1;
            }
        }
        wave_sync();
    }
}

// one workgroup per frame: seg_off[i] = bits of the frame's segments before i; frame_bits[f] = the frame's total
__global__ void __launch_bounds__(256) gif_scan_kernel(const GifFrame* __restrict__ frames, const unsigned long long* __restrict__ seg_bits,
                                                       unsigned long long* __restrict__ seg_off, unsigned long long* __restrict__ frame_bits) {
    __shared__ unsigned long long part[256];
    const GifFrame& F = frames[blockIdx.x];
    unsigned long long carry = 0;
    for (long long c0 = 0; c0 < F.nseg; c0 += 256) {
        const long long i = c0 + threadIdx.x;
        const unsigned long long v = i < F.nseg ? seg_bits[F.seg_base + i] : 0;
        part[threadIdx.x] = v;
        __syncthreads();
        for (int d = 1; d < 256; d <<= 1) {
            const unsigned long long add = threadIdx.x >= (unsigned) d ? part[threadIdx.x - d] : 0;
            __syncthreads();
            part[threadIdx.x] += add;
            __syncthreads();
        }
        if (i < F.nseg) seg_off[F.seg_base + i] = carry + part[threadIdx.x] - v;
        carry += part[255];
        __syncthreads();
    }
    if (threadIdx.x == 0) frame_bits[blockIdx.x] = carry;
}

// bits [lo, lo + cnt) (cnt <= 8) of a segment's bit string
__device__ inline unsigned seg_bits_at(const unsigned* __restrict__ sw, unsigned long long lo, int cnt) {
    const unsigned long long wi = lo >> 5;
    const unsigned long long v = (unsigned long long) sw[wi] | (unsigned long long) sw[wi + 1] << 32;
    return (unsigned) (v >> (lo & 31)) & ((1u << cnt) - 1u);
}

// data byte j of frame F: bits [8j, 8j + 8) of its segments' strings one after another
__device__ inline unsigned data_byte(const GifFrame& F, long long j, const unsigned* __restrict__ words, const unsigned long long* __restrict__ seg_bits,
                                     const unsigned long long* __restrict__ seg_off) {
    const unsigned long long bp = 8ull * (unsigned long long) j;
    long long lo = 0, hi = F.nseg - 1;                 // the last segment starting at or before bp
    while (lo < hi) {
        const long long mid = (lo + hi + 1) >> 1;
        if (seg_off[F.seg_base + mid] <= bp) lo = mid; else hi = mid - 1;
    }
    unsigned v = 0;
    for (long long t = lo; t < F.nseg; ++t) {
        const unsigned long long so = seg_off[F.seg_base + t];
        if (so >= bp + 8) break;
        const unsigned long long se = so + seg_bits[F.seg_base + t];
        const unsigned long long a = so > bp ? so : bp, e = se < bp + 8 ? se : bp + 8;
        if (a < e) v |= seg_bits_at(words + F.word_base + t * F.seg_words, a - so, (int) (e - a)) << (a - bp);
    }
    return v;
}

__global__ void __launch_bounds__(256) gif_gather_kernel(const GifFrame* __restrict__ frames, int n_frames, const unsigned* __restrict__ words,
                                                         const unsigned long long* __restrict__ seg_bits, const unsigned long long* __restrict__ seg_off,
                                                         const unsigned char* __restrict__ blob, unsigned char* __restrict__ file, long long total) {
    for (long long o = (long long) blockIdx.x * blockDim.x + threadIdx.x; o < total; o += (long long) gridDim.x * blockDim.x) {
        unsigned v = 0x3B;                             // trailer
        if (o < total - 1) {
            int lo = 0, hi = n_frames - 1;
            while (lo < hi) {
                const int mid = (lo + hi + 1) >> 1;
                if (frames[mid].file_off <= o) lo = mid; else hi = mid - 1;
            }
            const GifFrame& F = frames[lo];
            const long long r = o - F.file_off;
            if (r < F.prefix_len) v = blob[F.prefix_off + r];
            else {
                const long long j = r - F.prefix_len;  // sub-block stream: {len, up to 255 data bytes}..., 0
                const long long blk = j >> 8, rr = j & 255;
                if (j == F.stream_len - 1) v = 0;
                else if (rr == 0) v = (unsigned) min(255ll, F.data_bytes - 255 * blk);
                else v = data_byte(F, 255 * blk + rr - 1, words, seg_bits, seg_off);
            }
        }
        file[o] = (unsigned char) v;
    }
}

// ---- delta mode ----

// the 16 bytes at byte address addr (2-byte aligned, no more), put together from the two aligned chunks around them; the elements
// outside [lo, hi) read as 0 and are never loaded.  addr is the same in every lane modulo 16, so the branches are uniform.
__device__ inline uint4 load_chunk_at(uintptr_t addr, uintptr_t lo, uintptr_t hi) {
    const uintptr_t a = addr & ~(uintptr_t) 15;
    const unsigned sh = (unsigned) (addr & 15);
    const uint4 A = load_chunk(a, lo, hi);
    if (sh == 0) return A;
    const uint4 B = load_chunk(a + 16, lo, hi);
    const unsigned v[8] = {A.x, A.y, A.z, A.w, B.x, B.y, B.z, B.w};
    const unsigned d = sh >> 2;
    const bool half = (sh & 2) != 0;
    unsigned r[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        unsigned l = v[k], u = v[k + 1];
#pragma unroll
        for (int t = 1; t < 4; ++t)
            if (d == (unsigned) t) { l = v[k + t]; u = v[k + t + 1]; }
        r[k] = half ? (l >> 16 | u << 16) : l;
    }
    return make_uint4(r[0], r[1], r[2], r[3]);
}

__device__ inline bool pair_bad(unsigned v, unsigned K) { return (v & 0xFFFFu) >= K || (v >> 16) >= K; }

// Frame f >= 1 against frame f - 1, eight pixels (one aligned 16-byte chunk of frame f) per thread and step: the bounding box of the
// pixels that differ, reduced over the wave and added to box[4 * (f - 1) ..] with one atomic min / max per wave that saw a difference.
// blockIdx.y strides over the frames, blockIdx.x over a frame's chunks.  W * H < 2^32, so pixel numbers fit an unsigned.
__global__ void __launch_bounds__(256) gif_diff_kernel(const unsigned short* const* __restrict__ index, int n_frames, int W, long long npix,
                                                       int K, int* __restrict__ box, int* __restrict__ bad) {
    bool badc = false;
    for (int f = (int) blockIdx.y + 1; f < n_frames; f += (int) gridDim.y) {
        const uintptr_t clo = reinterpret_cast<uintptr_t>(index[f]), chi = clo + 2 * (uintptr_t) npix;
        const uintptr_t plo = reinterpret_cast<uintptr_t>(index[f - 1]), phi = plo + 2 * (uintptr_t) npix;
        const uintptr_t a0 = clo & ~(uintptr_t) 15;
        const long long nchunk = (long long) ((chi - a0 + 15) >> 4);
        int x0 = 0x7FFFFFFF, y0 = 0x7FFFFFFF, x1 = -1, y1 = -1;
        for (long long c = (long long) blockIdx.x * blockDim.x + threadIdx.x; c < nchunk; c += (long long) gridDim.x * blockDim.x) {
            const uintptr_t a = a0 + 16 * (uintptr_t) c;
            const long long p0 = ((long long) a - (long long) clo) / 2;          // pixel of the chunk's first element: -7 .. npix - 1
            const uint4 cu = load_chunk(a, clo, chi);
            const uint4 pv = load_chunk_at(plo + (uintptr_t) (2 * p0), plo, phi);
            badc = badc || pair_bad(cu.x, K) || pair_bad(cu.y, K) || pair_bad(cu.z, K) || pair_bad(cu.w, K)
                        || pair_bad(pv.x, K) || pair_bad(pv.y, K) || pair_bad(pv.z, K) || pair_bad(pv.w, K);
            const unsigned dx[4] = {cu.x ^ pv.x, cu.y ^ pv.y, cu.z ^ pv.z, cu.w ^ pv.w};
            if ((dx[0] | dx[1] | dx[2] | dx[3]) == 0) continue;                  // (elements outside the frames are 0 in both)
            const unsigned first = p0 > 0 ? (unsigned) p0 : 0u;
            int y = (int) (first / (unsigned) W), x = (int) (first % (unsigned) W);
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                if (p0 + j < 0) continue;
                if ((dx[j >> 1] >> (16 * (j & 1))) & 0xFFFFu) {
                    x0 = min(x0, x); x1 = max(x1, x); y0 = min(y0, y); y1 = max(y1, y);
                }
                if (++x == W) { x = 0; ++y; }
            }
        }
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) {
            x0 = min(x0, __shfl_xor(x0, d)); y0 = min(y0, __shfl_xor(y0, d));
            x1 = max(x1, __shfl_xor(x1, d)); y1 = max(y1, __shfl_xor(y1, d));
        }
        if ((threadIdx.x & 63) == 0 && x1 >= 0) {
            int* b = box + 4 * (f - 1);
            atomicMin(b + 0, x0); atomicMin(b + 1, y0); atomicMax(b + 2, x1); atomicMax(b + 3, y1);
        }
    }
    if (badc) *bad = 1;                            // (every thread that stores, stores the same value)
}

// Body of frame f's rectangle: eight consecutive body pixels per thread, one 16-byte store.  The sources are read element by element
// (a rectangle's rows start anywhere); both reads stay inside the frame because the rectangle does.
__global__ void __launch_bounds__(256) gif_body_kernel(const GifDelta* __restrict__ delta, int n_bodies, int W, int u) {
    for (int f = (int) blockIdx.y; f < n_bodies; f += (int) gridDim.y) {
        const GifDelta D = delta[f];
        const unsigned area = (unsigned) D.w * (unsigned) D.h;                   // <= W * H < 2^32
        const long long nchunk = ((long long) area + 7) >> 3;
        for (long long c = (long long) blockIdx.x * blockDim.x + threadIdx.x; c < nchunk; c += (long long) gridDim.x * blockDim.x) {
            const unsigned e0 = (unsigned) (8 * c);
            unsigned r = e0 / (unsigned) D.w, col = e0 % (unsigned) D.w;
            unsigned v[4] = {0, 0, 0, 0};
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                if ((long long) e0 + j < (long long) area) {
                    const size_t src = (size_t) (D.y + (int) r) * (size_t) W + (size_t) (D.x + (int) col);
                    const unsigned cv = D.cur[src], pv = D.prev[src];
                    v[j >> 1] |= (u >= 0 && cv == pv ? (unsigned) u : cv) << (16 * (j & 1));
                }
                if (++col == (unsigned) D.w) { col = 0; ++r; }
            }
            reinterpret_cast<uint4*>(D.body)[c] = make_uint4(v[0], v[1], v[2], v[3]);
        }
    }
}

// ---- local colour tables ("GIF encoding, local colour tables"): the two delta passes compare colours, not indices ----

// frame f - 1's written table to tab[0], frame f's to tab[1], one entry per thread of the workgroup (256); the barriers keep the
// readers of the pair before and of this pair apart
__device__ inline void load_tables(unsigned (*tab)[256], const GifLocal* __restrict__ local, int f) {
    __syncthreads();
    tab[0][threadIdx.x] = local[f - 1].rgb[threadIdx.x];
    tab[1][threadIdx.x] = local[f].rgb[threadIdx.x];
    __syncthreads();
}

// gif_diff_kernel with "differs" judged on the colour shown: the same grid, chunk loads, shifted predecessor and wave reduction.  The
// two tables are refilled whenever blockIdx.y's stride moves on (f is the same in every thread of a workgroup, so are the barriers).
// An index is checked against its own frame's K and masked to 8 bits before it addresses the table.  An element outside the frame was
// not loaded and is not compared: equal indices no longer mean equal colours, so the zeros standing for it must not reach the tables.
__global__ void __launch_bounds__(256) gif_diff_local_kernel(const unsigned short* const* __restrict__ index, int n_frames, int W, long long npix,
                                                             const GifLocal* __restrict__ local, int* __restrict__ box, int* __restrict__ bad) {
    __shared__ unsigned tab[2][256];
    int badf = 0x7FFFFFFF;
    for (int f = (int) blockIdx.y + 1; f < n_frames; f += (int) gridDim.y) {
        load_tables(tab, local, f);
        const unsigned Kp = (unsigned) local[f - 1].K, Kc = (unsigned) local[f].K;
        const uintptr_t clo = reinterpret_cast<uintptr_t>(index[f]), chi = clo + 2 * (uintptr_t) npix;
        const uintptr_t plo = reinterpret_cast<uintptr_t>(index[f - 1]), phi = plo + 2 * (uintptr_t) npix;
        const uintptr_t a0 = clo & ~(uintptr_t) 15;
        const long long nchunk = (long long) ((chi - a0 + 15) >> 4);
        int x0 = 0x7FFFFFFF, y0 = 0x7FFFFFFF, x1 = -1, y1 = -1;
        for (long long c = (long long) blockIdx.x * blockDim.x + threadIdx.x; c < nchunk; c += (long long) gridDim.x * blockDim.x) {
            const uintptr_t a = a0 + 16 * (uintptr_t) c;
            const long long p0 = ((long long) a - (long long) clo) / 2;          // pixel of the chunk's first element: -7 .. npix - 1
            const uint4 cu = load_chunk(a, clo, chi);
            const uint4 pv = load_chunk_at(plo + (uintptr_t) (2 * p0), plo, phi);
            if (pair_bad(cu.x, Kc) || pair_bad(cu.y, Kc) || pair_bad(cu.z, Kc) || pair_bad(cu.w, Kc)) badf = min(badf, f);
            if (pair_bad(pv.x, Kp) || pair_bad(pv.y, Kp) || pair_bad(pv.z, Kp) || pair_bad(pv.w, Kp)) badf = min(badf, f - 1);
            const unsigned ce[4] = {cu.x, cu.y, cu.z, cu.w}, pe[4] = {pv.x, pv.y, pv.z, pv.w};
            const unsigned first = p0 > 0 ? (unsigned) p0 : 0u;
            int y = (int) (first / (unsigned) W), x = (int) (first % (unsigned) W);
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                if (p0 + j < 0 || p0 + j >= npix) continue;
                const unsigned ci = (ce[j >> 1] >> (16 * (j & 1))) & 255u, pi = (pe[j >> 1] >> (16 * (j & 1))) & 255u;
                if (tab[1][ci] != tab[0][pi]) {
                    x0 = min(x0, x); x1 = max(x1, x); y0 = min(y0, y); y1 = max(y1, y);
                }
                if (++x == W) { x = 0; ++y; }
            }
        }
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) {
            x0 = min(x0, __shfl_xor(x0, d)); y0 = min(y0, __shfl_xor(y0, d));
            x1 = max(x1, __shfl_xor(x1, d)); y1 = max(y1, __shfl_xor(y1, d));
        }
        if ((threadIdx.x & 63) == 0 && x1 >= 0) {
            int* b = box + 4 * (f - 1);
            atomicMin(b + 0, x0); atomicMin(b + 1, y0); atomicMax(b + 2, x1); atomicMax(b + 3, y1);
        }
    }
    if (badf != 0x7FFFFFFF) atomicMin(bad, badf);
}

// gif_body_kernel with the same comparison; body b is frame b + 1 against frame b and takes its u from frame b + 1's record
__global__ void __launch_bounds__(256) gif_body_local_kernel(const GifDelta* __restrict__ delta, int n_bodies, int W,
                                                             const GifLocal* __restrict__ local) {
    __shared__ unsigned tab[2][256];
    for (int f = (int) blockIdx.y; f < n_bodies; f += (int) gridDim.y) {
        load_tables(tab, local, f + 1);
        const int u = local[f + 1].T;
        const GifDelta D = delta[f];
        const unsigned area = (unsigned) D.w * (unsigned) D.h;                   // <= W * H < 2^32
        const long long nchunk = ((long long) area + 7) >> 3;
        for (long long c = (long long) blockIdx.x * blockDim.x + threadIdx.x; c < nchunk; c += (long long) gridDim.x * blockDim.x) {
            const unsigned e0 = (unsigned) (8 * c);
            unsigned r = e0 / (unsigned) D.w, col = e0 % (unsigned) D.w;
            unsigned v[4] = {0, 0, 0, 0};
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                if ((long long) e0 + j < (long long) area) {
                    const size_t src = (size_t) (D.y + (int) r) * (size_t) W + (size_t) (D.x + (int) col);
                    const unsigned cv = D.cur[src], pv = D.prev[src];
                    v[j >> 1] |= (u >= 0 && tab[1][cv & 255u] == tab[0][pv & 255u] ? (unsigned) u : cv) << (16 * (j & 1));
                }
                if (++col == (unsigned) D.w) { col = 0; ++r; }
            }
            reinterpret_cast<uint4*>(D.body)[c] = make_uint4(v[0], v[1], v[2], v[3]);
        }
    }
}

} // namespace

void launch_gif_diff(const unsigned short* const* d_index, int n_frames, int W, int H, int K, int* d_box, int* d_bad, hipStream_t s) {
    const long long npix = (long long) W * H;
    long long gx = ((npix + 7) / 8 + 1 + 255) / 256;
    if (gx > 1024) gx = 1024;
    const int gy = n_frames - 1 < 65535 ? n_frames - 1 : 65535;
    hipLaunchKernelGGL(gif_diff_kernel, dim3((unsigned) gx, (unsigned) gy), dim3(256), 0, s, d_index, n_frames, W, npix, K, d_box, d_bad);
}

void launch_gif_body(const GifDelta* d_delta, int n_bodies, int W, int u, long long max_area, hipStream_t s) {
    long long gx = ((max_area + 7) / 8 + 255) / 256;
    if (gx > 1024) gx = 1024;
    if (gx < 1) gx = 1;
    const int gy = n_bodies < 65535 ? n_bodies : 65535;
    hipLaunchKernelGGL(gif_body_kernel, dim3((unsigned) gx, (unsigned) gy), dim3(256), 0, s, d_delta, n_bodies, W, u);
}

void launch_gif_lzw(const GifFrame* d_frames, int n_frames, long long n_segs, int K, int m, unsigned* d_words, unsigned long long* d_seg_bits,
                    unsigned long long* d_bad, const unsigned* d_rgb, int T, int lossy, hipStream_t s) {
    long long grid = (n_segs + GIF_CHAINS - 1) / GIF_CHAINS;
    if (grid > (1 << 20)) grid = 1 << 20;
    if (lossy > 0)
        hipLaunchKernelGGL((gif_lzw_kernel<true, false>), dim3((unsigned) grid), dim3(64 * GIF_CHAINS), 0, s, d_frames, n_frames, n_segs, K, m, d_words,
                           d_seg_bits, d_bad, d_rgb, T, lossy);
    else
        hipLaunchKernelGGL((gif_lzw_kernel<false, false>), dim3((unsigned) grid), dim3(64 * GIF_CHAINS), 0, s, d_frames, n_frames, n_segs, K, m, d_words,
                           d_seg_bits, d_bad, (const unsigned*) nullptr, -1, 0);
}

void launch_gif_lzw_local(const GifFrame* d_frames, int n_frames, long long n_segs, const GifLocal* d_local, unsigned* d_words,
                          unsigned long long* d_seg_bits, unsigned long long* d_bad, int lossy, hipStream_t s) {
    long long grid = (n_segs + GIF_CHAINS - 1) / GIF_CHAINS;
    if (grid > (1 << 20)) grid = 1 << 20;
    if (lossy > 0)
        hipLaunchKernelGGL((gif_lzw_kernel<true, true>), dim3((unsigned) grid), dim3(64 * GIF_CHAINS), 0, s, d_frames, n_frames, n_segs, 0, 0, d_words,
                           d_seg_bits, d_bad, d_local, -1, lossy);
    else
        hipLaunchKernelGGL((gif_lzw_kernel<false, true>), dim3((unsigned) grid), dim3(64 * GIF_CHAINS), 0, s, d_frames, n_frames, n_segs, 0, 0, d_words,
                           d_seg_bits, d_bad, d_local, -1, 0);
}

void launch_gif_diff_local(const unsigned short* const* d_index, int n_frames, int W, int H, const GifLocal* d_local, int* d_box, int* d_bad,
                           hipStream_t s) {
    const long long npix = (long long) W * H;
    long long gx = ((npix + 7) / 8 + 1 + 255) / 256;
    if (gx > 1024) gx = 1024;
    const int gy = n_frames - 1 < 65535 ? n_frames - 1 : 65535;
    hipLaunchKernelGGL(gif_diff_local_kernel, dim3((unsigned) gx, (unsigned) gy), dim3(256), 0, s, d_index, n_frames, W, npix, d_local, d_box, d_bad);
}

void launch_gif_body_local(const GifDelta* d_delta, int n_bodies, int W, const GifLocal* d_local, long long max_area, hipStream_t s) {
    long long gx = ((max_area + 7) / 8 + 255) / 256;
    if (gx > 1024) gx = 1024;
    if (gx < 1) gx = 1;
    const int gy = n_bodies < 65535 ? n_bodies : 65535;
    hipLaunchKernelGGL(gif_body_local_kernel, dim3((unsigned) gx, (unsigned) gy), dim3(256), 0, s, d_delta, n_bodies, W, d_local);
}

void launch_gif_scan(const GifFrame* d_frames, int n_frames, const unsigned long long* d_seg_bits, unsigned long long* d_seg_off,
                     unsigned long long* d_frame_bits, hipStream_t s) {
    hipLaunchKernelGGL(gif_scan_kernel, dim3((unsigned) n_frames), dim3(256), 0, s, d_frames, d_seg_bits, d_seg_off, d_frame_bits);
}

void launch_gif_gather(const GifFrame* d_frames, int n_frames, const unsigned* d_words, const unsigned long long* d_seg_bits,
                       const unsigned long long* d_seg_off, const unsigned char* d_blob, unsigned char* d_file, long long total, hipStream_t s) {
    long long grid = (total + 255) / 256;
    if (grid > 256 * 64) grid = 256 * 64;
    hipLaunchKernelGGL(gif_gather_kernel, dim3((unsigned) grid), dim3(256), 0, s, d_frames, n_frames, d_words, d_seg_bits, d_seg_off, d_blob, d_file, total);
}

} // namespace nq
