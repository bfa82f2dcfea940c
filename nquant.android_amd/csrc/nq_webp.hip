// nq_webp.hip -- lossless WebP (VP8L) bit strings from palette index maps on gfx950 (include/nquant_abi.h, "WebP encoding"; DESIGN.md
// "WebP encoder").
//
// After the colour-indexing transform a VP8L image is one byte per packed pixel (2 / 4 / 8 indices in it at K <= 16 / 4 / 2).  The
// packed image is cut into bands of 2^p packed rows; the entropy image gives every band a group of prefix codes of its own, so a band
// is one chain that sees only its own bytes -- the shape of a PNG segment with its dynamic block, and the chains run in parallel.
//   webp_chain_kernel   one wave per chain, one chain per workgroup: the band is packed into LDS, parsed 64 positions at a time (the
//                       PNG encoder's hash / greedy scheme: tokens to global scratch), the green and the distance code are built, and
//                       two bit strings are emitted: the five code headers, and the pixel data
//   webp_scan_kernel    per image: exclusive scan of the bit lengths of its segments (the host's bits, the headers, the data)
//   webp_gather_kernel  one thread per byte of the file: container bytes from the host's blob, image bytes ORed from the segments
//                       each overlaps, the RIFF padding byte
// An "image" of a call is whatever one VP8L chunk encodes: a whole index map, or a frame's changed rectangle read in place.
#include "nq_kernels.h"

namespace nq {

namespace {

constexpr int WEBP_HASH_BITS = 13;
constexpr unsigned WEBP_NONE = 0xFFFFu;    // "no position" in the head table (positions are < 32768)
constexpr int WEBP_WIN = 108;              // emit window, words: 31 carried bits + 64 items of <= 51 bits
constexpr int WEBP_GREEN = 280, WEBP_DIST = 40;   // 256 literals + 24 length prefixes (no colour cache); distance prefixes
constexpr int WEBP_MAX_MATCH = 258;

// the tables of one chain (LDS, after the band's bytes and the head table)
struct WebpTables {
    unsigned hist_g[WEBP_GREEN], hist_d[WEBP_DIST], hist_c[20];   // symbol counts: green, distance, code-length code
    unsigned W[2 * WEBP_GREEN];                        // tree node weights: the sorted leaves, then the internal nodes
    unsigned win[WEBP_WIN];                            // emit window
    unsigned short code_g[WEBP_GREEN], code_d[WEBP_DIST], code_c[20];   // canonical codes, bit-reversed
    unsigned short sorted[WEBP_GREEN], parent[2 * WEBP_GREEN];
    unsigned short cls[288];                           // code-length sequence: symbol | extra value << 8
    unsigned short cnt[16], next[16];
    unsigned char len_g[WEBP_GREEN], len_d[WEBP_DIST], len_c[20], depth[2 * WEBP_GREEN];
    int n_used, n_cls, ncl;
    static constexpr int WIN = WEBP_WIN;
};

#include "nq_lz.inc"                       // wave_sync, ballot64, ctz64, top64, build_code, BitOut, emit_items

// the order in which VP8L stores the lengths of the code-length code
__device__ const unsigned char kWebpClOrder[19] = {17, 18, 0, 1, 2, 3, 4, 5, 16, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15};

// {prefix symbol, extra bits, extra value} of a length or distance code v = d + 1
__device__ inline void prefix_symbol(unsigned d, unsigned& sym, unsigned& eb, unsigned& ev) {
    if (d < 4) { sym = d; eb = 0; ev = 0; return; }
    const unsigned nb = 31 - __clz(d);
    eb = nb - 1;
    sym = 2 * nb + ((d >> eb) & 1);
    ev = d & ((1u << eb) - 1);
}

// The prefix code of the nsym symbols counted in hist, built and written to the header string.  At most one used symbol (it is a
// literal or a distance prefix, so below 256): the simple form, and the symbol then costs no bits in the data (its length is set to
// 0).  Otherwise the normal form: the lengths of the code-length code, "all lengths follow", the nsym lengths in run-length symbols.
__device__ void emit_code(WebpTables& T, BitOut& B, const unsigned* hist, int nsym, unsigned char* lens, unsigned short* codes, int lane) {
    build_code(T, hist, nsym, 15, lens, codes, lane);
    const int used = T.n_used;
    const unsigned only = used ? T.sorted[0] & 255u : 0u;
    wave_sync();
    if (used <= 1) {
        if (lane == 0) lens[only] = 0;
        const bool wide = only > 1;
        emit_items(T, B, lane == 0 ? (1ull | (wide ? 4ull : 0ull) | (unsigned long long) only << 3) : 0ull, lane == 0 ? (wide ? 11 : 4) : 0, lane);
        return;
    }
    if (lane < 20) T.hist_c[lane] = 0;
    wave_sync();
    if (lane == 0) {
        int n = 0;
        auto put = [&](unsigned sym, unsigned extra) { T.cls[n++] = (unsigned short) (sym | extra << 8); T.hist_c[sym] += 1; };
        for (int i = 0; i < nsym;) {
            const unsigned v = lens[i];
            int r = 1;
            while (i + r < nsym && lens[i + r] == v) ++r;
            i += r;
            if (v == 0) {
                while (r >= 11) { const int c = min(r, 138); put(18, (unsigned) (c - 11)); r -= c; }
                if (r >= 3) { put(17, (unsigned) (r - 3)); r = 0; }
            } else {
                put(v, 0); --r;
                while (r >= 3) { const int c = min(r, 6); put(16, (unsigned) (c - 3)); r -= c; }
            }
            for (; r > 0; --r) put(v, 0);
        }
        T.n_cls = n;
    }
    wave_sync();
    build_code(T, T.hist_c, 19, 7, T.len_c, T.code_c, lane);
    if (lane == 0) {
        int ncl = 19;
        while (ncl > 4 && T.len_c[kWebpClOrder[ncl - 1]] == 0) --ncl;
        T.ncl = ncl;
    }
    wave_sync();
    {
        const int ncl = T.ncl;
        unsigned long long v = 0; int nb = 0;
        if (lane == 0) { v = (unsigned) (ncl - 4) << 1; nb = 5; }              // normal form, count of code-length-code lengths
        else if (lane <= ncl) { v = T.len_c[kWebpClOrder[lane - 1]]; nb = 3; }
        else if (lane == ncl + 1) nb = 1;                                       // 0: all nsym lengths follow
        emit_items(T, B, v, nb, lane);
    }
    const int n_cls = T.n_cls;
    for (int k0 = 0; k0 < n_cls; k0 += 64) {
        unsigned long long v = 0; int nb = 0;
        if (k0 + lane < n_cls) {
            const unsigned e = T.cls[k0 + lane], sym = e & 255u;
            nb = T.len_c[sym];
            v = (unsigned long long) T.code_c[sym] | (unsigned long long) (e >> 8) << nb;
            nb += sym == 16 ? 2 : sym == 17 ? 3 : sym == 18 ? 7 : 0;
        }
        emit_items(T, B, v, nb, lane);
    }
}

// the open word of a finished string goes out; returns its bit length (uniform)
__device__ inline unsigned long long close_string(WebpTables& T, BitOut& B, int lane) {
    if (lane == 0 && B.nb > 0) B.out[B.wpos] = T.win[0];
    wave_sync();
    if (lane == 0) T.win[0] = 0;
    wave_sync();
    return (unsigned long long) B.wpos * 32 + B.nb;
}

extern __shared__ uint4 webp_lds[];

// All 64 lanes of the wave work on one band; what is sequential (greedy selection, tree construction) runs on uniform values or in
// lane 0.  Every loop is bounded by the chain length, a table size or a symbol count; no workgroup waits for another.
__global__ void __launch_bounds__(64) webp_chain_kernel(const WebpImage* __restrict__ images, int n_images, long long n_chains, int buf_bytes,
                                                        unsigned* __restrict__ words, long long chain_words, unsigned long long* __restrict__ bits,
                                                        unsigned* __restrict__ tokens, long long tok_cap, int* __restrict__ bad) {
    unsigned char* buf = reinterpret_cast<unsigned char*>(webp_lds);
    unsigned short* head = reinterpret_cast<unsigned short*>(buf + buf_bytes);
    WebpTables& T = *reinterpret_cast<WebpTables*>(buf + buf_bytes + 2 * (1 << WEBP_HASH_BITS));
    const int lane = threadIdx.x;
    unsigned* __restrict__ tok = tokens + (long long) blockIdx.x * tok_cap;
    for (long long g = blockIdx.x; g < n_chains; g += gridDim.x) {
        int ilo = 0, ihi = n_images - 1;               // image of chain g: the last one whose first chain is <= g
        while (ilo < ihi) {
            const int mid = (ilo + ihi + 1) >> 1;
            if (images[mid].chain_base <= g) ilo = mid; else ihi = mid - 1;
        }
        const WebpImage& F = images[ilo];
        const int row0 = (int) (g - F.chain_base) * F.band_rows;
        const unsigned pw = (unsigned) F.pw, per = (unsigned) F.per, d = 8u / per, W = (unsigned) F.width, K = (unsigned) F.K;
        const int L = min(F.band_rows, F.height - row0) * (int) pw;             // <= tok_cap <= 32768
        // ---- stage: pack the band's bytes into LDS, four per lane and step ----
        for (int i = lane; i < (1 << WEBP_HASH_BITS) / 2; i += 64) reinterpret_cast<unsigned*>(head)[i] = 0xFFFFFFFFu;
        for (int i = lane; i < WEBP_GREEN; i += 64) T.hist_g[i] = 0;
        if (lane < WEBP_DIST) T.hist_d[lane] = 0;
        for (int i = lane; i < WEBP_WIN; i += 64) T.win[i] = 0;
        bool badc = false;
        for (int o4 = 4 * lane; o4 < L + 8; o4 += 256) {      // 8 zero bytes after the band: the match compare reads past its end
            unsigned word = 0;
            for (int j = 0; j < 4; ++j) {
                const int o = o4 + j;
                if (o >= L) break;
                const unsigned r = (unsigned) o / pw, c = (unsigned) o - r * pw;
                // the maps are read element by element: a rectangle's rows start at any x, nothing wider than 2 bytes is aligned
                const unsigned short* __restrict__ rowp = F.index + (long long) (row0 + (int) r) * F.pitch;
                const unsigned x0 = c * per;
                unsigned v = 0;
                for (unsigned k = 0; k < per; ++k) {
                    const unsigned x = x0 + k;
                    if (x >= W) break;
                    unsigned idx = rowp[x];
                    if (idx >= K) { badc = true; idx &= (1u << d) - 1u; }
                    v |= idx << (d * k);
                }
                word |= v << (8 * j);
            }
            reinterpret_cast<unsigned*>(buf)[o4 >> 2] = word;
        }
        wave_sync();
        // ---- parse: 64 positions per step ----
        int ntok = 0;
        int next_p = 0;                                // first position the parse has not covered
        for (int base = 0; base < L; base += 64) {
            const int p = base + lane;
            const bool valid = p + 2 < L;
            unsigned h = 0;
            if (valid) h = ((buf[p] | (unsigned) buf[p + 1] << 8 | (unsigned) buf[p + 2] << 16) * 0x9E3779B1u) >> (32 - WEBP_HASH_BITS);
            unsigned cand = valid ? head[h] : WEBP_NONE;
            wave_sync();
            if (valid) head[h] = (unsigned short) p;
            wave_sync();
            unsigned long long pending = ballot64(valid && head[h] != (unsigned short) p);
            wave_sync();
            // positions of this step that share a hash: each takes the one before it, the last one stays in the table
            for (int it = 0; it < 64 && pending; ++it) {
                const unsigned hv = __shfl(h, ctz64(pending));
                const bool mine = valid && h == hv;
                const unsigned long long mask = ballot64(mine);
                if (mine) {
                    const unsigned long long below = mask & ((1ull << lane) - 1ull);
                    if (below) cand = (unsigned) (base + top64(below));
                    if (lane == top64(mask)) head[h] = (unsigned short) p;
                }
                pending &= ~mask;
            }
            wave_sync();
            bool ok = valid && cand != WEBP_NONE;
            if (ok) ok = buf[cand] == buf[p] && buf[cand + 1] == buf[p + 1] && buf[cand + 2] == buf[p + 2];
            const unsigned long long M = ballot64(ok);
            const int end = min(base + 64, L);
            for (int it = 0; it < 64 && next_p < end; ++it) {
                const unsigned long long Mm = M >> (next_p - base);
                const int m = Mm ? next_p + ctz64(Mm) : end;          // literals [next_p, m), then a copy at m (if m < end)
                if (p >= next_p && p < m) {
                    const unsigned v = buf[p];
                    tok[ntok + (p - next_p)] = v;
                    atomicAdd(&T.hist_g[v], 1u);
                }
                ntok += m - next_p;
                next_p = m;
                if (m < end) {
                    const int q = (int) __shfl(cand, m - base);
                    const int cap = min(WEBP_MAX_MATCH, L - m);
                    const int o = 3 + 4 * lane;
                    unsigned x = 0;
                    if (o < cap) {
                        const unsigned a = buf[m + o] | (unsigned) buf[m + o + 1] << 8 | (unsigned) buf[m + o + 2] << 16 | (unsigned) buf[m + o + 3] << 24;
                        const unsigned c = buf[q + o] | (unsigned) buf[q + o + 1] << 8 | (unsigned) buf[q + o + 2] << 16 | (unsigned) buf[q + o + 3] << 24;
                        x = a ^ c;
                    }
                    const unsigned long long diff = ballot64(x != 0);
                    int len = cap;
                    if (diff) {
                        const int fl = ctz64(diff);
                        const unsigned xf = __shfl(x, fl);
                        len = min(cap, 3 + 4 * fl + ((__ffs((int) xf) - 1) >> 3));
                    }
                    if (lane == 0) {
                        const unsigned lc = (unsigned) (len - 3), dm = (unsigned) (m - q - 1);
                        tok[ntok] = 0x80000000u | lc << 16 | dm;
                        unsigned sym, eb, ev;
                        prefix_symbol(lc + 2u, sym, eb, ev);           // the length code is len: d = len - 1
                        T.hist_g[256 + sym] += 1;
                        prefix_symbol(dm + 120u, sym, eb, ev);         // the distance code is distance + 120: d = distance + 119
                        T.hist_d[sym] += 1;
                    }
                    ++ntok;
                    next_p = m + len;
                    wave_sync();
                }
            }
        }
        __threadfence();                               // the tokens are read back by other lanes below
        wave_sync();
        // ---- the five codes of the band's group: green, red (0), blue (0), alpha (255), distance ----
        unsigned* const cw = words + g * chain_words;
        BitOut B{cw, 0, 0};
        emit_code(T, B, T.hist_g, WEBP_GREEN, T.len_g, T.code_g, lane);
        {
            // three simple codes of one symbol: 1, count - 1 = 0, "8 bits" 0 / 1, the symbol
            const unsigned long long v = lane < 2 ? 1ull : lane == 2 ? (1ull | 4ull | 255ull << 3) : 0ull;
            emit_items(T, B, v, lane < 2 ? 4 : lane == 2 ? 11 : 0, lane);
        }
        emit_code(T, B, T.hist_d, WEBP_DIST, T.len_d, T.code_d, lane);
        const unsigned long long head_bits = close_string(T, B, lane);
        // ---- the pixel data ----
        B = BitOut{cw + WEBP_HEAD_WORDS, 0, 0};
        for (int k0 = 0; k0 < ntok; k0 += 64) {
            unsigned long long v = 0; int nb = 0;
            if (k0 + lane < ntok) {
                const unsigned t = tok[k0 + lane];
                if (t >> 31) {
                    unsigned sym, eb, ev;
                    prefix_symbol(((t >> 16) & 255u) + 2u, sym, eb, ev);
                    nb = T.len_g[256 + sym];
                    v = (unsigned long long) T.code_g[256 + sym] | (unsigned long long) ev << nb;
                    nb += (int) eb;
                    prefix_symbol((t & 0x7FFFu) + 120u, sym, eb, ev);
                    v |= ((unsigned long long) T.code_d[sym] | (unsigned long long) ev << T.len_d[sym]) << nb;
                    nb += T.len_d[sym] + (int) eb;
                } else {
                    nb = T.len_g[t];
                    v = T.code_g[t];
                }
            }
            emit_items(T, B, v, nb, lane);
        }
        const unsigned long long data_bits = close_string(T, B, lane);
        if (lane == 0) {
            bits[2 * g] = head_bits;
            bits[2 * g + 1] = data_bits;
        }
        if (badc) bad[ilo] = 1;
        __threadfence();                               // the next chain reuses the token scratch
        wave_sync();
    }
}

// segment t of image F (0: the host's bits; 1 .. nbands: the headers; then the data): its words and its bit length
struct WebpSeg { const unsigned* w; unsigned long long bits; };
__device__ inline WebpSeg webp_seg(const WebpImage& F, long long t, const unsigned* __restrict__ words, long long chain_words,
                                   const unsigned* __restrict__ pre, const unsigned long long* __restrict__ bits) {
    if (t == 0) return {pre + F.pre_word, (unsigned long long) F.pre_bits};
    const bool data = t > F.nbands;
    const long long c = F.chain_base + t - 1 - (data ? F.nbands : 0);
    return {words + c * chain_words + (data ? WEBP_HEAD_WORDS : 0), bits[2 * c + (data ? 1 : 0)]};
}

// one workgroup per image: off[image + 2 chain_base + t] = bits of the image's segments before t; res[image] = the image's bit length
__global__ void __launch_bounds__(256) webp_scan_kernel(const WebpImage* __restrict__ images, long long chain_words,
                                                        const unsigned long long* __restrict__ bits, unsigned long long* __restrict__ off,
                                                        unsigned long long* __restrict__ res) {
    __shared__ unsigned long long part[256];
    const WebpImage& F = images[blockIdx.x];
    const long long nseg = 1 + 2ll * F.nbands, seg_base = blockIdx.x + 2 * F.chain_base;
    unsigned long long carry = 0;
    for (long long c0 = 0; c0 < nseg; c0 += 256) {
        const long long i = c0 + threadIdx.x;
        const unsigned long long v = i < nseg ? webp_seg(F, i, nullptr, chain_words, nullptr, bits).bits : 0;
        part[threadIdx.x] = v;
        __syncthreads();
        for (int d = 1; d < 256; d <<= 1) {
            const unsigned long long add = threadIdx.x >= (unsigned) d ? part[threadIdx.x - d] : 0;
            __syncthreads();
            part[threadIdx.x] += add;
            __syncthreads();
        }
        if (i < nseg) off[seg_base + i] = carry + part[threadIdx.x] - v;
        carry += part[255];
        __syncthreads();
    }
    if (threadIdx.x == 0) res[blockIdx.x] = carry;
}

// bits [lo, lo + cnt) (cnt <= 8) of a segment's bit string
__device__ inline unsigned webp_bits_at(const unsigned* __restrict__ sw, unsigned long long lo, int cnt) {
    const unsigned long long wi = lo >> 5;
    const unsigned long long v = (unsigned long long) sw[wi] | (unsigned long long) sw[wi + 1] << 32;
    return (unsigned) (v >> (lo & 31)) & ((1u << cnt) - 1u);
}

// file layout of an image: prefix (container chunk headers, from the blob), data_bytes of its bit string, a zero byte if that is odd
__global__ void __launch_bounds__(256) webp_gather_kernel(const WebpImage* __restrict__ images, int n_images, const unsigned* __restrict__ words,
                                                          long long chain_words, const unsigned* __restrict__ pre,
                                                          const unsigned long long* __restrict__ bits, const unsigned long long* __restrict__ off,
                                                          const unsigned char* __restrict__ blob, unsigned char* __restrict__ file, long long total) {
    for (long long o = (long long) blockIdx.x * blockDim.x + threadIdx.x; o < total; o += (long long) gridDim.x * blockDim.x) {
        int ilo = 0, ihi = n_images - 1;
        while (ilo < ihi) {
            const int mid = (ilo + ihi + 1) >> 1;
            if (images[mid].file_off <= o) ilo = mid; else ihi = mid - 1;
        }
        const WebpImage& F = images[ilo];
        const long long r = o - F.file_off, j = r - F.prefix_len;
        unsigned v = 0;
        if (j < 0) v = blob[F.prefix_off + r];
        else if (j < F.data_bytes) {
            const long long nseg = 1 + 2ll * F.nbands, seg_base = ilo + 2 * F.chain_base;
            const unsigned long long bp = 8ull * (unsigned long long) j;
            long long lo = 0, hi = nseg - 1;           // the last segment starting at or before bp
            while (lo < hi) {
                const long long mid = (lo + hi + 1) >> 1;
                if (off[seg_base + mid] <= bp) lo = mid; else hi = mid - 1;
            }
            for (long long t = lo; t < nseg; ++t) {
                const unsigned long long so = off[seg_base + t];
                if (so >= bp + 8) break;
                const WebpSeg S = webp_seg(F, t, words, chain_words, pre, bits);
                const unsigned long long se = so + S.bits;
                const unsigned long long a = so > bp ? so : bp, e = se < bp + 8 ? se : bp + 8;
                if (a < e) v |= webp_bits_at(S.w, a - so, (int) (e - a)) << (a - bp);
            }
        }
        file[o] = (unsigned char) v;
    }
}

inline int webp_buf_bytes(int max_len) { return (max_len + 16 + 15) & ~15; }

} // namespace

size_t webp_chain_lds_bytes(int max_len) { return (size_t) webp_buf_bytes(max_len) + 2 * (1 << WEBP_HASH_BITS) + sizeof(WebpTables); }

hipError_t launch_webp_chains(const WebpImage* d_images, int n_images, long long n_chains, int max_len, int grid, unsigned* d_words,
                              unsigned long long* d_bits, unsigned* d_tokens, int* d_bad, hipStream_t s) {
    const size_t lds = webp_chain_lds_bytes(max_len);
    if (lds > 48 * 1024) {
        const hipError_t e = hipFuncSetAttribute((const void*) webp_chain_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int) lds);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(webp_chain_kernel, dim3((unsigned) grid), dim3(64), lds, s, d_images, n_images, n_chains, webp_buf_bytes(max_len), d_words,
                       webp_chain_words(max_len), d_bits, d_tokens, (long long) max_len, d_bad);
    return hipSuccess;
}

void launch_webp_scan(const WebpImage* d_images, int n_images, int max_len, const unsigned long long* d_bits, unsigned long long* d_off,
                      unsigned long long* d_res, hipStream_t s) {
    hipLaunchKernelGGL(webp_scan_kernel, dim3((unsigned) n_images), dim3(256), 0, s, d_images, webp_chain_words(max_len), d_bits, d_off, d_res);
}

void launch_webp_gather(const WebpImage* d_images, int n_images, int max_len, const unsigned* d_words, const unsigned* d_pre,
                        const unsigned long long* d_bits, const unsigned long long* d_off, const unsigned char* d_blob, unsigned char* d_file,
                        long long total, hipStream_t s) {
    long long grid = (total + 255) / 256;
    if (grid > 256 * 64) grid = 256 * 64;
    hipLaunchKernelGGL(webp_gather_kernel, dim3((unsigned) grid), dim3(256), 0, s, d_images, n_images, d_words, webp_chain_words(max_len), d_pre,
                       d_bits, d_off, d_blob, d_file, total);
}

} // namespace nq
