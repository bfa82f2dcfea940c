// nq_png.hip -- indexed PNG files from palette index maps on gfx950 (include/nquant_abi.h, "PNG encoding"; DESIGN.md "PNG encoder").
//
// An image's raw stream (per row: filter byte 0 + the indices packed at the bit depth) is cut into segments of S bytes.  Every segment
// is one deflate chain that sees only its own bytes and emits one dynamic-Huffman block, so the chains run in parallel; an image's
// deflate data is the chains' bit strings one after another (a block may start at any bit).
//   png_deflate_kernel  one wave per chain, one chain per workgroup: the segment is packed into LDS, parsed 64 positions at a time
//                       (hash heads in LDS, tokens to global scratch), the three Huffman codes are built and the block is emitted
//   png_scan_kernel     per image: exclusive scan of the segments' bit lengths, Adler-32 of the raw stream from the segments' partials
//   png_gather_kernel   one thread per byte of the files: header bytes from the host's blob, data bytes ORed from the <= 2 segments
//                       each overlaps (a block is longer than 8 bits), Adler-32, IEND
//   png_crc_kernel      CRC-32 of every data chunk (IDAT, or an APNG frame's fdAT): per-thread partials moved to the chunk's end by
//                       x^n mod P and XORed together
//   png_crc_store_kernel  the four CRC bytes into the files
// An "image" of a call is whatever one zlib stream encodes: a whole index map, or (APNG) a frame's changed rectangle read in place
// from two maps, with the unchanged pixels packed as one index.  Several images may lie in one file, each in a data chunk of its own.
#include "nq_kernels.h"

namespace nq {

namespace {

constexpr int PNG_HASH_BITS = 13;
constexpr unsigned PNG_NONE = 0xFFFFu;   // "no position" in the head table (positions are < 65535)
constexpr int PNG_WIN = 104;             // emit window, words: 31 carried bits + 64 items of <= 48 bits
constexpr int PNG_CRC_CHUNK = 128;       // bytes per thread of png_crc_kernel
constexpr unsigned ADLER_MOD = 65521u;

// the tables of one chain (LDS, after the segment bytes and the head table)
struct PngTables {
    unsigned hist_l[288], hist_d[32], hist_c[20];      // symbol counts: literal/length, distance, code-length code
    unsigned W[576];                                   // tree node weights: the sorted leaves, then the internal nodes
    unsigned win[PNG_WIN];                             // emit window
    unsigned short code_l[288], code_d[32], code_c[20];   // canonical codes, bit-reversed
    unsigned short sorted[288], parent[576];
    unsigned short cls[320];                           // code-length sequence: symbol | extra value << 8
    unsigned short cnt[16], next[16];
    unsigned char len_l[288], len_d[32], len_c[20], depth[576];
    int n_used, n_cls, hlit, hdist, hclen;
    static constexpr int WIN = PNG_WIN;
};

#include "nq_lz.inc"                     // wave_sync, ballot64, ctz64, top64, build_code, BitOut, emit_items

__device__ const unsigned char kClOrder[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};

// {symbol - 257, extra bits, extra value} of match length code lc = length - 3 (0..255)
__device__ inline void length_symbol(unsigned lc, unsigned& sym, unsigned& eb, unsigned& ev) {
    if (lc == 255) { sym = 285; eb = 0; ev = 0; return; }
    if (lc < 8) { sym = 257 + lc; eb = 0; ev = 0; return; }
    const unsigned nb = 31 - __clz(lc);
    eb = nb - 2;
    sym = 257 + 4 * eb + 4 + ((lc >> eb) & 3);
    ev = lc & ((1u << eb) - 1);
}
// the same for distance code dm = distance - 1 (0..32767)
__device__ inline void dist_symbol(unsigned dm, unsigned& sym, unsigned& eb, unsigned& ev) {
    if (dm < 4) { sym = dm; eb = 0; ev = 0; return; }
    const unsigned nb = 31 - __clz(dm);
    eb = nb - 1;
    sym = 2 * nb + ((dm >> eb) & 1);
    ev = dm & ((1u << eb) - 1);
}

extern __shared__ uint4 png_lds[];

// All 64 lanes of the wave work on one segment; what is sequential (greedy selection, tree construction) runs on uniform values
// or in lane 0.  Every loop is bounded by the segment length, a table size or a symbol count.  RECT = false: every
// image is a whole map, rows width elements apart -- the still-image encoder as it was before rectangles existed.  RECT = true: an
// image may be a rectangle inside a larger map (rows pitch elements apart) and a delta frame (prev, u).
template <bool RECT>
__global__ void __launch_bounds__(64) png_deflate_kernel(const PngImage* __restrict__ images, int n_images, long long n_segs, int buf_bytes,
                                                         unsigned* __restrict__ words, unsigned long long* __restrict__ seg_bits,
                                                         unsigned long long* __restrict__ seg_adler, unsigned* __restrict__ tokens,
                                                         long long tok_cap, unsigned long long* __restrict__ bad) {
    unsigned char* buf = reinterpret_cast<unsigned char*>(png_lds);
    unsigned short* head = reinterpret_cast<unsigned short*>(buf + buf_bytes);
    PngTables& T = *reinterpret_cast<PngTables*>(buf + buf_bytes + 2 * (1 << PNG_HASH_BITS));
    const int lane = threadIdx.x;
    unsigned* __restrict__ tok = tokens + (long long) blockIdx.x * tok_cap;
    for (long long g = blockIdx.x; g < n_segs; g += gridDim.x) {
        int ilo = 0, ihi = n_images - 1;               // image of segment g: the last one whose first segment is <= g
        while (ilo < ihi) {
            const int mid = (ilo + ihi + 1) >> 1;
            if (images[mid].seg_base <= g) ilo = mid; else ihi = mid - 1;
        }
        const PngImage& F = images[ilo];
        const long long s = g - F.seg_base;
        const long long b0 = s * F.seg_len;
        const int L = (int) min((long long) F.seg_len, F.raw_len - b0);
        const long long row0 = b0 / F.row_bytes;
        const unsigned col0 = (unsigned) (b0 % F.row_bytes);
        const unsigned rowb = (unsigned) F.row_bytes, d = (unsigned) F.depth, per = 8u / d, W = (unsigned) F.width, K = (unsigned) F.K;
        // ---- stage: pack the segment's bytes into LDS, four per lane and step; Adler-32 partial sums ----
        for (int i = lane; i < (1 << PNG_HASH_BITS) / 2; i += 64) reinterpret_cast<unsigned*>(head)[i] = 0xFFFFFFFFu;
        for (int i = lane; i < 288; i += 64) T.hist_l[i] = 0;
        if (lane < 32) T.hist_d[lane] = 0;
        if (lane < 20) T.hist_c[lane] = 0;
        for (int i = lane; i < PNG_WIN; i += 64) T.win[i] = 0;
        unsigned long long sumA = 0, sumB = 0;
        bool badc = false;
        for (int o4 = 4 * lane; o4 < L + 8; o4 += 256) {      // 8 zero bytes after the segment: the match compare reads past its end
            unsigned word = 0;
            for (int j = 0; j < 4; ++j) {
                const int o = o4 + j;
                if (o >= L) break;
                const unsigned t = col0 + (unsigned) o, r = t / rowb, c = t - r * rowb;
                unsigned v = 0;
                if (c) {
                    // the maps are read element by element: a rectangle's rows start at any x, nothing wider than 2 bytes is aligned
                    const long long ro = (row0 + r) * (RECT ? (long long) F.pitch : (long long) W);
                    const unsigned short* __restrict__ rowp = F.index + ro;
                    const unsigned x0 = (c - 1) * per;
                    for (unsigned k = 0; k < per; ++k) {
                        const unsigned x = x0 + k;
                        if (x >= W) break;
                        unsigned idx = rowp[x];
                        if (idx >= K) { badc = true; idx &= (1u << d) - 1u; }
                        else if constexpr (RECT) {            // a delta frame: a pixel equal to prev's packs as u (prev is uniform)
                            if (F.prev && F.prev[ro + x] == idx) idx = (unsigned) F.u;
                        }
                        v |= idx << (8 - d * (k + 1));
                    }
                }
                word |= v << (8 * j);
                sumA += v;
                sumB += (unsigned long long) (L - o) * v;
            }
            reinterpret_cast<unsigned*>(buf)[o4 >> 2] = word;
        }
        for (int dlt = 32; dlt > 0; dlt >>= 1) {
            sumA += __shfl_xor(sumA, dlt);
            sumB += __shfl_xor(sumB, dlt);
        }
        wave_sync();
        // ---- parse: 64 positions per step ----
        int ntok = 0;
        int next_p = 0;                                // first position the parse has not covered
        for (int base = 0; base < L; base += 64) {
            const int p = base + lane;
            const bool valid = p + 2 < L;
            unsigned h = 0;
            if (valid) h = ((buf[p] | (unsigned) buf[p + 1] << 8 | (unsigned) buf[p + 2] << 16) * 0x9E3779B1u) >> (32 - PNG_HASH_BITS);
            unsigned cand = valid ? head[h] : PNG_NONE;
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
            bool ok = valid && cand != PNG_NONE && (unsigned) p - cand <= 32768u;
            if (ok) ok = buf[cand] == buf[p] && buf[cand + 1] == buf[p + 1] && buf[cand + 2] == buf[p + 2];
            const unsigned long long M = ballot64(ok);
            const int end = min(base + 64, L);
            for (int it = 0; it < 64 && next_p < end; ++it) {
                const unsigned long long Mm = M >> (next_p - base);
                const int m = Mm ? next_p + ctz64(Mm) : end;          // literals [next_p, m), then a match at m (if m < end)
                if (p >= next_p && p < m) {
                    const unsigned v = buf[p];
                    tok[ntok + (p - next_p)] = v;
                    atomicAdd(&T.hist_l[v], 1u);
                }
                ntok += m - next_p;
                next_p = m;
                if (m < end) {
                    const int q = (int) __shfl(cand, m - base);
                    const int cap = min(258, L - m);
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
                        length_symbol(lc, sym, eb, ev);
                        T.hist_l[sym] += 1;
                        dist_symbol(dm, sym, eb, ev);
                        T.hist_d[sym] += 1;
                    }
                    ++ntok;
                    next_p = m + len;
                    wave_sync();
                }
            }
        }
        if (lane == 0) T.hist_l[256] += 1;
        __threadfence();                               // the tokens are read back by other lanes below
        wave_sync();
        // ---- codes ----
        build_code(T, T.hist_l, 286, 15, T.len_l, T.code_l, lane);
        build_code(T, T.hist_d, 30, 15, T.len_d, T.code_d, lane);
        if (lane == 0) {
            int hlit = 286, hdist = 30;
            while (hlit > 257 && T.len_l[hlit - 1] == 0) --hlit;
            while (hdist > 1 && T.len_d[hdist - 1] == 0) --hdist;
            T.hlit = hlit; T.hdist = hdist;
            const int nseq = hlit + hdist;
            int n = 0;
            auto at = [&](int i) -> unsigned { return i < hlit ? T.len_l[i] : T.len_d[i - hlit]; };
            auto put = [&](unsigned sym, unsigned extra) { T.cls[n++] = (unsigned short) (sym | extra << 8); T.hist_c[sym] += 1; };
            for (int i = 0; i < nseq;) {
                const unsigned v = at(i);
                int r = 1;
                while (i + r < nseq && at(i + r) == v) ++r;
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
            int hclen = 19;
            while (hclen > 4 && T.len_c[kClOrder[hclen - 1]] == 0) --hclen;
            T.hclen = hclen;
        }
        wave_sync();
        // ---- emit ----
        BitOut B{words + F.word_base + s * F.seg_words, 0, 0};
        {
            unsigned long long v = 0; int nb = 0;
            if (lane == 0) {
                v = (s == F.nseg - 1 ? 1u : 0u) | 2u << 1 | (unsigned) (T.hlit - 257) << 3 | (unsigned) (T.hdist - 1) << 8 | (unsigned) (T.hclen - 4) << 13;
                nb = 17;
            } else if (lane <= T.hclen) { v = T.len_c[kClOrder[lane - 1]]; nb = 3; }
            emit_items(T, B, v, nb, lane);
        }
        for (int k0 = 0; k0 < T.n_cls; k0 += 64) {
            unsigned long long v = 0; int nb = 0;
            if (k0 + lane < T.n_cls) {
                const unsigned e = T.cls[k0 + lane], sym = e & 255u;
                nb = T.len_c[sym];
                v = (unsigned long long) T.code_c[sym] | (unsigned long long) (e >> 8) << nb;
                nb += sym == 16 ? 2 : sym == 17 ? 3 : sym == 18 ? 7 : 0;
            }
            emit_items(T, B, v, nb, lane);
        }
        for (int k0 = 0; k0 < ntok; k0 += 64) {
            unsigned long long v = 0; int nb = 0;
            if (k0 + lane < ntok) {
                const unsigned t = tok[k0 + lane];
                if (t >> 31) {
                    unsigned sym, eb, ev;
                    length_symbol((t >> 16) & 255u, sym, eb, ev);
                    nb = T.len_l[sym];
                    v = (unsigned long long) T.code_l[sym] | (unsigned long long) ev << nb;
                    nb += (int) eb;
                    dist_symbol(t & 0x7FFFu, sym, eb, ev);
                    v |= ((unsigned long long) T.code_d[sym] | (unsigned long long) ev << T.len_d[sym]) << nb;
                    nb += T.len_d[sym] + (int) eb;
                } else {
                    nb = T.len_l[t];
                    v = T.code_l[t];
                }
            }
            emit_items(T, B, v, nb, lane);
        }
        emit_items(T, B, lane == 0 ? T.code_l[256] : 0, lane == 0 ? T.len_l[256] : 0, lane);
        if (lane == 0) {
            if (B.nb > 0) B.out[B.wpos] = T.win[0];
            seg_bits[g] = (unsigned long long) B.wpos * 32 + B.nb;
            seg_adler[g] = (sumA % ADLER_MOD) | (sumB % ADLER_MOD) << 32;
        }
        if (badc) bad[ilo] = 1;
        __threadfence();                               // the next segment reuses the token scratch
        wave_sync();
    }
}

// one workgroup per image: seg_off[i] = bits of the image's segments before i; res[2 * image] = the image's bit length,
// res[2 * image + 1] = Adler-32 of its raw stream
__global__ void __launch_bounds__(256) png_scan_kernel(const PngImage* __restrict__ images, const unsigned long long* __restrict__ seg_bits,
                                                       const unsigned long long* __restrict__ seg_adler, unsigned long long* __restrict__ seg_off,
                                                       unsigned long long* __restrict__ res) {
    __shared__ unsigned long long part[256];
    __shared__ unsigned pa[256], pb[256], pl[256];
    const PngImage& F = images[blockIdx.x];
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
    // Adler-32: thread t folds a run of consecutive segments into (A, B, length mod 65521), thread 0 folds the 256 runs in order
    const long long per = (F.nseg + 255) / 256, lo = min(F.nseg, per * threadIdx.x), hi = min(F.nseg, lo + per);
    unsigned A = 0, Bv = 0, Ln = 0;
    for (long long i = lo; i < hi; ++i) {
        const unsigned long long e = seg_adler[F.seg_base + i];
        const unsigned a = (unsigned) e, b = (unsigned) (e >> 32);
        const unsigned len = (unsigned) (min((long long) F.seg_len, F.raw_len - i * F.seg_len) % ADLER_MOD);
        Bv = (unsigned) ((Bv + (unsigned long long) len * A + b) % ADLER_MOD);
        A = (A + a) % ADLER_MOD;
        Ln = (Ln + len) % ADLER_MOD;
    }
    pa[threadIdx.x] = A; pb[threadIdx.x] = Bv; pl[threadIdx.x] = Ln;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned a = 1, b = 0;
        for (int t = 0; t < 256; ++t) {
            b = (unsigned) ((b + (unsigned long long) pl[t] * a + pb[t]) % ADLER_MOD);
            a = (a + pa[t]) % ADLER_MOD;
        }
        res[2 * blockIdx.x] = carry;
        res[2 * blockIdx.x + 1] = (unsigned long long) (b << 16 | a);
    }
}

// bits [lo, lo + cnt) (cnt <= 8) of a segment's bit string
__device__ inline unsigned seg_bits_at(const unsigned* __restrict__ sw, unsigned long long lo, int cnt) {
    const unsigned long long wi = lo >> 5;
    const unsigned long long v = (unsigned long long) sw[wi] | (unsigned long long) sw[wi + 1] << 32;
    return (unsigned) (v >> (lo & 31)) & ((1u << cnt) - 1u);
}

// deflate byte j of image F: bits [8j, 8j + 8) of its segments' strings one after another
__device__ inline unsigned data_byte(const PngImage& F, long long j, const unsigned* __restrict__ words, const unsigned long long* __restrict__ seg_bits,
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

// file layout of an image: prefix (.. zlib header, from the blob), data_bytes of deflate data, Adler-32, the data chunk's CRC
// (png_crc_store_kernel), the IEND chunk when the image ends a file
__global__ void __launch_bounds__(256) png_gather_kernel(const PngImage* __restrict__ images, int n_images, const unsigned* __restrict__ words,
                                                         const unsigned long long* __restrict__ seg_bits, const unsigned long long* __restrict__ seg_off,
                                                         const unsigned long long* __restrict__ res, const unsigned char* __restrict__ blob,
                                                         unsigned char* __restrict__ file, long long total) {
    const unsigned char iend[12] = {0, 0, 0, 0, 'I', 'E', 'N', 'D', 0xAE, 0x42, 0x60, 0x82};
    for (long long o = (long long) blockIdx.x * blockDim.x + threadIdx.x; o < total; o += (long long) gridDim.x * blockDim.x) {
        int lo = 0, hi = n_images - 1;
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (images[mid].file_off <= o) lo = mid; else hi = mid - 1;
        }
        const PngImage& F = images[lo];
        const long long r = o - F.file_off, j = r - F.prefix_len;
        unsigned v;
        if (j < 0) v = blob[F.prefix_off + r];
        else if (j < F.data_bytes) v = data_byte(F, j, words, seg_bits, seg_off);
        else if (j < F.data_bytes + 4) v = (unsigned) (res[2 * lo + 1] >> (8 * (3 - (j - F.data_bytes)))) & 255u;
        else if (j < F.data_bytes + 8) continue;
        else if (F.iend) v = iend[j - F.data_bytes - 8];
        else continue;
        file[o] = (unsigned char) v;
    }
}

// ---- CRC-32 (reflected, polynomial 0xEDB88320).  A register value is a polynomial over GF(2), bit 31 = x^0. ----
__device__ inline unsigned crc_mul(unsigned a, unsigned b) {          // a * b mod P
    unsigned p = 0;
    for (int i = 31; i >= 0; --i) {
        if ((a >> i) & 1u) p ^= b;
        b = (b >> 1) ^ ((b & 1u) ? 0xEDB88320u : 0u);
    }
    return p;
}
__device__ inline unsigned crc_x_pow_8n(unsigned long long n) {       // x^(8n) mod P
    unsigned r = 0x80000000u, sq = 0x00800000u;                       // x^0, x^8
    for (int i = 0; i < 64 && n; ++i, n >>= 1) {
        if (n & 1ull) r = crc_mul(r, sq);
        sq = crc_mul(sq, sq);
    }
    return r;
}

// The data chunk's CRC covers its type and data: bytes [file_off + prefix_len - crc_lead, + crc_lead + data_bytes + 4) (crc_lead: type,
// an fdAT's sequence number, zlib header; + 4: the Adler-32).  Thread c of an image takes
// bytes [128c, 128c + 128) of that range: their remainder with a zero register, times x^(8 * bytes after them); thread 0 adds the
// initial register 0xFFFFFFFF times x^(8 * all bytes).  The XOR of all of these is the register at the end.
__global__ void __launch_bounds__(256) png_crc_kernel(const PngImage* __restrict__ images, int n_images, const unsigned char* __restrict__ file,
                                                      long long n_chunks, unsigned* __restrict__ crc) {
    __shared__ unsigned table[256];
    {
        unsigned c = threadIdx.x;
        for (int k = 0; k < 8; ++k) c = (c >> 1) ^ ((c & 1u) ? 0xEDB88320u : 0u);
        table[threadIdx.x] = c;
    }
    __syncthreads();
    for (long long t = (long long) blockIdx.x * blockDim.x + threadIdx.x; t < n_chunks; t += (long long) gridDim.x * blockDim.x) {
        int lo = 0, hi = n_images - 1;
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (images[mid].crc_base <= t) lo = mid; else hi = mid - 1;
        }
        const PngImage& F = images[lo];
        const long long len = F.crc_lead + 4 + F.data_bytes, c = t - F.crc_base, a = c * PNG_CRC_CHUNK, e = min(len, a + PNG_CRC_CHUNK);
        const unsigned char* __restrict__ src = file + F.file_off + F.prefix_len - F.crc_lead;
        unsigned reg = 0;
        for (long long i = a; i < e; ++i) reg = table[(reg ^ src[i]) & 255u] ^ (reg >> 8);
        reg = crc_mul(reg, crc_x_pow_8n((unsigned long long) (len - e)));
        if (c == 0) reg ^= crc_mul(0xFFFFFFFFu, crc_x_pow_8n((unsigned long long) len));
        atomicXor(&crc[lo], reg);
    }
}

__global__ void __launch_bounds__(64) png_crc_store_kernel(const PngImage* __restrict__ images, int n_images, const unsigned* __restrict__ crc,
                                                           unsigned char* __restrict__ file) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_images) return;
    const PngImage& F = images[i];
    const unsigned v = ~crc[i];
    unsigned char* dst = file + F.file_off + F.prefix_len + F.data_bytes + 4;
    for (int k = 0; k < 4; ++k) dst[k] = (unsigned char) (v >> (8 * (3 - k)));
}

} // namespace

size_t png_deflate_lds_bytes(int max_seg_len) { return (size_t) png_buf_bytes(max_seg_len) + 2 * (1 << PNG_HASH_BITS) + sizeof(PngTables); }

hipError_t launch_png_deflate(const PngImage* d_images, int n_images, long long n_segs, int max_seg_len, int grid, bool rect, unsigned* d_words,
                              unsigned long long* d_seg_bits, unsigned long long* d_seg_adler, unsigned* d_tokens, unsigned long long* d_bad,
                              hipStream_t s) {
    const size_t lds = png_deflate_lds_bytes(max_seg_len);
    const auto kernel = rect ? png_deflate_kernel<true> : png_deflate_kernel<false>;
    if (lds > 48 * 1024) {
        const hipError_t e = hipFuncSetAttribute((const void*) kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int) lds);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(kernel, dim3((unsigned) grid), dim3(64), lds, s, d_images, n_images, n_segs, png_buf_bytes(max_seg_len), d_words,
                       d_seg_bits, d_seg_adler, d_tokens, (long long) max_seg_len, d_bad);
    return hipSuccess;
}

void launch_png_scan(const PngImage* d_images, int n_images, const unsigned long long* d_seg_bits, const unsigned long long* d_seg_adler,
                     unsigned long long* d_seg_off, unsigned long long* d_res, hipStream_t s) {
    hipLaunchKernelGGL(png_scan_kernel, dim3((unsigned) n_images), dim3(256), 0, s, d_images, d_seg_bits, d_seg_adler, d_seg_off, d_res);
}

void launch_png_gather(const PngImage* d_images, int n_images, const unsigned* d_words, const unsigned long long* d_seg_bits,
                       const unsigned long long* d_seg_off, const unsigned long long* d_res, const unsigned char* d_blob, unsigned char* d_file,
                       long long total, long long n_crc_chunks, unsigned* d_crc, hipStream_t s) {
    long long grid = (total + 255) / 256;
    if (grid > 256 * 64) grid = 256 * 64;
    hipLaunchKernelGGL(png_gather_kernel, dim3((unsigned) grid), dim3(256), 0, s, d_images, n_images, d_words, d_seg_bits, d_seg_off, d_res, d_blob,
                       d_file, total);
    grid = (n_crc_chunks + 255) / 256;
    if (grid > 256 * 64) grid = 256 * 64;
    hipLaunchKernelGGL(png_crc_kernel, dim3((unsigned) grid), dim3(256), 0, s, d_images, n_images, d_file, n_crc_chunks, d_crc);
    hipLaunchKernelGGL(png_crc_store_kernel, dim3((unsigned) ((n_images + 63) / 64)), dim3(64), 0, s, d_images, n_images, d_crc, d_file);
}

} // namespace nq
