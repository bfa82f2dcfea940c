// nq_lz.inc -- what the chains of nq_png.hip (deflate) and nq_webp.hip (VP8L) share: one wave works on one chain, its tables in LDS.
// Included inside the including file's anonymous namespace, after nq_kernels.h.  TT is the chain's table struct; it provides
//   unsigned W[], win[TT::WIN]; unsigned short sorted[], parent[], cnt[16], next[16]; unsigned char depth[]; int n_used;
// with W, parent and depth of twice the largest alphabet and sorted of the largest alphabet.

__device__ inline void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

__device__ inline unsigned long long ballot64(bool p) { return __ballot(p); }
__device__ inline int ctz64(unsigned long long v) { return __ffsll((long long) v) - 1; }
__device__ inline int top64(unsigned long long v) { return 63 - __clzll((long long) v); }

// Code lengths <= limit of the nsym symbols counted in hist (DESIGN.md 5c): the used symbols sorted by (count, symbol) -- by rank,
// all lanes --, Huffman's construction with two queues, depths cut to the limit with the Kraft sum repaired, lengths dealt out
// longest first in sorted order (lane 0).  Also the canonical codes, bit-reversed.
template <typename TT>
__device__ void build_code(TT& T, const unsigned* hist, int nsym, int limit, unsigned char* lens, unsigned short* codes, int lane) {
    if (lane == 0) T.n_used = 0;
    wave_sync();
    int used_here = 0;
    for (int s = lane; s < nsym; s += 64) {
        lens[s] = 0;
        const unsigned f = hist[s];
        if (!f) continue;
        int rank = 0;
        for (int j = 0; j < nsym; ++j) {
            const unsigned g = hist[j];
            rank += (g != 0 && (g < f || (g == f && j < s))) ? 1 : 0;
        }
        T.sorted[rank] = (unsigned short) s;
        T.W[rank] = f;
        ++used_here;
    }
    if (used_here) atomicAdd(&T.n_used, used_here);
    wave_sync();
    if (lane == 0) {
        const int n = T.n_used;
        if (n <= 1) lens[n ? T.sorted[0] : 0] = 1;
        else {
            int i = 0, j = n;
            for (int k = n; k < 2 * n - 1; ++k) {
                unsigned w = 0;
                for (int r = 0; r < 2; ++r) {
                    int t;
                    if (i < n && (j >= k || T.W[i] <= T.W[j])) t = i++; else t = j++;
                    w += T.W[t];
                    T.parent[t] = (unsigned short) k;
                }
                T.W[k] = w;
            }
            for (int l = 0; l <= limit; ++l) T.cnt[l] = 0;
            T.depth[2 * n - 2] = 0;
            for (int t = 2 * n - 3; t >= 0; --t) {
                const int d = min(T.depth[T.parent[t]] + 1, 255);
                T.depth[t] = (unsigned char) d;
                if (t < n) T.cnt[min(d, limit)]++;
            }
            unsigned total = 0;
            for (int l = 1; l <= limit; ++l) total += (unsigned) T.cnt[l] << (limit - l);
            for (; total > (1u << limit); --total) {              // at most n steps: every step removes one unit of the excess
                T.cnt[limit]--;
                int l = limit - 1;
                while (l > 1 && T.cnt[l] == 0) --l;
                T.cnt[l]--;
                T.cnt[l + 1] += 2;
            }
            int t = 0;
            for (int l = limit; l >= 1; --l)
                for (int c = T.cnt[l]; c > 0 && t < n; --c) lens[T.sorted[t++]] = (unsigned char) l;
        }
        // canonical codes (RFC 1951 3.2.2)
        for (int l = 0; l <= limit; ++l) T.cnt[l] = 0;
        for (int s = 0; s < nsym; ++s) T.cnt[lens[s]]++;
        T.cnt[0] = 0;
        unsigned code = 0;
        for (int l = 1; l <= limit; ++l) {
            code = (code + T.cnt[l - 1]) << 1;
            T.next[l] = (unsigned short) code;
        }
        for (int s = 0; s < nsym; ++s) {
            const int l = lens[s];
            codes[s] = l ? (unsigned short) (__brev((unsigned) T.next[l]++) >> (32 - l)) : 0;
        }
    }
    wave_sync();
}

// The bit writer of a chain: every lane hands in one item (value, nbits; nbits 0: none); the items go into the chain's bit string in
// lane order.  Whole words leave the LDS window for global memory, the open word stays in win[0].  TT::WIN words hold 31 carried bits
// and 64 items of the including file's longest item, plus two words an item's tail may touch.
struct BitOut {
    unsigned* out;
    long long wpos;
    int nb;
};
template <typename TT>
__device__ inline void emit_items(TT& T, BitOut& B, unsigned long long value, int nbits, int lane) {
    int incl = nbits;
    for (int d = 1; d < 64; d <<= 1) {
        const int t = __shfl_up(incl, d);
        if (lane >= d) incl += t;
    }
    const int total = __shfl(incl, 63);
    if (nbits) {
        const int off = B.nb + incl - nbits, w = off >> 5, sh = off & 31;
        const unsigned long long lo = value << sh;
        atomicOr(&T.win[w], (unsigned) lo);
        if ((unsigned) (lo >> 32)) atomicOr(&T.win[w + 1], (unsigned) (lo >> 32));
        const unsigned hi = sh ? (unsigned) (value >> (64 - sh)) : 0u;
        if (hi) atomicOr(&T.win[w + 2], hi);
    }
    wave_sync();
    const int tot = B.nb + total, full = tot >> 5;
    for (int i = lane; i < full; i += 64) B.out[B.wpos + i] = T.win[i];
    const unsigned carry = T.win[full];
    wave_sync();
    for (int i = lane; i < TT::WIN; i += 64) T.win[i] = i == 0 ? carry : 0u;
    wave_sync();
    B.wpos += full;
    B.nb = tot & 31;
}
