/* The CPU oracle (oracle/nq_oracle.c) alone at degenerate image and tile geometry: every shape of tests/test_gpu_tiny_geometry.py x six
 * pixel generators x both kinds x nMaxColors {1, 2, 3, 16, 256} x dither off / on through nqo_convert, and through nqo_prescan +
 * nqo_pnnquan + nqo_dither_tiled with tiles 4x4, 16x16, 7x5 and 1x1.  Every buffer is malloc'ed to its exact size, so a build with
 * -fsanitize=address,undefined sees any access past an image, a tile or a palette.  Prints the number of calls, how many of them the
 * reference would throw on (none), and an FNV-1a checksum of every output: the plain and the sanitized build must print the same line.
 * tests/test_oracle_tiny_cpu.py builds and runs both. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include "nq_oracle.h"

static uint64_t g_sum = 1469598103934665603ULL;
static void mix(const int32_t* v, size_t n) {
    for (size_t i = 0; i < n; ++i)
        for (int b = 0; b < 4; ++b) { g_sum ^= (uint64_t) ((((uint32_t) v[i]) >> (8 * b)) & 0xFFu); g_sum *= 1099511628211ULL; }
}
static uint64_t splitmix(uint64_t x) {
    x += 0x9E3779B97F4A7C15ULL;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ULL;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBULL;
    return x ^ (x >> 31);
}
/* generators: 0 uniform opaque, 1 gradient + noise, 2 three colours, 3 uniform with ~20 % alpha 0 and ~30 % semi-transparent pixels,
 * 4 one opaque colour, 5 every pixel 0 */
static int32_t pixel(int gen, int w, int h, int i, unsigned shape) {
    const uint64_t z = splitmix((uint64_t) i + 1 + 1000u * shape + (uint64_t) gen);
    uint32_t c = (uint32_t) (z & 0xFFFFFF), a = 255;
    const int x = i % w, y = i / w;
    switch (gen) {
    case 1: c = ((uint32_t) (255 * x / (w > 1 ? w - 1 : 1)) << 16) | ((uint32_t) (255 * y / (h > 1 ? h - 1 : 1)) << 8) | (uint32_t) (z & 0x1F); break;
    case 2: c = (uint32_t) (z % 3) * 0x3A5C71u; break;
    case 3: { const unsigned u = (unsigned) ((z >> 32) & 0xFF); a = u < 51 ? 0 : (u < 128 ? 16 + u : 255); break; }
    case 4: c = 0xFFFFFF; break;
    case 5: c = 0; a = 0; break;
    default: break;
    }
    return (int32_t) (c | (a << 24));
}

int main(void) {
    static const int SH[][2] = {{1, 1}, {2, 1}, {1, 2}, {2, 2}, {3, 1}, {1, 3}, {3, 3}, {2, 3}, {5, 4}, {4, 5}, {7, 7}, {8, 8}, {9, 8}, {15, 16},
                                {16, 15}, {17, 17}, {17, 1}, {1, 17}, {64, 1}, {1, 64}, {65, 1}, {1, 65}, {33, 3}, {3, 33}, {63, 2}, {2, 63}};
    static const int KS[] = {1, 2, 3, 16, 256};
    static const int TILES[][2] = {{4, 4}, {16, 16}, {7, 5}, {1, 1}};
    long converts = 0, dithers = 0, throws = 0;
    for (int kind = 0; kind < 2; ++kind)
        for (int gen = 0; gen < 6; ++gen)
            for (unsigned s = 0; s < sizeof SH / sizeof SH[0]; ++s) {
                const int w = SH[s][0], h = SH[s][1];
                const size_t n = (size_t) w * h;
                int32_t* img = malloc(n * sizeof *img);
                if (!img) return 2;
                for (size_t i = 0; i < n; ++i) img[i] = pixel(gen, w, h, (int) i, s);
                for (unsigned k = 0; k < sizeof KS / sizeof KS[0]; ++k)
                    for (int dither = 0; dither < 2; ++dither) {
                        const int nMax = KS[k];
                        int32_t* out = malloc(n * sizeof *out);
                        int32_t* idx = malloc(n * sizeof *idx);
                        int32_t* pal = malloc((size_t) (nMax < 2 ? 2 : nMax) * sizeof *pal);
                        if (!out || !idx || !pal) return 2;
                        int32_t K = 0;
                        nqo_quantizer* q = nqo_create(kind, img, w, h);
                        nqo_set_seed(q, 5);
                        ++converts;
                        if (nqo_convert(q, nMax, dither, out, idx, pal, &K) != 0) ++throws;
                        else {
                            mix(pal, (size_t) K); mix(idx, n); mix(out, n);
                            for (size_t i = 0; i < n; ++i)
                                if (idx[i] < 0 || idx[i] >= K || out[i] != pal[idx[i]]) { printf("bad index: kind %d gen %d %dx%d K %d\n", kind, gen, w, h, nMax); return 1; }
                        }
                        nqo_destroy(q);
                        if (nMax > 2) {
                            q = nqo_create(kind, img, w, h);
                            nqo_prescan(q, nMax);
                            const int kk = nqo_pnnquan(q, nMax, pal);
                            if (kk <= 0) ++throws;
                            else {
                                mix(pal, (size_t) kk);
                                for (unsigned t = 0; t < sizeof TILES / sizeof TILES[0]; ++t) {
                                    nqo_set_seed(q, 5);
                                    nqo_dither_tiled(q, pal, kk, dither, TILES[t][0], TILES[t][1], out, idx);
                                    ++dithers;
                                    mix(idx, n); mix(out, n);
                                    for (size_t i = 0; i < n; ++i)
                                        if (idx[i] < 0 || idx[i] >= kk) { printf("bad tiled index: kind %d gen %d %dx%d K %d\n", kind, gen, w, h, nMax); return 1; }
                                }
                            }
                            nqo_destroy(q);
                        }
                        free(out); free(idx); free(pal);
                    }
                free(img);
            }
    printf("oracle tiny: %ld converts, %ld tiled dithers, %ld throws, checksum %016llx\n", converts, dithers, throws, (unsigned long long) g_sum);
    return throws ? 1 : 0;
}
