/* tests/c/jni_fake/stub_abi.c -- a scripted stand-in for libnquant_hip.so: the fourteen nq_* functions that
 * nquant.android_amd/jni/nquant_jni.c calls, and nothing else.  No GPU, no HIP.  Every call but nq_last_error is recorded (a function
 * id, its arguments in signature order with pointers as addresses, then a few values read through the pointers, and in the last slot
 * whether a Java exception was pending when it was made), reads ALL of its inputs and writes ALL of its outputs with patterns -- so
 * that an address sanitizer sees a buffer that is too small --, and returns NQ_OK unless it is the call the test scripted to fail
 * (st_fail_call).  tests/test_jni_cpu.py links it with the shim and the fake JNI runtime.  Test infrastructure only. */
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include "nquant_abi.h"

#define ST_EXPORT __attribute__((visibility("default")))
#define ST_MAX_CALLS 64
#define ST_SLOTS 32

extern int64_t fj_get(int which);     /* fake_jni.c: 7 = an exception is pending */

enum { F_CREATE, F_DESTROY, F_GET_PARAMS, F_CONVERT, F_CONVERT_BATCH, F_CONVERT_FRAMES, F_GIF_MAX_BYTES, F_ENCODE_GIF, F_ENCODE_GIF_DELTA,
       F_PNG_MAX_BYTES, F_ENCODE_PNG, F_APNG_MAX_BYTES, F_ENCODE_APNG };

typedef struct { int fn; int64_t a[ST_SLOTS]; } st_call;

static struct {
    st_call calls[ST_MAX_CALLS];
    int ncalls, total_calls, last_error_calls;
    int fail_at, fail_status;
    int K, alpha;
    int64_t size, max_bytes, checksum;
    char error[128];
} s = { .K = 5, .size = 33, .max_bytes = 4096, .error = "scripted error" };

#define P(x) ((int64_t) (intptr_t) (x))

static st_call* record(int fn, int nargs, const int64_t* args) {
    static st_call overflow;
    st_call* c = s.ncalls < ST_MAX_CALLS ? &s.calls[s.ncalls++] : &overflow;
    memset(c, 0, sizeof *c);
    c->fn = fn;
    for (int i = 0; i < nargs; ++i) c->a[i] = args[i];
    c->a[ST_SLOTS - 1] = fj_get(7);
    s.total_calls++;
    return c;
}
#define RECORD(fn, ...) \
    const int64_t args_[] = {__VA_ARGS__}; \
    st_call* c = record(fn, (int) (sizeof args_ / sizeof args_[0]), args_); \
    int at = (int) (sizeof args_ / sizeof args_[0]); \
    (void) c; (void) at; \
    if (s.fail_at && s.total_calls == s.fail_at) return s.fail_status
#define EXTRA(v) (c->a[at++] = (int64_t) (v))

static int sizes_ok(int n, const int32_t* w, const int32_t* h) {
    if (n < 1 || !w || !h) return 0;
    for (int i = 0; i < n; ++i)
        if (w[i] < 1 || h[i] < 1) return 0;
    return 1;
}

static void read_all(const void* p, int64_t bytes) {
    const uint8_t* b = (const uint8_t*) p;
    for (int64_t i = 0; i < bytes; ++i) s.checksum += b[i];
}

static int scripted_K(int nMaxColors) {
    const int cap = nMaxColors > 2 ? nMaxColors : 2;
    return s.K < cap ? s.K : cap;
}

static void quantize(const uint32_t* in, int64_t px, int K, uint32_t* out_argb, uint16_t* out_index) {
    for (int64_t p = 0; p < px; ++p) {
        out_argb[p] = in[p] ^ 0x00FFFFFFu;
        if (out_index) out_index[p] = (uint16_t) (p % K);
    }
}

static void fill_palette(uint32_t* pal, int K, int image) {
    for (int j = 0; j < K; ++j) pal[j] = 0xFF000000u | (uint32_t) image << 16 | (uint32_t) j;
}

static int write_file(uint8_t* out, int64_t cap, int64_t* out_size) {
    *out_size = s.size;
    if (cap < s.size) return NQ_ERR_INVALID;
    for (int64_t i = 0; i < s.size; ++i) out[i] = (uint8_t) (i * 7 + 1);
    return NQ_OK;
}

/* ---- the fourteen ---- */
int nq_create(int kind, int device, nq_handle** out) {
    RECORD(F_CREATE, kind, device, P(out));
    *out = (nq_handle*) (intptr_t) (0x1000 + 16 * s.total_calls);
    return NQ_OK;
}

void nq_destroy(nq_handle* h) {
    const int64_t args[] = {P(h)};
    record(F_DESTROY, 1, args);
}

const char* nq_last_error(const nq_handle* h) { s.last_error_calls++; return s.error; }

int nq_get_params(const nq_handle* h, nq_params* out) {
    RECORD(F_GET_PARAMS, P(h), P(out));
    memset(out, 0, sizeof *out);
    out->transparentPixelIndex = s.alpha ? 3 : -1;
    return NQ_OK;
}

int nq_convert(nq_handle* h, const uint32_t* argb, int width, int height, int nMaxColors, int dither, int64_t rng_seed, int mode,
               uint32_t* out_argb, uint16_t* out_index, uint32_t* out_palette, int32_t* out_K) {
    RECORD(F_CONVERT, P(h), P(argb), width, height, nMaxColors, dither, rng_seed, mode, P(out_argb), P(out_index), P(out_palette), P(out_K));
    if (width < 1 || height < 1 || !argb || !out_argb) return NQ_ERR_INVALID;
    const int64_t px = (int64_t) width * height;
    EXTRA(argb[0]); EXTRA(argb[px - 1]);
    const int K = scripted_K(nMaxColors);
    quantize(argb, px, K, out_argb, out_index);
    fill_palette(out_palette, K, 0);
    *out_K = K;
    return NQ_OK;
}

int nq_convert_batch(nq_handle* const* hs, int n, const uint32_t* const* argb, const int32_t* widths, const int32_t* heights, int nMaxColors,
                     int dither, const int64_t* rng_seeds, int mode, uint32_t* const* out_argb, uint16_t* const* out_index,
                     uint32_t* out_palettes, int32_t palette_stride, int32_t* out_K) {
    RECORD(F_CONVERT_BATCH, P(hs), n, P(argb), P(widths), P(heights), nMaxColors, dither, P(rng_seeds), mode, P(out_argb), P(out_index),
           P(out_palettes), palette_stride, P(out_K));
    if (!sizes_ok(n, widths, heights)) return NQ_ERR_INVALID;
    EXTRA(P(hs[0])); EXTRA(P(hs[n - 1])); EXTRA(P(argb[0])); EXTRA(P(argb[n - 1])); EXTRA(P(out_argb[0])); EXTRA(P(out_argb[n - 1]));
    EXTRA(widths[0]); EXTRA(widths[n - 1]); EXTRA(heights[0]); EXTRA(heights[n - 1]); EXTRA(rng_seeds[0]); EXTRA(rng_seeds[n - 1]);
    for (int i = 0; i < n; ++i) {
        int K = scripted_K(nMaxColors) - i % 3;
        if (K < 1) K = 1;
        quantize(argb[i], (int64_t) widths[i] * heights[i], K, out_argb[i], out_index ? out_index[i] : NULL);
        fill_palette(out_palettes + (size_t) i * palette_stride, K, i);
        out_K[i] = K;
    }
    return NQ_OK;
}

int nq_convert_frames(nq_handle* h, int n, const uint32_t* const* argb, const int32_t* widths, const int32_t* heights, int nMaxColors,
                      int dither, const int64_t* rng_seeds, int mode, uint32_t* const* out_argb, uint16_t* const* out_index,
                      uint32_t* out_palette, int32_t* out_K) {
    RECORD(F_CONVERT_FRAMES, P(h), n, P(argb), P(widths), P(heights), nMaxColors, dither, P(rng_seeds), mode, P(out_argb), P(out_index),
           P(out_palette), P(out_K));
    if (!sizes_ok(n, widths, heights)) return NQ_ERR_INVALID;
    EXTRA(P(argb[0])); EXTRA(P(argb[n - 1])); EXTRA(P(out_argb[0])); EXTRA(P(out_argb[n - 1]));
    EXTRA(widths[0]); EXTRA(widths[n - 1]); EXTRA(heights[0]); EXTRA(heights[n - 1]); EXTRA(rng_seeds[0]); EXTRA(rng_seeds[n - 1]);
    const int K = scripted_K(nMaxColors);
    for (int i = 0; i < n; ++i) quantize(argb[i], (int64_t) widths[i] * heights[i], K, out_argb[i], out_index ? out_index[i] : NULL);
    fill_palette(out_palette, K, 0);
    *out_K = K;
    return NQ_OK;
}

int nq_gif_max_bytes(int n, const int32_t* widths, const int32_t* heights, int K, int segment_pixels, int64_t* out_bytes) {
    RECORD(F_GIF_MAX_BYTES, n, P(widths), P(heights), K, segment_pixels, P(out_bytes));
    if (!sizes_ok(n, widths, heights)) return NQ_ERR_INVALID;
    EXTRA(widths[0]); EXTRA(widths[n - 1]); EXTRA(heights[0]); EXTRA(heights[n - 1]);
    *out_bytes = s.max_bytes;
    return NQ_OK;
}

/* what the three animation encoders share: read every frame, the palette and the delays */
static void read_frames(st_call* c, int* pat, int n, const uint16_t* const* index, const int32_t* widths, const int32_t* heights, int width,
                        int height, const uint32_t* palette, int K, const int32_t* delays) {
    int at = *pat;
    EXTRA(P(index[0])); EXTRA(P(index[n - 1]));
    EXTRA(K > 0 ? palette[0] : 0); EXTRA(K > 0 ? palette[K - 1] : 0);
    EXTRA(delays ? delays[0] : -1); EXTRA(delays ? delays[n - 1] : -1);
    EXTRA(index[0][0]);
    const int64_t last = (int64_t) (widths ? widths[n - 1] : width) * (heights ? heights[n - 1] : height);
    EXTRA(index[n - 1][last - 1]);
    for (int i = 0; i < n; ++i) read_all(index[i], 2 * (int64_t) (widths ? widths[i] : width) * (heights ? heights[i] : height));
    read_all(palette, 4 * (int64_t) K);
    if (delays) read_all(delays, 4 * (int64_t) n);
    *pat = at;
}

int nq_encode_gif(nq_handle* h, int n, const uint16_t* const* index, const int32_t* widths, const int32_t* heights, const uint32_t* palette, int K,
                  const int32_t* delays_cs, int loop_count, int segment_pixels, uint8_t* out, int64_t cap, int64_t* out_size) {
    RECORD(F_ENCODE_GIF, P(h), n, P(index), P(widths), P(heights), P(palette), K, P(delays_cs), loop_count, segment_pixels, P(out), cap,
           P(out_size));
    if (!sizes_ok(n, widths, heights) || K < 1) return NQ_ERR_INVALID;
    EXTRA(widths[0]); EXTRA(widths[n - 1]); EXTRA(heights[0]); EXTRA(heights[n - 1]);
    read_frames(c, &at, n, index, widths, heights, 0, 0, palette, K, delays_cs);
    return write_file(out, cap, out_size);
}

int nq_encode_gif_delta(nq_handle* h, int n, const uint16_t* const* index, int width, int height, const uint32_t* palette, int K,
                        const int32_t* delays_cs, int loop_count, int segment_pixels, uint8_t* out, int64_t cap, int64_t* out_size,
                        int32_t* out_rects) {
    RECORD(F_ENCODE_GIF_DELTA, P(h), n, P(index), width, height, P(palette), K, P(delays_cs), loop_count, segment_pixels, P(out), cap,
           P(out_size), P(out_rects));
    if (n < 1 || width < 1 || height < 1 || K < 1) return NQ_ERR_INVALID;
    read_frames(c, &at, n, index, NULL, NULL, width, height, palette, K, delays_cs);
    return write_file(out, cap, out_size);
}

int nq_encode_apng(nq_handle* h, int n, const uint16_t* const* index, int width, int height, const uint32_t* palette, int K,
                   const int32_t* delays_cs, int loop_count, int segment_bytes, uint8_t* out, int64_t cap, int64_t* out_size, int32_t* out_rects) {
    RECORD(F_ENCODE_APNG, P(h), n, P(index), width, height, P(palette), K, P(delays_cs), loop_count, segment_bytes, P(out), cap, P(out_size),
           P(out_rects));
    if (n < 1 || width < 1 || height < 1 || K < 1) return NQ_ERR_INVALID;
    read_frames(c, &at, n, index, NULL, NULL, width, height, palette, K, delays_cs);
    return write_file(out, cap, out_size);
}

int nq_png_max_bytes(int n, const int32_t* widths, const int32_t* heights, const int32_t* K, int segment_bytes, int64_t* out_bytes) {
    RECORD(F_PNG_MAX_BYTES, n, P(widths), P(heights), P(K), segment_bytes, P(out_bytes));
    if (!sizes_ok(n, widths, heights)) return NQ_ERR_INVALID;
    EXTRA(widths[0]); EXTRA(heights[0]);
    *out_bytes = s.max_bytes;
    return NQ_OK;
}

int nq_encode_png(nq_handle* h, int n, const uint16_t* const* index, const int32_t* widths, const int32_t* heights, const uint32_t* palettes,
                  int32_t palette_stride, const int32_t* K, int segment_bytes, uint8_t* out, int64_t cap, int64_t* out_offsets) {
    RECORD(F_ENCODE_PNG, P(h), n, P(index), P(widths), P(heights), P(palettes), palette_stride, P(K), segment_bytes, P(out), cap,
           P(out_offsets));
    if (n != 1 || !sizes_ok(n, widths, heights) || K[0] < 1) return NQ_ERR_INVALID;
    EXTRA(widths[0]); EXTRA(heights[0]); EXTRA(K[0]);
    int64_t w = widths[0], hg = heights[0];
    read_frames(c, &at, 1, index, NULL, NULL, (int) w, (int) hg, palettes, K[0], NULL);
    out_offsets[0] = 0;
    return write_file(out, cap, &out_offsets[1]);
}

int nq_apng_max_bytes(int n, int width, int height, int segment_bytes, int64_t* out_bytes) {
    RECORD(F_APNG_MAX_BYTES, n, width, height, segment_bytes, P(out_bytes));
    if (n < 1 || width < 1 || height < 1) return NQ_ERR_INVALID;
    *out_bytes = s.max_bytes;
    return NQ_OK;
}

/* ---- the script and the record (ctypes) ---- */
ST_EXPORT void st_reset(void) {
    s.ncalls = s.total_calls = s.last_error_calls = 0;
    s.fail_at = 0;
    s.checksum = 0;
}
ST_EXPORT void st_script(int K, int64_t size, int64_t max_bytes, int alpha) { s.K = K; s.size = size; s.max_bytes = max_bytes; s.alpha = alpha; }
/* the k-th recorded call from the last st_reset (k >= 1) returns `status` and writes nothing */
ST_EXPORT void st_fail_call(int k, int status) { s.fail_at = k; s.fail_status = status; }
ST_EXPORT void st_set_error(const char* text) { snprintf(s.error, sizeof s.error, "%s", text); }
ST_EXPORT int st_ncalls(void) { return s.total_calls; }
ST_EXPORT int st_last_error_calls(void) { return s.last_error_calls; }
ST_EXPORT int st_call_fn(int i) { return i >= 0 && i < s.ncalls ? s.calls[i].fn : -1; }
ST_EXPORT int64_t st_call_arg(int i, int j) { return i >= 0 && i < s.ncalls && j >= 0 && j < ST_SLOTS ? s.calls[i].a[j] : -1; }
