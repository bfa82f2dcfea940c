/* tests/c/jni_fake/sweep_main.c -- the shim's failure sweeps as a standalone program: fake_jni.c + stub_abi.c + nquant_jni.c + this file,
 * built plain and with -fsanitize=address,undefined (tests/test_jni_cpu.py).  Every direct buffer is malloc'ed to its exact size, so a
 * read or write past it is a sanitizer report; every exit of the shim must free what it allocated, or the leak check reports it.
 * For each of the 16 native methods: valid arguments at n = 1, 17 and 600; an allocation failing at every allocating JNI call; the first
 * and the second nq_* call failing; every short / null / non-direct argument that applies.  After each call: no violation, nothing
 * outstanding, at most 16 live local references, and for the bad arguments one pending exception and no nq_* call.
 * Prints one line per problem and a summary; exit status 1 when there was a problem.  Test infrastructure only. */
#include <jni.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

/* fake_jni.c */
JNIEnv* fj_env(void);
jobject fj_new_int_array(const jint*, int64_t);
jobject fj_new_long_array(const jlong*, int64_t);
jobject fj_new_short_array(const jshort*, int64_t);
jobject fj_new_object_array(int64_t);
void fj_set_object(jobject, int64_t, jobject);
jobject fj_new_direct_buffer(void*, int64_t);
jobject fj_new_heap_buffer(int64_t);
void fj_release(jobject);
void fj_begin_call(void);
void fj_end_call(jobject);
int64_t fj_get(int);
const char* fj_violation_log(void);
const char* fj_exception_class(void);
void fj_exception_clear(void);
void fj_fail_alloc(int64_t);
/* stub_abi.c */
void st_reset(void);
void st_fail_call(int, int);
int st_ncalls(void);
/* nquant_jni.c */
#define NATIVE(name) Java_com_android_nQuant_PnnQuantizer_##name
jlong NATIVE(nqCreate)(JNIEnv*, jclass, jint, jint);
void NATIVE(nqDestroy)(JNIEnv*, jclass, jlong);
jintArray NATIVE(nqConvert)(JNIEnv*, jclass, jlong, jintArray, jint, jint, jint, jboolean, jlong, jint, jintArray, jshortArray);
jboolean NATIVE(nqHasAlpha)(JNIEnv*, jclass, jlong);
jobjectArray NATIVE(nqConvertBatch)(JNIEnv*, jclass, jlongArray, jobjectArray, jintArray, jintArray, jint, jboolean, jlongArray, jint, jobjectArray);
jintArray NATIVE(nqConvertFrames)(JNIEnv*, jclass, jlong, jobjectArray, jintArray, jintArray, jint, jboolean, jlongArray, jint, jobjectArray);
jlong NATIVE(nqGifMaxBytes)(JNIEnv*, jclass, jintArray, jintArray);
jlong NATIVE(nqEncodeGif)(JNIEnv*, jclass, jlong, jobjectArray, jintArray, jintArray, jintArray, jintArray, jint, jobject, jlong);
jlong NATIVE(nqEncodeGifDelta)(JNIEnv*, jclass, jlong, jobjectArray, jint, jint, jintArray, jintArray, jint, jobject, jlong);
jlong NATIVE(nqConvertFramesToGif)(JNIEnv*, jclass, jlong, jobjectArray, jintArray, jintArray, jint, jboolean, jlongArray, jint, jintArray, jint,
                                   jboolean, jobject, jlong);
jlong NATIVE(nqPngMaxBytes)(JNIEnv*, jclass, jint, jint);
jlong NATIVE(nqEncodePng)(JNIEnv*, jclass, jlong, jobject, jint, jint, jintArray, jobject, jlong);
jlong NATIVE(nqConvertToPng)(JNIEnv*, jclass, jlong, jobject, jint, jint, jint, jboolean, jlong, jint, jobject, jlong);
jlong NATIVE(nqApngMaxBytes)(JNIEnv*, jclass, jint, jint, jint);
jlong NATIVE(nqEncodeApng)(JNIEnv*, jclass, jlong, jobjectArray, jint, jint, jintArray, jintArray, jint, jobject, jlong);
jlong NATIVE(nqConvertFramesToApng)(JNIEnv*, jclass, jlong, jobjectArray, jint, jint, jint, jboolean, jlongArray, jint, jintArray, jint, jobject,
                                    jlong);

enum { M_CREATE, M_DESTROY, M_CONVERT, M_HAS_ALPHA, M_BATCH, M_FRAMES, M_GIF_MAX, M_ENC_GIF, M_ENC_GIF_DELTA, M_TO_GIF, M_PNG_MAX, M_ENC_PNG,
       M_TO_PNG, M_APNG_MAX, M_ENC_APNG, M_TO_APNG, M_TO_GIF_DELTA, N_METHODS };
static const char* const NAMES[N_METHODS] = {"nqCreate", "nqDestroy", "nqConvert", "nqHasAlpha", "nqConvertBatch", "nqConvertFrames", "nqGifMaxBytes",
    "nqEncodeGif", "nqEncodeGifDelta", "nqConvertFramesToGif", "nqPngMaxBytes", "nqEncodePng", "nqConvertToPng", "nqApngMaxBytes", "nqEncodeApng",
    "nqConvertFramesToApng", "nqConvertFramesToGif(delta)"};
#define BIT(m) (1u << (m))
static const unsigned PER_FRAME = BIT(M_BATCH) | BIT(M_FRAMES) | BIT(M_ENC_GIF) | BIT(M_ENC_GIF_DELTA) | BIT(M_TO_GIF) | BIT(M_ENC_APNG) |
                                  BIT(M_TO_APNG) | BIT(M_TO_GIF_DELTA);
static const unsigned ONE_SIZE = BIT(M_ENC_GIF_DELTA) | BIT(M_ENC_APNG) | BIT(M_TO_APNG) | BIT(M_TO_GIF_DELTA);
static const unsigned WRITES_FILE = BIT(M_ENC_GIF) | BIT(M_ENC_GIF_DELTA) | BIT(M_TO_GIF) | BIT(M_ENC_PNG) | BIT(M_TO_PNG) | BIT(M_ENC_APNG) |
                                    BIT(M_TO_APNG) | BIT(M_TO_GIF_DELTA);
static const unsigned RETURNS_OBJECT = BIT(M_CONVERT) | BIT(M_BATCH) | BIT(M_FRAMES);

enum { D_NONE, D_SHORT_WIDTHS, D_SHORT_SEEDS, D_NULL_SEEDS, D_SHORT_DELAYS, D_SHORT_OUT_ARRAY, D_SMALL_IN, D_SMALL_OUT, D_SMALL_INDEX, D_HEAP_IN,
       D_SMALL_FILE, D_HEAP_FILE, D_NULL_FILE, D_N_ZERO, D_SHORT_ARGB, D_SHORT_OUT_ARGB, D_SHORT_OUT_INDEX, D_NULL_PALETTE, D_TWO_SIZES, N_DEFECTS };
static const char* const DEFECTS[N_DEFECTS] = {"valid", "short widths", "short seeds", "null seeds", "short delaysCs", "short out[]", "small in buffer",
    "small out[] buffer", "small index buffer", "heap in buffer", "out smaller than cap", "heap out", "null out", "n == 0", "short argb", "short outArgb",
    "short outIndex", "null palette", "delta frames of two sizes"};
static const unsigned APPLIES[N_DEFECTS] = {
    ~0u,
    BIT(M_BATCH) | BIT(M_FRAMES) | BIT(M_ENC_GIF) | BIT(M_TO_GIF) | BIT(M_TO_GIF_DELTA),
    BIT(M_BATCH) | BIT(M_FRAMES) | BIT(M_TO_GIF) | BIT(M_TO_APNG) | BIT(M_TO_GIF_DELTA),
    BIT(M_BATCH) | BIT(M_FRAMES) | BIT(M_TO_GIF) | BIT(M_TO_APNG) | BIT(M_TO_GIF_DELTA),
    BIT(M_ENC_GIF) | BIT(M_ENC_GIF_DELTA) | BIT(M_ENC_APNG) | BIT(M_TO_GIF) | BIT(M_TO_APNG) | BIT(M_TO_GIF_DELTA),
    BIT(M_BATCH) | BIT(M_FRAMES),
    BIT(M_BATCH) | BIT(M_FRAMES) | BIT(M_TO_GIF) | BIT(M_TO_APNG) | BIT(M_TO_GIF_DELTA) | BIT(M_TO_PNG),
    BIT(M_BATCH) | BIT(M_FRAMES),
    BIT(M_ENC_GIF) | BIT(M_ENC_GIF_DELTA) | BIT(M_ENC_APNG) | BIT(M_ENC_PNG),
    BIT(M_BATCH) | BIT(M_FRAMES) | BIT(M_TO_GIF) | BIT(M_TO_APNG) | BIT(M_TO_GIF_DELTA) | BIT(M_TO_PNG),
    0, 0, 0,                                                        /* the three `out` defects: WRITES_FILE, set in main */
    BIT(M_BATCH) | BIT(M_FRAMES) | BIT(M_ENC_GIF) | BIT(M_ENC_GIF_DELTA) | BIT(M_TO_GIF) | BIT(M_ENC_APNG) | BIT(M_TO_APNG) | BIT(M_TO_GIF_DELTA),
    BIT(M_CONVERT), BIT(M_CONVERT), BIT(M_CONVERT),
    BIT(M_ENC_GIF) | BIT(M_ENC_GIF_DELTA) | BIT(M_ENC_APNG) | BIT(M_ENC_PNG),
    BIT(M_TO_GIF_DELTA),
};

#define CAP 64
typedef struct {
    int n;
    jobject handles, in, out, index, widths, heights, seeds, delays, palette, argb, out_argb, out_index, in1, index1, file;
    void* mem[4096]; int nmem;
    jobject objs[8192]; int nobjs;
} args_t;

static void* mem(args_t* a, size_t bytes) {
    void* p = calloc(bytes ? bytes : 1, 1);
    if (!p || a->nmem == 4096) abort();
    return a->mem[a->nmem++] = p;
}
static jobject own(args_t* a, jobject o) {
    if (a->nobjs == 8192) abort();
    return a->objs[a->nobjs++] = o;
}
static jobject int_array(args_t* a, int len, int first, int step) {
    jint* v = mem(a, sizeof(jint) * (size_t) len);
    for (int i = 0; i < len; ++i) v[i] = first + step * i;
    return own(a, fj_new_int_array(v, len));
}
/* an array of n direct buffers of elsize-byte elements, buffer i of w_i * h_i elements; the last one `short_by` elements smaller, or a heap buffer */
static jobject buffers(args_t* a, int n, int method, int w, int h, int elsize, int short_by, int last_is_heap) {
    jobject arr = own(a, fj_new_object_array(n));
    for (int i = 0; i < n; ++i) {
        const int one = (ONE_SIZE >> method) & 1;
        const int64_t px = (int64_t) (one ? w : w + i % 3) * (one ? h : h + i % 2) - (i == n - 1 ? short_by : 0);
        jobject b = i == n - 1 && last_is_heap ? fj_new_heap_buffer(1 << 20) : fj_new_direct_buffer(mem(a, (size_t) px * (size_t) elsize), px);
        fj_set_object(arr, i, own(a, b));
    }
    return arr;
}

static void make_args(args_t* a, int method, int n, int w, int h, int defect) {
    memset(a, 0, sizeof *a);
    const int one = (ONE_SIZE >> method) & 1;
    const int m = defect == D_N_ZERO ? 0 : n;
    a->n = n;
    jlong* hv = mem(a, sizeof(jlong) * (size_t) n);
    jlong* sv = mem(a, sizeof(jlong) * (size_t) n);
    for (int i = 0; i < n; ++i) { hv[i] = 0x5000 + 16 * i; sv[i] = 100 + i; }
    a->handles = own(a, fj_new_long_array(hv, m));
    a->seeds = defect == D_NULL_SEEDS ? NULL : own(a, fj_new_long_array(sv, defect == D_SHORT_SEEDS ? n - 1 : n));
    jint* wv = mem(a, sizeof(jint) * (size_t) n);
    jint* hgv = mem(a, sizeof(jint) * (size_t) n);
    for (int i = 0; i < n; ++i) { wv[i] = one ? w : w + i % 3; hgv[i] = one ? h : h + i % 2; }
    if (defect == D_TWO_SIZES) wv[n - 1]++;
    a->widths = own(a, fj_new_int_array(wv, defect == D_SHORT_WIDTHS ? n - 1 : n));
    a->heights = own(a, fj_new_int_array(hgv, n));
    a->delays = int_array(a, defect == D_SHORT_DELAYS ? n - 1 : n, 10, 1);
    a->palette = defect == D_NULL_PALETTE ? NULL : int_array(a, 5, (int) 0xFF000001, 3);
    a->in = buffers(a, m, method, w, h, 4, defect == D_SMALL_IN, defect == D_HEAP_IN);
    a->out = buffers(a, defect == D_SHORT_OUT_ARRAY ? n - 1 : m, method, w, h, 4, defect == D_SMALL_OUT, 0);
    a->index = buffers(a, m, method, w, h, 2, defect == D_SMALL_INDEX, 0);
    const int px = w * h;
    a->argb = int_array(a, px - (defect == D_SHORT_ARGB), 1000, 1);
    a->out_argb = int_array(a, px - (defect == D_SHORT_OUT_ARGB), 0, 0);
    a->out_index = own(a, fj_new_short_array(NULL, px - (defect == D_SHORT_OUT_INDEX)));
    a->in1 = defect == D_HEAP_IN ? own(a, fj_new_heap_buffer(1 << 20))
                                 : own(a, fj_new_direct_buffer(mem(a, 4 * (size_t) (px - (defect == D_SMALL_IN))), px - (defect == D_SMALL_IN)));
    a->index1 = own(a, fj_new_direct_buffer(mem(a, 2 * (size_t) (px - (defect == D_SMALL_INDEX))), px - (defect == D_SMALL_INDEX)));
    const int file_bytes = CAP - (defect == D_SMALL_FILE);
    a->file = defect == D_NULL_FILE ? NULL : defect == D_HEAP_FILE ? own(a, fj_new_heap_buffer(1 << 20))
                                                                   : own(a, fj_new_direct_buffer(mem(a, (size_t) file_bytes), file_bytes));
}

static void free_args(args_t* a) {
    for (int i = a->nobjs - 1; i >= 0; --i) fj_release(a->objs[i]);
    for (int i = 0; i < a->nmem; ++i) free(a->mem[i]);
}

static int64_t call(int method, args_t* a, int w, int h) {
    JNIEnv* env = fj_env();
    const jlong H = 0x5000;
    switch (method) {
    case M_CREATE: return NATIVE(nqCreate)(env, NULL, 1, 0);
    case M_DESTROY: NATIVE(nqDestroy)(env, NULL, H); return 0;
    case M_CONVERT: return (int64_t) (intptr_t) NATIVE(nqConvert)(env, NULL, H, a->argb, w, h, 16, 1, 77, 1, a->out_argb, a->out_index);
    case M_HAS_ALPHA: return NATIVE(nqHasAlpha)(env, NULL, H);
    case M_BATCH: return (int64_t) (intptr_t) NATIVE(nqConvertBatch)(env, NULL, a->handles, a->in, a->widths, a->heights, 16, 1, a->seeds, 1, a->out);
    case M_FRAMES: return (int64_t) (intptr_t) NATIVE(nqConvertFrames)(env, NULL, H, a->in, a->widths, a->heights, 16, 1, a->seeds, 1, a->out);
    case M_GIF_MAX: return NATIVE(nqGifMaxBytes)(env, NULL, a->widths, a->heights);
    case M_ENC_GIF: return NATIVE(nqEncodeGif)(env, NULL, H, a->index, a->widths, a->heights, a->palette, a->delays, 3, a->file, CAP);
    case M_ENC_GIF_DELTA: return NATIVE(nqEncodeGifDelta)(env, NULL, H, a->index, w, h, a->palette, a->delays, 3, a->file, CAP);
    case M_TO_GIF: case M_TO_GIF_DELTA:
        return NATIVE(nqConvertFramesToGif)(env, NULL, H, a->in, a->widths, a->heights, 16, 1, a->seeds, 1, a->delays, 3, method == M_TO_GIF_DELTA,
                                            a->file, CAP);
    case M_PNG_MAX: return NATIVE(nqPngMaxBytes)(env, NULL, w, h);
    case M_ENC_PNG: return NATIVE(nqEncodePng)(env, NULL, H, a->index1, w, h, a->palette, a->file, CAP);
    case M_TO_PNG: return NATIVE(nqConvertToPng)(env, NULL, H, a->in1, w, h, 16, 1, 77, 1, a->file, CAP);
    case M_APNG_MAX: return NATIVE(nqApngMaxBytes)(env, NULL, a->n, w, h);
    case M_ENC_APNG: return NATIVE(nqEncodeApng)(env, NULL, H, a->index, w, h, a->palette, a->delays, 3, a->file, CAP);
    case M_TO_APNG: return NATIVE(nqConvertFramesToApng)(env, NULL, H, a->in, w, h, 16, 1, a->seeds, 1, a->delays, 3, a->file, CAP);
    }
    abort();
}

static int problems, calls;

/* one bracketed call; what == 0: must succeed; 1: must leave exactly one exception; 2: as 1 and no nq_* call at all.  Returns the allocating
 * JNI calls it made. */
static int64_t run(int method, int n, int defect, int64_t fail_alloc, int fail_call, int what) {
    static args_t a;
    const int w = 3, h = 2;
    make_args(&a, method, n, w, h, defect);
    st_reset();
    if (fail_call) st_fail_call(fail_call, -1);
    const int64_t level = fj_get(4);
    fj_begin_call();
    fj_fail_alloc(fail_alloc);
    const int64_t res = call(method, &a, w, h);
    const int is_obj = (RETURNS_OBJECT >> method) & 1;
    fj_end_call(is_obj ? (jobject) (intptr_t) res : NULL);
    if (is_obj && res) fj_release((jobject) (intptr_t) res);
    calls++;
    char bad[512] = "";
    if (fj_get(0)) snprintf(bad, sizeof bad, "violations: %s", fj_violation_log());
    else if (fj_get(1)) snprintf(bad, sizeof bad, "%lld element pointers outstanding", (long long) fj_get(1));
    else if (fj_get(5)) snprintf(bad, sizeof bad, "a write through a pointer released with JNI_ABORT");
    else if (fj_get(3) > 16) snprintf(bad, sizeof bad, "peak of %lld live local references", (long long) fj_get(3));
    else if (fj_get(4) != level) snprintf(bad, sizeof bad, "object bytes %lld -> %lld", (long long) level, (long long) fj_get(4));
    else if (what == 0 && fj_get(7)) snprintf(bad, sizeof bad, "exception %s", fj_exception_class());
    else if (what != 0 && !fj_get(7)) snprintf(bad, sizeof bad, "no exception pending");
    else if (what == 2 && st_ncalls()) snprintf(bad, sizeof bad, "%d nq_* calls", st_ncalls());
    if (bad[0]) { problems++; printf("PROBLEM %s, n = %d, %s, fail_alloc %lld, fail_call %d: %s\n", NAMES[method], n, DEFECTS[defect], (long long) fail_alloc, fail_call, bad); }
    const int64_t allocs = fj_get(6);
    fj_exception_clear();
    free_args(&a);
    return allocs;
}

int main(void) {
    for (int m = 0; m < N_METHODS; ++m) {
        const int per_frame = (PER_FRAME >> m) & 1;
        const int64_t allocs = run(m, 3, D_NONE, 0, 0, 0);
        if (per_frame) { run(m, 1, D_NONE, 0, 0, 0); run(m, 17, D_NONE, 0, 0, 0); run(m, 600, D_NONE, 0, 0, 0); }
        for (int64_t k = 1; k <= allocs; ++k) run(m, 3, D_NONE, k, 0, 1);
        const int nq_calls = m == M_TO_GIF || m == M_TO_GIF_DELTA || m == M_TO_PNG || m == M_TO_APNG ? 2 : 1;
        if (m != M_DESTROY && m != M_HAS_ALPHA && m != M_GIF_MAX && m != M_PNG_MAX && m != M_APNG_MAX)
            for (int k = 1; k <= nq_calls; ++k) run(m, 3, D_NONE, 0, k, 1);
        for (int d = 1; d < N_DEFECTS; ++d) {
            const unsigned applies = d == D_SMALL_FILE || d == D_HEAP_FILE || d == D_NULL_FILE ? WRITES_FILE : APPLIES[d];
            if ((applies >> m) & 1) run(m, 3, d, 0, 0, 2);
        }
    }
    printf("sweep done: %d native methods, %d calls, %d problems\n", N_METHODS - 1, calls, problems);
    return problems ? 1 : 0;
}
