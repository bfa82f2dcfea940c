/*
 * nquant_jni.c -- JNI shim between the reference's Java API and libnquant_hip.so (include/nquant_abi.h).
 * NOT compiled in the build image (no JDK / jni.h there); build on a box with a JDK:
 *   gcc -shared -fPIC -I$JAVA_HOME/include -I$JAVA_HOME/include/linux -I../../include nquant_jni.c \
 *       -L.. -lnquant_hip -o libnquant_jni.so
 * Java side: ../java/com/android/nQuant/PnnQuantizer.java, PnnLABQuantizer.java (same class names, constructor and
 * convert()/hasAlpha() signatures as the reference: NQ/PnnQuantizer.java:35,409,458; NQ/PnnLABQuantizer.java:24).
 *
 * Rules every native method here keeps (tests/test_jni_cpu.py and tests/test_gpu_jni.py run them under a fake JNI runtime):
 *  * nothing from Java is trusted: every array and buffer is checked for null, every array length against the number of images or
 *    frames, every direct buffer's capacity against width*height (or `cap`), BEFORE any nq_* call; a heap buffer is refused;
 *  * local references stay bounded: a reference taken per element (GetObjectArrayElement, NewIntArray) is deleted in the same
 *    iteration, so a batch of any size stays within the 16 the JNI specification guarantees;
 *  * one exit: every method sets `err` and leaves through `done:`, where every element pointer is released (inputs and, on an
 *    error, outputs with JNI_ABORT), every malloc is freed and then at most one exception is thrown;
 *  * an exception that is already pending (the OutOfMemoryError of a failed JNI allocation) is never replaced, and no JNI function
 *    other than Release / DeleteLocalRef / ExceptionCheck is called while it is pending.
 */
#include <jni.h>
#include <stdint.h>
#include <stdlib.h>
#include "nquant_abi.h"

static const char OOM[] = "out of memory";

static void throw_rt(JNIEnv* env, const char* msg) {
    if ((*env)->ExceptionCheck(env)) return;                                     /* the first exception stays */
    jclass cls = (*env)->FindClass(env, "java/lang/RuntimeException");
    if (!cls) return;                                                            /* FindClass has raised its own */
    (*env)->ThrowNew(env, cls, msg && *msg ? msg : "nquant error");
    (*env)->DeleteLocalRef(env, cls);
}

/* pixels of a width x height image; 0 for sizes nq_* refuses anyway (then every buffer is large enough and nq_* reports the size) */
static int64_t pixels_of(jint w, jint h) { return w > 0 && h > 0 ? (int64_t) w * (int64_t) h : 0; }

/* a non-null Java array of exactly n elements? */
static int has_length(JNIEnv* env, jarray a, jsize n) { return a && (*env)->GetArrayLength(env, a) == n; }

/* The address of a direct buffer of at least `need` elements of its type; on failure NULL and *err set. */
static void* direct_buffer(JNIEnv* env, jobject buf, int64_t need, const char** err) {
    if (!buf) { *err = "a buffer is null"; return NULL; }
    void* p = (*env)->GetDirectBufferAddress(env, buf);
    if (!p) { *err = "a buffer is not a direct buffer"; return NULL; }
    if ((int64_t) (*env)->GetDirectBufferCapacity(env, buf) < need) { *err = "a direct buffer is smaller than the call needs"; return NULL; }
    return p;
}

/* dst[i] = address of the direct buffer bufs[i], which must hold at least w[i] * hg[i] elements (w == NULL: width * height for all).
 * One local reference at a time.  Returns NULL or the error text. */
static const char* direct_buffers(JNIEnv* env, jobjectArray bufs, jsize n, const jint* w, const jint* hg, jint width, jint height,
                                  void** dst) {
    const char* err = NULL;
    for (jsize i = 0; i < n && !err; ++i) {
        jobject b = (*env)->GetObjectArrayElement(env, bufs, i);
        dst[i] = direct_buffer(env, b, w ? pixels_of(w[i], hg[i]) : pixels_of(width, height), &err);
        (*env)->DeleteLocalRef(env, b);
    }
    return err;
}

/* a new int[K] holding palette[0..K); NULL with the JNI's exception pending when the allocation fails */
static jintArray new_palette(JNIEnv* env, const uint32_t* palette, int32_t K) {
    jintArray pal = (*env)->NewIntArray(env, K);
    if (pal) (*env)->SetIntArrayRegion(env, pal, 0, K, (const jint*) palette);
    return pal;
}

JNIEXPORT jlong JNICALL Java_com_android_nQuant_PnnQuantizer_nqCreate(JNIEnv* env, jclass c, jint kind, jint device) {
    nq_handle* h = NULL;
    if (nq_create(kind, device, &h) != NQ_OK) { throw_rt(env, nq_last_error(NULL)); return 0; }
    return (jlong) (intptr_t) h;
}

JNIEXPORT void JNICALL Java_com_android_nQuant_PnnQuantizer_nqDestroy(JNIEnv* env, jclass c, jlong h) {
    nq_destroy((nq_handle*) (intptr_t) h);
}

/* returns the palette; fills outArgb (w*h) and, when non-null, outIndex (w*h) */
JNIEXPORT jintArray JNICALL Java_com_android_nQuant_PnnQuantizer_nqConvert(JNIEnv* env, jclass c, jlong hh, jintArray argb,
        jint w, jint hgt, jint nMaxColors, jboolean dither, jlong seed, jint mode, jintArray outArgb, jshortArray outIndex) {
    nq_handle* h = (nq_handle*) (intptr_t) hh;
    const int cap = nMaxColors > 2 ? nMaxColors : 2;
    const int64_t px = pixels_of(w, hgt);
    const char* err = NULL;
    uint32_t* palette = NULL;
    jint *in = NULL, *out = NULL;
    jshort* idx = NULL;
    jintArray pal = NULL;
    int32_t K = 0;
    if (!argb || !outArgb) { err = "argb or outArgb is null"; goto done; }
    if ((*env)->GetArrayLength(env, argb) < px || (*env)->GetArrayLength(env, outArgb) < px ||
        (outIndex && (*env)->GetArrayLength(env, outIndex) < px)) { err = "an array is shorter than w * hgt"; goto done; }
    palette = (uint32_t*) malloc((size_t) cap * sizeof(uint32_t));               /* per call: two threads may convert different objects at once */
    if (!palette) { err = OOM; goto done; }
    /* The convert blocks on the GPU for up to seconds (the merge loop): plain Get/Release<Type>ArrayElements, not critical regions --
     * a critical region must be short and non-blocking and would stall the collector JVM-wide for the whole call. */
    if (!(in = (*env)->GetIntArrayElements(env, argb, NULL))) { err = OOM; goto done; }      /* OutOfMemoryError is pending */
    if (!(out = (*env)->GetIntArrayElements(env, outArgb, NULL))) { err = OOM; goto done; }
    if (outIndex && !(idx = (*env)->GetShortArrayElements(env, outIndex, NULL))) { err = OOM; goto done; }
    if (nq_convert(h, (const uint32_t*) in, w, hgt, nMaxColors, dither ? 1 : 0, seed, mode, (uint32_t*) out, (uint16_t*) idx, palette, &K) != NQ_OK)
        err = nq_last_error(h);                                                  /* convert() `throws Exception` */
done:
    if (idx) (*env)->ReleaseShortArrayElements(env, outIndex, idx, err ? JNI_ABORT : 0);
    if (out) (*env)->ReleaseIntArrayElements(env, outArgb, out, err ? JNI_ABORT : 0);
    if (in) (*env)->ReleaseIntArrayElements(env, argb, in, JNI_ABORT);          /* the input is never modified */
    if (!err) pal = new_palette(env, palette, K);
    free(palette);
    if (err) throw_rt(env, err);
    return pal;
}

JNIEXPORT jboolean JNICALL Java_com_android_nQuant_PnnQuantizer_nqHasAlpha(JNIEnv* env, jclass c, jlong hh) {
    nq_params p;
    if (nq_get_params((nq_handle*) (intptr_t) hh, &p) != NQ_OK) return JNI_FALSE;
    return p.transparentPixelIndex > -1 ? JNI_TRUE : JNI_FALSE;               /* NQ/PnnQuantizer.java:458-460 */
}

/* convertBatch(): direct IntBuffers in, direct IntBuffers out -> nq_convert_batch (uploads / read-backs overlapped; all merge
 * loops in one launch).  Returns int[n][] palettes. */
JNIEXPORT jobjectArray JNICALL Java_com_android_nQuant_PnnQuantizer_nqConvertBatch(JNIEnv* env, jclass c, jlongArray handles,
        jobjectArray in, jintArray widths, jintArray heights, jint nMaxColors, jboolean dither, jlongArray seeds, jint mode,
        jobjectArray out) {
    const int stride = nMaxColors > 2 ? nMaxColors : 2;
    const char* err = NULL;
    nq_handle** hs = NULL;
    const uint32_t** src = NULL;
    uint32_t** dst = NULL;
    uint32_t* palettes = NULL;
    int32_t* K = NULL;
    jlong *hh = NULL, *sd = NULL;
    jint *w = NULL, *hg = NULL;
    jobjectArray result = NULL;
    jsize n = 0;
    if (!handles || (n = (*env)->GetArrayLength(env, handles)) < 1) { err = "no images"; goto done; }
    if (!has_length(env, in, n) || !has_length(env, widths, n) || !has_length(env, heights, n) || !has_length(env, seeds, n) ||
        !has_length(env, out, n)) { err = "in, widths, heights, seeds and out need one entry per handle"; goto done; }
    hs = malloc(sizeof(*hs) * n);
    src = malloc(sizeof(*src) * n);
    dst = malloc(sizeof(*dst) * n);
    palettes = malloc(sizeof(uint32_t) * (size_t) stride * n);
    K = malloc(sizeof(int32_t) * n);
    if (!hs || !src || !dst || !palettes || !K) { err = OOM; goto done; }
    if (!(hh = (*env)->GetLongArrayElements(env, handles, NULL))) { err = OOM; goto done; }
    if (!(sd = (*env)->GetLongArrayElements(env, seeds, NULL))) { err = OOM; goto done; }
    if (!(w = (*env)->GetIntArrayElements(env, widths, NULL))) { err = OOM; goto done; }
    if (!(hg = (*env)->GetIntArrayElements(env, heights, NULL))) { err = OOM; goto done; }
    for (jsize i = 0; i < n; ++i) hs[i] = (nq_handle*) (intptr_t) hh[i];
    if ((err = direct_buffers(env, in, n, w, hg, 0, 0, (void**) src))) goto done;
    if ((err = direct_buffers(env, out, n, w, hg, 0, 0, (void**) dst))) goto done;
    if (nq_convert_batch(hs, n, src, (const int32_t*) w, (const int32_t*) hg, nMaxColors, dither ? 1 : 0, (const int64_t*) sd, mode, dst,
                         NULL, palettes, stride, K) != NQ_OK) { err = nq_last_error(hs[0]); goto done; }
    jclass int_array = (*env)->FindClass(env, "[I");
    if (!int_array) { err = OOM; goto done; }
    result = (*env)->NewObjectArray(env, n, int_array, NULL);
    (*env)->DeleteLocalRef(env, int_array);
    if (!result) { err = OOM; goto done; }
    for (jsize i = 0; i < n; ++i) {
        jintArray pal = new_palette(env, palettes + (size_t) i * stride, K[i]);
        if (!pal) { err = OOM; (*env)->DeleteLocalRef(env, result); result = NULL; break; }
        (*env)->SetObjectArrayElement(env, result, i, pal);
        (*env)->DeleteLocalRef(env, pal);
    }
done:
    if (hg) (*env)->ReleaseIntArrayElements(env, heights, hg, JNI_ABORT);
    if (w) (*env)->ReleaseIntArrayElements(env, widths, w, JNI_ABORT);
    if (sd) (*env)->ReleaseLongArrayElements(env, seeds, sd, JNI_ABORT);
    if (hh) (*env)->ReleaseLongArrayElements(env, handles, hh, JNI_ABORT);
    free(K); free(palettes); free(dst); free(src); free(hs);
    if (err) throw_rt(env, err);
    return result;
}

/* convertFrames(): one palette for a sequence of frames -> nq_convert_frames.  Direct IntBuffers in and out; returns the palette. */
JNIEXPORT jintArray JNICALL Java_com_android_nQuant_PnnQuantizer_nqConvertFrames(JNIEnv* env, jclass c, jlong hh, jobjectArray in,
        jintArray widths, jintArray heights, jint nMaxColors, jboolean dither, jlongArray seeds, jint mode, jobjectArray out) {
    nq_handle* h = (nq_handle*) (intptr_t) hh;
    const int cap = nMaxColors > 2 ? nMaxColors : 2;
    const char* err = NULL;
    const uint32_t** src = NULL;
    uint32_t** dst = NULL;
    uint32_t* palette = NULL;
    jlong* sd = NULL;
    jint *w = NULL, *hg = NULL;
    jintArray pal = NULL;
    int32_t K = 0;
    jsize n = 0;
    if (!in || (n = (*env)->GetArrayLength(env, in)) < 1) { err = "no frames"; goto done; }
    if (!has_length(env, widths, n) || !has_length(env, heights, n) || !has_length(env, seeds, n) || !has_length(env, out, n)) {
        err = "widths, heights, seeds and out need one entry per frame"; goto done;
    }
    src = malloc(sizeof(*src) * n);
    dst = malloc(sizeof(*dst) * n);
    palette = malloc(sizeof(uint32_t) * (size_t) cap);
    if (!src || !dst || !palette) { err = OOM; goto done; }
    if (!(sd = (*env)->GetLongArrayElements(env, seeds, NULL))) { err = OOM; goto done; }
    if (!(w = (*env)->GetIntArrayElements(env, widths, NULL))) { err = OOM; goto done; }
    if (!(hg = (*env)->GetIntArrayElements(env, heights, NULL))) { err = OOM; goto done; }
    if ((err = direct_buffers(env, in, n, w, hg, 0, 0, (void**) src))) goto done;
    if ((err = direct_buffers(env, out, n, w, hg, 0, 0, (void**) dst))) goto done;
    if (nq_convert_frames(h, n, src, (const int32_t*) w, (const int32_t*) hg, nMaxColors, dither ? 1 : 0, (const int64_t*) sd, mode, dst,
                          NULL, palette, &K) != NQ_OK) err = nq_last_error(h);
done:
    if (hg) (*env)->ReleaseIntArrayElements(env, heights, hg, JNI_ABORT);
    if (w) (*env)->ReleaseIntArrayElements(env, widths, w, JNI_ABORT);
    if (sd) (*env)->ReleaseLongArrayElements(env, seeds, sd, JNI_ABORT);
    if (!err) pal = new_palette(env, palette, K);
    free(palette); free(dst); free(src);
    if (err) throw_rt(env, err);
    return pal;
}

/* nqGifMaxBytes(): nq_gif_max_bytes for K = 256, the bound for every K; -1 when a size is invalid */
JNIEXPORT jlong JNICALL Java_com_android_nQuant_PnnQuantizer_nqGifMaxBytes(JNIEnv* env, jclass c, jintArray widths, jintArray heights) {
    if (!widths || !heights) return -1;
    const jsize n = (*env)->GetArrayLength(env, widths);
    if ((*env)->GetArrayLength(env, heights) != n) return -1;
    jint* w = (*env)->GetIntArrayElements(env, widths, NULL);
    jint* hg = w ? (*env)->GetIntArrayElements(env, heights, NULL) : NULL;
    int64_t bytes = -1;
    if (w && hg && nq_gif_max_bytes(n, (const int32_t*) w, (const int32_t*) hg, 256, 0, &bytes) != NQ_OK) bytes = -1;
    if (hg) (*env)->ReleaseIntArrayElements(env, heights, hg, JNI_ABORT);
    if (w) (*env)->ReleaseIntArrayElements(env, widths, w, JNI_ABORT);
    return (jlong) bytes;
}

/* encodeGif(): direct ShortBuffers of indices in, the file written to the direct ByteBuffer `out` (cap bytes) -> nq_encode_gif.
 * Returns the file size. */
JNIEXPORT jlong JNICALL Java_com_android_nQuant_PnnQuantizer_nqEncodeGif(JNIEnv* env, jclass c, jlong hh, jobjectArray index,
        jintArray widths, jintArray heights, jintArray palette, jintArray delaysCs, jint loopCount, jobject out, jlong cap) {
    nq_handle* h = (nq_handle*) (intptr_t) hh;
    const char* err = NULL;
    const uint16_t** src = NULL;
    jint *w = NULL, *hg = NULL, *pal = NULL, *d = NULL;
    int64_t size = -1;
    jsize n = 0;
    if (!index || (n = (*env)->GetArrayLength(env, index)) < 1) { err = "no frames"; goto done; }
    if (!has_length(env, widths, n) || !has_length(env, heights, n) || (delaysCs && !has_length(env, delaysCs, n))) {
        err = "widths, heights and delaysCs need one entry per frame"; goto done;
    }
    if (!palette) { err = "palette is null"; goto done; }
    const jsize K = (*env)->GetArrayLength(env, palette);
    uint8_t* file = (uint8_t*) direct_buffer(env, out, cap, &err);
    if (!file) goto done;
    if (!(src = malloc(sizeof(*src) * n))) { err = OOM; goto done; }
    if (!(w = (*env)->GetIntArrayElements(env, widths, NULL))) { err = OOM; goto done; }
    if (!(hg = (*env)->GetIntArrayElements(env, heights, NULL))) { err = OOM; goto done; }
    if (!(pal = (*env)->GetIntArrayElements(env, palette, NULL))) { err = OOM; goto done; }
    if (delaysCs && !(d = (*env)->GetIntArrayElements(env, delaysCs, NULL))) { err = OOM; goto done; }
    if ((err = direct_buffers(env, index, n, w, hg, 0, 0, (void**) src))) goto done;
    if (nq_encode_gif(h, n, src, (const int32_t*) w, (const int32_t*) hg, (const uint32_t*) pal, K, (const int32_t*) d, loopCount, 0, file, cap,
                      &size) != NQ_OK) err = nq_last_error(h);
done:
    if (d) (*env)->ReleaseIntArrayElements(env, delaysCs, d, JNI_ABORT);
    if (pal) (*env)->ReleaseIntArrayElements(env, palette, pal, JNI_ABORT);
    if (hg) (*env)->ReleaseIntArrayElements(env, heights, hg, JNI_ABORT);
    if (w) (*env)->ReleaseIntArrayElements(env, widths, w, JNI_ABORT);
    free(src);
    if (err) { throw_rt(env, err); return -1; }
    return (jlong) size;
}

/* encodeGifDelta() and encodeApng(): direct ShortBuffers of indices in (frames of one size), the file written to the direct ByteBuffer
 * `out` (cap bytes) -> nq_encode_gif_delta, or nq_encode_apng when `apng`.  Returns the file size. */
static jlong encode_one_size(JNIEnv* env, jlong hh, jobjectArray index, jint width, jint height, jintArray palette, jintArray delaysCs,
                             jint loopCount, jobject out, jlong cap, int apng) {
    nq_handle* h = (nq_handle*) (intptr_t) hh;
    const char* err = NULL;
    const uint16_t** src = NULL;
    jint *pal = NULL, *d = NULL;
    int64_t size = -1;
    jsize n = 0;
    if (!index || (n = (*env)->GetArrayLength(env, index)) < 1) { err = "no frames"; goto done; }
    if (delaysCs && !has_length(env, delaysCs, n)) { err = "delaysCs needs one entry per frame"; goto done; }
    if (!palette) { err = "palette is null"; goto done; }
    const jsize K = (*env)->GetArrayLength(env, palette);
    uint8_t* file = (uint8_t*) direct_buffer(env, out, cap, &err);
    if (!file) goto done;
    if (!(src = malloc(sizeof(*src) * n))) { err = OOM; goto done; }
    if (!(pal = (*env)->GetIntArrayElements(env, palette, NULL))) { err = OOM; goto done; }
    if (delaysCs && !(d = (*env)->GetIntArrayElements(env, delaysCs, NULL))) { err = OOM; goto done; }
    if ((err = direct_buffers(env, index, n, NULL, NULL, width, height, (void**) src))) goto done;
    const int rc = apng ? nq_encode_apng(h, n, src, width, height, (const uint32_t*) pal, K, (const int32_t*) d, loopCount, 0, file, cap, &size, NULL)
                        : nq_encode_gif_delta(h, n, src, width, height, (const uint32_t*) pal, K, (const int32_t*) d, loopCount, 0, file, cap, &size, NULL);
    if (rc != NQ_OK) err = nq_last_error(h);
done:
    if (d) (*env)->ReleaseIntArrayElements(env, delaysCs, d, JNI_ABORT);
    if (pal) (*env)->ReleaseIntArrayElements(env, palette, pal, JNI_ABORT);
    free(src);
    if (err) { throw_rt(env, err); return -1; }
    return (jlong) size;
}

/* encodeGifDelta(): as encodeGif for frames of one size, every frame after the first stored as the rectangle that changed ->
 * nq_encode_gif_delta.  Returns the file size. */
JNIEXPORT jlong JNICALL Java_com_android_nQuant_PnnQuantizer_nqEncodeGifDelta(JNIEnv* env, jclass c, jlong hh, jobjectArray index,
        jint width, jint height, jintArray palette, jintArray delaysCs, jint loopCount, jobject out, jlong cap) {
    return encode_one_size(env, hh, index, width, height, palette, delaysCs, loopCount, out, cap, 0);
}

/* convertFramesToGif() and convertFramesToApng(): nq_convert_frames of the n frames in[i] (w[i] x hg[i]) with index outputs (the ARGB
 * outputs go to scratch), then, on the same handle, the encoding of the index maps with the shared palette into the direct ByteBuffer
 * `out` (cap bytes): format 0 nq_encode_gif, 1 nq_encode_gif_delta, 2 nq_encode_apng (1 and 2: the frames have one size).  The caller
 * has checked n >= 1 and holds w and hg.  Returns the file size, or -1 with *perr set. */
static jlong frames_to_file(JNIEnv* env, nq_handle* h, jobjectArray in, jsize n, const jint* w, const jint* hg, jint nMaxColors,
                            jboolean dither, jlongArray seeds, jint mode, jintArray delaysCs, jint loopCount, int format, jobject out,
                            jlong cap, const char** perr) {
    const int pcap = nMaxColors > 2 ? nMaxColors : 2;
    const char* err = NULL;
    const uint32_t** src = NULL;
    uint32_t** argb = NULL;
    uint16_t** idx = NULL;
    uint32_t* palette = NULL;
    jlong* sd = NULL;
    jint* d = NULL;
    int32_t K = 0;
    int64_t size = -1;
    if (!seeds) { err = "seeds is null"; goto done; }
    if (!has_length(env, seeds, n) || (delaysCs && !has_length(env, delaysCs, n))) { err = "seeds and delaysCs need one entry per frame"; goto done; }
    for (jsize i = 1; format != 0 && i < n; ++i)
        if (w[i] != w[0] || hg[i] != hg[0]) { err = "delta mode: all frames must have one size"; goto done; }
    uint8_t* file = (uint8_t*) direct_buffer(env, out, cap, &err);
    if (!file) goto done;
    src = malloc(sizeof(*src) * n);
    argb = calloc(n, sizeof(*argb));
    idx = calloc(n, sizeof(*idx));
    palette = malloc(sizeof(uint32_t) * (size_t) pcap);
    if (!src || !argb || !idx || !palette) { err = OOM; goto done; }
    if ((err = direct_buffers(env, in, n, w, hg, 0, 0, (void**) src))) goto done;
    for (jsize i = 0; i < n; ++i) {
        const size_t px = (size_t) (w[i] > 0 ? w[i] : 1) * (size_t) (hg[i] > 0 ? hg[i] : 1);
        argb[i] = malloc(px * sizeof(uint32_t));
        idx[i] = malloc(px * sizeof(uint16_t));
        if (!argb[i] || !idx[i]) { err = OOM; goto done; }
    }
    if (!(sd = (*env)->GetLongArrayElements(env, seeds, NULL))) { err = OOM; goto done; }
    if (delaysCs && !(d = (*env)->GetIntArrayElements(env, delaysCs, NULL))) { err = OOM; goto done; }
    int rc = nq_convert_frames(h, n, src, (const int32_t*) w, (const int32_t*) hg, nMaxColors, dither ? 1 : 0, (const int64_t*) sd, mode,
                               argb, idx, palette, &K);
    if (rc == NQ_OK && format == 0)
        rc = nq_encode_gif(h, n, (const uint16_t* const*) idx, (const int32_t*) w, (const int32_t*) hg, palette, K, (const int32_t*) d,
                           loopCount, 0, file, cap, &size);
    else if (rc == NQ_OK && format == 1)
        rc = nq_encode_gif_delta(h, n, (const uint16_t* const*) idx, w[0], hg[0], palette, K, (const int32_t*) d, loopCount, 0, file, cap,
                                 &size, NULL);
    else if (rc == NQ_OK)
        rc = nq_encode_apng(h, n, (const uint16_t* const*) idx, w[0], hg[0], palette, K, (const int32_t*) d, loopCount, 0, file, cap, &size,
                            NULL);
    if (rc != NQ_OK) err = nq_last_error(h);
done:
    if (d) (*env)->ReleaseIntArrayElements(env, delaysCs, d, JNI_ABORT);
    if (sd) (*env)->ReleaseLongArrayElements(env, seeds, sd, JNI_ABORT);
    for (jsize i = 0; argb && idx && i < n; ++i) { free(argb[i]); free(idx[i]); }
    free(palette); free(idx); free(argb); free(src);
    *perr = err;
    return err ? -1 : (jlong) size;
}

/* convertFramesToGif(): nq_convert_frames with index outputs (the ARGB outputs go to scratch), then nq_encode_gif of the index maps
 * with the shared palette into the direct ByteBuffer `out` (cap bytes); delta: nq_encode_gif_delta instead, the frames must have one
 * size.  Returns the file size. */
JNIEXPORT jlong JNICALL Java_com_android_nQuant_PnnQuantizer_nqConvertFramesToGif(JNIEnv* env, jclass c, jlong hh, jobjectArray in,
        jintArray widths, jintArray heights, jint nMaxColors, jboolean dither, jlongArray seeds, jint mode, jintArray delaysCs, jint loopCount,
        jboolean delta, jobject out, jlong cap) {
    const char* err = NULL;
    jint *w = NULL, *hg = NULL;
    jlong size = -1;
    jsize n = 0;
    if (!in || (n = (*env)->GetArrayLength(env, in)) < 1) { err = "no frames"; goto done; }
    if (!has_length(env, widths, n) || !has_length(env, heights, n)) { err = "widths and heights need one entry per frame"; goto done; }
    if (!(w = (*env)->GetIntArrayElements(env, widths, NULL))) { err = OOM; goto done; }
    if (!(hg = (*env)->GetIntArrayElements(env, heights, NULL))) { err = OOM; goto done; }
    size = frames_to_file(env, (nq_handle*) (intptr_t) hh, in, n, w, hg, nMaxColors, dither, seeds, mode, delaysCs, loopCount, delta ? 1 : 0,
                          out, cap, &err);
done:
    if (hg) (*env)->ReleaseIntArrayElements(env, heights, hg, JNI_ABORT);
    if (w) (*env)->ReleaseIntArrayElements(env, widths, w, JNI_ABORT);
    if (err) { throw_rt(env, err); return -1; }
    return size;
}

/* nqPngMaxBytes(): nq_png_max_bytes of one image for K = 256, the bound for every K; -1 when the size is invalid */
JNIEXPORT jlong JNICALL Java_com_android_nQuant_PnnQuantizer_nqPngMaxBytes(JNIEnv* env, jclass c, jint width, jint height) {
    const int32_t w = width, hg = height;
    int64_t bytes = -1;
    if (nq_png_max_bytes(1, &w, &hg, NULL, 0, &bytes) != NQ_OK) bytes = -1;
    return (jlong) bytes;
}

/* encodePng(): a direct ShortBuffer of indices in, the file written to the direct ByteBuffer `out` (cap bytes) -> nq_encode_png.
 * Returns the file size. */
JNIEXPORT jlong JNICALL Java_com_android_nQuant_PnnQuantizer_nqEncodePng(JNIEnv* env, jclass c, jlong hh, jobject index, jint width,
        jint height, jintArray palette, jobject out, jlong cap) {
    nq_handle* h = (nq_handle*) (intptr_t) hh;
    const char* err = NULL;
    const int32_t w = width, hg = height;
    jint* pal = NULL;
    int64_t offs[2] = {0, -1};
    if (!palette) { err = "palette is null"; goto done; }
    const int32_t K = (*env)->GetArrayLength(env, palette);
    const uint16_t* src = (const uint16_t*) direct_buffer(env, index, pixels_of(width, height), &err);
    if (!src) goto done;
    uint8_t* file = (uint8_t*) direct_buffer(env, out, cap, &err);
    if (!file) goto done;
    if (!(pal = (*env)->GetIntArrayElements(env, palette, NULL))) { err = OOM; goto done; }
    if (nq_encode_png(h, 1, &src, &w, &hg, (const uint32_t*) pal, K, &K, 0, file, cap, offs) != NQ_OK) err = nq_last_error(h);
done:
    if (pal) (*env)->ReleaseIntArrayElements(env, palette, pal, JNI_ABORT);
    if (err) { throw_rt(env, err); return -1; }
    return (jlong) offs[1];
}

/* convertToPng(): nq_convert with the index output (the ARGB output goes to scratch), then nq_encode_png of the index map with the
 * image's palette into the direct ByteBuffer `out` (cap bytes).  Returns the file size. */
JNIEXPORT jlong JNICALL Java_com_android_nQuant_PnnQuantizer_nqConvertToPng(JNIEnv* env, jclass c, jlong hh, jobject in, jint width,
        jint height, jint nMaxColors, jboolean dither, jlong seed, jint mode, jobject out, jlong cap) {
    nq_handle* h = (nq_handle*) (intptr_t) hh;
    const size_t px = (size_t) (width > 0 ? width : 1) * (size_t) (height > 0 ? height : 1);
    const int pcap = nMaxColors > 2 ? nMaxColors : 2;
    const char* err = NULL;
    uint32_t* argb = NULL;
    uint16_t* idx = NULL;
    uint32_t* palette = NULL;
    const int32_t w = width, hg = height;
    int32_t K = 0;
    int64_t offs[2] = {0, -1};
    const uint32_t* pixels = (const uint32_t*) direct_buffer(env, in, pixels_of(width, height), &err);
    if (!pixels) goto done;
    uint8_t* file = (uint8_t*) direct_buffer(env, out, cap, &err);
    if (!file) goto done;
    argb = malloc(px * sizeof(uint32_t));
    idx = malloc(px * sizeof(uint16_t));
    palette = malloc(sizeof(uint32_t) * (size_t) pcap);
    if (!argb || !idx || !palette) { err = OOM; goto done; }
    int rc = nq_convert(h, pixels, width, height, nMaxColors, dither ? 1 : 0, seed, mode, argb, idx, palette, &K);
    const uint16_t* src = idx;
    if (rc == NQ_OK) rc = nq_encode_png(h, 1, &src, &w, &hg, palette, K, &K, 0, file, cap, offs);
    if (rc != NQ_OK) err = nq_last_error(h);
done:
    free(palette); free(idx); free(argb);
    if (err) { throw_rt(env, err); return -1; }
    return (jlong) offs[1];
}

/* nqApngMaxBytes(): nq_apng_max_bytes, the bound for every K; -1 when a size is invalid */
JNIEXPORT jlong JNICALL Java_com_android_nQuant_PnnQuantizer_nqApngMaxBytes(JNIEnv* env, jclass c, jint n, jint width, jint height) {
    int64_t bytes = -1;
    if (nq_apng_max_bytes(n, width, height, 0, &bytes) != NQ_OK) bytes = -1;
    return (jlong) bytes;
}

/* encodeApng(): direct ShortBuffers of indices in (frames of one size), the file written to the direct ByteBuffer `out` (cap bytes)
 * -> nq_encode_apng.  Returns the file size. */
JNIEXPORT jlong JNICALL Java_com_android_nQuant_PnnQuantizer_nqEncodeApng(JNIEnv* env, jclass c, jlong hh, jobjectArray index,
        jint width, jint height, jintArray palette, jintArray delaysCs, jint loopCount, jobject out, jlong cap) {
    return encode_one_size(env, hh, index, width, height, palette, delaysCs, loopCount, out, cap, 1);
}

/* convertFramesToApng(): nq_convert_frames of frames of one size with index outputs (the ARGB outputs go to scratch), then
 * nq_encode_apng of the index maps with the shared palette, on the same handle, into the direct ByteBuffer `out` (cap bytes).
 * Returns the file size. */
JNIEXPORT jlong JNICALL Java_com_android_nQuant_PnnQuantizer_nqConvertFramesToApng(JNIEnv* env, jclass c, jlong hh, jobjectArray in,
        jint width, jint height, jint nMaxColors, jboolean dither, jlongArray seeds, jint mode, jintArray delaysCs, jint loopCount,
        jobject out, jlong cap) {
    const char* err = NULL;
    jint *w = NULL, *hg = NULL;
    jlong size = -1;
    jsize n = 0;
    if (!in || (n = (*env)->GetArrayLength(env, in)) < 1) { err = "no frames"; goto done; }
    w = malloc(sizeof(jint) * n);
    hg = malloc(sizeof(jint) * n);
    if (!w || !hg) { err = OOM; goto done; }
    for (jsize i = 0; i < n; ++i) { w[i] = width; hg[i] = height; }
    size = frames_to_file(env, (nq_handle*) (intptr_t) hh, in, n, w, hg, nMaxColors, dither, seeds, mode, delaysCs, loopCount, 2, out, cap, &err);
done:
    free(hg); free(w);
    if (err) { throw_rt(env, err); return -1; }
    return size;
}
