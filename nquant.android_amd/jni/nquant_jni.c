/*
 * nquant_jni.c -- JNI shim between the reference's Java API and libnquant_hip.so (include/nquant_abi.h).
 * NOT compiled in the build image (no JDK / jni.h there); build on a box with a JDK:
 *   gcc -shared -fPIC -I$JAVA_HOME/include -I$JAVA_HOME/include/linux -I../../include nquant_jni.c \
 *       -L.. -lnquant_hip -o libnquant_jni.so
 * Java side: ../java/com/android/nQuant/PnnQuantizer.java, PnnLABQuantizer.java (same class names, constructor and
 * convert()/hasAlpha() signatures as the reference: NQ/PnnQuantizer.java:35,409,458; NQ/PnnLABQuantizer.java:24).
 */
#include <jni.h>
#include <stdint.h>
#include <stdlib.h>
#include "nquant_abi.h"

static void throw_rt(JNIEnv* env, const char* msg) {
    (*env)->ThrowNew(env, (*env)->FindClass(env, "java/lang/RuntimeException"), msg ? msg : "nquant error");
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
    uint32_t* palette = (uint32_t*) malloc((size_t) cap * sizeof(uint32_t));     /* per call: two threads may convert different objects at once */
    if (!palette) { throw_rt(env, "out of memory"); return NULL; }
    int32_t K = 0;
    /* The convert blocks on the GPU for up to seconds (the merge loop): plain Get/Release<Type>ArrayElements, not critical regions --
     * a critical region must be short and non-blocking and would stall the collector JVM-wide for the whole call. */
    jint* in = (*env)->GetIntArrayElements(env, argb, NULL);
    jint* out = (*env)->GetIntArrayElements(env, outArgb, NULL);
    jshort* idx = outIndex ? (*env)->GetShortArrayElements(env, outIndex, NULL) : NULL;
    if (!in || !out || (outIndex && !idx)) {
        if (idx) (*env)->ReleaseShortArrayElements(env, outIndex, idx, JNI_ABORT);
        if (out) (*env)->ReleaseIntArrayElements(env, outArgb, out, JNI_ABORT);
        if (in) (*env)->ReleaseIntArrayElements(env, argb, in, JNI_ABORT);
        free(palette);
        return NULL;                                                             /* OutOfMemoryError already pending */
    }
    int rc = nq_convert(h, (const uint32_t*) in, w, hgt, nMaxColors, dither ? 1 : 0, seed, mode,
                        (uint32_t*) out, (uint16_t*) idx, palette, &K);
    if (idx) (*env)->ReleaseShortArrayElements(env, outIndex, idx, 0);
    (*env)->ReleaseIntArrayElements(env, outArgb, out, 0);
    (*env)->ReleaseIntArrayElements(env, argb, in, JNI_ABORT);                   /* the input is never modified */
    if (rc != NQ_OK) { free(palette); throw_rt(env, nq_last_error(h)); return NULL; }        /* convert() `throws Exception` */
    jintArray pal = (*env)->NewIntArray(env, K);
    if (pal) (*env)->SetIntArrayRegion(env, pal, 0, K, (const jint*) palette);
    free(palette);
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
    const jsize n = (*env)->GetArrayLength(env, handles);
    const int stride = nMaxColors > 2 ? nMaxColors : 2;
    nq_handle** hs = malloc(sizeof(*hs) * n);
    const uint32_t** src = malloc(sizeof(*src) * n);
    uint32_t** dst = malloc(sizeof(*dst) * n);
    uint32_t* palettes = malloc(sizeof(uint32_t) * (size_t) stride * n);
    int32_t* K = malloc(sizeof(int32_t) * n);
    jlong* hh = (*env)->GetLongArrayElements(env, handles, NULL);
    jlong* sd = (*env)->GetLongArrayElements(env, seeds, NULL);
    jint* w = (*env)->GetIntArrayElements(env, widths, NULL);
    jint* hg = (*env)->GetIntArrayElements(env, heights, NULL);
    for (jsize i = 0; i < n; ++i) {
        hs[i] = (nq_handle*) (intptr_t) hh[i];
        src[i] = (const uint32_t*) (*env)->GetDirectBufferAddress(env, (*env)->GetObjectArrayElement(env, in, i));
        dst[i] = (uint32_t*) (*env)->GetDirectBufferAddress(env, (*env)->GetObjectArrayElement(env, out, i));
    }
    const int rc = nq_convert_batch(hs, n, src, (const int32_t*) w, (const int32_t*) hg, nMaxColors, dither ? 1 : 0,
                                    (const int64_t*) sd, mode, dst, NULL, palettes, stride, K);
    jobjectArray result = NULL;
    if (rc != NQ_OK) throw_rt(env, nq_last_error(hs[0]));
    else {
        result = (*env)->NewObjectArray(env, n, (*env)->FindClass(env, "[I"), NULL);
        for (jsize i = 0; i < n; ++i) {
            jintArray pal = (*env)->NewIntArray(env, K[i]);
            (*env)->SetIntArrayRegion(env, pal, 0, K[i], (const jint*) (palettes + (size_t) i * stride));
            (*env)->SetObjectArrayElement(env, result, i, pal);
        }
    }
    (*env)->ReleaseIntArrayElements(env, heights, hg, JNI_ABORT); (*env)->ReleaseIntArrayElements(env, widths, w, JNI_ABORT);
    (*env)->ReleaseLongArrayElements(env, seeds, sd, JNI_ABORT); (*env)->ReleaseLongArrayElements(env, handles, hh, JNI_ABORT);
    free(K); free(palettes); free(dst); free(src); free(hs);
    return result;
}

/* convertFrames(): one palette for a sequence of frames -> nq_convert_frames.  Direct IntBuffers in and out; returns the palette. */
JNIEXPORT jintArray JNICALL Java_com_android_nQuant_PnnQuantizer_nqConvertFrames(JNIEnv* env, jclass c, jlong hh, jobjectArray in,
        jintArray widths, jintArray heights, jint nMaxColors, jboolean dither, jlongArray seeds, jint mode, jobjectArray out) {
    nq_handle* h = (nq_handle*) (intptr_t) hh;
    const jsize n = (*env)->GetArrayLength(env, in);
    const int cap = nMaxColors > 2 ? nMaxColors : 2;
    const uint32_t** src = malloc(sizeof(*src) * (n > 0 ? n : 1));
    uint32_t** dst = malloc(sizeof(*dst) * (n > 0 ? n : 1));
    uint32_t* palette = malloc(sizeof(uint32_t) * (size_t) cap);
    if (!src || !dst || !palette) { free(palette); free(dst); free(src); throw_rt(env, "out of memory"); return NULL; }
    int32_t K = 0;
    jlong* sd = (*env)->GetLongArrayElements(env, seeds, NULL);
    jint* w = (*env)->GetIntArrayElements(env, widths, NULL);
    jint* hg = (*env)->GetIntArrayElements(env, heights, NULL);
    for (jsize i = 0; i < n; ++i) {
        src[i] = (const uint32_t*) (*env)->GetDirectBufferAddress(env, (*env)->GetObjectArrayElement(env, in, i));
        dst[i] = (uint32_t*) (*env)->GetDirectBufferAddress(env, (*env)->GetObjectArrayElement(env, out, i));
    }
    const int rc = nq_convert_frames(h, n, src, (const int32_t*) w, (const int32_t*) hg, nMaxColors, dither ? 1 : 0,
                                     (const int64_t*) sd, mode, dst, NULL, palette, &K);
    jintArray pal = NULL;
    if (rc != NQ_OK) throw_rt(env, nq_last_error(h));
    else {
        pal = (*env)->NewIntArray(env, K);
        if (pal) (*env)->SetIntArrayRegion(env, pal, 0, K, (const jint*) palette);
    }
    (*env)->ReleaseIntArrayElements(env, heights, hg, JNI_ABORT); (*env)->ReleaseIntArrayElements(env, widths, w, JNI_ABORT);
    (*env)->ReleaseLongArrayElements(env, seeds, sd, JNI_ABORT);
    free(palette); free(dst); free(src);
    return pal;
}

/* nqGifMaxBytes(): nq_gif_max_bytes for K = 256, the bound for every K; -1 when a size is invalid */
JNIEXPORT jlong JNICALL Java_com_android_nQuant_PnnQuantizer_nqGifMaxBytes(JNIEnv* env, jclass c, jintArray widths, jintArray heights) {
    const jsize n = (*env)->GetArrayLength(env, widths);
    if ((*env)->GetArrayLength(env, heights) != n) return -1;
    jint* w = (*env)->GetIntArrayElements(env, widths, NULL);
    jint* hg = (*env)->GetIntArrayElements(env, heights, NULL);
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
    const jsize n = (*env)->GetArrayLength(env, index);
    const uint16_t** src = malloc(sizeof(*src) * (n > 0 ? n : 1));
    if (!src) { throw_rt(env, "out of memory"); return -1; }
    for (jsize i = 0; i < n; ++i)
        src[i] = (const uint16_t*) (*env)->GetDirectBufferAddress(env, (*env)->GetObjectArrayElement(env, index, i));
    jint* w = (*env)->GetIntArrayElements(env, widths, NULL);
    jint* hg = (*env)->GetIntArrayElements(env, heights, NULL);
    jint* pal = (*env)->GetIntArrayElements(env, palette, NULL);
    jint* d = delaysCs ? (*env)->GetIntArrayElements(env, delaysCs, NULL) : NULL;
    const jsize K = (*env)->GetArrayLength(env, palette);
    int64_t size = -1;
    const int rc = nq_encode_gif(h, n, src, (const int32_t*) w, (const int32_t*) hg, (const uint32_t*) pal, K, (const int32_t*) d, loopCount, 0,
                                 (uint8_t*) (*env)->GetDirectBufferAddress(env, out), cap, &size);
    if (d) (*env)->ReleaseIntArrayElements(env, delaysCs, d, JNI_ABORT);
    (*env)->ReleaseIntArrayElements(env, palette, pal, JNI_ABORT);
    (*env)->ReleaseIntArrayElements(env, heights, hg, JNI_ABORT); (*env)->ReleaseIntArrayElements(env, widths, w, JNI_ABORT);
    free(src);
    if (rc != NQ_OK) { throw_rt(env, nq_last_error(h)); return -1; }
    return (jlong) size;
}

/* encodeGifDelta(): as encodeGif for frames of one size, every frame after the first stored as the rectangle that changed ->
 * nq_encode_gif_delta.  Returns the file size. */
JNIEXPORT jlong JNICALL Java_com_android_nQuant_PnnQuantizer_nqEncodeGifDelta(JNIEnv* env, jclass c, jlong hh, jobjectArray index,
        jint width, jint height, jintArray palette, jintArray delaysCs, jint loopCount, jobject out, jlong cap) {
    nq_handle* h = (nq_handle*) (intptr_t) hh;
    const jsize n = (*env)->GetArrayLength(env, index);
    const uint16_t** src = malloc(sizeof(*src) * (n > 0 ? n : 1));
    if (!src) { throw_rt(env, "out of memory"); return -1; }
    for (jsize i = 0; i < n; ++i)
        src[i] = (const uint16_t*) (*env)->GetDirectBufferAddress(env, (*env)->GetObjectArrayElement(env, index, i));
    jint* pal = (*env)->GetIntArrayElements(env, palette, NULL);
    jint* d = delaysCs ? (*env)->GetIntArrayElements(env, delaysCs, NULL) : NULL;
    const jsize K = (*env)->GetArrayLength(env, palette);
    int64_t size = -1;
    const int rc = nq_encode_gif_delta(h, n, src, width, height, (const uint32_t*) pal, K, (const int32_t*) d, loopCount, 0,
                                       (uint8_t*) (*env)->GetDirectBufferAddress(env, out), cap, &size, NULL);
    if (d) (*env)->ReleaseIntArrayElements(env, delaysCs, d, JNI_ABORT);
    (*env)->ReleaseIntArrayElements(env, palette, pal, JNI_ABORT);
    free(src);
    if (rc != NQ_OK) { throw_rt(env, nq_last_error(h)); return -1; }
    return (jlong) size;
}

/* convertFramesToGif(): nq_convert_frames with index outputs (the ARGB outputs go to scratch), then nq_encode_gif of the index maps
 * with the shared palette into the direct ByteBuffer `out` (cap bytes); delta: nq_encode_gif_delta instead, the frames must have one
 * size.  Returns the file size. */
JNIEXPORT jlong JNICALL Java_com_android_nQuant_PnnQuantizer_nqConvertFramesToGif(JNIEnv* env, jclass c, jlong hh, jobjectArray in,
        jintArray widths, jintArray heights, jint nMaxColors, jboolean dither, jlongArray seeds, jint mode, jintArray delaysCs, jint loopCount,
        jboolean delta, jobject out, jlong cap) {
    nq_handle* h = (nq_handle*) (intptr_t) hh;
    const jsize n = (*env)->GetArrayLength(env, in);
    const int pcap = nMaxColors > 2 ? nMaxColors : 2;
    const uint32_t** src = malloc(sizeof(*src) * (n > 0 ? n : 1));
    uint32_t** argb = calloc(n > 0 ? n : 1, sizeof(*argb));
    uint16_t** idx = calloc(n > 0 ? n : 1, sizeof(*idx));
    uint32_t* palette = malloc(sizeof(uint32_t) * (size_t) pcap);
    jint* w = (*env)->GetIntArrayElements(env, widths, NULL);
    jint* hg = (*env)->GetIntArrayElements(env, heights, NULL);
    jlong* sd = (*env)->GetLongArrayElements(env, seeds, NULL);
    jint* d = delaysCs ? (*env)->GetIntArrayElements(env, delaysCs, NULL) : NULL;
    int ok = src && argb && idx && palette && w && hg && sd;
    for (jsize i = 0; ok && i < n; ++i) {
        const size_t px = (size_t) (w[i] > 0 ? w[i] : 1) * (size_t) (hg[i] > 0 ? hg[i] : 1);
        src[i] = (const uint32_t*) (*env)->GetDirectBufferAddress(env, (*env)->GetObjectArrayElement(env, in, i));
        argb[i] = malloc(px * sizeof(uint32_t));
        idx[i] = malloc(px * sizeof(uint16_t));
        ok = argb[i] && idx[i];
    }
    int32_t K = 0;
    int64_t size = -1;
    int rc = NQ_OK;
    int one_size = 1;
    for (jsize i = 1; ok && delta && i < n; ++i) one_size = one_size && w[i] == w[0] && hg[i] == hg[0];
    if (ok && one_size) {
        rc = nq_convert_frames(h, n, src, (const int32_t*) w, (const int32_t*) hg, nMaxColors, dither ? 1 : 0, (const int64_t*) sd, mode,
                               argb, idx, palette, &K);
        if (rc == NQ_OK && delta)
            rc = nq_encode_gif_delta(h, n, (const uint16_t* const*) idx, n > 0 ? w[0] : 0, n > 0 ? hg[0] : 0, palette, K, (const int32_t*) d,
                                     loopCount, 0, (uint8_t*) (*env)->GetDirectBufferAddress(env, out), cap, &size, NULL);
        else if (rc == NQ_OK)
            rc = nq_encode_gif(h, n, (const uint16_t* const*) idx, (const int32_t*) w, (const int32_t*) hg, palette, K, (const int32_t*) d,
                               loopCount, 0, (uint8_t*) (*env)->GetDirectBufferAddress(env, out), cap, &size);
    }
    for (jsize i = 0; argb && idx && i < n; ++i) { free(argb[i]); free(idx[i]); }
    if (d) (*env)->ReleaseIntArrayElements(env, delaysCs, d, JNI_ABORT);
    if (sd) (*env)->ReleaseLongArrayElements(env, seeds, sd, JNI_ABORT);
    if (hg) (*env)->ReleaseIntArrayElements(env, heights, hg, JNI_ABORT);
    if (w) (*env)->ReleaseIntArrayElements(env, widths, w, JNI_ABORT);
    free(palette); free(idx); free(argb); free(src);
    if (!ok) { throw_rt(env, "out of memory"); return -1; }
    if (!one_size) { throw_rt(env, "delta mode: all frames must have one size"); return -1; }
    if (rc != NQ_OK) { throw_rt(env, nq_last_error(h)); return -1; }
    return (jlong) size;
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
    const uint16_t* src = (const uint16_t*) (*env)->GetDirectBufferAddress(env, index);
    const int32_t w = width, hg = height, K = (*env)->GetArrayLength(env, palette);
    jint* pal = (*env)->GetIntArrayElements(env, palette, NULL);
    if (!pal) { throw_rt(env, "out of memory"); return -1; }
    int64_t offs[2] = {0, -1};
    const int rc = nq_encode_png(h, 1, &src, &w, &hg, (const uint32_t*) pal, K, &K, 0, (uint8_t*) (*env)->GetDirectBufferAddress(env, out), cap, offs);
    (*env)->ReleaseIntArrayElements(env, palette, pal, JNI_ABORT);
    if (rc != NQ_OK) { throw_rt(env, nq_last_error(h)); return -1; }
    return (jlong) offs[1];
}

/* convertToPng(): nq_convert with the index output (the ARGB output goes to scratch), then nq_encode_png of the index map with the
 * image's palette into the direct ByteBuffer `out` (cap bytes).  Returns the file size. */
JNIEXPORT jlong JNICALL Java_com_android_nQuant_PnnQuantizer_nqConvertToPng(JNIEnv* env, jclass c, jlong hh, jobject in, jint width,
        jint height, jint nMaxColors, jboolean dither, jlong seed, jint mode, jobject out, jlong cap) {
    nq_handle* h = (nq_handle*) (intptr_t) hh;
    const size_t px = (size_t) (width > 0 ? width : 1) * (size_t) (height > 0 ? height : 1);
    const int pcap = nMaxColors > 2 ? nMaxColors : 2;
    uint32_t* argb = malloc(px * sizeof(uint32_t));
    uint16_t* idx = malloc(px * sizeof(uint16_t));
    uint32_t* palette = malloc(sizeof(uint32_t) * (size_t) pcap);
    const int32_t w = width, hg = height;
    int32_t K = 0;
    int64_t offs[2] = {0, -1};
    int rc = NQ_OK;
    const int ok = argb && idx && palette;
    if (ok) {
        rc = nq_convert(h, (const uint32_t*) (*env)->GetDirectBufferAddress(env, in), width, height, nMaxColors, dither ? 1 : 0, seed, mode,
                        argb, idx, palette, &K);
        const uint16_t* src = idx;
        if (rc == NQ_OK)
            rc = nq_encode_png(h, 1, &src, &w, &hg, palette, K, &K, 0, (uint8_t*) (*env)->GetDirectBufferAddress(env, out), cap, offs);
    }
    free(palette); free(idx); free(argb);
    if (!ok) { throw_rt(env, "out of memory"); return -1; }
    if (rc != NQ_OK) { throw_rt(env, nq_last_error(h)); return -1; }
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
    nq_handle* h = (nq_handle*) (intptr_t) hh;
    const jsize n = (*env)->GetArrayLength(env, index);
    const uint16_t** src = malloc(sizeof(*src) * (n > 0 ? n : 1));
    if (!src) { throw_rt(env, "out of memory"); return -1; }
    for (jsize i = 0; i < n; ++i)
        src[i] = (const uint16_t*) (*env)->GetDirectBufferAddress(env, (*env)->GetObjectArrayElement(env, index, i));
    jint* pal = (*env)->GetIntArrayElements(env, palette, NULL);
    jint* d = delaysCs ? (*env)->GetIntArrayElements(env, delaysCs, NULL) : NULL;
    const jsize K = (*env)->GetArrayLength(env, palette);
    int64_t size = -1;
    const int rc = nq_encode_apng(h, n, src, width, height, (const uint32_t*) pal, K, (const int32_t*) d, loopCount, 0,
                                  (uint8_t*) (*env)->GetDirectBufferAddress(env, out), cap, &size, NULL);
    if (d) (*env)->ReleaseIntArrayElements(env, delaysCs, d, JNI_ABORT);
    (*env)->ReleaseIntArrayElements(env, palette, pal, JNI_ABORT);
    free(src);
    if (rc != NQ_OK) { throw_rt(env, nq_last_error(h)); return -1; }
    return (jlong) size;
}

/* convertFramesToApng(): nq_convert_frames of frames of one size with index outputs (the ARGB outputs go to scratch), then
 * nq_encode_apng of the index maps with the shared palette, on the same handle, into the direct ByteBuffer `out` (cap bytes).
 * Returns the file size. */
JNIEXPORT jlong JNICALL Java_com_android_nQuant_PnnQuantizer_nqConvertFramesToApng(JNIEnv* env, jclass c, jlong hh, jobjectArray in,
        jint width, jint height, jint nMaxColors, jboolean dither, jlongArray seeds, jint mode, jintArray delaysCs, jint loopCount,
        jobject out, jlong cap) {
    nq_handle* h = (nq_handle*) (intptr_t) hh;
    const jsize n = (*env)->GetArrayLength(env, in);
    const jsize m = n > 0 ? n : 1;
    const int pcap = nMaxColors > 2 ? nMaxColors : 2;
    const size_t px = (size_t) (width > 0 ? width : 1) * (size_t) (height > 0 ? height : 1);
    const uint32_t** src = malloc(sizeof(*src) * m);
    uint32_t** argb = calloc(m, sizeof(*argb));
    uint16_t** idx = calloc(m, sizeof(*idx));
    int32_t* w = malloc(sizeof(int32_t) * m);
    int32_t* hg = malloc(sizeof(int32_t) * m);
    uint32_t* palette = malloc(sizeof(uint32_t) * (size_t) pcap);
    jlong* sd = seeds ? (*env)->GetLongArrayElements(env, seeds, NULL) : NULL;
    jint* d = delaysCs ? (*env)->GetIntArrayElements(env, delaysCs, NULL) : NULL;
    int ok = src && argb && idx && w && hg && palette && sd;
    for (jsize i = 0; ok && i < n; ++i) {
        src[i] = (const uint32_t*) (*env)->GetDirectBufferAddress(env, (*env)->GetObjectArrayElement(env, in, i));
        argb[i] = malloc(px * sizeof(uint32_t));
        idx[i] = malloc(px * sizeof(uint16_t));
        w[i] = width; hg[i] = height;
        ok = argb[i] && idx[i];
    }
    int32_t K = 0;
    int64_t size = -1;
    int rc = NQ_OK;
    if (ok) {
        rc = nq_convert_frames(h, n, src, w, hg, nMaxColors, dither ? 1 : 0, (const int64_t*) sd, mode, argb, idx, palette, &K);
        if (rc == NQ_OK)
            rc = nq_encode_apng(h, n, (const uint16_t* const*) idx, width, height, palette, K, (const int32_t*) d, loopCount, 0,
                                (uint8_t*) (*env)->GetDirectBufferAddress(env, out), cap, &size, NULL);
    }
    for (jsize i = 0; argb && idx && i < n; ++i) { free(argb[i]); free(idx[i]); }
    if (d) (*env)->ReleaseIntArrayElements(env, delaysCs, d, JNI_ABORT);
    if (sd) (*env)->ReleaseLongArrayElements(env, seeds, sd, JNI_ABORT);
    free(palette); free(hg); free(w); free(idx); free(argb); free(src);
    if (!seeds) { throw_rt(env, "seeds is null"); return -1; }
    if (!ok) { throw_rt(env, "out of memory"); return -1; }
    if (rc != NQ_OK) { throw_rt(env, nq_last_error(h)); return -1; }
    return (jlong) size;
}
