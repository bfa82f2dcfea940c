/* tests/c/jni_fake/fake_jni.c -- a small fake JNI runtime (see jni.h next to this file): the function table implemented over tagged
 * heap objects, strict where a JVM is lenient, so that mistakes of nquant.android_amd/jni/nquant_jni.c show up as counted violations
 * instead of as silent luck:
 *   * Get<Type>ArrayElements always hands out a COPY between two canary blocks; Release with mode 0 / JNI_COMMIT copies back,
 *     JNI_ABORT discards -- an output released with JNI_ABORT stays as it was, a write through an aborted pointer is counted
 *     (FJ_ABORTED_WRITES), a write past either end trips a canary, a release of a pointer that is not outstanding or with another
 *     array is a violation, not a crash;
 *   * every GetObjectArrayElement, New<Type>Array, NewObjectArray, FindClass and PopLocalFrame(result) creates a local reference;
 *     DeleteLocalRef and PopLocalFrame retire them; the live count and its peak are kept (the JNI specification guarantees 16);
 *   * at most one exception is pending; any call other than the Exception*, Release*, DeleteLocalRef, Push/PopLocalFrame functions
 *     made while one is pending is a violation, as under CheckJNI;
 *   * fj_fail_alloc(k): the k-th allocating JNI call from now (Get<Type>ArrayElements, New*Array, FindClass, PushLocalFrame,
 *     EnsureLocalCapacity) fails: NULL / JNI_ERR with a java/lang/OutOfMemoryError pending;
 *   * a direct buffer has an address and a capacity in elements; a heap buffer answers NULL and -1.
 * The fj_* functions are the plain C side for ctypes (tests/jni_fake.py).  One thread, one JNIEnv.  Test infrastructure only. */
#include <jni.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#define FJ_EXPORT __attribute__((visibility("default")))
#define MAGIC 0x4A4F424Au
#define CANARY 64
#define CANARY_BYTE 0xC5

enum { T_INT = 1, T_LONG, T_SHORT, T_OBJARR, T_DIRECT, T_HEAPBUF, T_CLASS };

typedef struct fobj {
    uint32_t magic;
    int tag, elsize, refs;        /* refs: the host's hold + live local references + object-array slots */
    int64_t len;                  /* arrays: elements; buffers: capacity in elements */
    void* data;                   /* arrays: the payload (owned); direct buffers: the address (not owned) */
    size_t bytes;
    char name[64];                /* classes */
} fobj;

typedef struct { void* user; unsigned char* base; fobj* arr; size_t bytes; } copy_rec;

static struct {
    fobj** objs; int nobjs, cap_objs;
    fobj** locals; int nlocals, cap_locals, peak_locals;
    int marks[64]; int nmarks;
    copy_rec* copies; int ncopies, cap_copies;
    int64_t obj_bytes, violations, aborted_writes, alloc_calls, fail_in, jni_calls;
    int pending;
    char exc_class[64], exc_msg[512];
    char log[4096];
} g;

static void violation(const char* fmt, ...) {
    char line[256];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(line, sizeof line, fmt, ap);
    va_end(ap);
    g.violations++;
    size_t used = strlen(g.log);
    if (used + strlen(line) + 2 < sizeof g.log) { strcat(g.log, line); strcat(g.log, "\n"); }
}

static void set_pending(const char* cls, const char* msg) {
    if (g.pending) { violation("exception %s thrown while %s is pending", cls, g.exc_class); return; }
    g.pending = 1;
    snprintf(g.exc_class, sizeof g.exc_class, "%s", cls);
    snprintf(g.exc_msg, sizeof g.exc_msg, "%s", msg ? msg : "");
}

/* ---- objects ---- */
static fobj* as_obj(const void* p) {
    if (!p) return NULL;
    for (int i = g.nobjs - 1; i >= 0; --i)
        if (g.objs[i] == p) return g.objs[i];
    return NULL;
}

static fobj* new_obj(int tag, int elsize, int64_t len, int with_payload) {
    fobj* o = calloc(1, sizeof *o);
    if (!o) abort();
    o->magic = MAGIC; o->tag = tag; o->elsize = elsize; o->len = len;
    o->bytes = sizeof *o;
    if (with_payload) {
        const size_t nb = (size_t) (len > 0 ? len : 0) * (size_t) elsize;
        o->data = calloc(nb ? nb : 1, 1);
        if (!o->data) abort();
        o->bytes += nb;
    }
    if (g.nobjs == g.cap_objs) {
        g.cap_objs = g.cap_objs ? 2 * g.cap_objs : 256;
        g.objs = realloc(g.objs, sizeof(fobj*) * g.cap_objs);
        if (!g.objs) abort();
    }
    g.objs[g.nobjs++] = o;
    g.obj_bytes += (int64_t) o->bytes;
    return o;
}

static void unref(fobj* o) {
    if (!o || --o->refs > 0) return;
    if (o->tag == T_OBJARR)
        for (int64_t i = 0; i < o->len; ++i) unref(((fobj**) o->data)[i]);
    for (int i = g.nobjs - 1; i >= 0; --i)
        if (g.objs[i] == o) { g.objs[i] = g.objs[--g.nobjs]; break; }
    g.obj_bytes -= (int64_t) o->bytes;
    if (o->tag != T_DIRECT) free(o->data);
    o->magic = 0;
    free(o);
}

static jobject add_local(fobj* o) {
    if (!o) return NULL;
    if (g.nlocals == g.cap_locals) {
        g.cap_locals = g.cap_locals ? 2 * g.cap_locals : 64;
        g.locals = realloc(g.locals, sizeof(fobj*) * g.cap_locals);
        if (!g.locals) abort();
    }
    g.locals[g.nlocals++] = o;
    o->refs++;
    if (g.nlocals > g.peak_locals) g.peak_locals = g.nlocals;
    return (jobject) o;
}

static void pop_locals_to(int mark) {
    while (g.nlocals > mark) unref(g.locals[--g.nlocals]);
}

/* every JNI function: counted; only a few may run while an exception is pending */
static void enter(const char* name, int allowed_while_pending) {
    g.jni_calls++;
    if (g.pending && !allowed_while_pending) violation("%s called while %s is pending", name, g.exc_class);
}

static int alloc_fails(void) {
    g.alloc_calls++;
    if (g.fail_in > 0 && --g.fail_in == 0) { set_pending("java/lang/OutOfMemoryError", "injected allocation failure"); return 1; }
    return 0;
}

static fobj* typed(const char* fn, const void* p, int tag) {
    fobj* o = as_obj(p);
    if (!o) { violation("%s: %s", fn, p ? "not an object" : "null object"); return NULL; }
    if (tag && o->tag != tag) { violation("%s: object of tag %d where tag %d is required", fn, o->tag, tag); return NULL; }
    return o;
}

/* ---- the table ---- */
static jclass f_FindClass(JNIEnv* env, const char* name) {
    enter("FindClass", 0);
    if (alloc_fails()) return NULL;
    fobj* o = new_obj(T_CLASS, 0, 0, 0);
    snprintf(o->name, sizeof o->name, "%s", name ? name : "");
    return add_local(o);
}

static jint f_ThrowNew(JNIEnv* env, jclass cls, const char* msg) {
    enter("ThrowNew", 0);
    fobj* c = typed("ThrowNew", cls, T_CLASS);
    if (!c) return JNI_ERR;
    set_pending(c->name, msg);
    return JNI_OK;
}

static jthrowable f_ExceptionOccurred(JNIEnv* env) { enter("ExceptionOccurred", 1); return NULL; }
static void f_ExceptionClear(JNIEnv* env) { enter("ExceptionClear", 1); g.pending = 0; }
static jboolean f_ExceptionCheck(JNIEnv* env) { enter("ExceptionCheck", 1); return g.pending ? JNI_TRUE : JNI_FALSE; }

static jint f_PushLocalFrame(JNIEnv* env, jint capacity) {
    enter("PushLocalFrame", 1);
    if (alloc_fails()) return JNI_ERR;
    if (g.nmarks == 64) { violation("PushLocalFrame: more than 64 frames"); return JNI_ERR; }
    g.marks[g.nmarks++] = g.nlocals;
    return JNI_OK;
}

static jobject f_PopLocalFrame(JNIEnv* env, jobject result) {
    enter("PopLocalFrame", 1);
    if (g.nmarks == 0) { violation("PopLocalFrame without PushLocalFrame"); return NULL; }
    fobj* r = result ? typed("PopLocalFrame", result, 0) : NULL;
    if (r) r->refs++;
    pop_locals_to(g.marks[--g.nmarks]);
    jobject out = add_local(r);
    if (r) unref(r);
    return out;
}

static void f_DeleteLocalRef(JNIEnv* env, jobject ref) {
    enter("DeleteLocalRef", 1);
    if (!ref) return;
    const int floor = g.nmarks ? g.marks[g.nmarks - 1] : 0;
    for (int i = g.nlocals - 1; i >= floor; --i)
        if ((jobject) g.locals[i] == ref) {
            fobj* o = g.locals[i];
            memmove(g.locals + i, g.locals + i + 1, sizeof(fobj*) * (size_t) (g.nlocals - i - 1));
            g.nlocals--;
            unref(o);
            return;
        }
    violation("DeleteLocalRef of a reference that is not live in this frame");
}

static jint f_EnsureLocalCapacity(JNIEnv* env, jint capacity) {
    enter("EnsureLocalCapacity", 0);
    return alloc_fails() ? JNI_ERR : JNI_OK;
}

static jsize f_GetArrayLength(JNIEnv* env, jarray a) {
    enter("GetArrayLength", 0);
    fobj* o = typed("GetArrayLength", a, 0);
    if (!o) return 0;
    if (o->tag < T_INT || o->tag > T_OBJARR) { violation("GetArrayLength: not an array (tag %d)", o->tag); return 0; }
    return (jsize) o->len;
}

static jobjectArray f_NewObjectArray(JNIEnv* env, jsize n, jclass cls, jobject init) {
    enter("NewObjectArray", 0);
    if (!typed("NewObjectArray", cls, T_CLASS)) return NULL;
    if (n < 0) { set_pending("java/lang/NegativeArraySizeException", ""); return NULL; }
    if (alloc_fails()) return NULL;
    return add_local(new_obj(T_OBJARR, (int) sizeof(fobj*), n, 1));
}

static jobject f_GetObjectArrayElement(JNIEnv* env, jobjectArray a, jsize i) {
    enter("GetObjectArrayElement", 0);
    fobj* o = typed("GetObjectArrayElement", a, T_OBJARR);
    if (!o) return NULL;
    if (i < 0 || i >= o->len) { violation("GetObjectArrayElement: index %d of %lld", (int) i, (long long) o->len);
                                set_pending("java/lang/ArrayIndexOutOfBoundsException", ""); return NULL; }
    return add_local(((fobj**) o->data)[i]);
}

static void f_SetObjectArrayElement(JNIEnv* env, jobjectArray a, jsize i, jobject v) {
    enter("SetObjectArrayElement", 0);
    fobj* o = typed("SetObjectArrayElement", a, T_OBJARR);
    if (!o) return;
    if (i < 0 || i >= o->len) { violation("SetObjectArrayElement: index %d of %lld", (int) i, (long long) o->len);
                                set_pending("java/lang/ArrayIndexOutOfBoundsException", ""); return; }
    fobj* e = v ? typed("SetObjectArrayElement", v, 0) : NULL;
    if (v && !e) return;
    if (e) e->refs++;
    unref(((fobj**) o->data)[i]);
    ((fobj**) o->data)[i] = e;
}

static jintArray f_NewIntArray(JNIEnv* env, jsize n) {
    enter("NewIntArray", 0);
    if (n < 0) { set_pending("java/lang/NegativeArraySizeException", ""); return NULL; }
    if (alloc_fails()) return NULL;
    return add_local(new_obj(T_INT, 4, n, 1));
}

static void* get_elements(const char* fn, jarray a, int tag, jboolean* is_copy) {
    enter(fn, 0);
    fobj* o = typed(fn, a, tag);
    if (!o) return NULL;
    if (alloc_fails()) return NULL;
    const size_t nb = (size_t) o->len * (size_t) o->elsize;
    unsigned char* base = malloc(nb + 2 * CANARY);
    if (!base) abort();
    memset(base, CANARY_BYTE, CANARY);
    memcpy(base + CANARY, o->data, nb);
    memset(base + CANARY + nb, CANARY_BYTE, CANARY);
    if (g.ncopies == g.cap_copies) {
        g.cap_copies = g.cap_copies ? 2 * g.cap_copies : 32;
        g.copies = realloc(g.copies, sizeof(copy_rec) * g.cap_copies);
        if (!g.copies) abort();
    }
    g.copies[g.ncopies++] = (copy_rec){base + CANARY, base, o, nb};
    g.obj_bytes += (int64_t) (nb + 2 * CANARY);
    if (is_copy) *is_copy = JNI_TRUE;
    return base + CANARY;
}

static void release_elements(const char* fn, jarray a, void* p, jint mode) {
    enter(fn, 1);
    int at = -1;
    for (int i = 0; i < g.ncopies; ++i)
        if (g.copies[i].user == p) { at = i; break; }
    if (at < 0) { violation("%s: the pointer is not outstanding", fn); return; }
    copy_rec r = g.copies[at];
    if ((jarray) r.arr != a) { violation("%s: the pointer belongs to another array", fn); return; }
    for (int i = 0; i < CANARY; ++i)
        if (r.base[i] != CANARY_BYTE || r.base[CANARY + r.bytes + i] != CANARY_BYTE) {
            violation("%s: a canary next to the elements was overwritten (array of %lld elements)", fn, (long long) r.arr->len);
            break;
        }
    if (mode != 0 && mode != JNI_COMMIT && mode != JNI_ABORT) violation("%s: mode %d", fn, (int) mode);
    if (mode == JNI_ABORT) {
        if (memcmp(r.user, r.arr->data, r.bytes) != 0) g.aborted_writes++;
    } else
        memcpy(r.arr->data, r.user, r.bytes);
    if (mode == JNI_COMMIT) return;
    g.copies[at] = g.copies[--g.ncopies];
    g.obj_bytes -= (int64_t) (r.bytes + 2 * CANARY);
    free(r.base);
}

static jint* f_GetIntArrayElements(JNIEnv* env, jintArray a, jboolean* c) { return get_elements("GetIntArrayElements", a, T_INT, c); }
static jlong* f_GetLongArrayElements(JNIEnv* env, jlongArray a, jboolean* c) { return get_elements("GetLongArrayElements", a, T_LONG, c); }
static jshort* f_GetShortArrayElements(JNIEnv* env, jshortArray a, jboolean* c) { return get_elements("GetShortArrayElements", a, T_SHORT, c); }
static void f_ReleaseIntArrayElements(JNIEnv* env, jintArray a, jint* p, jint m) { release_elements("ReleaseIntArrayElements", a, p, m); }
static void f_ReleaseLongArrayElements(JNIEnv* env, jlongArray a, jlong* p, jint m) { release_elements("ReleaseLongArrayElements", a, p, m); }
static void f_ReleaseShortArrayElements(JNIEnv* env, jshortArray a, jshort* p, jint m) { release_elements("ReleaseShortArrayElements", a, p, m); }

static void f_SetIntArrayRegion(JNIEnv* env, jintArray a, jsize start, jsize n, const jint* src) {
    enter("SetIntArrayRegion", 0);
    fobj* o = typed("SetIntArrayRegion", a, T_INT);
    if (!o) return;
    if (start < 0 || n < 0 || (int64_t) start + n > o->len) {
        violation("SetIntArrayRegion: [%d, %d) of %lld", (int) start, (int) start + (int) n, (long long) o->len);
        set_pending("java/lang/ArrayIndexOutOfBoundsException", "");
        return;
    }
    if (n) memcpy((jint*) o->data + start, src, sizeof(jint) * (size_t) n);
}

static void* f_GetDirectBufferAddress(JNIEnv* env, jobject b) {
    enter("GetDirectBufferAddress", 0);
    fobj* o = typed("GetDirectBufferAddress", b, 0);
    return o && o->tag == T_DIRECT ? o->data : NULL;
}

static jlong f_GetDirectBufferCapacity(JNIEnv* env, jobject b) {
    enter("GetDirectBufferCapacity", 0);
    fobj* o = typed("GetDirectBufferCapacity", b, 0);
    return o && o->tag == T_DIRECT ? (jlong) o->len : -1;
}

static const struct JNINativeInterface_ table = {
    f_FindClass, f_ThrowNew, f_ExceptionOccurred, f_ExceptionClear, f_ExceptionCheck, f_PushLocalFrame, f_PopLocalFrame, f_DeleteLocalRef,
    f_EnsureLocalCapacity, f_GetArrayLength, f_NewObjectArray, f_GetObjectArrayElement, f_SetObjectArrayElement, f_NewIntArray,
    f_GetIntArrayElements, f_GetLongArrayElements, f_GetShortArrayElements, f_ReleaseIntArrayElements, f_ReleaseLongArrayElements,
    f_ReleaseShortArrayElements, f_SetIntArrayRegion, f_GetDirectBufferAddress, f_GetDirectBufferCapacity,
};
static JNIEnv the_env = &table;

/* ---- the plain C side (ctypes) ---- */
FJ_EXPORT JNIEnv* fj_env(void) { return &the_env; }

static jobject host_owned(fobj* o) { o->refs = 1; return (jobject) o; }

static jobject new_array_from(int tag, int elsize, const void* src, int64_t len) {
    fobj* o = new_obj(tag, elsize, len, 1);
    if (src && len > 0) memcpy(o->data, src, (size_t) len * (size_t) elsize);
    return host_owned(o);
}
FJ_EXPORT jobject fj_new_int_array(const jint* src, int64_t len) { return new_array_from(T_INT, 4, src, len); }
FJ_EXPORT jobject fj_new_long_array(const jlong* src, int64_t len) { return new_array_from(T_LONG, 8, src, len); }
FJ_EXPORT jobject fj_new_short_array(const jshort* src, int64_t len) { return new_array_from(T_SHORT, 2, src, len); }
FJ_EXPORT jobject fj_new_object_array(int64_t len) { return host_owned(new_obj(T_OBJARR, (int) sizeof(fobj*), len, 1)); }
FJ_EXPORT void fj_set_object(jobject arr, int64_t i, jobject v) {
    fobj* o = as_obj(arr);
    fobj* e = as_obj(v);
    if (!o || o->tag != T_OBJARR || i < 0 || i >= o->len) abort();
    if (e) e->refs++;
    unref(((fobj**) o->data)[i]);
    ((fobj**) o->data)[i] = e;
}
/* a java.nio direct buffer over caller-owned memory: capacity in ELEMENTS of the buffer's type */
FJ_EXPORT jobject fj_new_direct_buffer(void* address, int64_t capacity) {
    fobj* o = new_obj(T_DIRECT, 1, capacity, 0);
    o->data = address;
    return host_owned(o);
}
FJ_EXPORT jobject fj_new_heap_buffer(int64_t capacity) { return host_owned(new_obj(T_HEAPBUF, 1, capacity, 0)); }
/* the host's hold ends (an object array lets go of its elements) */
FJ_EXPORT void fj_release(jobject o) {
    fobj* p = as_obj(o);
    if (!p) abort();
    unref(p);
}
FJ_EXPORT int fj_tag(jobject o) { fobj* p = as_obj(o); return p ? p->tag : 0; }
FJ_EXPORT int64_t fj_length(jobject o) { fobj* p = as_obj(o); return p ? p->len : -1; }
FJ_EXPORT const void* fj_data(jobject o) { fobj* p = as_obj(o); return p ? p->data : NULL; }
FJ_EXPORT jobject fj_object_element(jobject arr, int64_t i) {
    fobj* o = as_obj(arr);
    return o && o->tag == T_OBJARR && i >= 0 && i < o->len ? (jobject) ((fobj**) o->data)[i] : NULL;
}

/* a native call is bracketed by fj_begin_call / fj_end_call(result): begin resets the per-call counters; end hands the returned object
 * (if any) to the host, which must fj_release it, and retires every local reference that is still live, as a JVM does on return */
FJ_EXPORT void fj_begin_call(void) {
    g.peak_locals = g.nlocals;
    g.violations = g.aborted_writes = g.alloc_calls = g.jni_calls = 0;
    g.log[0] = 0;
}
FJ_EXPORT void fj_end_call(jobject result) {
    fobj* r = as_obj(result);
    if (result && !r) violation("the native method returned something that is not an object");
    if (r) r->refs++;
    if (g.nmarks) violation("%d local frame(s) pushed and not popped", g.nmarks);
    g.nmarks = 0;
    pop_locals_to(0);
    g.fail_in = 0;
}

enum { FJ_VIOLATIONS, FJ_OUTSTANDING, FJ_LIVE_LOCALS, FJ_PEAK_LOCALS, FJ_OBJECT_BYTES, FJ_ABORTED_WRITES, FJ_ALLOC_CALLS, FJ_PENDING,
       FJ_JNI_CALLS, FJ_OBJECTS };
FJ_EXPORT int64_t fj_get(int which) {
    switch (which) {
    case FJ_VIOLATIONS: return g.violations;
    case FJ_OUTSTANDING: return g.ncopies;
    case FJ_LIVE_LOCALS: return g.nlocals;
    case FJ_PEAK_LOCALS: return g.peak_locals;
    case FJ_OBJECT_BYTES: return g.obj_bytes;
    case FJ_ABORTED_WRITES: return g.aborted_writes;
    case FJ_ALLOC_CALLS: return g.alloc_calls;
    case FJ_PENDING: return g.pending;
    case FJ_JNI_CALLS: return g.jni_calls;
    case FJ_OBJECTS: return g.nobjs;
    }
    return -1;
}
FJ_EXPORT const char* fj_violation_log(void) { return g.log; }
FJ_EXPORT const char* fj_exception_class(void) { return g.pending ? g.exc_class : ""; }
FJ_EXPORT const char* fj_exception_message(void) { return g.pending ? g.exc_msg : ""; }
FJ_EXPORT void fj_exception_clear(void) { g.pending = 0; }
/* the k-th allocating JNI call from now fails (k >= 1; 0 = none) */
FJ_EXPORT void fj_fail_alloc(int64_t k) { g.fail_in = k; }
/* element pointers still outstanding are dropped (after a test that found some, so that the next test starts clean) */
FJ_EXPORT void fj_drop_outstanding(void) {
    while (g.ncopies) { copy_rec r = g.copies[--g.ncopies]; g.obj_bytes -= (int64_t) (r.bytes + 2 * CANARY); free(r.base); }
}
