// nq_abi.cpp -- C ABI of libnquant_hip.so (include/nquant_abi.h): handle, device workspace, and the control plane of
// the reference's convert() (scalar heuristics, GilbertCurve constructor ladder, curve tables).  All per-pixel and
// per-bin work is launched on the GPU (nq_kernels.hip); there is no CPU fallback.
//
// NQ/ = nQuant.master/src/main/java/com/android/nQuant/ in the reference.
#include "../../include/nquant_abi.h"
#include "nq_kernels.h"
#include <hip/hip_runtime.h>
#include <climits>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <algorithm>
#include <atomic>
#include <map>
#include <string>
#include <utility>
#include <vector>
#include <thread>
#include <exception>

using namespace nq;

static thread_local std::string g_create_error;

namespace {

const float kCoeffs[3][3] = {{0.299f, 0.587f, 0.114f}, {-0.14713f, -0.28886f, 0.436f}, {0.615f, -0.51499f, -0.10001f}};

// nq_get_device_bytes: bytes of device memory the library holds in this process (every DevBuf -- the workspaces, the per-call tables, the
// batch rings -- and the curve tables of get_path)
std::atomic<int64_t> g_device_bytes{0};

template <typename T> struct DevBuf {
    T* p = nullptr; size_t n = 0;
    ~DevBuf() { release(); }
    void release() {
        if (!p) return;
        (void) hipFree(p);
        g_device_bytes -= (int64_t) (n * sizeof(T));
        p = nullptr; n = 0;
    }
    hipError_t reserve(size_t count) {
        if (count <= n) return hipSuccess;
        release();
        hipError_t e = hipMalloc((void**) &p, count * sizeof(T));
        if (e == hipSuccess) { n = count; g_device_bytes += (int64_t) (n * sizeof(T)); }
        else p = nullptr;
        return e;
    }
};

// Java narrowing (control-plane use)
inline int j_d2i(double d) {
    if (d != d) return 0;
    if (d >= 2147483647.0) return 2147483647;
    if (d <= -2147483648.0) return (int) 0x80000000;
    return (int) d;
}
inline signed char j_d2b(double d) { return (signed char) (unsigned char) (j_d2i(d) & 0xFF); }
inline double sqr(double v) { return v * v; }

// GilbertCurve.initWeights (NQ/GilbertCurve.java:336-354): weights only (the zero boxes are enqueued by the kernel)
void init_weights(float* weights, int size) {
    const float weightRatio = (float) std::pow((double) (343.0f + 1.0f), (double) (1.0f / (size - 1.0f)));
    float weight = 1.0f, sumweight = 0.0f;
    for (int c = 0; c < size; ++c) {
        sumweight += (weights[size - c - 1] = weight);
        weight /= weightRatio;
    }
    weight = 0.0f;
    for (int c = 0; c < size; ++c) weight += (weights[c] /= sumweight);
    weights[0] += 1.0f - weight;
}

// GilbertCurve constructor (NQ/GilbertCurve.java:50-112); `weight` is the signed constructor parameter
GilbertConsts gilbert_consts(int K, double weight, bool hasSaliencies, bool dither) {
    GilbertConsts g;
    std::memset(&g, 0, sizeof g);
    const bool hasAlpha = weight < 0;
    g.hasAlphaW = hasAlpha; g.hasSaliencies = hasSaliencies; g.dither = dither;
    g.weightAbs = std::fabs(weight);
    g.margin = weight < .0025 ? 12 : weight < .004 ? 8 : 6;
    g.sortedByYDiff = K > 128 && weight >= .02 && (!hasAlpha || weight < .18);
    float beta = K > 4 ? (float) (.6f - .00625f * K) : 1;
    if (K > 4) {
        double boundary = .005 - .0000625 * K;
        beta = (float) (weight > boundary ? .25 : std::fmin(1.5, beta + K * weight));
        if (K > 16 && K <= 32 && weight < .003) beta += .075f;
        else if (weight < .0015 || (K > 32 && K < 256)) beta += .1f;
        if ((K >= 64 && (weight > .012 && weight < .0125)) || (weight > .025 && weight < .03)) beta += .05f;
        else if (K > 32 && K < 64 && weight < .015) beta = .55f;
        else if (K > 16 && K <= 32 && weight <= .005) beta += (float) (.05 + weight * K);
    }
    else beta *= .95f;
    if (K > 64 || (K > 4 && weight > .02)) beta *= .4f;
    if (K > 64 && weight < .02) beta = .18f;
    signed char DITHER_MAX = weight < .015 ? ((weight > .0025) ? (signed char) 25 : (signed char) 16) : (signed char) 9;
    if (weight > .99) { beta = (float) weight; DITHER_MAX = 25; }
    const double edge = hasAlpha ? 1 : std::exp(weight) - .25;
    const double deviation = weight > .002 ? -.25 : 1;
    signed char ditherMax = (hasAlpha || DITHER_MAX > 9) ? j_d2b(sqr(std::sqrt((double) DITHER_MAX) + edge * deviation))
                                                         : j_d2b(DITHER_MAX * (hasSaliencies ? 2 : 2.718281828459045));
    const int density = K > 16 ? 3200 : 1500;
    if (K / weight > 5000 && (weight > .045 || (weight > .01 && K < 64))) ditherMax = j_d2b(sqr(5 + edge));
    else if (weight < .03 && K / weight < density && K >= 16 && K < 256) ditherMax = j_d2b(sqr(5 + edge));
    g.thresold = DITHER_MAX > 9 ? -112 : -64;
    g.beta = beta; g.DITHER_MAX = DITHER_MAX; g.ditherMax = ditherMax;
    init_weights(g.weights, DITHER_MAX);
    init_weights(g.w1, 1); init_weights(g.w3, 3); init_weights(g.w7, 7); init_weights(g.w15, 15);
    return g;
}

// generalized Hilbert ("gilbert") curve, NQ/GilbertCurve.java:282-334 + run() :361-364: entries dx | dy << 16
inline int sgn(int v) { return (v > 0) - (v < 0); }
void gilbert_rec(std::vector<uint32_t>& out, int x, int y, int ax, int ay, int bx, int by) {
    const int w = std::abs(ax + ay), h = std::abs(bx + by);
    const int dax = sgn(ax), day = sgn(ay), dbx = sgn(bx), dby = sgn(by);
    if (h == 1) { for (int i = 0; i < w; ++i) { out.push_back((uint32_t) x | ((uint32_t) y << 16)); x += dax; y += day; } return; }
    if (w == 1) { for (int i = 0; i < h; ++i) { out.push_back((uint32_t) x | ((uint32_t) y << 16)); x += dbx; y += dby; } return; }
    int ax2 = ax / 2, ay2 = ay / 2, bx2 = bx / 2, by2 = by / 2;
    const int w2 = std::abs(ax2 + ay2), h2 = std::abs(bx2 + by2);
    if (2 * w > 3 * h) {
        if ((w2 % 2) != 0 && w > 2) { ax2 += dax; ay2 += day; }
        gilbert_rec(out, x, y, ax2, ay2, bx, by);
        gilbert_rec(out, x + ax2, y + ay2, ax - ax2, ay - ay2, bx, by);
        return;
    }
    if ((h2 % 2) != 0 && h > 2) { bx2 += dbx; by2 += dby; }
    gilbert_rec(out, x, y, bx2, by2, ax2, ay2);
    gilbert_rec(out, x + bx2, y + by2, ax, ay, bx - bx2, by - by2);
    gilbert_rec(out, x + (ax - dax) + (bx2 - dbx), y + (ay - day) + (by2 - dby), -bx2, -by2, -(ax - ax2), -(ay - ay2));
}
std::vector<uint32_t> gilbert_path(int w, int h) {
    std::vector<uint32_t> out;
    out.reserve((size_t) w * h);
    if (w <= 0 || h <= 0) return out;
    if (w >= h) gilbert_rec(out, 0, 0, w, 0, 0, h);
    else gilbert_rec(out, 0, 0, 0, h, w, 0);
    return out;
}

} // namespace

// per-pixel scratch that lives only inside one stage of one image: the handles of a batch share the first handle's
struct Scratch {
    DevBuf<unsigned short> keys_a, keys_b;
    DevBuf<int> vals_a, vals_b;
    DevBuf<unsigned char> sort_tmp;
    DevBuf<unsigned> seg;             // start[65536], end[65536], counters (+ padding), list of the occupied bins[65536], of the fat bins[1024]
    DevBuf<double> hist;              // [65536][5]
    DevBuf<int> init_cand;            // initial LAB pass: candidate lists {bin, bound}[65536][128], then the counts [65536]
    DevBuf<unsigned char> cell_lists; // closest lists, nearest lists (65536 x 32 each), then their counts (65536 each)
    DevBuf<float> saliency;           // saliency map of the image being dithered
    DevBuf<unsigned> lookup_todo;     // LOOKUP_ONLY: {count, pixel indices the float32 pass leaves to the exact pass}
    DevBuf<unsigned> dk_a, dk_b, di_a, di_b;   // distinct-colour sort scratch
    DevBuf<unsigned char> dtmp;
    DevBuf<unsigned long long> dheads;         // {colour, first index} pairs (uint2)
    DevBuf<float> cell_box;           // Lab bounding box of every 5-6-5 cell (palette independent, built once)
    bool cell_box_ready = false;
    bool lab_table = false;           // the palette's Lab stands behind the packed records of cell_lists (written with the lists now in it)
};

inline size_t path_bytes(int w, int hgt) { const size_t n = (size_t) w * hgt; return (n ? n : 1) * sizeof(uint32_t); }

struct nq_handle {
    int kind = 0, device = 0;
    hipStream_t stream = nullptr;
    std::string err;
    nq_params params;
    int tile_w = 0, tile_h = 0;       // 0 = automatic (pick_tile)
    float stage_ms[NQ_N_STAGES] = {0};
    Scratch own;
    Scratch* sc = &own;
    // device workspace
    DevBuf<int> d_palette, d_colors, d_tuple;
    DevBuf<uint32_t> d_in, d_out_argb;
    DevBuf<unsigned short> d_out_index;
    DevBuf<short> d_bincache, d_short;
    DevBuf<int> d_seqlog;             // REFERENCE_SEQUENTIAL + LAB + dither=false: colours getLab() saw during the pass (+ 1 counter)
    DevBuf<unsigned char> d_seqseen;  // ... and the palette entries it touched
    DevBuf<long long> d_scalars;      // [0] rng state, [1..3] scan3, [4..19] merge stats, [20..21] distinct-colour result, [24..39] team counters, [40] palette status
    DevBuf<int> live3;                // merge loop: two live lists + position index
    int use_lists = 1;
    int n_cus = 256;                  // compute units of the device (hipDeviceAttributeMultiprocessorCount): sizes merge workgroups / teams
    int merge_wall_s = 0;             // NQ_OPT_MERGE_WALL_SECONDS: watchdog of a merge loop, seconds of residency (0 = automatic)
    hipStream_t palette_stream = nullptr;   // stream the upload behind dev_palette was enqueued on ...
    bool palette_synced = false;            // ... unless the host has waited for d_palette's content since (then any stream may read it)
    DevBuf<float> d_user_sal;
    int band_y0 = 0, band_image_h = 0; // nq_set_band: this handle dithers a row band of a larger image (0, 0 = a whole image)
    int use_fast_dither = 1;          // NQ_OPT_FAST_DITHER: the specialised dither kernel where the configuration allows it
    // NQ_OPT_DITHER_CHAIN: 0 automatic, 1 the error chain in every step, 2 the fused light walk, 3 the split form, 4 the split form with the pixel-form light pass (a new handle starts from
    // the environment's NQ_DITHER_CHAIN = 0..4: whole-suite runs under one form, tests/fuzz_parity.py)
    int dither_chain = [] { const char* e = std::getenv("NQ_DITHER_CHAIN"); const int v = e ? std::atoi(e) : 0; return v >= 0 && v <= 4 ? v : 0; }();
    // batch entry points, finish phase: the image's chain pass and hand-back pass go onto chain_stream (the split form is "automatic"
    // there); chain_gate: behind the light kernel on the main stream, chain_done: behind the image's last kernel on chain_stream
    hipStream_t chain_stream = nullptr;
    hipEvent_t chain_gate = nullptr, chain_done = nullptr;
    bool chain_on_side = false;       // the last dither pass ended on chain_stream (chain_done was recorded there)
    // nq_convert_batch_device, finish phase with a prep stream: the image's lists, Lab table, saliency map and counter clear go onto
    // prep_stream (behind set_free, the end of the dither work of the image that had the scratch set before; null: the set is free);
    // prep_done: behind them on prep_stream, the handle's stream waits for it in front of the light pass
    hipStream_t prep_stream = nullptr;
    hipEvent_t prep_done = nullptr, set_free = nullptr;
    bool dither_events_fresh = false; // the last call on the handle was a stand-alone dither (events 5..7 are newer than stage_ms)
    int last_dither_fast = 0;         // diagnostics: 1 if the last dither pass ran gilbert_fast_kernel
    bool split_uncounted = false;     // ... it took the split form and its need count is not yet in nq_get_dither_split_stats
    int last_dither_failed_tiles = 0; // ... and how many tiles it handed back to the generic kernel (read lazily)
    DevBuf<int> d_failed;             // {need count, count, tile indices..., need list...}: failed_list(), launch_gilbert_fast (nq_kernels.h)
    DevBuf<float> scan_f;             // merge loop: position-indexed scan arrays (two generations)
    DevBuf<int> scan_i;
    DevBuf<float> scan_box;           // merge loop: bounding boxes of the 64-position blocks (1024 x 8 floats)
    DevBuf<nq::MergeJob> d_jobs;      // merge jobs of the current call (1, or the whole batch on the first handle)
    DevBuf<int> ring_argb[3];         // nq_convert_batch: device output ring (results leave for the host while the next image runs)
    DevBuf<unsigned short> ring_index[3];
    hipStream_t copy_stream = nullptr;
    hipStream_t lane_stream = nullptr;  // second lane of the batch entry points
    hipStream_t more_lanes[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};   // ... third to eighth
    long long merge_stats[16] = {0};
    std::vector<uint32_t> dev_palette;  // what d_palette holds, as far as the host knows (empty: unknown): an upload of the same entries is skipped
    uint32_t* fetched_palette = nullptr; int fetched_len = 0;      // palette_fetch -> palette_check
    long long merge_readback[37] = {0}; // d_scalars[4..41) as the merge kernel left it: one copy per image ([36] = status word)
    // nq_convert_batch_device (first handle of the batch): the palettes and the 37 read-back words of all merge jobs of the call come
    // back as ONE block -- gathered on the device (launch_merge_readback), then one copy into page-locked memory
    DevBuf<long long> d_readback;
    long long* h_readback = nullptr; size_t h_readback_words = 0;
    // page-locked landing slots of this handle's two scalar read-backs per image: [0..2] the pre-scan's scan3, [4] the bin count
    long long* pin = nullptr;
    int merge_variant[2] = {0, 0};     // nq_get_merge_variant: {workgroup-size code, helpers} launch_merge picked for this handle's last merge job
    long long team_stats[16] = {0};    // merge teams: {work records published, results used, timed-out waits, ticks waited, helpers, still speculating}
    DevBuf<unsigned long long> team;  // 256 u64 of hand-off words of this handle's merge team
    bool light_events = false;        // batch entry points: this image records only the stage events 0, 5, 6 (see rec)
    hipEvent_t bev[4] = {nullptr};    // batch entry points: phase boundaries on the launch stream (first handle of the batch)
    hipEvent_t lane_gate = nullptr;   // nq_convert_batch_device: what the first handle's stream holds at entry; the other lanes wait for it
    float batch_phase_ms[4] = {0};
    bool ext_distinct_valid = false, ext_distinct_many = false;  // nq_set_distinct: image-wide distinct colours (first-occurrence order) of the split pipeline
    std::vector<int32_t> ext_distinct;
    DevBuf<int> d_ints;               // [0] maxbins, [1] status, [8..71] occupied slots per 1024-slot slice
    DevBuf<int> heap;
    // nq_pnnquan_frames_device / nq_convert_frames_device: the frame table and the (frame, chunk) work list of the current call (host copies
    // stay alive for the asynchronous uploads), and while such a call runs: frames_active (the pixel source of distinct_colors /
    // palette_prepare is the frame table), reuse_lists (dither_device builds the candidate lists once and keeps them for the next
    // frames), rec_skip (stage boundaries a frame's dither pass does not record)
    std::vector<nq::FrameDesc> h_frames;
    std::vector<nq::FrameChunk> h_items;
    DevBuf<nq::FrameDesc> d_frames;
    DevBuf<nq::FrameChunk> d_items;
    int64_t frames_total = 0;
    bool frames_active = false, reuse_lists = false, lists_built = false;
    nq::ListsView saved_lv;
    unsigned rec_skip = 0;
    // nq_encode_gif_device: frame table, LZW scratch (bit strings; bit lengths, then bit offsets of the segments), read-back
    // ({frame bit lengths}[n], bad-index flag), header blob and the file being assembled; nq_encode_gif: the uploaded index maps
    std::vector<nq::GifFrame> h_gif;
    DevBuf<nq::GifFrame> d_gif;
    DevBuf<unsigned> gif_words;
    DevBuf<unsigned long long> gif_bits, gif_res;
    DevBuf<unsigned char> gif_blob, gif_file;
    DevBuf<unsigned short> gif_in;
    std::vector<uint8_t> h_gif_blob;
    // lossy mode: the file's colour table as the chains read it (256 entries 0x00RRGGBB)
    std::vector<unsigned> h_gif_rgb;
    DevBuf<unsigned> gif_rgb;
    // nq_encode_gif_delta_device: the frames' pointers, the changed pixels' boxes ({min x, min y, max x, max y}[n - 1], bad-index flag),
    // the body table and the cropped bodies the LZW chains read
    std::vector<int> h_gif_box;
    std::vector<nq::GifDelta> h_gif_delta;
    DevBuf<const unsigned short*> gif_ptrs;
    DevBuf<int> gif_box;
    DevBuf<nq::GifDelta> d_gif_delta;
    DevBuf<unsigned short> gif_body;
    // nq_encode_gif_local*: one record per frame (K, Kt, m, T and the written colour table)
    std::vector<nq::GifLocal> h_gif_local;
    DevBuf<nq::GifLocal> d_gif_local;
    // nq_encode_png_device: image table, token scratch of the resident chains, IDAT CRC registers; bit strings, bit lengths / offsets,
    // read-back, header blob, files and uploaded index maps live in the GIF buffers above (one encoder runs at a time on a handle)
    std::vector<nq::PngImage> h_png;
    DevBuf<nq::PngImage> d_png;
    DevBuf<unsigned> png_tokens, png_crc;
    DevBuf<unsigned long long> png_adler;
    // nq_hold_frames_device: the tables of frame pointers (source, index, output: n each; the host copy stays alive for the asynchronous
    // upload) and the per-frame held counters; nq_hold_frames stages its frames in d_in / d_out_index / d_out_argb
    std::vector<void*> h_hold_ptrs;
    DevBuf<void*> hold_ptrs;
    DevBuf<unsigned long long> hold_held;
    // nq_frame_signatures_device: the table of frame pointers (the host copy stays alive for the asynchronous upload) and the n * 1024
    // counters; nq_frame_signatures stages its frames in d_in; nq_detect_shots*: the signatures on the host
    std::vector<const uint32_t*> h_sig_ptrs;
    DevBuf<const uint32_t*> sig_ptrs;
    DevBuf<uint32_t> d_sig;
    std::vector<uint32_t> h_sig;
    // nq_refine_palette_device: the frame table and the call's state words (REFINE_* of nq_kernels.h; the host copies stay alive for the
    // asynchronous copies); nq_refine_palette stages its frames in d_in
    std::vector<nq::RefineFrame> h_refine_frames;
    DevBuf<nq::RefineFrame> d_refine_frames;
    std::vector<unsigned long long> h_refine;
    DevBuf<unsigned long long> d_refine;
    // nq_resample_frames_device: the tables of frame pointers (source, output: n each; the host copy stays alive for the asynchronous
    // upload); nq_resample_frames stages its frames in d_in and their reductions in d_out_argb
    std::vector<void*> h_resample_ptrs;
    DevBuf<void*> resample_ptrs;
    // nq_frames_from_yuv_device / nq_resample_frames_yuv_device: the table of plane and output pointers (y, u, v, output: n each; the host
    // copy stays alive for the asynchronous upload); the host forms stage the planes' byte spans in yuv_in and the outputs in d_out_argb
    std::vector<const void*> h_yuv_ptrs;
    DevBuf<const void*> yuv_ptrs;
    DevBuf<unsigned char> yuv_in;
    // nq_orient_frames_device: the tables of frame pointers (source, output: n each; the host copy stays alive for the asynchronous
    // upload).  The reducing *_oriented calls reduce into orient_tmp (the frames 16-byte aligned) and orient from there.
    std::vector<void*> h_orient_ptrs;
    DevBuf<void*> orient_ptrs;
    DevBuf<uint32_t> orient_tmp;
    // nq_dither_ordered_device: the frame table, the palette (256 words) and the 2 n statistics (the host copies stay alive for the
    // asynchronous uploads); nq_dither_ordered stages its frames in d_in / d_out_index / d_out_argb
    std::vector<nq::OrderedFrame> h_ordered_frames;
    DevBuf<nq::OrderedFrame> d_ordered_frames;
    std::vector<unsigned> h_ordered_pal;
    DevBuf<unsigned> d_ordered_pal;
    DevBuf<unsigned long long> d_ordered_stats;
    DevBuf<float> binf;               // f[4], cnt, err : 6 x 65536
    DevBuf<double> bind;              // d[4] : 4 x 65536
    DevBuf<int> bini;                 // nn, tm, mtm : 3 x 65536
    std::map<std::pair<int, int>, uint32_t*> paths;   // curve tables on the device, by shape: the shapes get_path keeps (both sides <= NQ_PATH_KEEP_SIDE)
    // ... and the larger shapes (a whole image in REFERENCE_SEQUENTIAL, a tile set beyond NQ_PATH_KEEP_SIDE): one grow-only table per shape
    // slot of a dither pass, holding the most recent shape asked for there
    DevBuf<uint32_t> big_path[4];
    int big_w[4] = {0, 0, 0, 0}, big_h[4] = {0, 0, 0, 0};
    hipEvent_t ev[NQ_N_STAGES + 1] = {nullptr};
    bool tables_ready = false;
    ~nq_handle() {
        for (auto& kv : paths) { (void) hipFree(kv.second); g_device_bytes -= (int64_t) path_bytes(kv.first.first, kv.first.second); }
        for (auto& e : ev) if (e) (void) hipEventDestroy(e);
        for (auto& e : bev) if (e) (void) hipEventDestroy(e);
        if (lane_gate) (void) hipEventDestroy(lane_gate);
        if (chain_gate) (void) hipEventDestroy(chain_gate);
        if (chain_done) (void) hipEventDestroy(chain_done);
        if (prep_done) (void) hipEventDestroy(prep_done);
        if (copy_stream) (void) hipStreamDestroy(copy_stream);
        if (lane_stream) (void) hipStreamDestroy(lane_stream);
        for (auto& ls : more_lanes) if (ls) (void) hipStreamDestroy(ls);
        if (h_readback) (void) hipHostFree(h_readback);
        if (pin) (void) hipHostFree(pin);
    }
};

// what the launches since the last check left behind: a failed hipFuncSetAttribute of a launch_* function (kept per thread by
// nq_kernels.hip) or the runtime's own last error
static inline hipError_t launch_status() {
    const hipError_t a = nq::take_launch_error(), b = hipGetLastError();
    return a != hipSuccess ? a : b;
}

// The failing macros write the text into a std::string the caller names and return the code.  NQ_FAIL / NQ_HIP name a handle's err,
// NQ_CMP_FAIL / NQ_CMP_HIP the thread's handle-free string (the stateless calls); code that serves both takes the string (*_TO).
#define NQ_FAIL_TO(err, code, ...) do { char _b[512]; std::snprintf(_b, sizeof _b, __VA_ARGS__); (err) = _b; return (code); } while (0)
#define NQ_HIP_TEXT(err, call, text) do { hipError_t _e = (call); if (_e != hipSuccess) { \
    NQ_FAIL_TO(err, NQ_ERR_HIP, "%s failed: %s (%s:%d)", text, hipGetErrorString(_e), __FILE__, __LINE__); } } while (0)
#define NQ_HIP_TO(err, call) NQ_HIP_TEXT(err, call, #call)
#define NQ_FAIL(h, code, ...) NQ_FAIL_TO((h)->err, code, __VA_ARGS__)
#define NQ_HIP(h, call) NQ_HIP_TEXT((h)->err, call, #call)
#define NQ_CMP_FAIL(code, ...) NQ_FAIL_TO(g_create_error, code, __VA_ARGS__)
#define NQ_CMP_HIP(call) NQ_HIP_TEXT(g_create_error, call, #call)

namespace {

// the first step of every entry point on a handle (a null handle is NQ_ERR_INVALID)
int use_device(nq_handle* h) {
    if (!h) return NQ_ERR_INVALID;
    NQ_HIP(h, hipSetDevice(h->device));
    if (!h->tables_ready) {
        double gamma[256];
        for (int ch = 0; ch < 256; ++ch) {         // CIELABConvertor.gammaToLinear (NQ/CIELABConvertor.java:71-75)
            const double c = ch / 255.0;
            gamma[ch] = c < 0.04045 ? c / 12.92 : std::pow((c + 0.055) / 1.055, 2.4);
        }
        upload_tables(gamma, std::exp(1.5), std::exp(1.75), h->stream);
        upload_tables_fast(gamma, std::exp(1.5), std::exp(1.75), h->stream);
        NQ_HIP(h, launch_status());
        int cus = 0;
        NQ_HIP(h, hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, h->device));
        if (cus > 0) h->n_cus = cus;
        NQ_HIP(h, h->d_scalars.reserve(64));
        NQ_HIP(h, h->d_ints.reserve(8 + 64));
        NQ_HIP(h, h->d_bincache.reserve(65536));
        if (!h->pin) NQ_HIP(h, hipHostMalloc((void**) &h->pin, 8 * sizeof(long long), hipHostMallocDefault));
        for (auto& e : h->ev) NQ_HIP(h, hipEventCreate(&e));
        for (auto& e : h->bev) NQ_HIP(h, hipEventCreate(&e));
        NQ_HIP(h, hipEventCreateWithFlags(&h->lane_gate, hipEventDisableTiming));
        h->tables_ready = true;
    }
    return NQ_OK;
}

DevParams dev_params(const nq_handle* h, int K) {
    const nq_params& p = h->params;
    DevParams d;
    d.kind = h->kind; d.K = K; d.hasSemi = p.hasSemiTransparency; d.hasAlpha = p.transparentPixelIndex > -1;
    d.transparentColor = p.transparentColor; d.isNano = p.isNano;
    d.binKeyed = h->kind == NQ_KIND_LAB ? (p.isNano != 0) : !(p.weight > .015);
    d.nMaxColors = p.nMaxColors; d.rewriteA0 = p.nMaxColors <= 2 && p.nMaxColors > 0;
    d.pad = 0;
    d.PR = p.PR; d.PG = p.PG; d.PB = p.PB; d.PA = p.PA; d.ratio = p.ratio; d.weight = p.weight;
    return d;
}

// the packed list records of the specialised kernels (nq_dither_fast.hip) live behind the lists and their counts
// the palette of a per-pixel pass on the device; skipped when d_palette already holds exactly these entries (convert(): the merge
// workgroup wrote them there and the host read them back -- one small copy per image less)
int upload_palette(nq_handle* h, const uint32_t* palette, int K) {
    const size_t cap = h->d_palette.n;
    NQ_HIP(h, h->d_palette.reserve((size_t) std::max(K, 2)));
    if (h->d_palette.n != cap) h->dev_palette.clear();          // (a new allocation)
    // (an earlier upload is ordered only against work on the stream it was enqueued on: after nq_set_stream the copy is repeated)
    const bool ordered = h->palette_synced || h->palette_stream == h->stream;
    if (ordered && (int) h->dev_palette.size() == K && std::memcmp(h->dev_palette.data(), palette, (size_t) K * sizeof(uint32_t)) == 0) return NQ_OK;
    h->dev_palette.clear();
    NQ_HIP(h, hipMemcpyAsync(h->d_palette.p, palette, K * sizeof(int), hipMemcpyHostToDevice, h->stream));
    h->dev_palette.assign(palette, palette + K);
    h->palette_stream = h->stream; h->palette_synced = false;
    return NQ_OK;
}
// nq_get_dither_split_stats: split-form dither passes of this process / of those, with the chain pass on a side stream / tiles their light
// kernels listed, counted when nq_get_dither_path reads a pass's counts back (once per pass)
static std::atomic<long long> g_split_passes{0}, g_split_side{0}, g_split_listed{0};
// the hand-back list of launch_gilbert_fast inside d_failed (one word in front of it: the need count of the split form, nq_kernels.h)
int* failed_list(nq_handle* h) { return h->d_failed.p + 1; }
size_t failed_words(const nq::TileGeom& T) { return 2 * ((size_t) T.tiles_x * T.tiles_y + 1); }
void* packed_lists(nq_handle* h) { return h->sc->cell_lists.p + 2 * (size_t) 65536 * 32 + 2 * 65536; }
// the Lab table of the palette whose lists the scratch set holds (nq_kernels.h launch_build_lists), or null where none was written
const void* lab_table(nq_handle* h) { return h->sc->lab_table ? (const unsigned char*) packed_lists(h) + nq::NQ_PACKED_BYTES : nullptr; }

// candidate lists per colour cell for this palette (nq_lists.inc); empty view = full scans
// sal_pixels != null: the saliency map of these n pixels is wanted in h->sc->saliency as well; *sal_done says whether it was built here
// (beside the LAB list builders, one launch) or is left to the caller
// d_failed != null: the hand-back count of the dither kernel this call is about to launch; *failed_cleared says whether the builders'
// launch zeroed it (LAB with nearest lists), else launch_gilbert_fast does
int prepare_lists(nq_handle* h, const DevParams& P, nq::ListsView* out, const int* sal_pixels = nullptr, int64_t sal_n = 0, int sal_subst = 0,
                  bool* sal_done = nullptr, int* d_failed = nullptr, bool* failed_cleared = nullptr) {
    if (sal_done) *sal_done = false;
    if (failed_cleared) *failed_cleared = false;
    out->closest = out->closestCount = out->nearest = out->nearestCount = nullptr;
    if (!h->use_lists || P.K > 256 || P.K < 8) return NQ_OK;
    const size_t LB = (size_t) 65536 * 32;
    // + the packed records of the specialised dither kernel (2 * LB = NQ_PACKED_BYTES) + the palette's Lab behind them
    NQ_HIP(h, h->sc->cell_lists.reserve(2 * LB + 2 * 65536 + nq::NQ_PACKED_BYTES + nq::NQ_LAB_TABLE_BYTES));
    h->sc->lab_table = false;
    unsigned char* base = h->sc->cell_lists.p;
    double wA, wR, wG, wB;
    if (h->kind == NQ_KIND_LAB) {
        // err of NQ/PnnLABQuantizer.java:421-445: PR(1-ratio) dr^2 + ... + ratio * sum_i (coeffs[i][c] d)^2
        double s[3] = {0, 0, 0};
        for (int i = 0; i < 3; ++i) for (int c = 0; c < 3; ++c) s[c] += (double) kCoeffs[i][c] * (double) kCoeffs[i][c];
        wR = P.PR * (1 - P.ratio) + P.ratio * s[0]; wG = P.PG * (1 - P.ratio) + P.ratio * s[1]; wB = P.PB * (1 - P.ratio) + P.ratio * s[2];
        wA = P.hasSemi ? P.PA : 0.0;
    } else {
        // NQ/PnnQuantizer.java:325-345
        double pr = P.PR, pg = P.PG, pb = P.PB, pa = P.PA;
        if (P.K < 3) pr = pg = pb = pa = 1;
        wR = pr; wG = pg; wB = pb; wA = P.hasSemi ? pa : 0.0;
    }
    // nearestColorIndex lists: LAB for the K > 32 metric; RGB for opaque images (no transparent colour: the scan starts at 0)
    const bool nearest = h->kind == NQ_KIND_LAB ? (P.K > 32 && !P.hasSemi) : (!P.hasSemi && !P.hasAlpha);
    if (nearest && h->kind == NQ_KIND_LAB && !h->sc->cell_box_ready) {
        NQ_HIP(h, h->sc->cell_box.reserve((size_t) 65536 * 6));
        launch_cell_lab_box(h->sc->cell_box.p, h->stream);
        h->sc->cell_box_ready = true;
    }
    if (sal_pixels) NQ_HIP(h, h->sc->saliency.reserve((size_t) sal_n));
    // (a negative ratio makes the closest error non-monotone in its terms: the list argument does not hold, full scans)
    if (!(h->kind == NQ_KIND_LAB && P.ratio < 0)) { out->closest = base; out->closestCount = base + 2 * LB; }
    if (nearest) { out->nearest = base + LB; out->nearestCount = base + 2 * LB + 65536; }
    // the packed records of the specialised kernels: written by the LAB builders themselves (NQ_PACK_IN_BUILDERS=0: by the separate
    // launch, as for the RGB kind -- the two must agree byte for byte, tests/test_gpu_batch_plumbing.py)
    const bool pack = h->use_fast_dither && fast_pack_wanted(P, *out);
    bool pack_in_builders = true;
    if (const char* e = std::getenv("NQ_PACK_IN_BUILDERS")) pack_in_builders = std::atoi(e) != 0;
    bool folded = false;
    const bool sal_built = launch_build_lists(P, h->d_palette.p, wA, wR, wG, wB, nearest, h->sc->cell_box.p, base, base + 2 * LB, base + LB,
                                              base + 2 * LB + 65536, h->stream, sal_pixels, sal_n, sal_pixels ? h->sc->saliency.p : nullptr, sal_subst,
                                              pack && pack_in_builders ? packed_lists(h) : nullptr, d_failed, &folded);
    if (sal_done) *sal_done = sal_built;
    if (failed_cleared) *failed_cleared = folded && d_failed;
    h->sc->lab_table = pack && pack_in_builders && folded;
    if (pack && !(folded && pack_in_builders)) launch_pack_lists(*out, packed_lists(h), h->stream);
    return NQ_OK;
}

// prepare_lists of one dither pass; in a frames call (reuse_lists) the lists of the first frame serve every later frame -- same palette,
// same params, so the same lists -- and a saliency map wanted there is left to the caller (launch_saliency)
int lists_for_call(nq_handle* h, const DevParams& P, nq::ListsView* out, const int* sal_pixels = nullptr, int64_t sal_n = 0, int sal_subst = 0,
                   bool* sal_done = nullptr, int* d_failed = nullptr, bool* failed_cleared = nullptr) {
    if (h->reuse_lists && h->lists_built) {
        if (sal_done) *sal_done = false;
        if (failed_cleared) *failed_cleared = false;
        *out = h->saved_lv;
        return NQ_OK;
    }
    const int rc = prepare_lists(h, P, out, sal_pixels, sal_n, sal_subst, sal_done, d_failed, failed_cleared);
    if (!rc && h->reuse_lists) { h->saved_lv = *out; h->lists_built = true; }
    return rc;
}

// The curve table of shape w x hgt for shape slot `slot` (0..3: full tile, right column, bottom row, corner) of a dither pass.
// What a handle keeps: shapes with both sides <= NQ_PATH_KEEP_SIDE stay for the handle's life (the tiles of PARALLEL_TILED and their
// remainders: at most NQ_PATH_KEEP_SIDE^2 shapes of at most 4 * NQ_PATH_KEEP_SIDE^2 bytes, 4 MB); of the larger shapes -- the whole
// image in REFERENCE_SEQUENTIAL, a tile set beyond that side -- only the most recent one per slot, in a grow-only buffer, and slots
// of one pass that want the same shape share it.  So a handle holds at most four tables of the largest shapes it has seen, not one
// per image size.  (Rewriting a slot is ordered on the handle's stream behind the pass that read it; a regrowing hipFree waits.  In a
// batch call the passes of every handle run on the FIRST handle's stream: like the handle's other buffers, a slot is safe to rewrite
// once the batch call's work has completed, which include/nquant_abi.h states as the precondition of the next call on any of its handles.)
constexpr int NQ_PATH_KEEP_SIDE = 32;

hipError_t upload_path(nq_handle* h, uint32_t* d, const std::vector<uint32_t>& p) {
    hipError_t e = hipMemcpyAsync(d, p.data(), p.size() * sizeof(uint32_t), hipMemcpyHostToDevice, h->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);   // p goes out of scope
    return e;
}

int get_path(nq_handle* h, int w, int hgt, int slot, const uint32_t** out) {
    if (w > NQ_PATH_KEEP_SIDE || hgt > NQ_PATH_KEEP_SIDE) {
        for (int t = 0; t <= slot; ++t)       // (earlier slots are settled for this pass; later ones may still be rewritten by it)
            if (h->big_w[t] == w && h->big_h[t] == hgt) { *out = h->big_path[t].p; return NQ_OK; }
        std::vector<uint32_t> p = gilbert_path(w, hgt);
        h->big_w[slot] = h->big_h[slot] = 0;
        NQ_HIP(h, h->big_path[slot].reserve(p.size() ? p.size() : 1));
        hipError_t e = upload_path(h, h->big_path[slot].p, p);
        if (e != hipSuccess) NQ_FAIL(h, NQ_ERR_HIP, "curve table upload failed: %s", hipGetErrorString(e));
        h->big_w[slot] = w; h->big_h[slot] = hgt;
        *out = h->big_path[slot].p;
        return NQ_OK;
    }
    auto key = std::make_pair(w, hgt);
    auto it = h->paths.find(key);
    if (it == h->paths.end()) {
        std::vector<uint32_t> p = gilbert_path(w, hgt);
        uint32_t* d = nullptr;
        NQ_HIP(h, hipMalloc((void**) &d, path_bytes(w, hgt)));
        hipError_t e = upload_path(h, d, p);
        if (e != hipSuccess) { (void) hipFree(d); NQ_FAIL(h, NQ_ERR_HIP, "curve table upload failed: %s", hipGetErrorString(e)); }
        g_device_bytes += (int64_t) path_bytes(w, hgt);
        it = h->paths.emplace(key, d).first;
    }
    *out = it->second;
    return NQ_OK;
}

nq::Bins bins_of(nq_handle* h) {
    nq::Bins B;
    for (int c = 0; c < 4; ++c) { B.f[c] = h->binf.p + (size_t) c * 65536; B.d[c] = h->bind.p + (size_t) c * 65536; }
    B.cnt = h->binf.p + (size_t) 4 * 65536; B.err = h->binf.p + (size_t) 5 * 65536;
    B.nn = h->bini.p; B.tm = h->bini.p + 65536; B.mtm = h->bini.p + 2 * 65536;
    return B;
}

int reserve_palette_ws(nq_handle* h, int64_t n) {
    NQ_HIP(h, h->sc->vals_a.reserve((size_t) n)); NQ_HIP(h, h->sc->vals_b.reserve((size_t) n));
    NQ_HIP(h, h->sc->sort_tmp.reserve(sort_temp_bytes(n) + 256));
    NQ_HIP(h, h->sc->seg.reserve(3 * 65536 + 64 + 1024));     // start[65536], end[65536], counters, occupied-bin list[65536], fat-bin list[1024]
    NQ_HIP(h, h->sc->hist.reserve((size_t) 65536 * 5));
    if (h->kind == 1) NQ_HIP(h, h->sc->init_cand.reserve((size_t) 65536 * 128 * 2 + 65536));
    NQ_HIP(h, h->binf.reserve((size_t) 6 * 65536)); NQ_HIP(h, h->bind.reserve((size_t) 4 * 65536));
    NQ_HIP(h, h->bini.reserve((size_t) 3 * 65536)); NQ_HIP(h, h->heap.reserve(2 * (65536 + 2)));
    NQ_HIP(h, h->live3.reserve((size_t) 3 * 65536));
    NQ_HIP(h, h->scan_f.reserve((size_t) 2 * 10 * 65536 + 256)); NQ_HIP(h, h->scan_i.reserve((size_t) 2 * 65536));
    NQ_HIP(h, h->scan_box.reserve((size_t) 1024 * 8));
    NQ_HIP(h, h->team.reserve(256));
    return NQ_OK;
}

// number of distinct colours of the image as the histogram sees it (= pixelMap.size() after the histogram); when it is
// <= cap the colours are returned in first-occurrence order (the insertion order of the reference's HashMap).
// d_argb == nullptr: the pixels are the frame sequence of the running frames call (global first-occurrence indices)
int distinct_colors(nq_handle* h, const uint32_t* d_argb, int64_t n, int64_t cap, int64_t* out_count, std::vector<int32_t>* out_colors) {
    if (!d_argb && !h->frames_active) NQ_FAIL(h, NQ_ERR_INVALID, "distinct colours without pixels (internal error)");
    const bool want = out_colors != nullptr && cap > 0;
    NQ_HIP(h, h->sc->dk_a.reserve((size_t) n)); NQ_HIP(h, h->sc->dk_b.reserve((size_t) n));
    if (want) { NQ_HIP(h, h->sc->di_a.reserve((size_t) n)); NQ_HIP(h, h->sc->di_b.reserve((size_t) n)); NQ_HIP(h, h->sc->dheads.reserve((size_t) cap + 1)); }
    const size_t tb = sort32_temp_bytes(n, want) + 256;
    NQ_HIP(h, h->sc->dtmp.reserve(tb));
    unsigned long long* d_out = reinterpret_cast<unsigned long long*>(h->d_scalars.p + 20);
    if (!d_argb)
        launch_frames_pass(FRAMES_SUBST, h->d_frames.p, (int) h->h_frames.size(), h->d_items.p, (int) h->h_items.size(), nullptr, h->sc->dk_a.p,
                           want ? h->sc->di_a.p : nullptr, h->params.transparentColor, 0, h->stream);
    launch_distinct((const int*) d_argb, n, h->params.transparentColor, h->sc->dk_a.p, h->sc->dk_b.p, want ? h->sc->di_a.p : nullptr,
                    want ? h->sc->di_b.p : nullptr, h->sc->dtmp.p, tb, d_out, want ? (void*) h->sc->dheads.p : nullptr, (unsigned) cap, h->stream);
    unsigned long long res[2] = {0, 0};
    NQ_HIP(h, hipMemcpyAsync(res, d_out, sizeof res, hipMemcpyDeviceToHost, h->stream));
    NQ_HIP(h, hipStreamSynchronize(h->stream));
    NQ_HIP(h, launch_status());
    *out_count = (int64_t) res[0];
    if (want && (int64_t) res[0] <= cap) {
        std::vector<unsigned long long> heads(res[0]);
        NQ_HIP(h, hipMemcpy(heads.data(), h->sc->dheads.p, res[0] * sizeof(unsigned long long), hipMemcpyDeviceToHost));
        // uint2 {colour, index} little endian: low word = colour, high word = first index
        std::vector<std::pair<uint32_t, uint32_t>> byIndex;
        for (unsigned long long v : heads) byIndex.emplace_back((uint32_t) (v >> 32), (uint32_t) (v & 0xFFFFFFFFu));
        std::sort(byIndex.begin(), byIndex.end());
        out_colors->clear();
        for (auto& pr : byIndex) out_colors->push_back((int32_t) pr.second);
    }
    return NQ_OK;
}

// keySet() order of java.util.HashMap<Integer, ?> for keys inserted in the given order (OpenJDK 8+; treeified buckets ignored):
// capacity 16 doubling while size > 0.75 capacity; bucket = (h ^ h >>> 16) & (capacity - 1), h = key; insertion order inside
std::vector<int32_t> java_hashmap_keyset(const std::vector<int32_t>& inserted) {
    size_t cap = 16;
    while ((double) inserted.size() > 0.75 * (double) cap) cap <<= 1;
    std::vector<std::vector<int32_t>> buckets(cap);
    for (int32_t k : inserted) { uint32_t hh = (uint32_t) k; hh ^= hh >> 16; buckets[hh & (cap - 1)].push_back(k); }
    std::vector<int32_t> out;
    for (auto& b : buckets) for (int32_t k : b) out.push_back(k);
    return out;
}

// the scalar part of convert() after the pre-scan (NQ/PnnQuantizer.java:431-436)
void apply_scan(nq_handle* h, int nMaxColors, int64_t transparent_index, uint32_t transparent_color, int64_t semi_count) {
    nq_params& p = h->params;
    p.kind = h->kind; p.nMaxColors = nMaxColors;
    p.transparentPixelIndex = transparent_index >= 0 ? (int32_t) transparent_index : -1;
    p.transparentColor = (int32_t) 0x00FFFFFFu;                       // Color.argb(0,255,255,255) (:22)
    if (transparent_index >= 0 && nMaxColors > 2) p.transparentColor = (int32_t) transparent_color;   // :421-424
    p.hasSemiTransparency = semi_count > 0;
    if (nMaxColors <= 32) p.PR = p.PG = p.PB = p.PA = 1;
    else { p.PR = kCoeffs[0][0]; p.PG = kCoeffs[0][1]; p.PB = kCoeffs[0][2]; p.PA = .3333; }
    p.ratio = .5; p.weight = 1; p.isNano = 0; p.texicab = 0; p.quan_rt = 1; p.maxbins = 0; p.paletteLength = 0;
    p.distinctColors = 0;
}

// stage boundary i on the handle's stream.  An event record costs the GPU ~3 us of queue time, eight of them per image of a big batch
// 0.9 % of the batch: the batch entry points keep all eight for their first images only, the rest record the start and the two ends of
// the per-pixel pass (what bench.py's roofline needs)
void rec(nq_handle* h, int i) {
    if (h->light_events && ((i >= 1 && i <= 4) || i == 7)) return;
    if ((h->rec_skip >> i) & 1u) return;
    (void) hipEventRecord(h->ev[i], h->stream);
}

// what palette_prepare leaves for the merge launch and palette_finish; merge == false: the palette is already final
struct PaletteJob {
    bool merge = false;
    nq_handle* h = nullptr;           // the handle the job was prepared on (merge_launch records the variant there)
    nq::MergeJob mj;
    int plen = 0;
};

// pnnquan after the histogram(s) exist on the device, up to the initial find_nn pass (P4..P8)
int palette_prepare(nq_handle* h, const double* d_hists, int n_bands, int nMaxColors, uint32_t* out_palette, int32_t* out_K,
                    const uint32_t* d_argb, int64_t n_pixels, PaletteJob* job) {
    job->merge = false; job->h = h;
    h->merge_variant[0] = h->merge_variant[1] = 0;      // (no merge job yet: an early return leaves it that way)
    nq_params& p = h->params;
    const int kind = h->kind;
    nq::Bins B = bins_of(h);
    int* d_maxbins = h->d_ints.p;
    launch_compact(kind, d_hists, n_bands, B, d_maxbins, h->d_ints.p + 8, h->stream);
    int* const pin_maxbins = reinterpret_cast<int*>(h->pin + 4);
    NQ_HIP(h, hipMemcpyAsync(pin_maxbins, d_maxbins, sizeof(int), hipMemcpyDeviceToHost, h->stream));
    NQ_HIP(h, hipStreamSynchronize(h->stream));
    const int maxbins = *pin_maxbins;
    if (maxbins <= 0) NQ_FAIL(h, NQ_ERR_INVALID, "empty image");
    p.maxbins = maxbins;
    short quan_rt = 1;
    int fn = 0;
    bool texicab = false;
    double proportional = 0;
    if (kind == NQ_KIND_RGB) {
        // NQ/PnnQuantizer.java:172-182
        if (nMaxColors < 16) quan_rt = -1;
        p.weight = std::fmin(0.9, nMaxColors * 1.0 / maxbins);
        if (p.weight < .04 && p.PG >= kCoeffs[0][1]) {
            p.PR = p.PG = p.PB = p.PA = 1;
            if (nMaxColors >= 64) quan_rt = 0;
        }
        if (quan_rt > 0) fn = nMaxColors < 64 ? 1 : 2;
        else if (quan_rt < 0) fn = 3;
    } else {
        // NQ/PnnLABQuantizer.java:175-241
        proportional = sqr(nMaxColors) / maxbins;
        if ((p.transparentPixelIndex >= 0 || p.hasSemiTransparency) && nMaxColors < 32) quan_rt = -1;
        p.weight = std::fmin(0.9, nMaxColors * 1.0 / maxbins);
        p.isNano = p.weight <= .015;
        const double weight = p.weight;
        if ((nMaxColors < 16 && weight < .0075) || weight < .001 || (weight > .0015 && weight < .0022)) quan_rt = 2;
        if (weight < .04 && p.PG < 1 && p.PG >= kCoeffs[0][1]) {
            if (nMaxColors >= 64) quan_rt = 0;
        }
        if (nMaxColors > 16 && nMaxColors < 64) {
            double weightB = nMaxColors / 8000.0;
            if (std::fabs(weightB - weight) < .001) quan_rt = 2;
        }
        if (maxbins <= nMaxColors) {
            // pixelMap.size() <= nMaxColors is only possible here (every occupied bin holds >= 1 distinct colour)
            int64_t cnt = 0;
            std::vector<int32_t> inserted;
            if (d_argb || h->frames_active) {               // (a frames call: the sequence's colours, d_argb == nullptr)
                int rcd = distinct_colors(h, d_argb, n_pixels, nMaxColors, &cnt, &inserted);
                if (rcd) return rcd;
            } else if (h->ext_distinct_valid) {                 // split pipeline: the caller merged the bands' lists
                inserted = h->ext_distinct;
                cnt = h->ext_distinct_many ? (int64_t) nMaxColors + 1 : (int64_t) inserted.size();
            } else
                NQ_FAIL(h, NQ_ERR_UNSUPPORTED, "<= nMaxColors occupied bins in the multi-band path: exchange the bands' distinct colours "
                        "(nq_band_distinct_device / nq_set_distinct) before nq_palette_from_histograms_device "
                        "(NQ/PnnLABQuantizer.java:193-206)");
            p.distinctColors = (!d_argb && !h->frames_active && h->ext_distinct_many) ? 0 : cnt;     // (0 = not known: "more than nMaxColors")
            if (cnt <= nMaxColors) {
                // NQ/PnnLABQuantizer.java:193-206: palette = pixelMap.keySet() in HashMap order, a transparent colour swapped to slot 0
                std::vector<int32_t> keys = java_hashmap_keyset(inserted);
                int k = 0;
                for (int32_t pixel : keys) {
                    out_palette[k++] = (uint32_t) pixel;
                    if (k > 1 && (((uint32_t) pixel) >> 24) == 0) { out_palette[k - 1] = out_palette[0]; out_palette[0] = (uint32_t) pixel; }
                }
                p.quan_rt = quan_rt; p.texicab = 0; p.paletteLength = k;
                *out_K = k;
                rec(h, 2); rec(h, 3); rec(h, 4); rec(h, 5);
                return NQ_OK;
            }
        }
        if (quan_rt > 0) fn = quan_rt > 1 ? 4 : (nMaxColors < 64 ? 2 : 1);
        texicab = proportional > .0225 && !p.hasSemiTransparency;
        if (p.hasSemiTransparency) p.ratio = .5;
        else if (quan_rt != 0 && nMaxColors < 64) {
            if (proportional > .018 && proportional < .022) p.ratio = std::fmin(1.0, proportional + weight * std::exp(3.13));
            else if (proportional > .1) p.ratio = std::fmin(1.0, 1.0 - weight);
            else if (proportional > .04) p.ratio = std::fmin(1.0, weight * std::exp(1.56));
            else if (proportional > .025 && (weight < .002 || weight > .0022)) p.ratio = std::fmin(1.0, proportional + weight * std::exp(3.66));
            else p.ratio = std::fmin(1.0, proportional + weight * std::exp(1.718));
        }
        else if (nMaxColors > 256) p.ratio = std::fmin(1.0, 1 - 1.0 / proportional);
        else p.ratio = std::fmin(1.0, 1 - weight * .7);
        if (!p.hasSemiTransparency && quan_rt < 0) p.ratio = std::fmin(1.0, weight * std::exp(3.13));
    }
    p.quan_rt = quan_rt; p.texicab = texicab;
    launch_quanfn(B.cnt, maxbins, fn, h->stream);

    nq::NNParams np;
    np.kind = kind; np.hasSemi = p.hasSemiTransparency; np.texicab = texicab;
    np.ratio = p.ratio; np.PR = p.PR; np.PG = p.PG; np.PB = p.PB; np.PA = p.PA;
    np.pgLessThanCoeff = p.PG < kCoeffs[0][1];
    np.rgbTheta = 2.0;
    if (const char* t = std::getenv("NQ_RGB_THETA")) {           // tests: 1.0 makes the checked assumption fail often (fallback path)
        const double v = std::atof(t);
        if (v >= 1.0 && v <= 1e6) np.rgbTheta = v;
    }
    rec(h, 2);
    launch_find_nn_init(np, B, maxbins, h->scan_box.p, h->sc->init_cand.p, h->stream);
    rec(h, 3);
    if (kind == NQ_KIND_LAB) {
        // NQ/PnnLABQuantizer.java:259-264: ratio retuned AFTER the initial pass
        const double weight = p.weight;
        if (quan_rt > 0 && nMaxColors < 64 && proportional > .035 && proportional < .1) {
            const int dir = proportional > .04 ? 1 : -1;
            const double margin = dir > 0 ? .002 : .0025;
            const double delta = weight > margin && weight < .003 ? 1.872 : 1.632;
            p.ratio = std::fmin(1.0, proportional + dir * weight * std::exp(delta));
            np.ratio = p.ratio;
        }
    }
    const int extbins = maxbins - nMaxColors;
    job->merge = true;
    job->mj.np = np; job->mj.B = B; job->mj.maxbins = maxbins; job->mj.extbins = extbins;
    job->mj.heap = h->heap.p; job->mj.live3 = h->live3.p; job->mj.scan_f = h->scan_f.p; job->mj.scan_i = h->scan_i.p; job->mj.scan_box = h->scan_box.p;
    job->mj.stats = h->d_scalars.p + 4;       // [4..19] the 16 counters of nq_get_merge_stats, [24..31] the team counters
    job->mj.team = h->team.p; job->mj.helpers = 0;
    job->plen = extbins > 0 ? nMaxColors : maxbins;
    // the merge workgroup also fills the palette (P10)
    NQ_HIP(h, h->d_palette.reserve((size_t) std::max(job->plen, 2)));
    h->dev_palette.clear();                   // (the merge workgroup is about to write it)
    job->mj.plen = job->plen; job->mj.palette = h->d_palette.p; job->mj.status = reinterpret_cast<int*>(h->d_scalars.p + 40);
    return NQ_OK;
}

// the merge loops (P9) of n prepared images in one launch per kind, on the stream of `owner`
// order (nullable): order[j] = the index in jobs[] of the j-th job of owner->d_jobs
int merge_launch(nq_handle* owner, const PaletteJob* const* jobs, int n, std::vector<int>* order = nullptr) {
    std::vector<nq::MergeJob> host;
    std::vector<nq_handle*> of;                             // host[i] is the job of handle of[i]
    int n_lab = 0;
    if (order) order->clear();
    for (int pass = 1; pass >= 0; --pass) {                 // LAB jobs first, then RGB
        for (int i = 0; i < n; ++i)
            if (jobs[i]->merge && jobs[i]->mj.np.kind == pass) {
                host.push_back(jobs[i]->mj); of.push_back(jobs[i]->h);
                if (order) order->push_back(i);
            }
        if (pass == 1) n_lab = (int) host.size();
    }
    if (host.empty()) return NQ_OK;
    // merge teams: when the loops of one kind in this call leave CUs free (one 512-thread workgroup per CU), every loop gets helper
    // workgroups that evaluate find_nn speculatively (nq_merge.inc); their hand-off words start zeroed.  The two kinds run one after
    // the other on this stream, so each is sized on its own.
    const int n_rgb = (int) host.size() - n_lab;
    const int helpers_lab = nq::merge_team_helpers(n_lab, (int) host.size(), owner->n_cus),
              helpers_rgb = nq::merge_team_helpers(n_rgb, (int) host.size(), owner->n_cus);
    // watchdog (stats[14] = 2 -> NQ_ERR_TIME_LIMIT): seconds of RESIDENCY a loop may take.  Automatic: 60 s + 1 ms per bin and per loop that
    // shares a CU with it (the slowest legitimate loop measured -- 65 536 bins, four loops per CU -- takes < 10 s; a time-sliced or
    // shared device is slower, hence the margin and NQ_OPT_MERGE_WALL_SECONDS)
    const int per_cu = std::max(1, ((int) host.size() + owner->n_cus - 1) / owner->n_cus);
    for (int i = 0; i < (int) host.size(); ++i) {
        const long long secs = owner->merge_wall_s > 0 ? owner->merge_wall_s : 60LL + ((long long) host[i].maxbins * per_cu) / 1000;
        host[i].wall_ticks = secs * 100000000LL;
        host[i].helpers = i < n_lab ? helpers_lab : helpers_rgb;
        if (host[i].helpers > 0) NQ_HIP(owner, hipMemsetAsync(host[i].team, 0, 256 * sizeof(unsigned long long), owner->stream));
    }
    NQ_HIP(owner, owner->d_jobs.reserve(host.size()));
    NQ_HIP(owner, hipMemcpyAsync(owner->d_jobs.p, host.data(), host.size() * sizeof(nq::MergeJob), hipMemcpyHostToDevice, owner->stream));
    NQ_HIP(owner, hipStreamSynchronize(owner->stream));    // `host` goes out of scope
    int variant_lab[2] = {0, 0}, variant_rgb[2] = {0, 0};
    NQ_HIP(owner, launch_merge(1, owner->d_jobs.p, n_lab, (int) host.size(), owner->n_cus, helpers_lab, owner->stream, variant_lab));
    NQ_HIP(owner, launch_merge(0, owner->d_jobs.p + n_lab, n_rgb, (int) host.size(), owner->n_cus, helpers_rgb, owner->stream, variant_rgb));
    NQ_HIP(owner, launch_status());
    for (int i = 0; i < (int) host.size(); ++i)
        if (of[i]) std::memcpy(of[i]->merge_variant, i < n_lab ? variant_lab : variant_rgb, sizeof of[i]->merge_variant);
    return NQ_OK;
}

// read-back of the palette the merge workgroup wrote (P10): the copies are enqueued by palette_fetch and looked at by palette_check
// once the stream has been waited for (a batch waits ONCE for all its images, not once per image)
int palette_fetch(nq_handle* h, const PaletteJob& job, uint32_t* out_palette) {
    rec(h, 5);
    NQ_HIP(h, hipMemcpyAsync(out_palette, h->d_palette.p, job.plen * sizeof(int), hipMemcpyDeviceToHost, h->stream));
    h->fetched_palette = out_palette; h->fetched_len = job.plen;
    NQ_HIP(h, hipMemcpyAsync(h->merge_readback, h->d_scalars.p + 4, sizeof h->merge_readback, hipMemcpyDeviceToHost, h->stream));
    return NQ_OK;
}
int palette_check(nq_handle* h, const PaletteJob& job, int32_t* out_K) {
    std::memcpy(h->merge_stats, h->merge_readback, sizeof h->merge_stats);
    std::memcpy(h->team_stats, h->merge_readback + 20, sizeof h->team_stats);
    const int status = (int) (h->merge_readback[36] & 0xFFFFFFFFLL);
    if (h->fetched_palette) { h->dev_palette.assign(h->fetched_palette, h->fetched_palette + h->fetched_len); h->palette_synced = true; }   // (read back and waited for)
    h->fetched_palette = nullptr;
    if (h->merge_stats[14] == 2)
        NQ_FAIL(h, NQ_ERR_TIME_LIMIT, "merge loop stopped at its time limit (a slow, shared or time-sliced device: the state was sound; call again, or "
                                      "raise NQ_OPT_MERGE_WALL_SECONDS)");
    if (h->merge_stats[14]) NQ_FAIL(h, NQ_ERR_UNSUPPORTED, "merge loop stopped by its watchdog (more than maxbins^2/2 find_nn calls, or an empty heap)");
    if (status) NQ_FAIL(h, NQ_ERR_REFERENCE_THROWS, "ColorUtils.setAlphaComponent: alpha outside 0..255 (the reference throws IllegalArgumentException)");
    h->params.paletteLength = job.plen;
    *out_K = job.plen;
    return NQ_OK;
}
int palette_finish(nq_handle* h, const PaletteJob& job, uint32_t* out_palette, int32_t* out_K) {
    int rc = palette_fetch(h, job, out_palette);
    if (rc) return rc;
    NQ_HIP(h, hipStreamSynchronize(h->stream));
    NQ_HIP(h, launch_status());
    return palette_check(h, job, out_K);
}

// the palette of one image: prepare(&job) fills the job, then the merge loop and the read-back
template <typename Prepare> int palette_of(nq_handle* h, uint32_t* out_palette, int32_t* out_K, Prepare prepare) {
    PaletteJob job;
    int rc = prepare(&job);
    if (rc || !job.merge) return rc;
    const PaletteJob* jp = &job;
    rc = merge_launch(h, &jp, 1);
    if (rc) return rc;
    rec(h, 4);
    return palette_finish(h, job, out_palette, out_K);
}

// the histogram's parameters (after apply_scan) and its sort workspace on the handle's scratch (after reserve_palette_ws)
void hist_setup(const nq_handle* h, nq::HistParams* hp, nq::SortWorkspace* ws) {
    const nq_params& p = h->params;
    hp->hasSemi = p.hasSemiTransparency; hp->hasTransp = p.nMaxColors < 64 || p.transparentPixelIndex >= 0;
    hp->transparentColor = p.transparentColor; hp->rewriteTransparent = 0;
    ws->keys_a = h->sc->keys_a.p; ws->keys_b = h->sc->keys_b.p; ws->vals_a = h->sc->vals_a.p; ws->vals_b = h->sc->vals_b.p;
    ws->tmp = h->sc->sort_tmp.p; ws->tmp_bytes = h->sc->sort_tmp.n; ws->seg_start = h->sc->seg.p; ws->seg_end = h->sc->seg.p + 65536;
}

// pnnquan of n pixels once the pre-scan's scalars are back (one image, or the frame table: d_argb == nullptr): apply_scan, the
// <= 2-colour palette, then the histogram over the keys that keys(hp, ws) lays out in the workspace, and palette_prepare
template <typename Keys>
int palette_after_scan(nq_handle* h, const long long* scan3, const uint32_t* d_argb, int64_t n, int nMaxColors, uint32_t* out_palette,
                       int32_t* out_K, PaletteJob* job, Keys keys) {
    apply_scan(h, nMaxColors, scan3[0], (uint32_t) scan3[1], scan3[2]);
    h->merge_variant[0] = h->merge_variant[1] = 0;
    rec(h, 1);
    nq_params& p = h->params;
    if (nMaxColors <= 2) {
        // NQ/PnnQuantizer.java:441-452
        p.weight = 1;
        if (p.transparentPixelIndex >= 0) { out_palette[0] = (uint32_t) p.transparentColor; out_palette[1] = 0xFF000000u; }
        else { out_palette[0] = 0xFF000000u; out_palette[1] = 0xFFFFFFFFu; }
        p.paletteLength = nMaxColors; *out_K = nMaxColors;
        rec(h, 2); rec(h, 3); rec(h, 4); rec(h, 5);
        return NQ_OK;
    }
    int rc = reserve_palette_ws(h, n);
    if (rc) return rc;
    nq::HistParams hp;
    nq::SortWorkspace ws;
    hist_setup(h, &hp, &ws);
    keys(hp, ws);
    return palette_prepare(h, h->sc->hist.p, 1, nMaxColors, out_palette, out_K, d_argb, n, job);
}

// alpha pre-scan + histogram + palette_prepare
int pnnquan_prepare(nq_handle* h, const uint32_t* d_argb, int width, int height, int nMaxColors, uint32_t* out_palette, int32_t* out_K,
                    PaletteJob* job) {
    job->merge = false;
    if (!d_argb || width <= 0 || height <= 0 || !out_palette || !out_K) NQ_FAIL(h, NQ_ERR_INVALID, "bad argument");
    if (nMaxColors < 1 || nMaxColors > 32767) NQ_FAIL(h, NQ_ERR_INVALID, "nMaxColors out of range");
    const int64_t n = (int64_t) width * height;
    if (n > 2147483647LL) NQ_FAIL(h, NQ_ERR_INVALID, "image larger than a Java int[]");
    long long* d_scan3 = h->d_scalars.p + 1;
    rec(h, 0);
    // the common case (nMaxColors >= 64: 5-6-5 keys unless the scan finds transparency) gets the sort words with the scan's read
    bool words = false;
    if (nMaxColors >= 64) {
        int rcw = reserve_palette_ws(h, n);
        if (rcw) return rcw;
        words = launch_front((const int*) d_argb, n, d_scan3, h->sc->vals_a.p, (int) 0x00FFFFFFu, h->sc->seg.p + 2 * 65536, h->stream);
    }
    if (!words) launch_prescan((const int*) d_argb, n, 0, d_scan3, h->stream);
    NQ_HIP(h, hipMemcpyAsync(h->pin, d_scan3, 3 * sizeof(long long), hipMemcpyDeviceToHost, h->stream));
    NQ_HIP(h, hipStreamSynchronize(h->stream));
    const long long scan3[3] = {h->pin[0], h->pin[1], h->pin[2]};
    return palette_after_scan(h, scan3, d_argb, n, nMaxColors, out_palette, out_K, job, [&](const nq::HistParams& hp, const nq::SortWorkspace& ws) {
        // (the speculative words hold 5-6-5 keys and the default transparent colour: right exactly for an image without transparency)
        const bool words_ready = words && !hp.hasSemi && !hp.hasTransp;
        launch_histogram(h->kind, (const int*) d_argb, n, hp, ws, h->sc->hist.p, h->stream, words_ready, /* occ_cleared by launch_front */ words_ready);
    });
}

int pnnquan_device(nq_handle* h, const uint32_t* d_argb, int width, int height, int nMaxColors, uint32_t* out_palette, int32_t* out_K) {
    return palette_of(h, out_palette, out_K, [&](PaletteJob* job) {
        return pnnquan_prepare(h, d_argb, width, height, nMaxColors, out_palette, out_K, job);
    });
}

// ---- one palette for a sequence of frames (nq_pnnquan_frames_device / nq_convert_frames_device) ----
// Arguments of a frames call, checked from the host arrays alone (no device memory is touched): *out_total = pixels of the sequence
// (when wanted)
int frames_check(nq_handle* h, int n, const uint32_t* const* d_argb, const int32_t* widths, const int32_t* heights, int nMaxColors,
                 bool for_dither, int64_t* out_total) {
    if (n <= 0 || !d_argb || !widths || !heights) NQ_FAIL(h, NQ_ERR_INVALID, "bad argument (n = %d)", n);
    if (nMaxColors < 1 || nMaxColors > (for_dither ? 8192 : 32767)) NQ_FAIL(h, NQ_ERR_INVALID, "nMaxColors out of range");
    int64_t total = 0;
    for (int i = 0; i < n; ++i) {
        if (!d_argb[i]) NQ_FAIL(h, NQ_ERR_INVALID, "frame %d: null pixel pointer", i);
        if (widths[i] <= 0 || heights[i] <= 0) NQ_FAIL(h, NQ_ERR_INVALID, "frame %d: bad size %d x %d", i, widths[i], heights[i]);
        if (for_dither && (widths[i] > 65535 || heights[i] > 65535)) NQ_FAIL(h, NQ_ERR_INVALID, "frame %d: side > 65535", i);
        total += (int64_t) widths[i] * heights[i];
        if (total > 2147483647LL) NQ_FAIL(h, NQ_ERR_INVALID, "the sequence holds more pixels than a Java int[] (frame %d)", i);
    }
    if (out_total) *out_total = total;
    return NQ_OK;
}

// the frame table and the (frame, chunk) work list of this call, uploaded on the handle's stream
int frames_upload(nq_handle* h, int n, const uint32_t* const* d_argb, const int32_t* widths, const int32_t* heights) {
    h->h_frames.clear(); h->h_items.clear();
    int64_t off = 0;
    for (int i = 0; i < n; ++i) {
        const int64_t px = (int64_t) widths[i] * heights[i];
        h->h_frames.push_back({(const int*) d_argb[i], (long long) px, (long long) off});
        for (int64_t b = 0; b < px; b += NQ_FRAME_CHUNK)
            h->h_items.push_back({i, (int) std::min<int64_t>(NQ_FRAME_CHUNK, px - b), (long long) b});
        off += px;
    }
    h->frames_total = off;
    NQ_HIP(h, h->d_frames.reserve(h->h_frames.size()));
    NQ_HIP(h, h->d_items.reserve(h->h_items.size()));
    NQ_HIP(h, hipMemcpyAsync(h->d_frames.p, h->h_frames.data(), h->h_frames.size() * sizeof(nq::FrameDesc), hipMemcpyHostToDevice, h->stream));
    NQ_HIP(h, hipMemcpyAsync(h->d_items.p, h->h_items.data(), h->h_items.size() * sizeof(nq::FrameChunk), hipMemcpyHostToDevice, h->stream));
    return NQ_OK;
}

// the per-call state of a frames call, cleared on every way out
struct FramesScope {
    nq_handle* h;
    explicit FramesScope(nq_handle* hh) : h(hh) { h->frames_active = true; h->reuse_lists = false; h->lists_built = false; h->rec_skip = 0; }
    ~FramesScope() { h->frames_active = false; h->reuse_lists = false; h->lists_built = false; h->rec_skip = 0; }
};

// pnnquan_prepare over the frame table (frames_upload first): the pre-scan with global indices, the histogram words of all frames in one
// buffer at their global offsets -- then the histogram, compaction and the initial find_nn pass exactly as for one image of N pixels
int pnnquan_frames_prepare(nq_handle* h, int nMaxColors, uint32_t* out_palette, int32_t* out_K, PaletteJob* job) {
    job->merge = false;
    const int64_t n = h->frames_total;
    const int nf = (int) h->h_frames.size(), ni = (int) h->h_items.size();
    long long* d_scan3 = h->d_scalars.p + 1;
    rec(h, 0);
    // the common case (nMaxColors >= 64) gets the speculative 5-6-5 sort words with the scan's read, as front_kernel does for one image
    const bool words = nMaxColors >= 64;
    if (words) {
        int rcw = reserve_palette_ws(h, n);
        if (rcw) return rcw;
    }
    launch_frames_pass(words ? FRAMES_FRONT : FRAMES_SCAN, h->d_frames.p, nf, h->d_items.p, ni, d_scan3,
                       words ? reinterpret_cast<unsigned*>(h->sc->vals_a.p) : nullptr, nullptr, (int) 0x00FFFFFFu, 0, h->stream);
    long long scan3[3];
    NQ_HIP(h, hipMemcpyAsync(scan3, d_scan3, sizeof scan3, hipMemcpyDeviceToHost, h->stream));
    NQ_HIP(h, hipStreamSynchronize(h->stream));
    NQ_HIP(h, launch_status());
    return palette_after_scan(h, scan3, nullptr, n, nMaxColors, out_palette, out_K, job, [&](const nq::HistParams& hp, const nq::SortWorkspace& ws) {
        if (!(words && !hp.hasSemi && !hp.hasTransp))
            launch_frames_pass(FRAMES_KEYS, h->d_frames.p, nf, h->d_items.p, ni, nullptr, reinterpret_cast<unsigned*>(h->sc->vals_a.p), nullptr,
                               hp.transparentColor, hp.hasSemi ? 2 : hp.hasTransp ? 1 : 0, h->stream);
        launch_histogram(h->kind, nullptr, n, hp, ws, h->sc->hist.p, h->stream, true);
    });
}

// the dither modes of include/nquant_abi.h (the static GilbertCurve / BlueNoise entry points have no LOOKUP_ONLY form)
int check_mode(nq_handle* h, int mode, bool lookup_only_ok = true) {
    if (mode != NQ_MODE_PARALLEL_TILED && mode != NQ_MODE_REFERENCE_SEQUENTIAL && !(lookup_only_ok && mode == NQ_MODE_LOOKUP_ONLY))
        NQ_FAIL(h, NQ_ERR_INVALID, "unknown mode %d", mode);
    return NQ_OK;
}

// nq_gilbert_dither / nq_bluenoise_dither: the static entry points of the reference run the same stages with caller-supplied
// saliencies / weight instead of the ones dither() derives
struct StageOverride { bool gilbert_only = false, blue_only = false; const float* d_sal = nullptr; bool hasSal = false; double weight = 0; float blueWeight = 1.f; };

int dither_device(nq_handle* h, const uint32_t* d_argb, int width, int height, const uint32_t* palette, int K, int dither,
                  int64_t seed, int mode, uint32_t* d_out_argb, uint16_t* d_out_index, const StageOverride& ov = StageOverride()) {
    if (!d_argb || width <= 0 || height <= 0 || !palette || K < 1 || !d_out_argb) NQ_FAIL(h, NQ_ERR_INVALID, "bad argument");
    if (width > 65535 || height > 65535) NQ_FAIL(h, NQ_ERR_INVALID, "image side > 65535");
    if (K > 8192) NQ_FAIL(h, NQ_ERR_UNSUPPORTED, "palettes above 8192 entries do not fit the LDS staging");
    const int64_t n = (int64_t) width * height;
    nq_params& p = h->params;
    { int rcp = upload_palette(h, palette, K); if (rcp) return rcp; }
    if (!d_out_index) { NQ_HIP(h, h->d_out_index.reserve((size_t) n)); d_out_index = h->d_out_index.p; }
    // stage events 5..7 belong to THIS call only once it has recorded all of them (set at the successful exits below); until then
    // nq_get_stage_ms reports what the last finished convert left
    h->dither_events_fresh = false;
    // Finish phase of a batch with a prep stream: what builds the scratch set's content for this image -- lists, Lab table, saliency map,
    // the hand-back counts' clear -- runs there, behind the set's previous user (set_free) and, where the palette was uploaded just now,
    // behind that copy (prep_done serves as the marker on the handle's stream first).  PrepScope puts the handle's stream back.
    struct PrepScope {
        nq_handle* h; hipStream_t main;
        ~PrepScope() { h->stream = main; }
    } prep_scope{h, h->stream};
    const bool prep = h->prep_stream && h->prep_stream != h->stream && mode != NQ_MODE_LOOKUP_ONLY;
    if (h->set_free) NQ_HIP(h, hipStreamWaitEvent(prep ? h->prep_stream : h->stream, h->set_free, 0));
    if (prep && !h->palette_synced) {
        NQ_HIP(h, hipEventRecord(h->prep_done, h->stream));
        NQ_HIP(h, hipStreamWaitEvent(h->prep_stream, h->prep_done, 0));
    }

    if (mode == NQ_MODE_LOOKUP_ONLY) {
        DevParams P = dev_params(h, K);
        nq::ListsView lv;
        int rcl = lists_for_call(h, P, &lv);
        if (rcl) return rcl;
        const bool fast_lookup = h->use_fast_dither && fast_lookup_eligible(P, lv);
        if (fast_lookup) NQ_HIP(h, h->sc->lookup_todo.reserve((size_t) n + 1));
        rec(h, 5);       // stage "dither" = the lookup kernels alone (the candidate lists are built in front of them), "bluenoise" = 0
        if (fast_lookup)
            launch_fast_lookup_only(P, lv, h->d_palette.p, packed_lists(h), (const int*) d_argb, n, d_out_index, (int*) d_out_argb,
                                    h->sc->lookup_todo.p, h->stream);
        else
            launch_lookup_only(P, h->d_palette.p, lv, (const int*) d_argb, n, d_out_index, (int*) d_out_argb, h->stream);
        rec(h, 6); rec(h, 7);
        NQ_HIP(h, launch_status());
        h->dither_events_fresh = true;
        return NQ_OK;
    }
    { int rcm = check_mode(h, mode); if (rcm) return rcm; }
    const bool sequential = mode == NQ_MODE_REFERENCE_SEQUENTIAL;

    // dither(): RGB NQ/PnnQuantizer.java:393-407, LAB NQ/PnnLABQuantizer.java:493-522
    // The reference negates the field once per convert() (dither() runs once per object); here dither may be called repeatedly on
    // one handle, so the negation holds for this call only and the handle keeps the value pnnquan left.
    struct WeightGuard { double& w; double saved; ~WeightGuard() { w = saved; } } weight_guard{p.weight, p.weight};
    const bool staged = ov.gilbert_only || ov.blue_only;
    if (p.hasSemiTransparency && !staged) p.weight = -std::fabs(p.weight);
    bool hasSal = false, salSubst = false;
    if (staged) hasSal = ov.hasSal;
    else if (h->kind == NQ_KIND_LAB) {
        if (p.nMaxColors > 2 && p.nMaxColors < 128) { hasSal = true; salSubst = true; }       // pnnquan :135,:155-156
        else if (dither && (K <= 256 || p.weight > .99)) { hasSal = true; }                   // :499-508
    }
    const bool post = ov.blue_only || (!ov.gilbert_only && !dither && K > 32);
    float blueWeight = staged ? ov.blueWeight : 1.0f;
    const bool seq_lab_post = !staged && post && h->kind == NQ_KIND_LAB && sequential;   // needs pixelMap.size() AFTER the gilbert pass
    if (!staged && post && h->kind == NQ_KIND_LAB && !sequential) {
        if (p.distinctColors <= 0) {
            int64_t cnt = 0;
            int rcd = distinct_colors(h, d_argb, n, 0, &cnt, nullptr);
            if (rcd) return rcd;
            p.distinctColors = cnt;
        }
        const double delta = sqr(K) / (double) p.distinctColors;
        blueWeight = delta > 0.023 ? 1.0f : (float) (37.013 * delta + 0.906);
    }
    DevParams P = dev_params(h, K);
    GilbertConsts G = gilbert_consts(K, staged ? ov.weight : p.weight, hasSal, dither != 0);
    G.salSubst = salSubst;

    TileGeom T;
    std::memset(&T, 0, sizeof T);
    T.width = width; T.height = height;
    const bool banded = h->band_image_h > 0;
    if (banded && (sequential || h->band_y0 + height > h->band_image_h))
        NQ_FAIL(h, NQ_ERR_INVALID, "nq_set_band: the band [%d, %d) does not fit the image height %d (or REFERENCE_SEQUENTIAL mode)", h->band_y0, h->band_y0 + height, h->band_image_h);
    const int rule_h = banded ? h->band_image_h : height;          // the automatic tile follows the WHOLE image
    if (sequential) { T.tile_w = width; T.tile_h = height; }
    // (a band clamps the tile to the WHOLE image here, as the automatic rule does: tile_base below counts the image's tile rows, and a
    // last band lower than the tile would otherwise number its tiles -- their random streams -- by its own height)
    else if (h->tile_w > 0 && h->tile_h > 0) { T.tile_w = std::min(h->tile_w, width); T.tile_h = std::min(h->tile_h, rule_h); }
    else {
        // automatic: 8x8 when that yields >= 2 wavefronts of chains per SIMD (131072 chains), else 4x4.  The tile size does not change
        // the measured dither quality, it sets how many chains run in parallel and how much LDS a chain's staged indices
        // take: 16x16 (the round-1 choice for images beyond 5793^2) ran the 16384^2 pass in 22.7 ms, 8x8 in 12.5 ms
        int tsz = 4;
        {
            const int cand = 8;
            const int64_t tiles = (int64_t) ((width + cand - 1) / cand) * ((rule_h + cand - 1) / cand);
            if (tiles >= 131072) tsz = cand;
        }
        // (the sorted-by-yDiff queue takes the same rule since round 4: its tile chains start in the queue's steady state, nq_dither.inc)
        T.tile_w = std::min(tsz, width); T.tile_h = std::min(tsz, rule_h);
    }
    if (banded) {
        // (T.tile_h <= the image height here; the band's own height clamps it only after tile_base is known)
        if (h->band_y0 % T.tile_h != 0 || (h->band_y0 + height != h->band_image_h && height % T.tile_h != 0))
            NQ_FAIL(h, NQ_ERR_INVALID, "nq_set_band: band origin %d / rows %d must be multiples of the tile height %d", h->band_y0, height, T.tile_h);
        T.y_origin = h->band_y0;
        T.tile_base = (h->band_y0 / T.tile_h) * ((width + T.tile_w - 1) / T.tile_w);
        T.tile_h = std::min(T.tile_h, height);
    }
    T.tiles_x = (width + T.tile_w - 1) / T.tile_w; T.tiles_y = (height + T.tile_h - 1) / T.tile_h;
    const int rw = width - (T.tiles_x - 1) * T.tile_w, rh = height - (T.tiles_y - 1) * T.tile_h;
    const int sw[4] = {T.tile_w, rw, T.tile_w, rw}, shh[4] = {T.tile_h, T.tile_h, rh, rh};
    for (int s = 0; s < 4; ++s) {
        int rc = get_path(h, sw[s], shh[s], s, &T.path[s]);
        if (rc) return rc;
        T.path_len[s] = sw[s] * shh[s]; T.shape_w[s] = sw[s]; T.shape_h[s] = shh[s];
    }
    if (sequential && !ov.blue_only) NQ_HIP(h, hipMemsetAsync(h->d_bincache.p, 0xFF, 65536 * sizeof(short), h->stream));   // (BlueNoise.dither alone continues the caches)
    nq::ListsView lv;
    bool sal_done = false;
    const bool want_sal = !staged && hasSal;            // (the map of THIS call's pixels; the builders and the map share one launch where they can)
    // (the specialised dither kernel's hand-back list is sized here, so that the builders' launch can clear its count)
    const bool maybe_fast = !ov.blue_only && !sequential && h->use_fast_dither && K > 32 && K <= 256;
    bool failed_cleared = false;
    if (maybe_fast) NQ_HIP(h, h->d_failed.reserve(failed_words(T)));
    // (A/B timing, prep stream only: NQ_FINISH_SAL = 1 / 2: the saliency map as a launch of its own in front of / behind the list
    // builders on the prep stream, 3: on the handle's stream in front of the light pass)
    int sal_own = 0;
    if (prep && want_sal) if (const char* e = std::getenv("NQ_FINISH_SAL")) { const int v = std::atoi(e); if (v >= 1 && v <= 3) sal_own = v; }
    if (prep) h->stream = h->prep_stream;
    if (sal_own) NQ_HIP(h, h->sc->saliency.reserve((size_t) n));
    if (sal_own == 1) { launch_saliency(P, salSubst ? 1 : 0, (const int*) d_argb, n, h->sc->saliency.p, h->stream); sal_done = true; }
    { bool folded_sal = false;
      int rcl = lists_for_call(h, P, &lv, want_sal && !sal_own ? (const int*) d_argb : nullptr, n, salSubst ? 1 : 0, &folded_sal,
                               maybe_fast ? failed_list(h) : nullptr, &failed_cleared);
      if (rcl) return rcl;
      sal_done = sal_done || folded_sal; }
    const float* d_sal = nullptr;
    if (staged) d_sal = hasSal ? ov.d_sal : nullptr;
    else if (hasSal) {
        NQ_HIP(h, h->sc->saliency.reserve((size_t) n));
        if (!sal_done && sal_own != 3) launch_saliency(P, salSubst ? 1 : 0, (const int*) d_argb, n, h->sc->saliency.p, h->stream);
        d_sal = h->sc->saliency.p;
    }
    if (prep) {
        NQ_HIP(h, hipEventRecord(h->prep_done, h->prep_stream));
        h->stream = prep_scope.main;
        NQ_HIP(h, hipStreamWaitEvent(h->stream, h->prep_done, 0));
        if (sal_own == 3) launch_saliency(P, salSubst ? 1 : 0, (const int*) d_argb, n, h->sc->saliency.p, h->stream);
    }
    // stage "palette_fill" ends here: it includes the candidate-list build and the saliency map -- except behind a prep stream, where it
    // is what the launch stream still waits of them
    rec(h, 5);
    int log_cap = 0;
    if (seq_lab_post) {
        // every colour handed to nearestColorIndex on a cache miss (<= 3 lookups per pixel) + a flag per palette entry
        if (3 * n + 16 > 2147483647LL) NQ_FAIL(h, NQ_ERR_INVALID, "image too large for the sequential pixelMap log");
        log_cap = (int) (3 * n + 16);
        NQ_HIP(h, h->d_seqlog.reserve((size_t) log_cap + 4));
        NQ_HIP(h, h->d_seqseen.reserve((size_t) K));
        NQ_HIP(h, hipMemsetAsync(h->d_seqlog.p + log_cap, 0, sizeof(int), h->stream));
        NQ_HIP(h, hipMemsetAsync(h->d_seqseen.p, 0, (size_t) K, h->stream));
    }
    const int* d_tile_list = nullptr;
    hipStream_t tail_stream = h->stream;          // where the dither pass ends: the side stream once a chain pass went there
    h->chain_on_side = false;
    h->last_dither_fast = 0;
    h->split_uncounted = false;
    if (ov.blue_only) { /* BlueNoise.dither alone: the indices are already in d_out_index */ }
    else {
    if (!sequential && h->use_fast_dither && gilbert_fast_eligible(P, G, T, lv)) {
        // production path (nq_dither_fast.hip); the tiles it cannot finish come back as a list for the generic kernel below
        NQ_HIP(h, h->d_failed.reserve(failed_words(T)));
        // NQ_OPT_DITHER_CHAIN.  Automatic: the split form with the chain pass on the side stream in the finish phase of a batch (chain_stream
        // set) -- with the pixel-form light pass where the tile size allows --, the fused light walk everywhere else
        int chain_mode = nq::FAST_CHAIN_FUSED;
        if (h->dither_chain == 1) chain_mode = nq::FAST_CHAIN_ALWAYS;
        else if (h->dither_chain == 3) chain_mode = nq::FAST_CHAIN_SPLIT;
        else if (h->dither_chain == 4 || (h->dither_chain == 0 && h->chain_stream)) chain_mode = nq::FAST_CHAIN_PIXEL;
        const bool split = (chain_mode == nq::FAST_CHAIN_SPLIT || chain_mode == nq::FAST_CHAIN_PIXEL) && nq::gilbert_fast_split_eligible(P, G);
        const bool side = split && h->chain_stream && h->chain_stream != h->stream;
        if (split) ++g_split_passes;
        if (side) ++g_split_side;
        h->split_uncounted = split;
        NQ_HIP(h, launch_gilbert_fast(P, G, T, lv, (const int*) d_argb, d_sal, h->d_palette.p, (long long) seed, d_out_index,
                                      post ? nullptr : (int*) d_out_argb, failed_list(h), packed_lists(h), h->stream, failed_cleared,
                                      chain_mode, side ? h->chain_stream : nullptr, side ? h->chain_gate : nullptr, lab_table(h)));
        if (side) tail_stream = h->chain_stream;
        d_tile_list = failed_list(h);
        h->last_dither_fast = 1;
    }
    launch_gilbert(P, G, T, lv, (const int*) d_argb, d_sal, h->d_palette.p, h->d_bincache.p, (long long) seed, sequential ? 1 : 0,
                   h->d_scalars.p, d_out_index, post ? nullptr : (int*) d_out_argb,
                   seq_lab_post ? h->d_seqlog.p : nullptr, seq_lab_post ? h->d_seqlog.p + log_cap : nullptr,
                   seq_lab_post ? h->d_seqseen.p : nullptr, log_cap, d_tile_list, tail_stream);
    if (tail_stream != h->stream) { NQ_HIP(h, hipEventRecord(h->chain_done, tail_stream)); h->chain_on_side = true; }
    }
    rec(h, 6);
    if (seq_lab_post) {
        // pixelMap.size() at NQ/PnnLABQuantizer.java:512 = |{image colours as the histogram saw them} U {colours looked up on a
        // nearest-cache miss} U {palette entries those lookups touched}| (getLab memoises all three).  Debugging mode: on the host.
        int count = 0;
        NQ_HIP(h, hipMemcpyAsync(&count, h->d_seqlog.p + log_cap, sizeof(int), hipMemcpyDeviceToHost, h->stream));
        NQ_HIP(h, hipStreamSynchronize(h->stream));
        if (count > log_cap) NQ_FAIL(h, NQ_ERR_HIP, "sequential pixelMap log overflow (internal error)");
        std::vector<int32_t> all((size_t) n + count);
        std::vector<unsigned char> seen(K);
        NQ_HIP(h, hipMemcpy(all.data(), d_argb, (size_t) n * sizeof(int), hipMemcpyDeviceToHost));
        if (count) NQ_HIP(h, hipMemcpy(all.data() + n, h->d_seqlog.p, (size_t) count * sizeof(int), hipMemcpyDeviceToHost));
        NQ_HIP(h, hipMemcpy(seen.data(), h->d_seqseen.p, (size_t) K, hipMemcpyDeviceToHost));
        for (int64_t i = 0; i < n; ++i)
            if ((((uint32_t) all[i]) >> 24) <= 0xF) all[i] = p.transparentColor;      // the histogram's substitution (:141-142)
        for (int i = 0; i < K; ++i) if (seen[i]) all.push_back((int32_t) palette[i]);
        std::sort(all.begin(), all.end());
        const int64_t distinct = (int64_t) (std::unique(all.begin(), all.end()) - all.begin());
        const double delta = sqr(K) / (double) distinct;
        blueWeight = delta > 0.023 ? 1.0f : (float) (37.013 * delta + 0.906);
    }
    if (post && !sequential && h->use_fast_dither && fast_lookup_eligible(P, lv))
        launch_fast_bluenoise(P, lv, h->d_palette.p, packed_lists(h), (const int*) d_argb, width, height, T.y_origin, blueWeight, (long long) seed,
                              d_out_index, (int*) d_out_argb, h->stream);
    else if (post)
        launch_bluenoise(P, h->d_palette.p, lv, (const int*) d_argb, width, height, T.y_origin, blueWeight, (long long) seed, sequential ? 1 : 0,
                         h->d_bincache.p, h->d_scalars.p, d_out_index, (int*) d_out_argb, h->stream);
    rec(h, 7);
    NQ_HIP(h, launch_status());
    h->dither_events_fresh = true;
    return NQ_OK;
}

void finish_timing(nq_handle* h) {
    // {prescan, histogram, nn_init, merge, palette_fill, dither, bluenoise, total}
    for (int i = 0; i < 7; ++i) {
        float ms = 0;
        if (h->light_events && i != 5) { h->stage_ms[i] = -1.0f; continue; }      // (not recorded: see rec)
        if (hipEventElapsedTime(&ms, h->ev[i], h->ev[i + 1]) != hipSuccess) ms = 0;
        h->stage_ms[i] = ms;
    }
    float tot = 0;
    if (hipEventElapsedTime(&tot, h->ev[0], h->ev[h->light_events ? 6 : 7]) != hipSuccess) tot = 0;
    h->stage_ms[7] = tot;
    h->dither_events_fresh = false;
}

void finish_batch_timing(nq_handle* h0) {
    for (int i = 0; i < 3; ++i) {
        float ms = 0;
        if (hipEventElapsedTime(&ms, h0->bev[i], h0->bev[i + 1]) != hipSuccess) ms = 0;
        h0->batch_phase_ms[i] = ms;
    }
    float tot = 0;
    if (hipEventElapsedTime(&tot, h0->bev[0], h0->bev[3]) != hipSuccess) tot = 0;
    h0->batch_phase_ms[3] = tot;
}

// ---- host forms: the caller's n arrays (px[i] elements each; one image: n = 1) lie end to end in a handle buffer, array i at dev[i] ----
template <typename T> int stage_room(nq_handle* h, DevBuf<T>& buf, int n, const size_t* px, T** dev) {
    size_t total = 0;
    for (int i = 0; i < n; ++i) total += px[i];
    NQ_HIP(h, buf.reserve(total));
    for (int i = 0; i < n; ++i) dev[i] = i ? dev[i - 1] + px[i - 1] : buf.p;
    return NQ_OK;
}
// ... uploaded from the caller's arrays
template <typename T, typename S> int stage_in(nq_handle* h, DevBuf<T>& buf, int n, const size_t* px, const S* const* src, T** dev) {
    static_assert(sizeof(T) == sizeof(S), "staged element size");
    int rc = stage_room(h, buf, n, px, dev);
    if (rc) return rc;
    for (int i = 0; i < n; ++i) NQ_HIP(h, hipMemcpyAsync(dev[i], src[i], px[i] * sizeof(T), hipMemcpyHostToDevice, h->stream));
    return NQ_OK;
}
// ... and read back to them in the same layout (dst[i] == null: not wanted)
template <typename T, typename S> int stage_out(nq_handle* h, const DevBuf<T>& buf, int n, const size_t* px, S* const* dst) {
    static_assert(sizeof(T) == sizeof(S), "staged element size");
    size_t off = 0;
    for (int i = 0; i < n; ++i) {
        if (dst[i]) NQ_HIP(h, hipMemcpyAsync(dst[i], buf.p + off, px[i] * sizeof(T), hipMemcpyDeviceToHost, h->stream));
        off += px[i];
    }
    return NQ_OK;
}

// A host form runs its staging and device work in body(); on failure the stream is waited for too, so no copy from or to the
// caller's buffers outlives the call (on success the body's own read-back wait, or the device form's, has done that)
template <typename Body> int host_form(nq_handle* h, Body body) {
    const int rc = body();
    if (rc) (void) hipStreamSynchronize(h->stream);
    return rc;
}

// The host form of an image entry point over n caller images: pixels in d_in; when results are wanted (out_argb or out_index given),
// room for them in d_out_argb / d_out_index (reserved first: growing a buffer frees the old one, which waits for the device);
// step(d_in, d_out_argb, d_out_index) on the device copies; then the wanted results read back and waited for
template <typename Step>
int host_images(nq_handle* h, int n, const size_t* px, const uint32_t* const* argb, uint32_t* const* out_argb, uint16_t* const* out_index,
                Step step) {
    return host_form(h, [&]() -> int {
        std::vector<uint32_t*> d_in(n), d_out(n);
        std::vector<uint16_t*> d_index(n);
        const bool results = out_argb || out_index;
        int rc = results ? stage_room(h, h->d_out_argb, n, px, d_out.data()) : NQ_OK;
        if (!rc && results) rc = stage_room(h, h->d_out_index, n, px, d_index.data());
        if (!rc) rc = stage_in(h, h->d_in, n, px, argb, d_in.data());
        if (!rc) rc = step(d_in.data(), d_out.data(), d_index.data());
        if (!rc && out_argb) rc = stage_out(h, h->d_out_argb, n, px, out_argb);
        if (!rc && out_index) rc = stage_out(h, h->d_out_index, n, px, out_index);
        if (rc || !results) return rc;
        NQ_HIP(h, hipStreamSynchronize(h->stream));
        return NQ_OK;
    });
}

// ---- palette refinement (nq_refine.hip) ----
// the arguments of every form, from the host arrays alone (no device work): the sizes first, then the pointers
int refine_check(nq_handle* h, int n, const uint32_t* const* argb, const int32_t* widths, const int32_t* heights, const uint32_t* io_palette,
                 int K, int iterations, const int64_t* out_sse, const int32_t* out_passes, int64_t* out_total) {
    if (n < 1) NQ_FAIL(h, NQ_ERR_INVALID, "n = %d: at least one frame", n);
    if (K < 1 || K > 256) NQ_FAIL(h, NQ_ERR_INVALID, "K = %d: must be 1..256", K);
    if (iterations < 0 || iterations > 64) NQ_FAIL(h, NQ_ERR_INVALID, "iterations = %d: must be 0..64", iterations);
    if (!argb || !widths || !heights) NQ_FAIL(h, NQ_ERR_INVALID, "the array of frame pointers, widths or heights is NULL");
    if (!io_palette || !out_sse || !out_passes) NQ_FAIL(h, NQ_ERR_INVALID, "io_palette, out_sse or out_passes is NULL");
    int64_t total = 0;
    for (int i = 0; i < n; ++i) {
        if (widths[i] < 1 || widths[i] > 65535 || heights[i] < 1 || heights[i] > 65535)
            NQ_FAIL(h, NQ_ERR_INVALID, "frame %d: %d x %d: sides must be 1..65535", i, widths[i], heights[i]);
        total += (int64_t) widths[i] * heights[i];
        if (total > 2147483647ll) NQ_FAIL(h, NQ_ERR_INVALID, "the sequence holds more than 2^31 - 1 pixels (frame %d)", i);
    }
    for (int i = 0; i < n; ++i)
        if (!argb[i] || ((uintptr_t) argb[i] & 3)) NQ_FAIL(h, NQ_ERR_INVALID, "frame %d: pixel pointer NULL or not 4-byte aligned", i);
    *out_total = total;
    return NQ_OK;
}

// nq_refine_palette_device after the checks: frame table and state go up, all passes are enqueued, the results come back in one copy
int refine_device(nq_handle* h, int n, const uint32_t* const* d_argb, const int32_t* widths, const int32_t* heights, int64_t total,
                  uint32_t* io_palette, int K, int iterations, int64_t* out_sse, int64_t* out_counts, int32_t* out_passes) {
    std::vector<nq::RefineFrame>& t = h->h_refine_frames;
    t.resize(n);
    bool vec = true;                                // the 16-byte path needs every frame aligned to it
    for (int i = 0; i < n; ++i) {
        t[i] = {reinterpret_cast<const unsigned*>(d_argb[i]), (long long) widths[i] * heights[i]};
        vec = vec && !((uintptr_t) d_argb[i] & 15);
    }
    std::vector<unsigned long long>& st = h->h_refine;
    st.assign(nq::REFINE_STATE_WORDS, 0ull);
    std::memcpy(st.data() + nq::REFINE_PALETTE, io_palette, (size_t) K * sizeof(uint32_t));
    NQ_HIP(h, h->d_refine_frames.reserve(n));
    NQ_HIP(h, h->d_refine.reserve(nq::REFINE_STATE_WORDS));
    NQ_HIP(h, hipMemcpyAsync(h->d_refine_frames.p, t.data(), n * sizeof(nq::RefineFrame), hipMemcpyHostToDevice, h->stream));
    NQ_HIP(h, hipMemcpyAsync(h->d_refine.p, st.data(), st.size() * sizeof(unsigned long long), hipMemcpyHostToDevice, h->stream));
    launch_refine(h->d_refine_frames.p, n, (long long) total, vec, h->n_cus, K, iterations, h->d_refine.p, h->stream);
    NQ_HIP(h, launch_status());
    NQ_HIP(h, hipMemcpyAsync(st.data() + nq::REFINE_DONE, h->d_refine.p + nq::REFINE_DONE,
                             (nq::REFINE_STATE_WORDS - nq::REFINE_DONE) * sizeof(unsigned long long), hipMemcpyDeviceToHost, h->stream));
    NQ_HIP(h, hipStreamSynchronize(h->stream));
    std::memcpy(io_palette, st.data() + nq::REFINE_PALETTE, (size_t) K * sizeof(uint32_t));
    for (int j = 0; j <= iterations; ++j) out_sse[j] = (int64_t) st[nq::REFINE_SSE_OUT + j];
    if (out_counts) for (int k = 0; k < K; ++k) out_counts[k] = (int64_t) st[nq::REFINE_COUNTS + k];
    *out_passes = (int32_t) st[nq::REFINE_PASSES];
    return NQ_OK;
}

// both forms of nq_refine_palette (host: the frames lie in d_in, every one on a 16-byte boundary)
int refine_call(nq_handle* h, bool host, int n, const uint32_t* const* argb, const int32_t* widths, const int32_t* heights,
                uint32_t* io_palette, int K, int iterations, int64_t* out_sse, int64_t* out_counts, int32_t* out_passes) {
    if (!h) return NQ_ERR_INVALID;
    int64_t total = 0;
    int rc = refine_check(h, n, argb, widths, heights, io_palette, K, iterations, out_sse, out_passes, &total);
    if (rc) return rc;
    rc = use_device(h);
    if (rc) return rc;
    if (!host) return refine_device(h, n, argb, widths, heights, total, io_palette, K, iterations, out_sse, out_counts, out_passes);
    return host_form(h, [&]() -> int {
        std::vector<const uint32_t*> d_src(n);
        size_t room = 0;
        for (int i = 0; i < n; ++i) room += ((size_t) widths[i] * heights[i] + 3) & ~(size_t) 3;
        NQ_HIP(h, h->d_in.reserve(room));
        size_t at = 0;
        for (int i = 0; i < n; ++i) {
            const size_t px = (size_t) widths[i] * heights[i];
            d_src[i] = h->d_in.p + at;
            NQ_HIP(h, hipMemcpyAsync(h->d_in.p + at, argb[i], px * sizeof(uint32_t), hipMemcpyHostToDevice, h->stream));
            at += (px + 3) & ~(size_t) 3;
        }
        return refine_device(h, n, d_src.data(), widths, heights, total, io_palette, K, iterations, out_sse, out_counts, out_passes);
    });
}

// the `refine` argument of the nq_convert_frames_refined forms
int refine_check_convert(nq_handle* h, int refine, int nMaxColors) {
    if (refine < 0 || refine > 64) NQ_FAIL(h, NQ_ERR_INVALID, "refine = %d: must be 0..64", refine);
    if (refine > 0 && nMaxColors > 256) NQ_FAIL(h, NQ_ERR_INVALID, "refine needs nMaxColors <= 256");
    return NQ_OK;
}

// ---- setup shared by the batch entry points ----
// the batch's arguments, from the host arrays alone (hs[0] is not null); `host`: every image's pointers and size as well
int batch_check(nq_handle* const* hs, int n, const uint32_t* const* argb, const int32_t* widths, const int32_t* heights, int nMaxColors,
                const int64_t* rng_seeds, uint32_t* const* out_argb, const uint32_t* out_palettes, int32_t palette_stride, const int32_t* out_K,
                bool host) {
    nq_handle* h0 = hs[0];
    if (!argb || !widths || !heights || !rng_seeds || !out_argb || !out_palettes || !out_K) NQ_FAIL(h0, NQ_ERR_INVALID, "bad argument");
    if (palette_stride < std::max(nMaxColors, 2)) NQ_FAIL(h0, NQ_ERR_INVALID, "palette_stride < max(nMaxColors, 2)");
    for (int i = 0; i < n; ++i) {
        if (host && (!hs[i] || !argb[i] || !out_argb[i] || widths[i] <= 0 || heights[i] <= 0)) NQ_FAIL(h0, NQ_ERR_INVALID, "bad argument for image %d", i);
        if (!hs[i]) NQ_FAIL(h0, NQ_ERR_INVALID, "null handle in batch");
        if (hs[i]->device != h0->device) NQ_FAIL(h0, NQ_ERR_INVALID, "handles of a batch must share one device");
        for (int j = 0; j < i; ++j) if (hs[j] == hs[i]) NQ_FAIL(h0, NQ_ERR_INVALID, "a handle appears twice in the batch");
    }
    return NQ_OK;
}

// a failure on handle h of the batch, reported on the first handle
int batch_fail(nq_handle* h0, nq_handle* h, int rc) { if (h != h0) h0->err = h->err; return rc; }

// use_device on every handle: tables and events on the handle's own stream, before the batch redirects it
int batch_use_device(nq_handle* const* hs, int n) {
    for (int i = 0; i < n; ++i) {
        int rc = use_device(hs[i]);
        if (rc) return batch_fail(hs[0], hs[i], rc);
        if (i) NQ_HIP(hs[0], hipStreamSynchronize(hs[i]->stream));
    }
    return NQ_OK;
}

// what a batch call redirects -- every handle's stream, scratch and light_events -- put back on every way out, and the events handed
// to it destroyed
struct BatchGuard {
    nq_handle* const* hs; int n;
    std::vector<hipStream_t> streams;
    std::vector<hipEvent_t> events;
    hipStream_t side[4] = {nullptr, nullptr, nullptr, nullptr};    // the finish phase's side streams (chain streams, prep stream), once work may be on them
    BatchGuard(nq_handle* const* hh, int nn) : hs(hh), n(nn) { for (int i = 0; i < n; ++i) streams.push_back(hs[i]->stream); }
    ~BatchGuard() {
        // (a chain pass or a list build of a call that failed half-way may still run there, writing a scratch set or a handle's d_failed)
        for (hipStream_t s : side) if (s) (void) hipStreamSynchronize(s);
        for (int i = 0; i < n; ++i) {
            hs[i]->stream = streams[i]; hs[i]->sc = &hs[i]->own; hs[i]->light_events = false;
            hs[i]->chain_stream = nullptr; hs[i]->prep_stream = nullptr; hs[i]->set_free = nullptr;
        }
        for (hipEvent_t e : events) (void) hipEventDestroy(e);
    }
};

// nq_nearest_index (out_index: nearestColorIndex) or nq_closest_tuple (out_closest4: closestColorIndex's four candidates) of M host colours
int color_lookup(nq_handle* h, const uint32_t* palette, int K, const uint32_t* colors, int64_t M, int16_t* out_index, int32_t* out_closest4) {
    int rc = use_device(h);
    if (rc) return rc;
    if (!palette || K < 1 || K > 8192 || !colors || M < 0 || !(out_index || out_closest4)) NQ_FAIL(h, NQ_ERR_INVALID, "bad argument");
    if (M == 0) return NQ_OK;
    const size_t m = (size_t) M, m4 = 4 * m;
    return host_form(h, [&]() -> int {
        int* d_colors = nullptr;
        int16_t* d_index = nullptr;
        int32_t* d_tuple = nullptr;
        rc = upload_palette(h, palette, K);
        if (!rc) rc = out_index ? stage_room(h, h->d_short, 1, &m, &d_index) : stage_room(h, h->d_tuple, 1, &m4, &d_tuple);
        if (!rc) rc = stage_in(h, h->d_colors, 1, &m, &colors, &d_colors);
        DevParams P = dev_params(h, K);
        nq::ListsView lv;
        if (!rc) rc = prepare_lists(h, P, &lv);
        if (rc) return rc;
        const bool fast = h->use_fast_dither && fast_lookup_eligible(P, lv);
        if (d_index && fast) launch_fast_nearest_index(P, lv, h->d_palette.p, packed_lists(h), d_colors, M, d_index, h->stream);
        else if (d_index) launch_nearest_index(P, h->d_palette.p, lv, d_colors, M, d_index, h->stream);
        else if (fast) launch_fast_closest_tuple(P, lv, h->d_palette.p, packed_lists(h), d_colors, M, d_tuple, h->stream);
        else launch_closest_tuple(P, h->d_palette.p, lv, d_colors, M, d_tuple, h->stream);
        NQ_HIP(h, launch_status());
        rc = out_index ? stage_out(h, h->d_short, 1, &m, &out_index) : stage_out(h, h->d_tuple, 1, &m4, &out_closest4);
        if (rc) return rc;
        NQ_HIP(h, hipStreamSynchronize(h->stream));
        return NQ_OK;
    });
}

} // namespace

extern "C" {

int nq_abi_version(void) { return NQ_ABI_VERSION; }

int nq_create(int kind, int device, nq_handle** out) {
    if (!out) { g_create_error = "out is NULL"; return NQ_ERR_INVALID; }
    *out = nullptr;
    if (kind != NQ_KIND_RGB && kind != NQ_KIND_LAB) { g_create_error = "unknown kind"; return NQ_ERR_INVALID; }
    int count = 0;
    hipError_t e = hipGetDeviceCount(&count);
    if (e != hipSuccess || count <= 0) {
        g_create_error = "no HIP device available (libnquant_hip has no CPU fallback)";
        return NQ_ERR_NO_DEVICE;
    }
    if (device < 0 || device >= count) { g_create_error = "device ordinal out of range"; return NQ_ERR_INVALID; }
    nq_handle* h = new nq_handle();
    h->kind = kind; h->device = device;
    std::memset(&h->params, 0, sizeof h->params);
    h->params.kind = kind; h->params.transparentPixelIndex = -1; h->params.transparentColor = (int32_t) 0x00FFFFFFu;
    h->params.PR = 0.299; h->params.PG = 0.587; h->params.PB = 0.114; h->params.PA = .3333; h->params.ratio = .5; h->params.weight = 1;
    int rc = use_device(h);
    if (rc) { g_create_error = h->err; delete h; return rc; }
    *out = h;
    return NQ_OK;
}

void nq_destroy(nq_handle* h) {
    if (!h) return;
    (void) hipSetDevice(h->device);
    (void) hipStreamSynchronize(h->stream);
    delete h;
}

const char* nq_last_error(const nq_handle* h) { return h ? h->err.c_str() : g_create_error.c_str(); }

int nq_set_stream(nq_handle* h, void* hip_stream) {
    if (!h) return NQ_ERR_INVALID;
    h->stream = (hipStream_t) hip_stream;
    return NQ_OK;
}
int nq_set_tile(nq_handle* h, int tile_w, int tile_h) {
    if (!h) return NQ_ERR_INVALID;
    if (tile_w <= 0 || tile_h <= 0) { tile_w = 0; tile_h = 0; }
    h->tile_w = tile_w; h->tile_h = tile_h;
    return NQ_OK;
}
int nq_set_band(nq_handle* h, int y0, int image_height) {
    if (!h) return NQ_ERR_INVALID;
    if (y0 < 0 || image_height < 0 || (image_height == 0 && y0 != 0) || (image_height > 0 && y0 >= image_height))
        NQ_FAIL(h, NQ_ERR_INVALID, "nq_set_band: bad origin %d / image height %d", y0, image_height);
    h->band_y0 = y0; h->band_image_h = image_height;
    return NQ_OK;
}
int nq_get_list_counts(nq_handle* h, uint8_t* closest_counts, uint8_t* nearest_counts) {
    if (!h || !closest_counts || !nearest_counts) return NQ_ERR_INVALID;
    if (!h->sc->cell_lists.p) NQ_FAIL(h, NQ_ERR_INVALID, "no lists built yet");
    const size_t LB = (size_t) 65536 * 32;
    NQ_HIP(h, hipMemcpy(closest_counts, h->sc->cell_lists.p + 2 * LB, 65536, hipMemcpyDeviceToHost));
    NQ_HIP(h, hipMemcpy(nearest_counts, h->sc->cell_lists.p + 2 * LB + 65536, 65536, hipMemcpyDeviceToHost));
    return NQ_OK;
}
int nq_set_option(nq_handle* h, int option, int value) {
    if (!h) return NQ_ERR_INVALID;
    if (option == NQ_OPT_CELL_LISTS) { h->use_lists = value != 0; return NQ_OK; }
    if (option == NQ_OPT_FAST_DITHER) { h->use_fast_dither = value != 0; return NQ_OK; }
    if (option == NQ_OPT_DITHER_CHAIN) { h->dither_chain = value >= 0 && value <= 4 ? (int) value : 1; return NQ_OK; }
    if (option == NQ_OPT_MERGE_WALL_SECONDS) { h->merge_wall_s = value > 0 ? value : 0; return NQ_OK; }
    NQ_FAIL(h, NQ_ERR_INVALID, "unknown option %d", option);
}
int nq_selftest_ciede(nq_handle* h, const float* lab_pairs, int64_t n, uint32_t* out9) {
    int rc = use_device(h);
    if (rc) return rc;
    if (!lab_pairs || n <= 0 || !out9) NQ_FAIL(h, NQ_ERR_INVALID, "bad argument");
    float* d_in = nullptr; unsigned* d_out = nullptr;
    NQ_HIP(h, hipMalloc((void**) &d_in, (size_t) n * 6 * sizeof(float)));
    hipError_t e = hipMalloc((void**) &d_out, (size_t) n * 9 * sizeof(unsigned));
    if (e == hipSuccess) e = hipMemcpyAsync(d_in, lab_pairs, (size_t) n * 6 * sizeof(float), hipMemcpyHostToDevice, h->stream);
    if (e == hipSuccess) { launch_ciede_selftest(d_in, n, d_out, h->stream); e = hipGetLastError(); }
    if (e == hipSuccess) e = hipMemcpyAsync(out9, d_out, (size_t) n * 9 * sizeof(unsigned), hipMemcpyDeviceToHost, h->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    (void) hipFree(d_in); if (d_out) (void) hipFree(d_out);
    if (e != hipSuccess) NQ_FAIL(h, NQ_ERR_HIP, "nq_selftest_ciede: %s", hipGetErrorString(e));
    return NQ_OK;
}
int nq_selftest_fast(nq_handle* h, int which, const void* in, int64_t n, uint32_t* out) {
    int rc = use_device(h);
    if (rc) return rc;
    if (which < 0 || which >= NQ_FAST_ST_MODES || !in || n <= 0 || !out) NQ_FAIL(h, NQ_ERR_INVALID, "nq_selftest_fast: bad argument");
    // per mode: bytes of an explicit input record (0 = a range header {first, count, a0, a1}), output words per element (0 = the four
    // words of a counting form), end of the range's domain
    static const struct { int rec_bytes, out_words; int64_t domain; } k_mode[] = {
        {0, 2, (int64_t) 1 << 32}, {0, 3, 1 << 24}, {8, 3, 0}, {0, 1, (int64_t) 1 << 31}, {0, 0, (int64_t) 1 << 31}, {8, 1, 0}, {0, 0, 1 << 30},
        {24, 3, 0}, {0, 3, 1 << 24}, {0, 3, 1 << 24}, {0, 3, 1 << 24}, {0, 1, 1 << 24}, {8, 1, 0}, {4, 2, 0}, {4, 1, 0}, {8, 1, 0}, {8, 66, 0}};
    static_assert(sizeof k_mode / sizeof k_mode[0] == NQ_FAST_ST_MODES && NQ_FAST_ST_MODES == NQ_FAST_ST_JUMP + 1, "one row per NQ_FAST_ST_* mode, in their order");
    const auto& m = k_mode[which];
    const bool counting = m.out_words == 0;
    if (!counting && n > ((int64_t) 1 << 26)) NQ_FAIL(h, NQ_ERR_INVALID, "nq_selftest_fast: more than 2^26 elements in one call");
    int64_t first = 0, a0 = 0, a1 = 0;
    const void* up = in;              // what goes to the device
    size_t up_bytes = (size_t) n * (size_t) m.rec_bytes;
    if (m.rec_bytes == 0) {
        const int64_t* hdr = (const int64_t*) in;
        first = hdr[0]; a0 = hdr[2]; a1 = hdr[3];
        if (hdr[1] != n || first < 0 || first > m.domain || n > m.domain - first) NQ_FAIL(h, NQ_ERR_INVALID, "nq_selftest_fast: range outside the domain");
        up = nullptr;
        if (which == NQ_FAST_ST_CLOSEST_ERR && (a0 < 0 || a0 > 7)) NQ_FAIL(h, NQ_ERR_INVALID, "nq_selftest_fast: sign mask");
        if (which == NQ_FAST_ST_YDIFF_RANGE) {
            if (a1 < 0 || (a1 >> 1) > 32) NQ_FAIL(h, NQ_ERR_INVALID, "nq_selftest_fast: more than 32 thresholds");
            up = hdr + 4; up_bytes = (size_t) (a1 >> 1) * sizeof(double);
        }
    }
    const bool wants_palette = which == NQ_FAST_ST_NEAR_D32 || which == NQ_FAST_ST_NEAR_D32_PAIRS || which == NQ_FAST_ST_NEAR_SAFE;
    const int K = (int) h->dev_palette.size();
    if (wants_palette && (K < 1 || K > 256 || !h->d_palette.p)) NQ_FAIL(h, NQ_ERR_INVALID, "nq_selftest_fast: no palette of at most 256 entries on the device (run a lookup first)");
    if (which == NQ_FAST_ST_NEAR_D32 && (a0 < 0 || a0 >= K)) NQ_FAIL(h, NQ_ERR_INVALID, "nq_selftest_fast: palette index");
    const DevParams P = dev_params(h, wants_palette ? K : 0);
    const size_t out_bytes = counting ? 16 : (size_t) n * (size_t) m.out_words * sizeof(uint32_t);
    const uint64_t count_init[2] = {0, ~(uint64_t) 0};
    void* d_in = nullptr; unsigned* d_out = nullptr;
    hipError_t e = hipMalloc((void**) &d_out, out_bytes);
    if (e == hipSuccess && up_bytes) e = hipMalloc(&d_in, up_bytes);
    if (e == hipSuccess && up_bytes) e = hipMemcpyAsync(d_in, up, up_bytes, hipMemcpyHostToDevice, h->stream);
    if (e == hipSuccess && counting) e = hipMemcpyAsync(d_out, count_init, 16, hipMemcpyHostToDevice, h->stream);
    if (e == hipSuccess) { launch_fast_selftest(P, wants_palette ? h->d_palette.p : nullptr, which, d_in, first, n, a0, a1, d_out, h->stream); e = hipGetLastError(); }
    if (e == hipSuccess) e = hipMemcpyAsync(out, d_out, out_bytes, hipMemcpyDeviceToHost, h->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    if (d_in) (void) hipFree(d_in);
    if (d_out) (void) hipFree(d_out);
    if (e != hipSuccess) NQ_FAIL(h, NQ_ERR_HIP, "nq_selftest_fast: %s", hipGetErrorString(e));
    return NQ_OK;
}
int nq_get_dither_path(nq_handle* h, int32_t* out_fast, int32_t* out_failed_tiles) {
    if (!h) return NQ_ERR_INVALID;
    if (out_fast) *out_fast = h->last_dither_fast;
    if (out_failed_tiles) {
        *out_failed_tiles = 0;
        if (h->last_dither_fast && h->d_failed.p) {
            NQ_HIP(h, hipStreamSynchronize(h->stream));
            int cnt[2] = {0, 0};                   // {need count of the split form, hand-back count}
            NQ_HIP(h, hipMemcpy(cnt, h->d_failed.p, sizeof(cnt), hipMemcpyDeviceToHost));
            *out_failed_tiles = cnt[1];
            if (h->split_uncounted) { g_split_listed += cnt[0]; h->split_uncounted = false; }
        }
    }
    return NQ_OK;
}
int nq_get_dither_split_stats(int64_t* out3) {
    if (!out3) return NQ_ERR_INVALID;
    out3[0] = g_split_passes.load(); out3[1] = g_split_side.load(); out3[2] = g_split_listed.load();
    return NQ_OK;
}
int nq_get_params(const nq_handle* h, nq_params* out) {
    if (!h || !out) return NQ_ERR_INVALID;
    *out = h->params;
    return NQ_OK;
}
int nq_set_params(nq_handle* h, const nq_params* in) {
    if (!h || !in) return NQ_ERR_INVALID;
    h->params = *in; h->params.kind = h->kind;
    return NQ_OK;
}
int nq_get_merge_stats(const nq_handle* h, int64_t* out8) {
    if (!h || !out8) return NQ_ERR_INVALID;
    std::memcpy(out8, h->merge_stats, 16 * sizeof(long long));
    return NQ_OK;
}
int nq_get_team_stats(const nq_handle* h, int64_t* out16) {
    if (!h || !out16) return NQ_ERR_INVALID;
    std::memcpy(out16, h->team_stats, sizeof h->team_stats);
    return NQ_OK;
}
int nq_get_device_bytes(int64_t* out) {
    if (!out) return NQ_ERR_INVALID;
    *out = g_device_bytes.load();
    return NQ_OK;
}
int nq_get_merge_variant(const nq_handle* h, int32_t* out_threads, int32_t* out_helpers) {
    if (!h || !out_threads || !out_helpers) return NQ_ERR_INVALID;
    *out_threads = h->merge_variant[0]; *out_helpers = h->merge_variant[1];
    return NQ_OK;
}
int nq_get_batch_phase_ms(const nq_handle* h0, float* out4) {
    if (!h0 || !out4) return NQ_ERR_INVALID;
    std::memcpy(out4, h0->batch_phase_ms, sizeof h0->batch_phase_ms);
    return NQ_OK;
}
int nq_get_stage_ms(const nq_handle* h, float* out8) {
    if (!h || !out8) return NQ_ERR_INVALID;
    std::memcpy(out8, h->stage_ms, sizeof h->stage_ms);
    if (h->dither_events_fresh) {
        // a stand-alone nq_dither[_device] call (asynchronous: no finish_timing there): its two stages, once their events have completed
        float ms = 0;
        if (hipEventElapsedTime(&ms, h->ev[5], h->ev[6]) == hipSuccess) out8[5] = ms;
        if (hipEventElapsedTime(&ms, h->ev[6], h->ev[7]) == hipSuccess) out8[6] = ms;
    }
    return NQ_OK;
}

int nq_pnnquan_device(nq_handle* h, const uint32_t* d_argb, int width, int height, int nMaxColors,
                      uint32_t* out_palette, int32_t* out_K) {
    int rc = use_device(h);
    if (rc) return rc;
    return pnnquan_device(h, d_argb, width, height, nMaxColors, out_palette, out_K);
}

int nq_pnnquan(nq_handle* h, const uint32_t* argb, int width, int height, int nMaxColors, uint32_t* out_palette, int32_t* out_K) {
    int rc = use_device(h);
    if (rc) return rc;
    if (!argb || width <= 0 || height <= 0) NQ_FAIL(h, NQ_ERR_INVALID, "bad argument");
    const size_t px = (size_t) width * height;
    return host_images(h, 1, &px, &argb, nullptr, nullptr, [&](auto in, auto, auto) {
        return pnnquan_device(h, in[0], width, height, nMaxColors, out_palette, out_K);
    });
}

int nq_dither_device(nq_handle* h, const uint32_t* d_argb, int width, int height, const uint32_t* palette, int K,
                     int dither, int64_t rng_seed, int mode, uint32_t* d_out_argb, uint16_t* d_out_index) {
    int rc = use_device(h);
    if (rc) return rc;
    return dither_device(h, d_argb, width, height, palette, K, dither, rng_seed, mode, d_out_argb, d_out_index);
}

int nq_dither(nq_handle* h, const uint32_t* argb, int width, int height, const uint32_t* palette, int K,
              int dither, int64_t rng_seed, int mode, uint32_t* out_argb, uint16_t* out_index) {
    int rc = use_device(h);
    if (rc) return rc;
    if (!argb || !out_argb || width <= 0 || height <= 0) NQ_FAIL(h, NQ_ERR_INVALID, "bad argument");
    const size_t px = (size_t) width * height;
    return host_images(h, 1, &px, &argb, &out_argb, &out_index, [&](auto in, auto out, auto index) {
        return dither_device(h, in[0], width, height, palette, K, dither, rng_seed, mode, out[0], index[0]);
    });
}

// GilbertCurve.dither(width, height, pixels, palette, ditherable, saliencies, weight, dither) (NQ/GilbertCurve.java:367-373)
int nq_gilbert_dither(nq_handle* h, int width, int height, const uint32_t* pixels, const uint32_t* palette, int K, const float* saliencies,
                      double weight, int dither, int64_t rng_seed, int mode, int32_t* out_qpixels, uint16_t* out_index) {
    int rc = use_device(h);
    if (rc) return rc;
    if (!pixels || !out_qpixels || width <= 0 || height <= 0) NQ_FAIL(h, NQ_ERR_INVALID, "bad argument");
    rc = check_mode(h, mode, false);
    if (rc) return rc;
    const size_t px = (size_t) width * height;
    std::vector<uint16_t> idx(px);
    uint16_t* const idx_out = idx.data();
    // :278-279: qPixels holds ARGB only when dithering or K <= 32, palette indices otherwise
    uint32_t* const argb_out = dither || K <= 32 ? (uint32_t*) out_qpixels : nullptr;
    rc = host_images(h, 1, &px, &pixels, &argb_out, &idx_out, [&](auto in, auto out, auto index) {
        StageOverride ov;
        ov.gilbert_only = true; ov.hasSal = saliencies != nullptr; ov.weight = weight;
        float* d_sal = nullptr;
        const int rcs = saliencies ? stage_in(h, h->d_user_sal, 1, &px, &saliencies, &d_sal) : NQ_OK;
        if (rcs) return rcs;
        ov.d_sal = d_sal;
        return dither_device(h, in[0], width, height, palette, K, dither, rng_seed, mode, out[0], index[0], ov);
    });
    if (rc) return rc;
    if (!argb_out) for (size_t i = 0; i < px; ++i) out_qpixels[i] = idx[i];
    if (out_index) std::memcpy(out_index, idx.data(), px * sizeof(uint16_t));
    return NQ_OK;
}

// BlueNoise.dither(width, height, pixels, palette, ditherable, qPixels, weight) (NQ/BlueNoise.java:207-222): qPixels holds palette
// indices on entry and ARGB on return
int nq_bluenoise_dither(nq_handle* h, int width, int height, const uint32_t* pixels, const uint32_t* palette, int K, int32_t* io_qpixels,
                        float weight, int64_t rng_seed, int mode, uint16_t* out_index) {
    int rc = use_device(h);
    if (rc) return rc;
    if (!pixels || !io_qpixels || width <= 0 || height <= 0 || !palette || K < 1) NQ_FAIL(h, NQ_ERR_INVALID, "bad argument");
    rc = check_mode(h, mode, false);
    if (rc) return rc;
    const size_t px = (size_t) width * height;
    std::vector<uint16_t> idx(px);
    for (size_t i = 0; i < px; ++i) {
        if (io_qpixels[i] < 0 || io_qpixels[i] >= K) NQ_FAIL(h, NQ_ERR_INVALID, "qPixels[%zu] = %d is not a palette index", i, io_qpixels[i]);
        idx[i] = (uint16_t) io_qpixels[i];
    }
    const uint16_t* const idx_in = idx.data();
    uint32_t* const argb_out = (uint32_t*) io_qpixels;
    return host_images(h, 1, &px, &pixels, &argb_out, &out_index, [&](auto in, auto out, auto index) -> int {
        const int rci = stage_in(h, h->d_out_index, 1, &px, &idx_in, index);
        if (rci) return rci;
        NQ_HIP(h, hipStreamSynchronize(h->stream));        // (the indices are in place before the pass)
        StageOverride ov;
        ov.blue_only = true; ov.blueWeight = weight; ov.weight = h->params.weight;
        return dither_device(h, in[0], width, height, palette, K, 0, rng_seed, mode, out[0], index[0], ov);
    });
}

int nq_convert_device(nq_handle* h, const uint32_t* d_argb, int width, int height, int nMaxColors, int dither,
                      int64_t rng_seed, int mode, uint32_t* d_out_argb, uint16_t* d_out_index,
                      uint32_t* out_palette, int32_t* out_K) {
    int rc = use_device(h);
    if (rc) return rc;
    rc = pnnquan_device(h, d_argb, width, height, nMaxColors, out_palette, out_K);
    if (rc) return rc;
    rc = dither_device(h, d_argb, width, height, out_palette, *out_K, dither, rng_seed, mode, d_out_argb, d_out_index);
    if (rc) return rc;
    NQ_HIP(h, hipStreamSynchronize(h->stream));
    finish_timing(h);
    return NQ_OK;
}

// ---- one palette for a sequence of frames ----
int nq_pnnquan_frames_device(nq_handle* h, int n, const uint32_t* const* d_argb, const int32_t* widths, const int32_t* heights,
                             int nMaxColors, uint32_t* out_palette, int32_t* out_K) {
    if (!h) return NQ_ERR_INVALID;
    int rc = frames_check(h, n, d_argb, widths, heights, nMaxColors, false, nullptr);
    if (rc) return rc;
    if (!out_palette || !out_K) NQ_FAIL(h, NQ_ERR_INVALID, "bad argument");
    rc = use_device(h);
    if (rc) return rc;
    FramesScope scope(h);
    rc = frames_upload(h, n, d_argb, widths, heights);
    if (rc) return rc;
    return palette_of(h, out_palette, out_K, [&](PaletteJob* job) { return pnnquan_frames_prepare(h, nMaxColors, out_palette, out_K, job); });
}

int nq_convert_frames_refined_device(nq_handle* h, int n, const uint32_t* const* d_argb, const int32_t* widths, const int32_t* heights,
                                     int nMaxColors, int refine, int dither, const int64_t* rng_seeds, int mode,
                                     uint32_t* const* d_out_argb, uint16_t* const* d_out_index, uint32_t* out_palette, int32_t* out_K) {
    if (!h) return NQ_ERR_INVALID;
    int64_t total = 0;
    int rc = frames_check(h, n, d_argb, widths, heights, nMaxColors, true, &total);
    if (rc) return rc;
    rc = refine_check_convert(h, refine, nMaxColors);
    if (rc) return rc;
    for (int i = 0; refine > 0 && i < n; ++i)
        if ((uintptr_t) d_argb[i] & 3) NQ_FAIL(h, NQ_ERR_INVALID, "frame %d: refine needs a 4-byte aligned pixel pointer", i);
    if (!rng_seeds || !d_out_argb || !out_palette || !out_K) NQ_FAIL(h, NQ_ERR_INVALID, "bad argument");
    for (int i = 0; i < n; ++i) if (!d_out_argb[i]) NQ_FAIL(h, NQ_ERR_INVALID, "frame %d: null output pointer", i);
    rc = check_mode(h, mode);
    if (rc) return rc;
    rc = use_device(h);
    if (rc) return rc;
    FramesScope scope(h);
    rc = frames_upload(h, n, d_argb, widths, heights);
    if (rc) return rc;
    rc = palette_of(h, out_palette, out_K, [&](PaletteJob* job) { return pnnquan_frames_prepare(h, nMaxColors, out_palette, out_K, job); });
    if (rc) return rc;
    const int K = *out_K;
    if (refine > 0) {                               // `refine` update passes over the same frames; the params stay pnnquan's
        int64_t sse[65];
        int32_t passes = 0;
        rc = refine_device(h, n, d_argb, widths, heights, total, out_palette, K, refine, sse, nullptr, &passes);
        if (rc) return rc;
    }
    nq_params& p = h->params;
    // the BlueNoise weight of convert(n, false) counts the SEQUENCE's distinct colours (what dither_device would count for one image)
    if (h->kind == NQ_KIND_LAB && !dither && K > 32 && mode == NQ_MODE_PARALLEL_TILED && p.distinctColors <= 0) {
        int64_t cnt = 0;
        rc = distinct_colors(h, nullptr, total, 0, &cnt, nullptr);
        if (rc) return rc;
        p.distinctColors = cnt;
    }
    // frame after frame on the stream, no host wait in between; the candidate lists are built for the first frame only.  Stage events:
    // `dither` runs from the first frame's dither pass to the last frame's end (BlueNoise post-passes included, `bluenoise` = 0)
    h->frames_active = false;
    h->reuse_lists = true;
    for (int i = 0; i < n; ++i) {
        if (n > 1) h->rec_skip = i == 0 ? (1u << 6 | 1u << 7) : (1u << 5 | 1u << 6 | 1u << 7);
        rc = dither_device(h, d_argb[i], widths[i], heights[i], out_palette, K, dither, rng_seeds[i], mode, d_out_argb[i],
                           d_out_index ? d_out_index[i] : nullptr);
        if (rc) { h->err = "frame " + std::to_string(i) + ": " + h->err; return rc; }
    }
    h->rec_skip = 0;
    if (n > 1) { rec(h, 6); rec(h, 7); }
    NQ_HIP(h, hipStreamSynchronize(h->stream));
    finish_timing(h);
    return NQ_OK;
}

int nq_convert_frames_device(nq_handle* h, int n, const uint32_t* const* d_argb, const int32_t* widths, const int32_t* heights,
                             int nMaxColors, int dither, const int64_t* rng_seeds, int mode,
                             uint32_t* const* d_out_argb, uint16_t* const* d_out_index, uint32_t* out_palette, int32_t* out_K) {
    return nq_convert_frames_refined_device(h, n, d_argb, widths, heights, nMaxColors, 0, dither, rng_seeds, mode, d_out_argb, d_out_index,
                                            out_palette, out_K);
}

int nq_convert_frames_refined(nq_handle* h, int n, const uint32_t* const* argb, const int32_t* widths, const int32_t* heights,
                              int nMaxColors, int refine, int dither, const int64_t* rng_seeds, int mode,
                              uint32_t* const* out_argb, uint16_t* const* out_index, uint32_t* out_palette, int32_t* out_K) {
    if (!h) return NQ_ERR_INVALID;
    int rc = frames_check(h, n, argb, widths, heights, nMaxColors, true, nullptr);
    if (rc) return rc;
    rc = refine_check_convert(h, refine, nMaxColors);
    if (rc) return rc;
    if (!out_argb || !rng_seeds || !out_palette || !out_K) NQ_FAIL(h, NQ_ERR_INVALID, "bad argument");
    for (int i = 0; i < n; ++i) if (!out_argb[i]) NQ_FAIL(h, NQ_ERR_INVALID, "frame %d: null output pointer", i);
    rc = check_mode(h, mode);
    if (rc) return rc;
    rc = use_device(h);
    if (rc) return rc;
    std::vector<size_t> px(n);
    for (int i = 0; i < n; ++i) px[i] = (size_t) widths[i] * heights[i];
    return host_images(h, n, px.data(), argb, out_argb, out_index, [&](auto in, auto out, auto index) {
        return nq_convert_frames_refined_device(h, n, in, widths, heights, nMaxColors, refine, dither, rng_seeds, mode, out, index, out_palette,
                                                out_K);
    });
}

int nq_convert_frames(nq_handle* h, int n, const uint32_t* const* argb, const int32_t* widths, const int32_t* heights,
                      int nMaxColors, int dither, const int64_t* rng_seeds, int mode,
                      uint32_t* const* out_argb, uint16_t* const* out_index, uint32_t* out_palette, int32_t* out_K) {
    return nq_convert_frames_refined(h, n, argb, widths, heights, nMaxColors, 0, dither, rng_seeds, mode, out_argb, out_index, out_palette, out_K);
}

// Finish phase of the batch entry points: every handle's chain_stream for the dither passes that follow.  With S scratch sets (the per-pixel
// scratch of the first S handles) image i takes set i % S; a set goes prep(i) -> light(i) -> chain and hand-back(i), and its next user
// starts behind chain_done of image i - S.  The caller joins the last S images at the end of the phase.  Two forms:
//  - with a prep stream (*prep set; nq_convert_batch_device with n >= 2): lists, Lab table, saliency map and counter clear of image i go
//    onto *prep (dither_device, prep_stream), beside the light pass of the images in front of it; S = min(4, n) sets, the chain passes
//    alternate over two side streams (NQ_FINISH_CHAIN_STREAMS=1: one).  With four sets the prep stream runs up to two images ahead and
//    nothing else throttles it.  Launch, prep and two chain streams: four streams, the lanes of the prepare phase again.
//  - without (prep == null, a single image, or NQ_FINISH_PREP=0): the lists stay on the launch stream; S = 2, one side stream, sets by
//    image parity, and image i on side stream i % (S - 1).
// NQ_FINISH_SETS = 2..4 overrides S in both, bounded by the number of handles.  *sets = S, side[0..2] = the chain streams and side[3] = the
// prep stream, or *sets = 0 with NQ_DITHER_SIDE_STREAM=0 (A/B timing): the split form in plain serial order on the main stream, no
// prep stream.  The BatchGuard of the call takes chain_stream, prep_stream and set_free back.
int finish_side_streams(nq_handle* h0, nq_handle* const* hs, int n, int* sets, hipStream_t side[4], hipStream_t* prep = nullptr) {
    *sets = 0;
    side[0] = side[1] = side[2] = side[3] = nullptr;
    if (prep) *prep = nullptr;
    bool use_side = true;
    if (const char* e = std::getenv("NQ_DITHER_SIDE_STREAM")) use_side = std::atoi(e) != 0;
    if (!use_side) {
        for (int i = 0; i < n; ++i) hs[i]->chain_stream = hs[i]->stream;
        return NQ_OK;
    }
    bool use_prep = prep && n > 1;
    if (const char* e = std::getenv("NQ_FINISH_PREP")) use_prep = use_prep && std::atoi(e) != 0;
    int S = use_prep ? 4 : 2;
    if (const char* e = std::getenv("NQ_FINISH_SETS")) { const int v = std::atoi(e); if (v >= 2 && v <= 4) S = v; }
    S = std::max(2, std::min(S, n));
    int C = S - 1;                    // chain streams
    if (use_prep) {
        C = 2;
        if (const char* e = std::getenv("NQ_FINISH_CHAIN_STREAMS")) { const int v = std::atoi(e); if (v == 1 || v == 2) C = v; }
    }
    auto lane = [&](int k) -> hipStream_t* { return k == 0 ? &h0->lane_stream : &h0->more_lanes[k - 1]; };
    for (int k = 0; k < C + (use_prep ? 1 : 0); ++k)
        if (!*lane(k)) NQ_HIP(h0, hipStreamCreateWithFlags(lane(k), hipStreamNonBlocking));
    for (int k = 0; k < C; ++k) side[k] = *lane(k);
    if (use_prep) side[3] = *prep = *lane(C);
    for (int i = 0; i < n; ++i) {
        if (!hs[i]->chain_gate) NQ_HIP(h0, hipEventCreateWithFlags(&hs[i]->chain_gate, hipEventDisableTiming));
        if (!hs[i]->chain_done) NQ_HIP(h0, hipEventCreateWithFlags(&hs[i]->chain_done, hipEventDisableTiming));
        if (use_prep && !hs[i]->prep_done) NQ_HIP(h0, hipEventCreateWithFlags(&hs[i]->prep_done, hipEventDisableTiming));
        hs[i]->chain_stream = side[i % C];
        hs[i]->prep_stream = side[3];
    }
    *sets = S;
    return NQ_OK;
}

int nq_convert_batch_device(nq_handle* const* hs, int n, const uint32_t* const* d_argb, const int32_t* widths, const int32_t* heights,
                            int nMaxColors, int dither, const int64_t* rng_seeds, int mode,
                            uint32_t* const* d_out_argb, uint16_t* const* d_out_index,
                            uint32_t* out_palettes, int32_t palette_stride, int32_t* out_K) {
    if (!hs || n <= 0 || !hs[0]) return NQ_ERR_INVALID;
    nq_handle* h0 = hs[0];
    int rc = batch_check(hs, n, d_argb, widths, heights, nMaxColors, rng_seeds, d_out_argb, out_palettes, palette_stride, out_K, false);
    if (rc) return rc;
    // The per-image stages in front of the merge loops run on FOUR lanes by default, eight at most (image i: stream and per-pixel scratch of
    // lane i % L; the scratch is that of the first L handles): while the host waits for a read-back of one image, and while a kernel with a
    // long tail or a small grid runs (the fullest bin's chain of the histogram, the list compactions), the queued kernels of the
    // other lanes keep the GPU busy (NQ_BATCH_LANES = 1..8 overrides).  The merge launch joins the lanes.
    BatchGuard guard(hs, n);
    for (int i = 0; i < n; ++i) hs[i]->light_events = i >= 16;
    rc = batch_use_device(hs, n);
    if (rc) return rc;
    if (n > 1 && !h0->lane_stream) NQ_HIP(h0, hipStreamCreateWithFlags(&h0->lane_stream, hipStreamNonBlocking));
    int L = std::min(n, 4);          // (measured on 1024 images of 4096^2, ONE issuing thread: prepare phase 640 / 557 / 552 / 543 us per image with 1 / 2 / 3 / 4 lanes)
    if (const char* f = std::getenv("NQ_BATCH_LANES")) { const int t = std::atoi(f); if (t >= 1 && t <= 8) L = std::min(t, n); }
    hipStream_t lane_s[8] = {h0->stream, n > 1 ? h0->lane_stream : h0->stream, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    Scratch* lane_sc[8] = {&h0->own, n > 1 ? &hs[1]->own : &h0->own, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    for (int k = 2; k < L; ++k) {
        if (!h0->more_lanes[k - 2]) NQ_HIP(h0, hipStreamCreateWithFlags(&h0->more_lanes[k - 2], hipStreamNonBlocking));
        lane_s[k] = h0->more_lanes[k - 2]; lane_sc[k] = &hs[k]->own;
    }
    for (int i = 0; i < n; ++i) { hs[i]->stream = lane_s[i % L]; hs[i]->sc = lane_sc[i % L]; }
    std::vector<PaletteJob> jobs(n);
    std::vector<const PaletteJob*> jp(n);
    (void) hipEventRecord(h0->bev[0], lane_s[0]);
    // The lanes are streams of their own (non-blocking: they do not follow the NULL stream either), and the caller may have queued the
    // producer of d_argb[] on the first handle's stream: every other lane starts behind what that stream holds now.  No host wait; the
    // join in front of the merge launch orders the other direction.  (tests/test_gpu_streams.py, part B)
    for (int k = 1; k < L; ++k)
        if (lane_s[k] != lane_s[0]) {
            if (k == 1) NQ_HIP(h0, hipEventRecord(h0->lane_gate, lane_s[0]));
            NQ_HIP(h0, hipStreamWaitEvent(lane_s[k], h0->lane_gate, 0));
        }
    {
        // One host thread per lane (round 4): pnnquan_prepare waits twice for the device per image (the pre-scan's scalars, the bin count),
        // and a single issuing thread that blocks there leaves the other lanes without new work -- only two images ever overlapped.  Lane k's
        // thread walks the images k, k + L, ... in order (they share lane k's scratch); handles, streams and scratch sets of different lanes
        // are disjoint, the launch-error slot is per thread.
        std::vector<int> lane_rc(L, NQ_OK), lane_bad(L, -1);
        auto lane_work = [&](int k) {
            int at = k;
            try {                                        // (nothing may leave a lane's thread: an escaping exception would end the process)
                if (hipSetDevice(h0->device) != hipSuccess) { lane_rc[k] = NQ_ERR_HIP; lane_bad[k] = k; hs[k]->err = "hipSetDevice failed in a batch lane"; return; }
                for (int i = k; i < n; i += L) {
                    at = i;
                    const int rc = pnnquan_prepare(hs[i], d_argb[i], widths[i], heights[i], nMaxColors, out_palettes + (size_t) i * palette_stride,
                                                   out_K + i, &jobs[i]);
                    if (rc) { lane_rc[k] = rc; lane_bad[k] = i; return; }
                    jp[i] = &jobs[i];
                }
                // the launch errors of this lane's prepares are kept on this thread: only it can see them
                const hipError_t e = launch_status();
                if (e != hipSuccess) {
                    lane_rc[k] = NQ_ERR_HIP; lane_bad[k] = at;
                    hs[at]->err = std::string("launch_status() failed in a batch lane: ") + hipGetErrorString(e);
                }
            } catch (const std::exception& e) {
                lane_rc[k] = NQ_ERR_HIP; lane_bad[k] = at;
                try { hs[at]->err = std::string("exception in a batch lane: ") + e.what(); } catch (...) {}
            } catch (...) { lane_rc[k] = NQ_ERR_HIP; lane_bad[k] = at; }
        };
        std::vector<std::thread> workers;
        std::vector<int> inline_lanes;                   // (a lane whose thread could not be created is walked by the caller's thread)
        for (int k = 1; k < L; ++k) {
            try { workers.emplace_back(lane_work, k); } catch (const std::exception&) { inline_lanes.push_back(k); }
        }
        lane_work(0);
        for (int k : inline_lanes) lane_work(k);
        for (auto& t : workers) t.join();
        // a failed lane ends the call: the kernels the other lanes have queued write their handles' buffers and the lane scratch, and the
        // lane streams do not synchronise with the handles' own streams -- nothing of this call may still run when the handles are used again
        if (std::any_of(lane_rc.begin(), lane_rc.end(), [](int r) { return r != NQ_OK; }))
            for (int k = 0; k < L; ++k) (void) hipStreamSynchronize(lane_s[k]);
        for (int k = 0; k < L; ++k)
            if (lane_rc[k]) return batch_fail(h0, hs[lane_bad[k] >= 0 && lane_bad[k] < n ? lane_bad[k] : 0], lane_rc[k]);
    }
    for (int k = 1; k < L; ++k) NQ_HIP(h0, hipStreamSynchronize(lane_s[k]));          // every prepare has been issued: join before the merge launch
    (void) hipEventRecord(h0->bev[1], lane_s[0]);
    std::vector<int> order;
    rc = merge_launch(h0, jp.data(), n, &order);
    if (rc) return rc;
    (void) hipEventRecord(h0->bev[2], lane_s[0]);
    // behind the merge launch everything runs on lane 0 again: two dither kernels side by side would only slow each other down
    for (int i = 0; i < n; ++i) { hs[i]->stream = lane_s[0]; hs[i]->sc = lane_sc[0]; }
    for (int i = 0; i < n; ++i) if (jobs[i].merge) rec(hs[i], 4);
    // every palette of the batch comes back behind ONE wait; the per-image passes then follow each other on the stream with no
    // host round trip in between (a wait per image left the GPU idle for ~0.1 ms of every image's ~1 ms).  And in ONE copy: a kernel
    // gathers every job's palette and read-back words (palette_fetch's two copies per image) into one block, which lands in page-locked
    // memory; slot j of it belongs to image order[j].  (Stage event 5 is recorded by the image's dither pass.)
    const size_t n_jobs = order.size();
    size_t slot_words = 0;
    if (n_jobs) {
        int max_plen = 0;
        for (int i : order) max_plen = std::max(max_plen, jobs[i].plen);
        slot_words = 37 + ((size_t) max_plen + 1) / 2;
        NQ_HIP(h0, h0->d_readback.reserve(n_jobs * slot_words));
        if (h0->h_readback_words < n_jobs * slot_words) {
            if (h0->h_readback) { (void) hipHostFree(h0->h_readback); h0->h_readback = nullptr; h0->h_readback_words = 0; }
            NQ_HIP(h0, hipHostMalloc((void**) &h0->h_readback, n_jobs * slot_words * sizeof(long long), hipHostMallocDefault));
            h0->h_readback_words = n_jobs * slot_words;
        }
        nq::launch_merge_readback(h0->d_jobs.p, (int) n_jobs, h0->d_readback.p, (long long) slot_words, lane_s[0]);
        NQ_HIP(h0, hipMemcpyAsync(h0->h_readback, h0->d_readback.p, n_jobs * slot_words * sizeof(long long), hipMemcpyDeviceToHost, lane_s[0]));
    }
    NQ_HIP(h0, hipStreamSynchronize(lane_s[0]));
    NQ_HIP(h0, launch_status());
    for (size_t j = 0; j < n_jobs; ++j) {
        const int i = order[j];
        const long long* slot = h0->h_readback + j * slot_words;
        uint32_t* pal = out_palettes + (size_t) i * palette_stride;
        std::memcpy(hs[i]->merge_readback, slot, sizeof hs[i]->merge_readback);
        std::memcpy(pal, slot + 37, (size_t) jobs[i].plen * sizeof(uint32_t));
        hs[i]->fetched_palette = pal; hs[i]->fetched_len = jobs[i].plen;       // (what palette_fetch leaves for palette_check)
    }
    for (int i = 0; i < n; ++i)
        if (jobs[i].merge) {
            rc = palette_check(hs[i], jobs[i], out_K + i);
            if (rc) return batch_fail(h0, hs[i], rc);
        }
    // The chain pass and the hand-back pass of image i (a few wavefronts, one chain's latency) run on a side stream beside the lists,
    // saliency map and light kernel of image i + 1 (dither_device, chain_stream).  What they read of the per-image scratch -- saliency plane,
    // list records -- rotates through S sets (finish_side_streams); image i's side work ends before image i + S reuses its set, and the main
    // stream waits for it at the end of the phase.  With a prep stream the lists and the saliency map of image i + 1 run there, beside the
    // light kernel of image i, and the main stream keeps the light kernels alone.
    int S = 0;
    hipStream_t prep = nullptr;
    rc = finish_side_streams(h0, hs, n, &S, guard.side, &prep);
    if (rc) return batch_fail(h0, h0, rc);
    for (int i = 0; i < n; ++i) {
        uint32_t* pal = out_palettes + (size_t) i * palette_stride;
        if (S) {
            hs[i]->sc = &hs[n > 1 ? i % S : 0]->own;
            // the set's first writer waits for the dither work of image i - S: the prep stream (dither_device, set_free), else this stream
            if (prep) hs[i]->set_free = i >= S ? hs[i - S]->chain_done : nullptr;
            else if (i >= S && hs[i - S]->chain_on_side) NQ_HIP(h0, hipStreamWaitEvent(lane_s[0], hs[i - S]->chain_done, 0));
        }
        rc = dither_device(hs[i], d_argb[i], widths[i], heights[i], pal, out_K[i], dither, rng_seeds[i], mode, d_out_argb[i],
                           d_out_index ? d_out_index[i] : nullptr);
        if (rc) return batch_fail(h0, hs[i], rc);
        // (a pass that ended on this stream: chain_done marks its end here, for the prep stream of image i + S)
        if (prep && !hs[i]->chain_on_side && i + S < n) NQ_HIP(h0, hipEventRecord(hs[i]->chain_done, lane_s[0]));
    }
    // (the prep stream needs no join of its own: this stream has waited for prep_done of the last image, and the stream runs in order)
    for (int i = std::max(0, n - std::max(S, 2)); i < n; ++i)
        if (hs[i]->chain_on_side) NQ_HIP(h0, hipStreamWaitEvent(lane_s[0], hs[i]->chain_done, 0));
    (void) hipEventRecord(h0->bev[3], lane_s[0]);
    NQ_HIP(h0, hipStreamSynchronize(lane_s[0]));
    for (int i = 0; i < n; ++i) finish_timing(hs[i]);
    finish_batch_timing(h0);
    return NQ_OK;
}

// Host-buffer form of the batch: uploads run ahead of the per-image stages on a copy stream, every image's result is copied
// back while the next image is dithered (a ring of three device output buffers), so only the inputs (4 B/pixel) and the
// quantizer state stay resident for the whole batch.
int nq_convert_batch(nq_handle* const* hs, int n, const uint32_t* const* argb, const int32_t* widths, const int32_t* heights,
                     int nMaxColors, int dither, const int64_t* rng_seeds, int mode,
                     uint32_t* const* out_argb, uint16_t* const* out_index,
                     uint32_t* out_palettes, int32_t palette_stride, int32_t* out_K) {
    if (!hs || n <= 0 || !hs[0]) return NQ_ERR_INVALID;
    nq_handle* h0 = hs[0];
    int rc = batch_check(hs, n, argb, widths, heights, nMaxColors, rng_seeds, out_argb, out_palettes, palette_stride, out_K, true);
    if (rc) return rc;
    BatchGuard guard(hs, n);
    rc = batch_use_device(hs, n);
    if (rc) return rc;
    size_t max_px = 0;
    for (int i = 0; i < n; ++i) {
        max_px = std::max(max_px, (size_t) widths[i] * heights[i]);
        NQ_HIP(h0, hs[i]->d_in.reserve((size_t) widths[i] * heights[i]));
        hs[i]->stream = h0->stream; hs[i]->sc = &h0->own;
    }
    constexpr int RING = 3;
    for (int r = 0; r < RING; ++r) { NQ_HIP(h0, h0->ring_argb[r].reserve(max_px)); NQ_HIP(h0, h0->ring_index[r].reserve(max_px)); }
    if (!h0->copy_stream) NQ_HIP(h0, hipStreamCreateWithFlags(&h0->copy_stream, hipStreamNonBlocking));
    hipStream_t cs = h0->copy_stream;
    auto new_event = [&](hipEvent_t* e) -> hipError_t {
        hipError_t rc = hipEventCreateWithFlags(e, hipEventDisableTiming);
        if (rc == hipSuccess) guard.events.push_back(*e);
        return rc;
    };
    std::vector<hipEvent_t> ev_up(n), ev_done(n), ev_dl(n);
    for (int i = 0; i < n; ++i) { NQ_HIP(h0, new_event(&ev_up[i])); NQ_HIP(h0, new_event(&ev_done[i])); NQ_HIP(h0, new_event(&ev_dl[i])); }
    int uploaded = 0;
    auto upload_until = [&](int last) -> int {          // asynchronous when the caller's buffers are page-locked
        for (; uploaded <= last && uploaded < n; ++uploaded) {
            const int i = uploaded;
            NQ_HIP(h0, hipMemcpyAsync(hs[i]->d_in.p, argb[i], (size_t) widths[i] * heights[i] * sizeof(int), hipMemcpyHostToDevice, cs));
            NQ_HIP(h0, hipEventRecord(ev_up[i], cs));
        }
        return NQ_OK;
    };
    std::vector<PaletteJob> jobs(n);
    std::vector<const PaletteJob*> jp(n);
    (void) hipEventRecord(h0->bev[0], h0->stream);
    for (int i = 0; i < n; ++i) {
        rc = upload_until(i + 2);
        if (rc) return rc;
        NQ_HIP(h0, hipStreamWaitEvent(h0->stream, ev_up[i], 0));
        rc = pnnquan_prepare(hs[i], hs[i]->d_in.p, widths[i], heights[i], nMaxColors,
                             out_palettes + (size_t) i * palette_stride, out_K + i, &jobs[i]);
        if (rc) return batch_fail(h0, hs[i], rc);
        jp[i] = &jobs[i];
    }
    (void) hipEventRecord(h0->bev[1], h0->stream);
    rc = merge_launch(h0, jp.data(), n);
    if (rc) return rc;
    (void) hipEventRecord(h0->bev[2], h0->stream);
    for (int i = 0; i < n; ++i) if (jobs[i].merge) rec(hs[i], 4);
    // (the chain pass of image i beside the light kernel of image i + 1, S scratch sets in rotation: as in nq_convert_batch_device)
    int S = 0;
    rc = finish_side_streams(h0, hs, n, &S, guard.side);
    if (rc) return batch_fail(h0, h0, rc);
    for (int i = 0; i < n; ++i) {
        uint32_t* pal = out_palettes + (size_t) i * palette_stride;
        if (jobs[i].merge) {
            rc = palette_finish(hs[i], jobs[i], pal, out_K + i);
            if (rc) return batch_fail(h0, hs[i], rc);
        }
        const int r = i % RING;
        if (i >= RING) NQ_HIP(h0, hipStreamWaitEvent(h0->stream, ev_dl[i - RING], 0));     // the slot's previous result has left
        if (S) {
            hs[i]->sc = &hs[n > 1 ? i % S : 0]->own;
            if (i >= S && hs[i - S]->chain_on_side) NQ_HIP(h0, hipStreamWaitEvent(h0->stream, hs[i - S]->chain_done, 0));
        }
        rc = dither_device(hs[i], hs[i]->d_in.p, widths[i], heights[i], pal, out_K[i], dither, rng_seeds[i], mode,
                           (uint32_t*) h0->ring_argb[r].p, h0->ring_index[r].p);
        if (rc) return batch_fail(h0, hs[i], rc);
        NQ_HIP(h0, hipEventRecord(ev_done[i], h0->stream));
        NQ_HIP(h0, hipStreamWaitEvent(cs, ev_done[i], 0));
        if (hs[i]->chain_on_side) NQ_HIP(h0, hipStreamWaitEvent(cs, hs[i]->chain_done, 0));
        const size_t px = (size_t) widths[i] * heights[i];
        NQ_HIP(h0, hipMemcpyAsync(out_argb[i], h0->ring_argb[r].p, px * sizeof(int), hipMemcpyDeviceToHost, cs));
        if (out_index && out_index[i])
            NQ_HIP(h0, hipMemcpyAsync(out_index[i], h0->ring_index[r].p, px * sizeof(uint16_t), hipMemcpyDeviceToHost, cs));
        NQ_HIP(h0, hipEventRecord(ev_dl[i], cs));
    }
    for (int i = std::max(0, n - std::max(S, 2)); i < n; ++i)
        if (hs[i]->chain_on_side) NQ_HIP(h0, hipStreamWaitEvent(h0->stream, hs[i]->chain_done, 0));
    (void) hipEventRecord(h0->bev[3], h0->stream);
    NQ_HIP(h0, hipStreamSynchronize(h0->stream));
    NQ_HIP(h0, hipStreamSynchronize(cs));
    for (int i = 0; i < n; ++i) finish_timing(hs[i]);
    finish_batch_timing(h0);
    return NQ_OK;
}

int nq_convert(nq_handle* h, const uint32_t* argb, int width, int height, int nMaxColors, int dither,
               int64_t rng_seed, int mode, uint32_t* out_argb, uint16_t* out_index, uint32_t* out_palette, int32_t* out_K) {
    int rc = use_device(h);
    if (rc) return rc;
    if (!argb || !out_argb || width <= 0 || height <= 0) NQ_FAIL(h, NQ_ERR_INVALID, "bad argument");
    const size_t px = (size_t) width * height;
    return host_images(h, 1, &px, &argb, &out_argb, &out_index, [&](auto in, auto out, auto index) {
        return nq_convert_device(h, in[0], width, height, nMaxColors, dither, rng_seed, mode, out[0], index[0], out_palette, out_K);
    });
}

int nq_nearest_index(nq_handle* h, const uint32_t* palette, int K, const uint32_t* colors, int64_t M, int16_t* out_index) {
    return color_lookup(h, palette, K, colors, M, out_index, nullptr);
}

int nq_closest_tuple(nq_handle* h, const uint32_t* palette, int K, const uint32_t* colors, int64_t M, int32_t* out_closest4) {
    return color_lookup(h, palette, K, colors, M, nullptr, out_closest4);
}

int nq_band_scan_device(nq_handle* h, const uint32_t* d_argb, int64_t n_pixels, int64_t index_offset, int nMaxColors, int64_t* d_scan3) {
    int rc = use_device(h);
    if (rc) return rc;
    if (!d_argb || n_pixels <= 0 || !d_scan3) NQ_FAIL(h, NQ_ERR_INVALID, "bad argument");
    (void) nMaxColors;
    launch_prescan((const int*) d_argb, n_pixels, index_offset, (long long*) d_scan3, h->stream);
    NQ_HIP(h, launch_status());
    return NQ_OK;
}

int nq_set_scan(nq_handle* h, int nMaxColors, int64_t transparent_index, uint32_t transparent_color, int64_t semi_count) {
    if (!h) return NQ_ERR_INVALID;
    apply_scan(h, nMaxColors, transparent_index, transparent_color, semi_count);
    // a new image's split round: the distinct colours handed over for the image before say nothing about this one (they used to stay valid
    // for the handle's life, and a later few-colours image without nq_set_distinct took its palette from them instead of NQ_ERR_UNSUPPORTED)
    h->ext_distinct_valid = false; h->ext_distinct_many = false; h->ext_distinct.clear();
    return NQ_OK;
}

int nq_band_distinct_device(nq_handle* h, const uint32_t* d_argb, int64_t n_pixels, int cap, int64_t* out_count, uint32_t* out_colors) {
    int rc = use_device(h);
    if (rc) return rc;
    if (!d_argb || n_pixels <= 0 || cap < 1 || !out_count || !out_colors) NQ_FAIL(h, NQ_ERR_INVALID, "bad argument");
    std::vector<int32_t> cols;
    rc = distinct_colors(h, d_argb, n_pixels, cap, out_count, &cols);
    if (rc) return rc;
    if (*out_count <= cap) std::memcpy(out_colors, cols.data(), cols.size() * sizeof(int32_t));
    return NQ_OK;
}

int nq_band_color_presence_device(nq_handle* h, const uint32_t* d_argb, int64_t n_pixels, uint8_t* d_presence, int cap_other,
                                  int64_t* out_other_count, uint32_t* out_other) {
    int rc = use_device(h);
    if (rc) return rc;
    if (!d_argb || n_pixels <= 0 || !d_presence || cap_other < 1 || !out_other_count || !out_other) NQ_FAIL(h, NQ_ERR_INVALID, "bad argument");
    const unsigned slots = 1u << 18;
    if ((unsigned) cap_other > slots / 2) NQ_FAIL(h, NQ_ERR_INVALID, "cap_other above %u", slots / 2);
    NQ_HIP(h, h->sc->dk_a.reserve((size_t) slots + 2));
    unsigned* d_set = h->sc->dk_a.p;
    unsigned* d_cnt = d_set + slots;
    launch_color_presence((const int*) d_argb, n_pixels, h->params.transparentColor, d_presence, d_set, slots, d_cnt, h->stream);
    NQ_HIP(h, launch_status());
    unsigned cnt[2] = {0, 0};
    NQ_HIP(h, hipMemcpyAsync(cnt, d_cnt, sizeof cnt, hipMemcpyDeviceToHost, h->stream));
    NQ_HIP(h, hipStreamSynchronize(h->stream));
    if (cnt[1] || cnt[0] > (unsigned) cap_other) { *out_other_count = -1; return NQ_OK; }      // too many non-opaque colours: caller decides
    std::vector<unsigned> set(slots);
    NQ_HIP(h, hipMemcpy(set.data(), d_set, (size_t) slots * sizeof(unsigned), hipMemcpyDeviceToHost));
    int64_t k = 0;
    for (unsigned v : set) if (v != 0xFFFFFFFFu && k < cap_other) out_other[k++] = v;
    *out_other_count = k;
    return NQ_OK;
}

int nq_set_distinct(nq_handle* h, int64_t count, const uint32_t* colors) {
    if (!h) return NQ_ERR_INVALID;
    h->ext_distinct_valid = true;
    h->ext_distinct_many = count < 0;
    h->ext_distinct.clear();
    if (count > 0) {
        if (!colors) NQ_FAIL(h, NQ_ERR_INVALID, "bad argument");
        h->ext_distinct.assign((const int32_t*) colors, (const int32_t*) colors + count);
    }
    return NQ_OK;
}

int nq_band_histogram_device(nq_handle* h, const uint32_t* d_argb, int64_t n_pixels, double* d_hist) {
    int rc = use_device(h);
    if (rc) return rc;
    if (!d_argb || n_pixels <= 0 || !d_hist) NQ_FAIL(h, NQ_ERR_INVALID, "bad argument");
    rc = reserve_palette_ws(h, n_pixels);
    if (rc) return rc;
    nq::HistParams hp;
    nq::SortWorkspace ws;
    hist_setup(h, &hp, &ws);
    launch_histogram(h->kind, (const int*) d_argb, n_pixels, hp, ws, d_hist, h->stream);
    NQ_HIP(h, launch_status());
    return NQ_OK;
}

int nq_palette_from_histograms_device(nq_handle* h, const double* d_hists, int n_bands, int nMaxColors,
                                      uint32_t* out_palette, int32_t* out_K) {
    int rc = use_device(h);
    if (rc) return rc;
    if (!d_hists || n_bands < 1 || !out_palette || !out_K || nMaxColors < 3) NQ_FAIL(h, NQ_ERR_INVALID, "bad argument");
    rc = reserve_palette_ws(h, 1);
    if (rc) return rc;
    return palette_of(h, out_palette, out_K, [&](PaletteJob* job) {
        return palette_prepare(h, d_hists, n_bands, nMaxColors, out_palette, out_K, nullptr, 0, job);
    });
}

} // extern "C"

// ---- GIF encoding (nq_gif.hip) ----
namespace {

constexpr int kGifDefaultSegment = 16384;

// most bits a segment of L pixels can take: at most L - 1 codes for misses, a Clear code per table reset (one per >= 3838 new
// entries), the frame's first Clear, the last code and the terminator, each at most 12 bits wide
inline long long gif_seg_bits_max(long long L) { return 12 * (L + 3 + L / 3838); }
inline long long gif_seg_len(long long px, int segment_pixels) { return std::min<long long>(segment_pixels ? segment_pixels : kGifDefaultSegment, px); }
inline long long gif_stream_len(long long data_bytes) { return data_bytes + (data_bytes + 254) / 255 + 1; }
constexpr long long kGifHeaderMax = 6 + 7 + 3 * 256 + 19, kGifFrameHeadMax = 8 + 10 + 1;

// the arguments nq_gif_max_bytes takes; false + the reason otherwise
bool gif_check_shape(int n, const int32_t* widths, const int32_t* heights, int K, int segment_pixels, char* why, size_t len) {
    if (n < 1) { std::snprintf(why, len, "n = %d: at least one frame", n); return false; }
    if (!widths || !heights) { std::snprintf(why, len, "widths / heights is NULL"); return false; }
    if (K < 1 || K > 256) { std::snprintf(why, len, "K = %d: a GIF colour table holds 1..256 entries", K); return false; }
    if (segment_pixels < 0) { std::snprintf(why, len, "segment_pixels = %d < 0", segment_pixels); return false; }
    for (int i = 0; i < n; ++i)
        if (widths[i] < 1 || widths[i] > 65535 || heights[i] < 1 || heights[i] > 65535) {
            std::snprintf(why, len, "frame %d: %d x %d, sides must be 1..65535", i, widths[i], heights[i]); return false;
        }
    return true;
}

// everything but the index pointers, checked from the host arrays alone (no device work)
int gif_check(nq_handle* h, int n, const int32_t* widths, const int32_t* heights, const uint32_t* palette, int K, const int32_t* delays_cs,
              int loop_count, int segment_pixels, int lossy, const uint8_t* out, int64_t cap, int64_t* out_size) {
    char why[256];
    if (!gif_check_shape(n, widths, heights, K, segment_pixels, why, sizeof why)) NQ_FAIL(h, NQ_ERR_INVALID, "%s", why);
    if (lossy < 0 || lossy > 255) NQ_FAIL(h, NQ_ERR_INVALID, "lossy = %d: must be 0..255", lossy);
    if (!palette || !out_size) NQ_FAIL(h, NQ_ERR_INVALID, "palette / out_size is NULL");
    if (loop_count < -1 || loop_count > 65535) NQ_FAIL(h, NQ_ERR_INVALID, "loop_count = %d: must be -1..65535", loop_count);
    if (delays_cs)
        for (int i = 0; i < n; ++i)
            if (delays_cs[i] < 0 || delays_cs[i] > 65535) NQ_FAIL(h, NQ_ERR_INVALID, "frame %d: delay %d outside 0..65535", i, delays_cs[i]);
    if (cap < 0 || (!out && cap > 0)) NQ_FAIL(h, NQ_ERR_INVALID, "out is NULL or cap < 0");
    return NQ_OK;
}

int gif_check_index(nq_handle* h, int n, const uint16_t* const* index) {
    if (!index) NQ_FAIL(h, NQ_ERR_INVALID, "index is NULL");
    for (int i = 0; i < n; ++i)
        if (!index[i] || ((uintptr_t) index[i] & 1)) NQ_FAIL(h, NQ_ERR_INVALID, "frame %d: index pointer NULL or not 2-byte aligned", i);
    return NQ_OK;
}

// where a frame sits on the screen
struct GifRect { int x, y, w, h; };

// Local colour tables ("GIF encoding, local colour tables"): what frame i's header takes from its own palette instead of from the
// call: its graphic control extension's packed byte (< 0: no extension) and transparent index byte.  Its K, Kt, m, T and written
// table are h->h_gif_local[i], which the chains and the two delta passes read from h->d_gif_local.
struct GifLocalHead { int gce, tr; };

inline int gif_color_bits(int Kt) {
    int N = 0;
    while ((1 << (N + 1)) < std::max(Kt, 2)) ++N;
    return N;
}

// The file of n index maps (device memory, map i is rects[i].w x rects[i].h and drawn at rects[i].x, rects[i].y) on a W x H screen.
// Kt sizes the colour table and the code size (K palette entries + the delta mode's unchanged index); gce < 0: no graphic control
// extensions, else their packed byte; tr: their transparent index byte and the screen's background index.  The caller has zeroed
// nothing: the bad-index flag is this function's own.  lossy > 0: the chains may take a colour within `lossy` of a pixel's own
// ("GIF encoding, lossy mode"); T: the index they neither replace nor substitute, -1 when the file has no transparent index.
// loc (NULL: one global table): one entry per frame; the file has no global table, every frame has a local one, and palette .. tr and T
// are not read: the caller has filled h->h_gif_local and copied it to h->d_gif_local.
int gif_encode_maps(nq_handle* h, int n, const uint16_t* const* d_index, const GifRect* rects, int W, int H, const uint32_t* palette, int K,
                    int Kt, int gce, int tr, int bg, const int32_t* delays_cs, int loop_count, int segment_pixels, int T, int lossy,
                    uint8_t* out, int64_t cap, int64_t* out_size, const GifLocalHead* loc = nullptr) {
    const int N = gif_color_bits(Kt);
    const int m = std::max(2, N + 1);
    if (lossy > 0 && !loc) {                              // the colour table as the file holds it: alpha dropped, zeros from entry K on
        h->h_gif_rgb.assign(256, 0u);
        for (int i = 0; i < K; ++i) h->h_gif_rgb[i] = palette[i] & 0xFFFFFFu;
        NQ_HIP(h, h->gif_rgb.reserve(256));
        NQ_HIP(h, hipMemcpyAsync(h->gif_rgb.p, h->h_gif_rgb.data(), 256 * sizeof(unsigned), hipMemcpyHostToDevice, h->stream));
    }
    // frame table: segments and their scratch
    h->h_gif.assign(n, nq::GifFrame{});
    long long segs = 0, words = 0;
    for (int i = 0; i < n; ++i) {
        nq::GifFrame& F = h->h_gif[i];
        const long long px = (long long) rects[i].w * rects[i].h, S = gif_seg_len(px, segment_pixels);
        F.index = d_index[i]; F.npix = px; F.seg_len = (int) S;
        F.nseg = (px + S - 1) / S; F.seg_base = segs; F.seg_words = gif_seg_bits_max(S) / 32 + 2; F.word_base = words;
        segs += F.nseg; words += F.nseg * F.seg_words;
    }
    NQ_HIP(h, h->d_gif.reserve(n));
    NQ_HIP(h, h->gif_words.reserve((size_t) words));
    NQ_HIP(h, h->gif_bits.reserve(2 * (size_t) segs));
    NQ_HIP(h, h->gif_res.reserve((size_t) n + 1));
    NQ_HIP(h, hipMemcpyAsync(h->d_gif.p, h->h_gif.data(), n * sizeof(nq::GifFrame), hipMemcpyHostToDevice, h->stream));
    NQ_HIP(h, hipMemsetAsync(h->gif_res.p + n, loc ? 0xFF : 0, sizeof(unsigned long long), h->stream));
    if (loc)
        launch_gif_lzw_local(h->d_gif.p, n, segs, h->d_gif_local.p, h->gif_words.p, h->gif_bits.p, h->gif_res.p + n, lossy, h->stream);
    else
        launch_gif_lzw(h->d_gif.p, n, segs, Kt, m, h->gif_words.p, h->gif_bits.p, h->gif_res.p + n, lossy > 0 ? h->gif_rgb.p : nullptr, T, lossy,
                       h->stream);
    launch_gif_scan(h->d_gif.p, n, h->gif_bits.p, h->gif_bits.p + segs, h->gif_res.p, h->stream);
    NQ_HIP(h, launch_status());
    std::vector<unsigned long long> res((size_t) n + 1);
    NQ_HIP(h, hipMemcpyAsync(res.data(), h->gif_res.p, res.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost, h->stream));
    NQ_HIP(h, hipStreamSynchronize(h->stream));
    if (loc && res[n] != ~0ull) {
        const int f = (int) std::min<unsigned long long>(res[n], (unsigned long long) n - 1);
        NQ_FAIL(h, NQ_ERR_INVALID, "frame %d: the index map holds an index >= its K = %d", f, h->h_gif_local[f].K);
    }
    if (!loc && res[n]) NQ_FAIL(h, NQ_ERR_INVALID, "an index map holds an index >= K = %d", K);
    // file layout: header + per frame {extension, descriptor, m, sub-blocks} + trailer; the header bytes go to the device in one blob
    std::vector<uint8_t>& blob = h->h_gif_blob;
    blob.clear();
    auto u16 = [&](int v) { blob.push_back((uint8_t) (v & 255)); blob.push_back((uint8_t) (v >> 8)); };
    blob.insert(blob.end(), {'G', 'I', 'F', '8', '9', 'a'});
    u16(W); u16(H);
    blob.push_back((uint8_t) (loc ? 0x70 : 0xF0 | N)); blob.push_back((uint8_t) bg); blob.push_back(0);
    for (int i = 0; !loc && i < (1 << (N + 1)); ++i) {
        const uint32_t c = i < K ? palette[i] : 0;
        blob.push_back((uint8_t) (c >> 16)); blob.push_back((uint8_t) (c >> 8)); blob.push_back((uint8_t) c);
    }
    if (n > 1 && loop_count >= 0) {
        blob.insert(blob.end(), {0x21, 0xFF, 0x0B, 'N', 'E', 'T', 'S', 'C', 'A', 'P', 'E', '2', '.', '0', 0x03, 0x01});
        u16(loop_count); blob.push_back(0);
    }
    long long total = 0;
    for (int i = 0; i < n; ++i) {
        nq::GifFrame& F = h->h_gif[i];
        const size_t start = i == 0 ? 0 : blob.size();
        const int gce_i = loc ? loc[i].gce : gce, tr_i = loc ? loc[i].tr : tr;
        if (gce_i >= 0) {
            blob.insert(blob.end(), {0x21, 0xF9, 0x04, (uint8_t) gce_i});
            u16(delays_cs ? delays_cs[i] : 0); blob.push_back((uint8_t) tr_i); blob.push_back(0);
        }
        blob.push_back(0x2C); u16(rects[i].x); u16(rects[i].y); u16(rects[i].w); u16(rects[i].h);
        if (loc) {                                  // the frame's own table, then its own m
            const nq::GifLocal& P = h->h_gif_local[i];
            const int Ni = gif_color_bits(P.Kt);
            blob.push_back((uint8_t) (0x80 | Ni));
            for (int j = 0; j < (1 << (Ni + 1)); ++j) {
                const unsigned c = P.rgb[j];
                blob.push_back((uint8_t) (c >> 16)); blob.push_back((uint8_t) (c >> 8)); blob.push_back((uint8_t) c);
            }
            blob.push_back((uint8_t) P.m);
        } else {
            blob.push_back(0);
            blob.push_back((uint8_t) m);
        }
        F.prefix_off = (long long) start; F.prefix_len = (int) (blob.size() - start);
        F.data_bytes = (long long) ((res[i] + 7) / 8); F.stream_len = gif_stream_len(F.data_bytes);
        F.file_off = total;
        total += F.prefix_len + F.stream_len;
    }
    total += 1;                                     // trailer
    *out_size = total;
    if (cap < total) NQ_FAIL(h, NQ_ERR_INVALID, "cap = %lld bytes < the file's %lld", (long long) cap, total);
    NQ_HIP(h, h->gif_blob.reserve(blob.size()));
    NQ_HIP(h, h->gif_file.reserve((size_t) total));
    NQ_HIP(h, hipMemcpyAsync(h->gif_blob.p, blob.data(), blob.size(), hipMemcpyHostToDevice, h->stream));
    NQ_HIP(h, hipMemcpyAsync(h->d_gif.p, h->h_gif.data(), n * sizeof(nq::GifFrame), hipMemcpyHostToDevice, h->stream));
    launch_gif_gather(h->d_gif.p, n, h->gif_words.p, h->gif_bits.p, h->gif_bits.p + segs, h->gif_blob.p, h->gif_file.p, total, h->stream);
    NQ_HIP(h, launch_status());
    NQ_HIP(h, hipMemcpyAsync(out, h->gif_file.p, (size_t) total, hipMemcpyDeviceToHost, h->stream));
    NQ_HIP(h, hipStreamSynchronize(h->stream));
    return NQ_OK;
}

// nq_encode_gif_device: whole frames at (0, 0), disposal 2
int gif_encode(nq_handle* h, int n, const uint16_t* const* d_index, const int32_t* widths, const int32_t* heights, const uint32_t* palette,
               int K, const int32_t* delays_cs, int loop_count, int segment_pixels, int lossy, uint8_t* out, int64_t cap, int64_t* out_size) {
    int t = -1;                                     // GIF has 1-bit transparency: the first entry with alpha 0, other alphas are dropped
    for (int i = 0; i < K && t < 0; ++i) if ((palette[i] >> 24) == 0) t = i;
    std::vector<GifRect> rects(n);
    int W = 0, H = 0;
    for (int i = 0; i < n; ++i) {
        rects[i] = {0, 0, (int) widths[i], (int) heights[i]};
        W = std::max(W, (int) widths[i]); H = std::max(H, (int) heights[i]);
    }
    const int gce = n > 1 || t >= 0 ? (n > 1 ? 2 << 2 : 0) | (t >= 0 ? 1 : 0) : -1;
    return gif_encode_maps(h, n, d_index, rects.data(), W, H, palette, K, K, gce, t >= 0 ? t : 0, t >= 0 ? t : 0, delays_cs, loop_count,
                           segment_pixels, t, lossy, out, cap, out_size);
}

// The rectangles of n >= 2 frames of one size (device memory): frame 0 whole, frame i >= 1 the bounding box of the pixels that differ
// from frame i - 1 (1 x 1 at (0, 0) when none does).  One difference pass over all frames and one small read-back; an index >= K
// anywhere in any frame is NQ_ERR_INVALID.  Shared by the delta GIF and the APNG encoder.  local: "differ" is judged on the colours
// h->d_gif_local gives the indices and every frame is checked against its own K (K is not read).
int changed_rects(nq_handle* h, int n, const uint16_t* const* d_index, int W, int H, int K, std::vector<GifRect>* out, bool local = false) {
    std::vector<int>& box = h->h_gif_box;
    box.assign(4 * (size_t) (n - 1) + 1, local ? INT_MAX : 0);
    for (int i = 0; i < n - 1; ++i) { box[4 * i] = box[4 * i + 1] = INT_MAX; box[4 * i + 2] = box[4 * i + 3] = -1; }
    NQ_HIP(h, h->gif_ptrs.reserve(n));
    NQ_HIP(h, h->gif_box.reserve(box.size()));
    NQ_HIP(h, hipMemcpyAsync(h->gif_ptrs.p, d_index, n * sizeof(*d_index), hipMemcpyHostToDevice, h->stream));
    NQ_HIP(h, hipMemcpyAsync(h->gif_box.p, box.data(), box.size() * sizeof(int), hipMemcpyHostToDevice, h->stream));
    if (local)
        launch_gif_diff_local(h->gif_ptrs.p, n, W, H, h->d_gif_local.p, h->gif_box.p, h->gif_box.p + 4 * (size_t) (n - 1), h->stream);
    else
        launch_gif_diff(h->gif_ptrs.p, n, W, H, K, h->gif_box.p, h->gif_box.p + 4 * (size_t) (n - 1), h->stream);
    NQ_HIP(h, launch_status());
    NQ_HIP(h, hipMemcpyAsync(box.data(), h->gif_box.p, box.size() * sizeof(int), hipMemcpyDeviceToHost, h->stream));
    NQ_HIP(h, hipStreamSynchronize(h->stream));
    if (local && box[4 * (size_t) (n - 1)] != INT_MAX) {
        const int f = std::min(std::max(box[4 * (size_t) (n - 1)], 0), n - 1);
        NQ_FAIL(h, NQ_ERR_INVALID, "frame %d: the index map holds an index >= its K = %d", f, h->h_gif_local[f].K);
    }
    if (!local && box[4 * (size_t) (n - 1)]) NQ_FAIL(h, NQ_ERR_INVALID, "an index map holds an index >= K = %d", K);
    std::vector<GifRect>& rects = *out;
    rects.assign(n, GifRect{});
    rects[0] = {0, 0, W, H};
    for (int i = 1; i < n; ++i) {
        const int* b = &box[4 * (size_t) (i - 1)];
        GifRect& r = rects[i];
        if (b[2] < 0) r = {0, 0, 1, 1};             // nothing changed
        else r = {b[0], b[1], b[2] - b[0] + 1, b[3] - b[1] + 1};
        if (r.x < 0 || r.y < 0 || r.w < 1 || r.h < 1 || r.x + r.w > W || r.y + r.h > H)
            NQ_FAIL(h, NQ_ERR_HIP, "frame %d: the difference pass returned the box %d %d %d %d", i, b[0], b[1], b[2], b[3]);
    }
    return NQ_OK;
}

// nq_encode_gif_delta_device after the argument checks (n >= 2): difference pass, one read-back of the boxes, body pass, then the
// bodies are encoded like any index maps.  loc (NULL: one global table): both passes compare colours and every frame has its own u,
// from h->h_gif_local / h->d_gif_local; palette and K are not read.
int gif_encode_delta(nq_handle* h, int n, const uint16_t* const* d_index, int W, int H, const uint32_t* palette, int K,
                     const int32_t* delays_cs, int loop_count, int segment_pixels, int lossy, uint8_t* out, int64_t cap, int64_t* out_size,
                     int32_t* out_rects, const GifLocalHead* loc = nullptr) {
    const int u = K <= 255 ? K : -1;                // the "unchanged" index, transparent in every frame
    std::vector<GifRect> rects;
    const int rc0 = changed_rects(h, n, d_index, W, H, K, &rects, loc != nullptr);
    if (rc0) return rc0;
    size_t room = 0;
    long long max_area = 1;
    for (int i = 1; i < n; ++i) {
        const long long area = (long long) rects[i].w * rects[i].h;
        room += (size_t) ((area + 7) & ~7ll);
        max_area = std::max(max_area, area);
    }
    NQ_HIP(h, h->gif_body.reserve(room));
    NQ_HIP(h, h->d_gif_delta.reserve(n - 1));
    h->h_gif_delta.assign(n - 1, nq::GifDelta{});
    std::vector<const uint16_t*> maps(n);
    maps[0] = d_index[0];
    size_t at = 0;
    for (int i = 1; i < n; ++i) {
        const GifRect& r = rects[i];
        h->h_gif_delta[i - 1] = {d_index[i], d_index[i - 1], h->gif_body.p + at, r.x, r.y, r.w, r.h};
        maps[i] = h->gif_body.p + at;
        at += (size_t) (((long long) r.w * r.h + 7) & ~7ll);
    }
    NQ_HIP(h, hipMemcpyAsync(h->d_gif_delta.p, h->h_gif_delta.data(), (n - 1) * sizeof(nq::GifDelta), hipMemcpyHostToDevice, h->stream));
    if (loc) launch_gif_body_local(h->d_gif_delta.p, n - 1, W, h->d_gif_local.p, max_area, h->stream);
    else launch_gif_body(h->d_gif_delta.p, n - 1, W, u, max_area, h->stream);
    NQ_HIP(h, launch_status());
    // The chains below check against Kt, so an index == K in frame 0 (read in place, not through a body) passes them: it is the
    // difference pass above that has checked frame 0, as the predecessor of frame 1, and every other frame against K.
    const int rc = gif_encode_maps(h, n, maps.data(), rects.data(), W, H, palette, K, K + (u >= 0 ? 1 : 0), 1 << 2 | (u >= 0 ? 1 : 0),
                                   u >= 0 ? u : 0, 0, delays_cs, loop_count, segment_pixels, u, lossy, out, cap, out_size, loc);
    if (rc) return rc;
    if (out_rects)
        for (int i = 0; i < n; ++i) { out_rects[4 * i] = rects[i].x; out_rects[4 * i + 1] = rects[i].y; out_rects[4 * i + 2] = rects[i].w; out_rects[4 * i + 3] = rects[i].h; }
    return NQ_OK;
}

// the checks both delta forms share, done from the host arguments alone; ws / hs: the size repeated per frame for the shared checks
int gif_delta_check(nq_handle* h, int n, const uint16_t* const* index, int width, int height, const uint32_t* palette, int K,
                    const int32_t* delays_cs, int loop_count, int segment_pixels, int lossy, const uint8_t* out, int64_t cap,
                    int64_t* out_size, std::vector<int32_t>* ws, std::vector<int32_t>* hs) {
    if (n < 1) NQ_FAIL(h, NQ_ERR_INVALID, "n = %d: at least one frame", n);
    ws->assign(n, width); hs->assign(n, height);
    int rc = gif_check(h, n, ws->data(), hs->data(), palette, K, delays_cs, loop_count, segment_pixels, lossy, out, cap, out_size);
    if (rc) return rc;
    if (n > 1)
        for (int i = 0; i < K; ++i)
            if ((palette[i] >> 24) == 0)
                NQ_FAIL(h, NQ_ERR_INVALID, "palette entry %d is transparent (alpha 0): frames that keep the canvas cannot un-paint a pixel, "
                        "use nq_encode_gif", i);
    return gif_check_index(h, n, index);
}

void gif_whole_rect(int32_t* out_rects, int width, int height) {
    if (out_rects) { out_rects[0] = out_rects[1] = 0; out_rects[2] = width; out_rects[3] = height; }
}

// The four memory forms behind the exports; lossy = 0 is the lossless call ("GIF encoding, lossy mode").
int gif_device_call(nq_handle* h, int n, const uint16_t* const* d_index, const int32_t* widths, const int32_t* heights,
                    const uint32_t* palette, int K, const int32_t* delays_cs, int loop_count, int segment_pixels, int lossy,
                    uint8_t* out, int64_t cap, int64_t* out_size) {
    if (!h) return NQ_ERR_INVALID;
    int rc = gif_check(h, n, widths, heights, palette, K, delays_cs, loop_count, segment_pixels, lossy, out, cap, out_size);
    if (rc) return rc;
    rc = gif_check_index(h, n, d_index);
    if (rc) return rc;
    rc = use_device(h);
    if (rc) return rc;
    return gif_encode(h, n, d_index, widths, heights, palette, K, delays_cs, loop_count, segment_pixels, lossy, out, cap, out_size);
}

int gif_host_call(nq_handle* h, int n, const uint16_t* const* index, const int32_t* widths, const int32_t* heights,
                  const uint32_t* palette, int K, const int32_t* delays_cs, int loop_count, int segment_pixels, int lossy,
                  uint8_t* out, int64_t cap, int64_t* out_size) {
    if (!h) return NQ_ERR_INVALID;
    int rc = gif_check(h, n, widths, heights, palette, K, delays_cs, loop_count, segment_pixels, lossy, out, cap, out_size);
    if (rc) return rc;
    rc = gif_check_index(h, n, index);
    if (rc) return rc;
    rc = use_device(h);
    if (rc) return rc;
    std::vector<size_t> px(n);
    for (int i = 0; i < n; ++i) px[i] = (size_t) widths[i] * heights[i];
    std::vector<uint16_t*> dev(n);
    return host_form(h, [&]() {
        rc = stage_in(h, h->gif_in, n, px.data(), index, dev.data());
        return rc ? rc : gif_encode(h, n, dev.data(), widths, heights, palette, K, delays_cs, loop_count, segment_pixels, lossy, out, cap, out_size);
    });
}

int gif_delta_device_call(nq_handle* h, int n, const uint16_t* const* d_index, int width, int height, const uint32_t* palette, int K,
                          const int32_t* delays_cs, int loop_count, int segment_pixels, int lossy, uint8_t* out, int64_t cap,
                          int64_t* out_size, int32_t* out_rects) {
    if (!h) return NQ_ERR_INVALID;
    std::vector<int32_t> ws, hs;
    int rc = gif_delta_check(h, n, d_index, width, height, palette, K, delays_cs, loop_count, segment_pixels, lossy, out, cap, out_size, &ws, &hs);
    if (rc) return rc;
    rc = use_device(h);
    if (rc) return rc;
    if (n > 1)
        return gif_encode_delta(h, n, d_index, width, height, palette, K, delays_cs, loop_count, segment_pixels, lossy, out, cap, out_size, out_rects);
    rc = gif_encode(h, n, d_index, ws.data(), hs.data(), palette, K, delays_cs, loop_count, segment_pixels, lossy, out, cap, out_size);
    if (rc == NQ_OK) gif_whole_rect(out_rects, width, height);
    return rc;
}

int gif_delta_host_call(nq_handle* h, int n, const uint16_t* const* index, int width, int height, const uint32_t* palette, int K,
                        const int32_t* delays_cs, int loop_count, int segment_pixels, int lossy, uint8_t* out, int64_t cap,
                        int64_t* out_size, int32_t* out_rects) {
    if (!h) return NQ_ERR_INVALID;
    std::vector<int32_t> ws, hs;
    int rc = gif_delta_check(h, n, index, width, height, palette, K, delays_cs, loop_count, segment_pixels, lossy, out, cap, out_size, &ws, &hs);
    if (rc) return rc;
    rc = use_device(h);
    if (rc) return rc;
    std::vector<size_t> px(n, (size_t) width * height);
    std::vector<uint16_t*> dev(n);
    return host_form(h, [&]() {
        rc = stage_in(h, h->gif_in, n, px.data(), index, dev.data());
        if (rc) return rc;
        if (n > 1)
            return gif_encode_delta(h, n, dev.data(), width, height, palette, K, delays_cs, loop_count, segment_pixels, lossy, out, cap, out_size,
                                    out_rects);
        rc = gif_encode(h, n, dev.data(), ws.data(), hs.data(), palette, K, delays_cs, loop_count, segment_pixels, lossy, out, cap, out_size);
        if (rc == NQ_OK) gif_whole_rect(out_rects, width, height);
        return rc;
    });
}

// ---- local colour tables ----

// the checks of both local calls, from the host arguments alone: gif_check's list, then K and the palettes
int gif_local_check(nq_handle* h, int n, const int32_t* widths, const int32_t* heights, const uint32_t* palettes, int32_t palette_stride,
                    const int32_t* K, const int32_t* delays_cs, int loop_count, int segment_pixels, int lossy, const uint8_t* out, int64_t cap,
                    int64_t* out_size, bool delta) {
    int rc = gif_check(h, n, widths, heights, palettes, 256, delays_cs, loop_count, segment_pixels, lossy, out, cap, out_size);
    if (rc) return rc;
    if (!K) NQ_FAIL(h, NQ_ERR_INVALID, "K is NULL");
    for (int i = 0; i < n; ++i) {
        if (K[i] < 1 || K[i] > 256) NQ_FAIL(h, NQ_ERR_INVALID, "frame %d: K = %d: a GIF colour table holds 1..256 entries", i, K[i]);
        if (palette_stride < K[i]) NQ_FAIL(h, NQ_ERR_INVALID, "frame %d: palette_stride = %d < K = %d", i, palette_stride, K[i]);
    }
    if (delta && n > 1)
        for (int i = 0; i < n; ++i)
            for (int j = 0; j < K[i]; ++j)
                if ((palettes[(size_t) i * palette_stride + j] >> 24) == 0)
                    NQ_FAIL(h, NQ_ERR_INVALID, "frame %d: palette entry %d is transparent (alpha 0): frames that keep the canvas cannot "
                            "un-paint a pixel, use nq_encode_gif_local", i, j);
    return NQ_OK;
}

// h->h_gif_local and the frames' header values from the palettes, copied to h->d_gif_local.  delta: Kt and T follow u, else t.
int gif_local_tables(nq_handle* h, int n, const uint32_t* palettes, int32_t palette_stride, const int32_t* K, bool delta,
                     std::vector<GifLocalHead>* heads) {
    h->h_gif_local.assign(n, nq::GifLocal{});
    heads->assign(n, GifLocalHead{});
    for (int i = 0; i < n; ++i) {
        nq::GifLocal& P = h->h_gif_local[i];
        const uint32_t* pal = palettes + (size_t) i * palette_stride;
        P.K = K[i];
        for (int j = 0; j < P.K; ++j) P.rgb[j] = pal[j] & 0xFFFFFFu;
        if (delta) {
            P.T = P.K <= 255 ? P.K : -1;            // u
            P.Kt = P.K + (P.T >= 0 ? 1 : 0);
            (*heads)[i] = {1 << 2 | (P.T >= 0 ? 1 : 0), P.T >= 0 ? P.T : 0};
        } else {
            P.T = -1;                               // t
            for (int j = 0; j < P.K && P.T < 0; ++j) if ((pal[j] >> 24) == 0) P.T = j;
            P.Kt = P.K;
            (*heads)[i] = {n > 1 || P.T >= 0 ? (n > 1 ? 2 << 2 : 0) | (P.T >= 0 ? 1 : 0) : -1, P.T >= 0 ? P.T : 0};
        }
        P.m = std::max(2, gif_color_bits(P.Kt) + 1);
    }
    NQ_HIP(h, h->d_gif_local.reserve(n));
    NQ_HIP(h, hipMemcpyAsync(h->d_gif_local.p, h->h_gif_local.data(), n * sizeof(nq::GifLocal), hipMemcpyHostToDevice, h->stream));
    return NQ_OK;
}

// nq_encode_gif_local_device after the checks: whole frames at (0, 0), disposal 2, every frame under its own table
int gif_local_encode(nq_handle* h, int n, const uint16_t* const* d_index, const int32_t* widths, const int32_t* heights,
                     const uint32_t* palettes, int32_t palette_stride, const int32_t* K, const int32_t* delays_cs, int loop_count,
                     int segment_pixels, int lossy, uint8_t* out, int64_t cap, int64_t* out_size) {
    std::vector<GifLocalHead> heads;
    const int rc = gif_local_tables(h, n, palettes, palette_stride, K, false, &heads);
    if (rc) return rc;
    std::vector<GifRect> rects(n);
    int W = 0, H = 0;
    for (int i = 0; i < n; ++i) {
        rects[i] = {0, 0, (int) widths[i], (int) heights[i]};
        W = std::max(W, (int) widths[i]); H = std::max(H, (int) heights[i]);
    }
    return gif_encode_maps(h, n, d_index, rects.data(), W, H, nullptr, 0, 0, -1, 0, 0, delays_cs, loop_count, segment_pixels, -1, lossy, out, cap,
                           out_size, heads.data());
}

// nq_encode_gif_local_delta_device after the checks; n = 1 is the full-frame file
int gif_local_encode_delta(nq_handle* h, int n, const uint16_t* const* d_index, int width, int height, const uint32_t* palettes,
                           int32_t palette_stride, const int32_t* K, const int32_t* delays_cs, int loop_count, int segment_pixels, int lossy,
                           uint8_t* out, int64_t cap, int64_t* out_size, int32_t* out_rects) {
    if (n == 1) {
        const int32_t w = width, ht = height;
        const int rc = gif_local_encode(h, 1, d_index, &w, &ht, palettes, palette_stride, K, delays_cs, loop_count, segment_pixels, lossy, out,
                                        cap, out_size);
        if (rc == NQ_OK) gif_whole_rect(out_rects, width, height);
        return rc;
    }
    std::vector<GifLocalHead> heads;
    const int rc = gif_local_tables(h, n, palettes, palette_stride, K, true, &heads);
    if (rc) return rc;
    return gif_encode_delta(h, n, d_index, width, height, nullptr, 0, delays_cs, loop_count, segment_pixels, lossy, out, cap, out_size, out_rects,
                            heads.data());
}

} // namespace

extern "C" {

// The bound of the same frames under one global table, nq_gif_max_bytes(.., 256, ..), counts
//   6 + 7 + 768 (global table) + 19 (loop block) + 1 (trailer)  and per frame  8 (extension) + 10 (descriptor) + 1 (m) + the stream's bound,
// the extension and the loop block for every n, n = 1 included, and the stream's bound for any K.  A file with local tables is
//   6 + 7 + (n > 1: 19) + 1  and per frame  (0 or 8) + 10 + 3 * 2^(N_i+1) <= 768 + 1 + the same stream,
// so it is at most that bound - 768 + 768 * n.  Adding 768 * n without taking the global table off keeps the arithmetic in one place
// and is 768 bytes loose (787 for n = 1 without an extension).
int nq_gif_local_max_bytes(int n, const int32_t* widths, const int32_t* heights, int segment_pixels, int64_t* out_bytes) {
    const int rc = nq_gif_max_bytes(n, widths, heights, 256, segment_pixels, out_bytes);
    if (rc == NQ_OK) *out_bytes += 768ll * n;
    return rc;
}

int nq_encode_gif_local_device(nq_handle* h, int n, const uint16_t* const* d_index, const int32_t* widths, const int32_t* heights,
                               const uint32_t* palettes, int32_t palette_stride, const int32_t* K, const int32_t* delays_cs, int loop_count,
                               int segment_pixels, int lossy, uint8_t* out, int64_t cap, int64_t* out_size) {
    if (!h) return NQ_ERR_INVALID;
    int rc = gif_local_check(h, n, widths, heights, palettes, palette_stride, K, delays_cs, loop_count, segment_pixels, lossy, out, cap, out_size,
                             false);
    if (rc) return rc;
    rc = gif_check_index(h, n, d_index);
    if (rc) return rc;
    rc = use_device(h);
    if (rc) return rc;
    return gif_local_encode(h, n, d_index, widths, heights, palettes, palette_stride, K, delays_cs, loop_count, segment_pixels, lossy, out, cap,
                            out_size);
}

int nq_encode_gif_local(nq_handle* h, int n, const uint16_t* const* index, const int32_t* widths, const int32_t* heights,
                        const uint32_t* palettes, int32_t palette_stride, const int32_t* K, const int32_t* delays_cs, int loop_count,
                        int segment_pixels, int lossy, uint8_t* out, int64_t cap, int64_t* out_size) {
    if (!h) return NQ_ERR_INVALID;
    int rc = gif_local_check(h, n, widths, heights, palettes, palette_stride, K, delays_cs, loop_count, segment_pixels, lossy, out, cap, out_size,
                             false);
    if (rc) return rc;
    rc = gif_check_index(h, n, index);
    if (rc) return rc;
    rc = use_device(h);
    if (rc) return rc;
    std::vector<size_t> px(n);
    for (int i = 0; i < n; ++i) px[i] = (size_t) widths[i] * heights[i];
    std::vector<uint16_t*> dev(n);
    return host_form(h, [&]() {
        rc = stage_in(h, h->gif_in, n, px.data(), index, dev.data());
        return rc ? rc : gif_local_encode(h, n, dev.data(), widths, heights, palettes, palette_stride, K, delays_cs, loop_count, segment_pixels,
                                          lossy, out, cap, out_size);
    });
}

int nq_encode_gif_local_delta_device(nq_handle* h, int n, const uint16_t* const* d_index, int width, int height, const uint32_t* palettes,
                                     int32_t palette_stride, const int32_t* K, const int32_t* delays_cs, int loop_count, int segment_pixels,
                                     int lossy, uint8_t* out, int64_t cap, int64_t* out_size, int32_t* out_rects) {
    if (!h) return NQ_ERR_INVALID;
    if (n < 1) NQ_FAIL(h, NQ_ERR_INVALID, "n = %d: at least one frame", n);
    const std::vector<int32_t> ws(n, width), hs(n, height);
    int rc = gif_local_check(h, n, ws.data(), hs.data(), palettes, palette_stride, K, delays_cs, loop_count, segment_pixels, lossy, out, cap,
                             out_size, true);
    if (rc) return rc;
    rc = gif_check_index(h, n, d_index);
    if (rc) return rc;
    rc = use_device(h);
    if (rc) return rc;
    return gif_local_encode_delta(h, n, d_index, width, height, palettes, palette_stride, K, delays_cs, loop_count, segment_pixels, lossy, out,
                                  cap, out_size, out_rects);
}

int nq_encode_gif_local_delta(nq_handle* h, int n, const uint16_t* const* index, int width, int height, const uint32_t* palettes,
                              int32_t palette_stride, const int32_t* K, const int32_t* delays_cs, int loop_count, int segment_pixels,
                              int lossy, uint8_t* out, int64_t cap, int64_t* out_size, int32_t* out_rects) {
    if (!h) return NQ_ERR_INVALID;
    if (n < 1) NQ_FAIL(h, NQ_ERR_INVALID, "n = %d: at least one frame", n);
    const std::vector<int32_t> ws(n, width), hs(n, height);
    int rc = gif_local_check(h, n, ws.data(), hs.data(), palettes, palette_stride, K, delays_cs, loop_count, segment_pixels, lossy, out, cap,
                             out_size, true);
    if (rc) return rc;
    rc = gif_check_index(h, n, index);
    if (rc) return rc;
    rc = use_device(h);
    if (rc) return rc;
    std::vector<size_t> px(n, (size_t) width * height);
    std::vector<uint16_t*> dev(n);
    return host_form(h, [&]() {
        rc = stage_in(h, h->gif_in, n, px.data(), index, dev.data());
        return rc ? rc : gif_local_encode_delta(h, n, dev.data(), width, height, palettes, palette_stride, K, delays_cs, loop_count,
                                                segment_pixels, lossy, out, cap, out_size, out_rects);
    });
}

int nq_gif_max_bytes(int n, const int32_t* widths, const int32_t* heights, int K, int segment_pixels, int64_t* out_bytes) {
    char why[256];
    if (!out_bytes || !gif_check_shape(n, widths, heights, K, segment_pixels, why, sizeof why)) return NQ_ERR_INVALID;
    long long total = kGifHeaderMax + 1;
    for (int i = 0; i < n; ++i) {
        const long long px = (long long) widths[i] * heights[i], S = gif_seg_len(px, segment_pixels), full = px / S, rest = px % S;
        const long long bits = full * gif_seg_bits_max(S) + (rest ? gif_seg_bits_max(rest) : 0);
        total += kGifFrameHeadMax + gif_stream_len((bits + 7) / 8);
    }
    *out_bytes = total;
    return NQ_OK;
}

int nq_encode_gif_device(nq_handle* h, int n, const uint16_t* const* d_index, const int32_t* widths, const int32_t* heights,
                         const uint32_t* palette, int K, const int32_t* delays_cs, int loop_count, int segment_pixels,
                         uint8_t* out, int64_t cap, int64_t* out_size) {
    return gif_device_call(h, n, d_index, widths, heights, palette, K, delays_cs, loop_count, segment_pixels, 0, out, cap, out_size);
}

int nq_encode_gif(nq_handle* h, int n, const uint16_t* const* index, const int32_t* widths, const int32_t* heights,
                  const uint32_t* palette, int K, const int32_t* delays_cs, int loop_count, int segment_pixels,
                  uint8_t* out, int64_t cap, int64_t* out_size) {
    return gif_host_call(h, n, index, widths, heights, palette, K, delays_cs, loop_count, segment_pixels, 0, out, cap, out_size);
}

int nq_encode_gif_delta_device(nq_handle* h, int n, const uint16_t* const* d_index, int width, int height, const uint32_t* palette, int K,
                               const int32_t* delays_cs, int loop_count, int segment_pixels, uint8_t* out, int64_t cap, int64_t* out_size,
                               int32_t* out_rects) {
    return gif_delta_device_call(h, n, d_index, width, height, palette, K, delays_cs, loop_count, segment_pixels, 0, out, cap, out_size, out_rects);
}

int nq_encode_gif_delta(nq_handle* h, int n, const uint16_t* const* index, int width, int height, const uint32_t* palette, int K,
                        const int32_t* delays_cs, int loop_count, int segment_pixels, uint8_t* out, int64_t cap, int64_t* out_size,
                        int32_t* out_rects) {
    return gif_delta_host_call(h, n, index, width, height, palette, K, delays_cs, loop_count, segment_pixels, 0, out, cap, out_size, out_rects);
}

int nq_encode_gif_lossy_device(nq_handle* h, int n, const uint16_t* const* d_index, const int32_t* widths, const int32_t* heights,
                               const uint32_t* palette, int K, const int32_t* delays_cs, int loop_count, int segment_pixels, int lossy,
                               uint8_t* out, int64_t cap, int64_t* out_size) {
    return gif_device_call(h, n, d_index, widths, heights, palette, K, delays_cs, loop_count, segment_pixels, lossy, out, cap, out_size);
}

int nq_encode_gif_lossy(nq_handle* h, int n, const uint16_t* const* index, const int32_t* widths, const int32_t* heights,
                        const uint32_t* palette, int K, const int32_t* delays_cs, int loop_count, int segment_pixels, int lossy,
                        uint8_t* out, int64_t cap, int64_t* out_size) {
    return gif_host_call(h, n, index, widths, heights, palette, K, delays_cs, loop_count, segment_pixels, lossy, out, cap, out_size);
}

int nq_encode_gif_delta_lossy_device(nq_handle* h, int n, const uint16_t* const* d_index, int width, int height, const uint32_t* palette,
                                     int K, const int32_t* delays_cs, int loop_count, int segment_pixels, int lossy, uint8_t* out, int64_t cap,
                                     int64_t* out_size, int32_t* out_rects) {
    return gif_delta_device_call(h, n, d_index, width, height, palette, K, delays_cs, loop_count, segment_pixels, lossy, out, cap, out_size,
                                 out_rects);
}

int nq_encode_gif_delta_lossy(nq_handle* h, int n, const uint16_t* const* index, int width, int height, const uint32_t* palette, int K,
                              const int32_t* delays_cs, int loop_count, int segment_pixels, int lossy, uint8_t* out, int64_t cap,
                              int64_t* out_size, int32_t* out_rects) {
    return gif_delta_host_call(h, n, index, width, height, palette, K, delays_cs, loop_count, segment_pixels, lossy, out, cap, out_size,
                               out_rects);
}

} // extern "C"

// ---- PNG encoding (nq_png.hip) ----
namespace {

constexpr int kPngDefaultSegment = 32768, kPngMaxSegment = 65535;

// most bits the block of a segment of L bytes can take: 17 bits of block header, 19 x 3 bits of code-length-code lengths, at most
// 286 + 30 code-length symbols of <= 7 + 7 bits, an end-of-block code of <= 15 bits (4513 in all), and per token a literal of <= 15
// bits for one byte or a match of <= 15 + 5 + 15 + 13 bits for at least three: <= 16 bits per byte
inline long long png_seg_bits_max(long long L) { return 4544 + 16 * L; }
inline int png_depth(int K) { return K <= 2 ? 1 : K <= 4 ? 2 : K <= 16 ? 4 : 8; }
inline long long png_row_bytes_at(int w, int depth) { return 1 + ((long long) w * depth + 7) / 8; }
inline long long png_row_bytes(int w, int K) { return png_row_bytes_at(w, png_depth(K)); }
inline long long png_seg_len(long long raw, int segment_bytes) { return std::min<long long>(segment_bytes ? segment_bytes : kPngDefaultSegment, raw); }
// signature, IHDR, PLTE, tRNS, IDAT length + type, zlib header | Adler-32, IDAT CRC, IEND
inline long long png_prefix_max(int K) { return 8 + 25 + (12 + 3 * K) + (12 + K) + 8 + 2; }
constexpr long long kPngSuffix = 4 + 4 + 12;

inline long long png_image_max(int w, int h, int K, int segment_bytes) {
    const long long raw = (long long) h * png_row_bytes(w, K), S = png_seg_len(raw, segment_bytes), full = raw / S, rest = raw % S;
    const long long bits = full * png_seg_bits_max(S) + (rest ? png_seg_bits_max(rest) : 0);
    return png_prefix_max(K) + (bits + 7) / 8 + kPngSuffix;
}

// the arguments nq_png_max_bytes takes; false + the reason otherwise
bool png_check_shape(int n, const int32_t* widths, const int32_t* heights, const int32_t* K, int segment_bytes, char* why, size_t len) {
    if (n < 1) { std::snprintf(why, len, "n = %d: at least one image", n); return false; }
    if (!widths || !heights) { std::snprintf(why, len, "widths / heights is NULL"); return false; }
    if (segment_bytes < 0 || segment_bytes > kPngMaxSegment) { std::snprintf(why, len, "segment_bytes = %d: must be 0..%d", segment_bytes, kPngMaxSegment); return false; }
    for (int i = 0; i < n; ++i) {
        if (widths[i] < 1 || widths[i] > 65535 || heights[i] < 1 || heights[i] > 65535) {
            std::snprintf(why, len, "image %d: %d x %d, sides must be 1..65535", i, widths[i], heights[i]); return false;
        }
        const int k = K ? K[i] : 256;
        if (k < 1 || k > 256) { std::snprintf(why, len, "image %d: K = %d, a PNG palette holds 1..256 entries", i, k); return false; }
        if (png_image_max(widths[i], heights[i], k, segment_bytes) > 2147483647ll) {
            std::snprintf(why, len, "image %d: %d x %d, the file's bound exceeds 2^31 - 1 bytes", i, widths[i], heights[i]); return false;
        }
    }
    return true;
}

int png_check(nq_handle* h, int n, const uint16_t* const* index, const int32_t* widths, const int32_t* heights, const uint32_t* palettes,
              int32_t palette_stride, const int32_t* K, int segment_bytes, const uint8_t* out, int64_t cap, int64_t* out_offsets) {
    char why[256];
    if (!K) NQ_FAIL(h, NQ_ERR_INVALID, "K is NULL");
    if (!png_check_shape(n, widths, heights, K, segment_bytes, why, sizeof why)) NQ_FAIL(h, NQ_ERR_INVALID, "%s", why);
    if (!palettes || !out_offsets) NQ_FAIL(h, NQ_ERR_INVALID, "palettes / out_offsets is NULL");
    for (int i = 0; i < n; ++i)
        if (palette_stride < K[i]) NQ_FAIL(h, NQ_ERR_INVALID, "palette_stride = %d < K = %d of image %d", palette_stride, K[i], i);
    if (cap < 0 || (!out && cap > 0)) NQ_FAIL(h, NQ_ERR_INVALID, "out is NULL or cap < 0");
    if (!index) NQ_FAIL(h, NQ_ERR_INVALID, "index is NULL");
    for (int i = 0; i < n; ++i)
        if (!index[i] || ((uintptr_t) index[i] & 1)) NQ_FAIL(h, NQ_ERR_INVALID, "image %d: index pointer NULL or not 2-byte aligned", i);
    return NQ_OK;
}

uint32_t png_crc32(const uint8_t* p, size_t n) {
    uint32_t c = 0xFFFFFFFFu;
    for (size_t i = 0; i < n; ++i) {
        c ^= p[i];
        for (int k = 0; k < 8; ++k) c = (c >> 1) ^ ((c & 1u) ? 0xEDB88320u : 0u);
    }
    return ~c;
}

// The chains of the n images in h->h_png (index, prev, width, height, pitch, K, depth, u filled in by the caller): segments and their
// scratch, one deflate launch and one scan for all of them, one read-back.  res[2 i] = image i's deflate bit length, res[2 n + i] != 0:
// image i holds an index >= its K.  *out_segs: chains of the call.
int png_chains(nq_handle* h, int n, int segment_bytes, std::vector<unsigned long long>* out_res, long long* out_segs) {
    long long segs = 0, words = 0;
    int max_seg = 1;
    bool rect = false;                              // any image that is a rectangle of a larger map or a delta frame
    for (int i = 0; i < n; ++i) {
        nq::PngImage& F = h->h_png[i];
        rect = rect || F.prev != nullptr || F.pitch != F.width;
        F.row_bytes = (int) png_row_bytes_at(F.width, F.depth);
        F.raw_len = (long long) F.height * F.row_bytes;
        F.seg_len = (int) png_seg_len(F.raw_len, segment_bytes);
        F.nseg = (F.raw_len + F.seg_len - 1) / F.seg_len; F.seg_base = segs; F.seg_words = png_seg_bits_max(F.seg_len) / 32 + 2; F.word_base = words;
        segs += F.nseg; words += F.nseg * F.seg_words;
        max_seg = std::max(max_seg, F.seg_len);
    }
    const int grid = (int) std::min<long long>(segs, 4ll * std::max(h->n_cus, 1));
    NQ_HIP(h, h->d_png.reserve(n));
    NQ_HIP(h, h->gif_words.reserve((size_t) words));
    NQ_HIP(h, h->gif_bits.reserve(2 * (size_t) segs));
    NQ_HIP(h, h->png_adler.reserve((size_t) segs));
    NQ_HIP(h, h->gif_res.reserve(3 * (size_t) n));
    NQ_HIP(h, h->png_tokens.reserve((size_t) grid * max_seg));
    NQ_HIP(h, h->png_crc.reserve(n));
    NQ_HIP(h, hipMemcpyAsync(h->d_png.p, h->h_png.data(), n * sizeof(nq::PngImage), hipMemcpyHostToDevice, h->stream));
    NQ_HIP(h, hipMemsetAsync(h->gif_res.p + 2 * n, 0, n * sizeof(unsigned long long), h->stream));
    NQ_HIP(h, launch_png_deflate(h->d_png.p, n, segs, max_seg, grid, rect, h->gif_words.p, h->gif_bits.p, h->png_adler.p, h->png_tokens.p,
                                 h->gif_res.p + 2 * n, h->stream));
    launch_png_scan(h->d_png.p, n, h->gif_bits.p, h->png_adler.p, h->gif_bits.p + segs, h->gif_res.p, h->stream);
    NQ_HIP(h, launch_status());
    out_res->assign(3 * (size_t) n, 0);
    NQ_HIP(h, hipMemcpyAsync(out_res->data(), h->gif_res.p, out_res->size() * sizeof(unsigned long long), hipMemcpyDeviceToHost, h->stream));
    NQ_HIP(h, hipStreamSynchronize(h->stream));
    *out_segs = segs;
    return NQ_OK;
}

// the bytes the host writes, in one blob: chunks with their CRC, and the head of a data chunk (its CRC is the device's)
struct PngBlob {
    std::vector<uint8_t>& b;
    size_t chunk_at = 0;
    void u16(uint32_t v) { b.push_back((uint8_t) (v >> 8)); b.push_back((uint8_t) v); }
    void u32(uint32_t v) { for (int k = 3; k >= 0; --k) b.push_back((uint8_t) (v >> (8 * k))); }
    void begin(uint32_t len, const char* type) { u32(len); chunk_at = b.size(); b.insert(b.end(), type, type + 4); }
    void end() { u32(png_crc32(b.data() + chunk_at, b.size() - chunk_at)); }
    // signature, IHDR, PLTE, tRNS (only when some entry's alpha is not 255: the alpha bytes up to the last such entry)
    void head(int w, int hgt, int depth, const uint32_t* pal, int K) {
        b.insert(b.end(), {0x89, 'P', 'N', 'G', 0x0D, 0x0A, 0x1A, 0x0A});
        begin(13, "IHDR"); u32((uint32_t) w); u32((uint32_t) hgt);
        b.insert(b.end(), {(uint8_t) depth, 3, 0, 0, 0}); end();
        begin((uint32_t) (3 * K), "PLTE");
        for (int k = 0; k < K; ++k) { b.push_back((uint8_t) (pal[k] >> 16)); b.push_back((uint8_t) (pal[k] >> 8)); b.push_back((uint8_t) pal[k]); }
        end();
        int nt = 0;
        for (int k = 0; k < K; ++k) if ((pal[k] >> 24) != 255) nt = k + 1;
        if (nt) {
            begin((uint32_t) nt, "tRNS");
            for (int k = 0; k < nt; ++k) b.push_back((uint8_t) (pal[k] >> 24));
            end();
        }
    }
    // length, type and (seq >= 0: an fdAT's sequence number) of the data chunk around data_bytes of deflate data, then the zlib header:
    // deflate, 32 KiB window; no dictionary, fastest; 0x7801 is a multiple of 31.  Returns crc_lead.
    int data_head(long long data_bytes, long long seq) {
        u32((uint32_t) ((seq >= 0 ? 4 : 0) + 2 + data_bytes + 4));
        const char* type = seq >= 0 ? "fdAT" : "IDAT";
        b.insert(b.end(), type, type + 4);
        if (seq >= 0) u32((uint32_t) seq);
        b.push_back(0x78); b.push_back(0x01);
        return seq >= 0 ? 10 : 6;
    }
};

// place image i (its prefix is blob[start ..)) at *total; the CRC and, with iend, the IEND chunk follow its data
void png_place(nq::PngImage& F, const std::vector<uint8_t>& blob, size_t start, int crc_lead, bool iend, long long* total, long long* crc_chunks) {
    F.prefix_off = (long long) start; F.prefix_len = (int) (blob.size() - start);
    F.crc_lead = crc_lead; F.iend = iend ? 1 : 0;
    F.file_off = *total; F.crc_base = *crc_chunks;
    *total += F.prefix_len + F.data_bytes + 8 + (iend ? 12 : 0);
    *crc_chunks += (crc_lead + 4 + F.data_bytes + 127) / 128;
}

// blob and placed image table -> the `total` bytes of the files in `out`
int png_assemble(nq_handle* h, int n, long long segs, long long total, long long crc_chunks, uint8_t* out) {
    const std::vector<uint8_t>& blob = h->h_gif_blob;
    NQ_HIP(h, h->gif_blob.reserve(blob.size()));
    NQ_HIP(h, h->gif_file.reserve((size_t) total));
    NQ_HIP(h, hipMemcpyAsync(h->gif_blob.p, blob.data(), blob.size(), hipMemcpyHostToDevice, h->stream));
    NQ_HIP(h, hipMemcpyAsync(h->d_png.p, h->h_png.data(), n * sizeof(nq::PngImage), hipMemcpyHostToDevice, h->stream));
    NQ_HIP(h, hipMemsetAsync(h->png_crc.p, 0, n * sizeof(unsigned), h->stream));
    launch_png_gather(h->d_png.p, n, h->gif_words.p, h->gif_bits.p, h->gif_bits.p + segs, h->gif_res.p, h->gif_blob.p, h->gif_file.p, total,
                      crc_chunks, h->png_crc.p, h->stream);
    NQ_HIP(h, launch_status());
    NQ_HIP(h, hipMemcpyAsync(out, h->gif_file.p, (size_t) total, hipMemcpyDeviceToHost, h->stream));
    NQ_HIP(h, hipStreamSynchronize(h->stream));
    return NQ_OK;
}

int png_encode(nq_handle* h, int n, const uint16_t* const* d_index, const int32_t* widths, const int32_t* heights, const uint32_t* palettes,
               int32_t palette_stride, const int32_t* K, int segment_bytes, uint8_t* out, int64_t cap, int64_t* out_offsets) {
    h->h_png.assign(n, nq::PngImage{});
    for (int i = 0; i < n; ++i) {
        nq::PngImage& F = h->h_png[i];
        F.index = d_index[i]; F.width = F.pitch = widths[i]; F.height = heights[i]; F.K = K[i]; F.depth = png_depth(K[i]); F.u = -1;
    }
    std::vector<unsigned long long> res;
    long long segs = 0;
    const int rc = png_chains(h, n, segment_bytes, &res, &segs);
    if (rc) return rc;
    for (int i = 0; i < n; ++i)
        if (res[2 * n + i]) NQ_FAIL(h, NQ_ERR_INVALID, "image %d: the index map holds an index >= K = %d", i, K[i]);
    // per image the bytes in front of the deflate data: signature, IHDR, PLTE, tRNS, IDAT length and type, zlib header
    h->h_gif_blob.clear();
    PngBlob blob{h->h_gif_blob};
    long long total = 0, crc_chunks = 0;
    for (int i = 0; i < n; ++i) {
        nq::PngImage& F = h->h_png[i];
        const size_t start = blob.b.size();
        blob.head(widths[i], heights[i], F.depth, palettes + (size_t) i * palette_stride, K[i]);
        F.data_bytes = (long long) ((res[2 * i] + 7) / 8);
        const int lead = blob.data_head(F.data_bytes, -1);
        out_offsets[i] = total;
        png_place(F, blob.b, start, lead, true, &total, &crc_chunks);
    }
    out_offsets[n] = total;
    if (cap < total) NQ_FAIL(h, NQ_ERR_INVALID, "cap = %lld bytes < the files' %lld", (long long) cap, total);
    return png_assemble(h, n, segs, total, crc_chunks, out);
}

// ---- APNG: one file of n frames of one size over one palette (include/nquant_abi.h "APNG encoding") ----
// signature .. tRNS + acTL + frame 0's fcTL; every later frame an fcTL more than a still image's IDAT; an fdAT's sequence number
constexpr long long kApngExtra = 20 + 38;

// the arguments nq_apng_max_bytes takes; false + the reason otherwise
bool apng_check_shape(int n, int width, int height, int segment_bytes, char* why, size_t len) {
    if (n < 1) { std::snprintf(why, len, "n = %d: at least one frame", n); return false; }
    const int32_t w = width, hg = height;
    return png_check_shape(1, &w, &hg, nullptr, segment_bytes, why, len);
}

int apng_check(nq_handle* h, int n, const uint16_t* const* index, int width, int height, const uint32_t* palette, int K,
               const int32_t* delays_cs, int loop_count, int segment_bytes, const uint8_t* out, int64_t cap, int64_t* out_size) {
    char why[256];
    if (!apng_check_shape(n, width, height, segment_bytes, why, sizeof why)) NQ_FAIL(h, NQ_ERR_INVALID, "%s", why);
    if (K < 1 || K > 256) NQ_FAIL(h, NQ_ERR_INVALID, "K = %d: a PNG palette holds 1..256 entries", K);
    if (!palette || !out_size) NQ_FAIL(h, NQ_ERR_INVALID, "palette / out_size is NULL");
    if (loop_count < 0) NQ_FAIL(h, NQ_ERR_INVALID, "loop_count = %d: must be >= 0 (0 = for ever)", loop_count);
    if (delays_cs)
        for (int i = 0; i < n; ++i)
            if (delays_cs[i] < 0 || delays_cs[i] > 65535) NQ_FAIL(h, NQ_ERR_INVALID, "frame %d: delay %d outside 0..65535", i, delays_cs[i]);
    if (cap < 0 || (!out && cap > 0)) NQ_FAIL(h, NQ_ERR_INVALID, "out is NULL or cap < 0");
    return gif_check_index(h, n, index);
}

// nq_encode_apng_device after the argument checks
int apng_encode(nq_handle* h, int n, const uint16_t* const* d_index, int W, int H, const uint32_t* palette, int K, const int32_t* delays_cs,
                int loop_count, int segment_bytes, uint8_t* out, int64_t cap, int64_t* out_size, int32_t* out_rects) {
    if (n == 1) {                                   // a still image: nq_encode_png's file
        const int32_t w = W, hg = H, k = K;
        int64_t offs[2] = {0, -1};
        const int rc = png_encode(h, 1, d_index, &w, &hg, palette, K, &k, segment_bytes, out, cap, offs);
        if (offs[1] >= 0) *out_size = offs[1];
        if (rc == NQ_OK) gif_whole_rect(out_rects, W, H);
        return rc;
    }
    // one mode per file, from the palette alone: mark (opaque palette with room for u: unchanged pixels are index u, alpha 0, blended
    // OVER) or crop (the rectangle replaces what was there)
    bool opaque = true;
    for (int i = 0; i < K; ++i) opaque = opaque && (palette[i] >> 24) == 255;
    const int u = opaque && K <= 255 ? K : -1, Kt = K + (u >= 0 ? 1 : 0), depth = png_depth(Kt);
    std::vector<uint32_t> pal(palette, palette + K);
    if (u >= 0) pal.push_back(0);
    std::vector<GifRect> rects;
    int rc = changed_rects(h, n, d_index, W, H, K, &rects);      // (also the index >= K check of every frame)
    if (rc) return rc;
    h->h_png.assign(n, nq::PngImage{});
    for (int i = 0; i < n; ++i) {
        nq::PngImage& F = h->h_png[i];
        const GifRect& r = rects[i];
        const size_t first = (size_t) r.y * W + r.x;
        F.index = d_index[i] + first;
        F.prev = u >= 0 && i > 0 ? d_index[i - 1] + first : nullptr;
        F.width = r.w; F.height = r.h; F.pitch = W; F.K = K; F.depth = depth; F.u = u;
    }
    std::vector<unsigned long long> res;
    long long segs = 0;
    rc = png_chains(h, n, segment_bytes, &res, &segs);
    if (rc) return rc;
    for (int i = 0; i < n; ++i)
        if (res[2 * n + i]) NQ_FAIL(h, NQ_ERR_INVALID, "frame %d: the index map holds an index >= K = %d", i, K);
    h->h_gif_blob.clear();
    PngBlob blob{h->h_gif_blob};
    long long total = 0, crc_chunks = 0;
    uint32_t seq = 0;
    for (int i = 0; i < n; ++i) {
        nq::PngImage& F = h->h_png[i];
        const GifRect& r = rects[i];
        const size_t start = blob.b.size();
        if (i == 0) {
            blob.head(W, H, depth, pal.data(), Kt);
            blob.begin(8, "acTL"); blob.u32((uint32_t) n); blob.u32((uint32_t) loop_count); blob.end();
        }
        blob.begin(26, "fcTL");
        blob.u32(seq++); blob.u32((uint32_t) r.w); blob.u32((uint32_t) r.h); blob.u32((uint32_t) r.x); blob.u32((uint32_t) r.y);
        blob.u16((uint32_t) (delays_cs ? delays_cs[i] : 0)); blob.u16(100);
        blob.b.push_back(0); blob.b.push_back((uint8_t) (u >= 0 && i > 0 ? 1 : 0));      // dispose NONE; blend SOURCE / OVER
        blob.end();
        F.data_bytes = (long long) ((res[2 * i] + 7) / 8);
        const int lead = blob.data_head(F.data_bytes, i == 0 ? -1 : (long long) seq++);
        png_place(F, blob.b, start, lead, i == n - 1, &total, &crc_chunks);
    }
    *out_size = total;
    if (cap < total) NQ_FAIL(h, NQ_ERR_INVALID, "cap = %lld bytes < the file's %lld", (long long) cap, total);
    rc = png_assemble(h, n, segs, total, crc_chunks, out);
    if (rc) return rc;
    if (out_rects)
        for (int i = 0; i < n; ++i) { out_rects[4 * i] = rects[i].x; out_rects[4 * i + 1] = rects[i].y; out_rects[4 * i + 2] = rects[i].w; out_rects[4 * i + 3] = rects[i].h; }
    return NQ_OK;
}

} // namespace

extern "C" {

int nq_png_max_bytes(int n, const int32_t* widths, const int32_t* heights, const int32_t* K, int segment_bytes, int64_t* out_bytes) {
    char why[256];
    if (!out_bytes || !png_check_shape(n, widths, heights, K, segment_bytes, why, sizeof why)) return NQ_ERR_INVALID;
    long long total = 0;
    for (int i = 0; i < n; ++i) total += png_image_max(widths[i], heights[i], K ? K[i] : 256, segment_bytes);
    *out_bytes = total;
    return NQ_OK;
}

int nq_encode_png_device(nq_handle* h, int n, const uint16_t* const* d_index, const int32_t* widths, const int32_t* heights,
                         const uint32_t* palettes, int32_t palette_stride, const int32_t* K, int segment_bytes,
                         uint8_t* out, int64_t cap, int64_t* out_offsets) {
    if (!h) return NQ_ERR_INVALID;
    int rc = png_check(h, n, d_index, widths, heights, palettes, palette_stride, K, segment_bytes, out, cap, out_offsets);
    if (rc) return rc;
    rc = use_device(h);
    if (rc) return rc;
    return png_encode(h, n, d_index, widths, heights, palettes, palette_stride, K, segment_bytes, out, cap, out_offsets);
}

int nq_encode_png(nq_handle* h, int n, const uint16_t* const* index, const int32_t* widths, const int32_t* heights,
                  const uint32_t* palettes, int32_t palette_stride, const int32_t* K, int segment_bytes,
                  uint8_t* out, int64_t cap, int64_t* out_offsets) {
    if (!h) return NQ_ERR_INVALID;
    int rc = png_check(h, n, index, widths, heights, palettes, palette_stride, K, segment_bytes, out, cap, out_offsets);
    if (rc) return rc;
    rc = use_device(h);
    if (rc) return rc;
    std::vector<size_t> px(n);
    for (int i = 0; i < n; ++i) px[i] = (size_t) widths[i] * heights[i];
    std::vector<uint16_t*> dev(n);
    return host_form(h, [&]() {
        rc = stage_in(h, h->gif_in, n, px.data(), index, dev.data());
        return rc ? rc : png_encode(h, n, dev.data(), widths, heights, palettes, palette_stride, K, segment_bytes, out, cap, out_offsets);
    });
}

int nq_apng_max_bytes(int n, int width, int height, int segment_bytes, int64_t* out_bytes) {
    char why[256];
    if (!out_bytes || !apng_check_shape(n, width, height, segment_bytes, why, sizeof why)) return NQ_ERR_INVALID;
    *out_bytes = (long long) n * png_image_max(width, height, 256, segment_bytes) + kApngExtra;
    return NQ_OK;
}

int nq_encode_apng_device(nq_handle* h, int n, const uint16_t* const* d_index, int width, int height, const uint32_t* palette, int K,
                          const int32_t* delays_cs, int loop_count, int segment_bytes, uint8_t* out, int64_t cap, int64_t* out_size,
                          int32_t* out_rects) {
    if (!h) return NQ_ERR_INVALID;
    int rc = apng_check(h, n, d_index, width, height, palette, K, delays_cs, loop_count, segment_bytes, out, cap, out_size);
    if (rc) return rc;
    rc = use_device(h);
    if (rc) return rc;
    return apng_encode(h, n, d_index, width, height, palette, K, delays_cs, loop_count, segment_bytes, out, cap, out_size, out_rects);
}

int nq_encode_apng(nq_handle* h, int n, const uint16_t* const* index, int width, int height, const uint32_t* palette, int K,
                   const int32_t* delays_cs, int loop_count, int segment_bytes, uint8_t* out, int64_t cap, int64_t* out_size,
                   int32_t* out_rects) {
    if (!h) return NQ_ERR_INVALID;
    int rc = apng_check(h, n, index, width, height, palette, K, delays_cs, loop_count, segment_bytes, out, cap, out_size);
    if (rc) return rc;
    rc = use_device(h);
    if (rc) return rc;
    std::vector<size_t> px(n, (size_t) width * height);
    std::vector<uint16_t*> dev(n);
    return host_form(h, [&]() {
        rc = stage_in(h, h->gif_in, n, px.data(), index, dev.data());
        return rc ? rc : apng_encode(h, n, dev.data(), width, height, palette, K, delays_cs, loop_count, segment_bytes, out, cap, out_size,
                                     out_rects);
    });
}

} // extern "C"

// ---- what the frame-input and frame-sequence stages share: every piece fails into the string it is given and enqueues
// on the stream it is given, so the stages on a handle (h->err, h->stream) and the handle-free ones (g_create_error, their own
// stream) use the same code ----
namespace {

// The tail of a stage's pointer table: the host vector `t` (kept in the handle) goes up into the device table `d`, grown first.
// The call may return with this upload only enqueued, and the next call on the handle rewrites `t` and may regrow `d`.  Both are
// safe for the reason the encoders' table uploads are: the runtime copies a small pageable source into its own staging memory before
// hipMemcpyAsync returns, and DevBuf::reserve frees through hipFree, which waits for the device.  Held by tests/test_gpu_streams.py
// (two asynchronous calls back to back behind a gated stream, the second with more frames): a runtime that read the source later
// would fail there, and the tables would then need page-locked slots guarded by events.
template <typename T> int upload_table(std::string& err, hipStream_t s, const std::vector<T>& t, DevBuf<T>& d) {
    NQ_HIP_TO(err, d.reserve(t.size()));
    NQ_HIP_TO(err, hipMemcpyAsync(d.p, t.data(), t.size() * sizeof(T), hipMemcpyHostToDevice, s));
    return NQ_OK;
}

// A buffer of a call, [begin, end) in bytes; out: the call writes it.
struct Span { uintptr_t begin, end; bool out; };

// Whether an output overlaps a source or another output (the sources may overlap each other: they are only read; a buffer that
// begins where another ends is apart from it): in the order of their first bytes, a buffer overlaps an earlier one exactly when it
// begins before the furthest end seen so far.
bool output_overlaps(std::vector<Span>& spans) {
    std::sort(spans.begin(), spans.end(), [](const Span& a, const Span& b) { return a.begin < b.begin; });
    uintptr_t end_any = 0, end_out = 0;
    for (const Span& sp : spans) {
        if (sp.begin < (sp.out ? end_any : end_out)) return true;
        end_any = std::max(end_any, sp.end);
        if (sp.out) end_out = std::max(end_out, sp.end);
    }
    return false;
}

// crop, target and flags of a reducing call on width x height frames
int reduce_check(std::string& err, int width, int height, int crop_x, int crop_y, int crop_w, int crop_h, int dst_width, int dst_height,
                 int flags) {
    if (crop_w < 1 || crop_h < 1 || crop_x < 0 || crop_y < 0 || crop_x > width - crop_w || crop_y > height - crop_h)
        NQ_FAIL_TO(err, NQ_ERR_INVALID, "crop %d x %d at (%d, %d): empty or outside the %d x %d frame", crop_w, crop_h, crop_x, crop_y, width,
                   height);
    if (dst_width < 1 || dst_width > crop_w || dst_height < 1 || dst_height > crop_h)
        NQ_FAIL_TO(err, NQ_ERR_INVALID, "target %d x %d: sides must be 1 .. the crop's (%d x %d); this call only reduces", dst_width, dst_height,
                   crop_w, crop_h);
    if (flags & ~NQ_RESAMPLE_LINEAR) NQ_FAIL_TO(err, NQ_ERR_INVALID, "flags = 0x%x: unknown bits", (unsigned) flags);
    return NQ_OK;
}

// The host form of a stage over ARGB frames: the n sources of src_px words go up into d_in and the m outputs of out_px words are
// staged in d_out, every frame a multiple of 4 words from the last (16-byte aligned: the vector paths); device(sources, outputs) runs
// the device form on the staged copies; the outputs come back and are waited for.  On failure the stream is waited for too, so no
// copy from or to the caller's buffers outlives the call.
template <typename Device>
int argb_host(std::string& err, hipStream_t s, DevBuf<uint32_t>& d_in, DevBuf<uint32_t>& d_out, int n, const uint32_t* const* src,
              size_t src_px, int m, uint32_t* const* dst, size_t out_px, Device device) {
    const size_t spitch = (src_px + 3) & ~(size_t) 3, dpitch = (out_px + 3) & ~(size_t) 3;
    auto body = [&]() -> int {
        NQ_HIP_TO(err, d_in.reserve(n * spitch));
        NQ_HIP_TO(err, d_out.reserve(m * dpitch));
        std::vector<const uint32_t*> d_src(n);
        std::vector<uint32_t*> d_dst(m);
        for (int i = 0; i < n; ++i) {
            d_src[i] = d_in.p + i * spitch;
            NQ_HIP_TO(err, hipMemcpyAsync(d_in.p + i * spitch, src[i], src_px * sizeof(uint32_t), hipMemcpyHostToDevice, s));
        }
        for (int j = 0; j < m; ++j) d_dst[j] = d_out.p + j * dpitch;
        const int rc = device(d_src.data(), d_dst.data());
        if (rc) return rc;
        for (int j = 0; j < m; ++j) NQ_HIP_TO(err, hipMemcpyAsync(dst[j], d_dst[j], out_px * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
        NQ_HIP_TO(err, hipStreamSynchronize(s));
        return NQ_OK;
    };
    const int rc = body();
    if (rc) (void) hipStreamSynchronize(s);
    return rc;
}

// The n frames of a YUV 4:2:0 call with samples of type S (uint8_t, or uint16_t for the 10-bit formats): plane pointers (host arrays),
// one geometry (strides and step in samples) and one flag word.
template <typename S> struct PlaneFrames {
    int n;
    const S* const* y; const S* const* u; const S* const* v;
    int width, height, y_stride, c_stride, c_step, flags;
    // bytes from a plane's first sample to one past its last
    uintptr_t y_span() const { return ((uintptr_t) (height - 1) * (uintptr_t) y_stride + (uintptr_t) width) * sizeof(S); }
    uintptr_t c_span() const {
        return ((uintptr_t) ((height + 1) / 2 - 1) * (uintptr_t) c_stride + (uintptr_t) ((width + 1) / 2 - 1) * (uintptr_t) c_step + 1) * sizeof(S);
    }
    // the planes' spans and the outputs of dst_bytes each, for output_overlaps
    std::vector<Span> spans(uint32_t* const* dst, uintptr_t dst_bytes) const {
        std::vector<Span> sp;
        sp.reserve(4 * (size_t) n);
        for (int i = 0; i < n; ++i) {
            sp.push_back({(uintptr_t) y[i], (uintptr_t) y[i] + y_span(), false});
            sp.push_back({(uintptr_t) u[i], (uintptr_t) u[i] + c_span(), false});
            sp.push_back({(uintptr_t) v[i], (uintptr_t) v[i] + c_span(), false});
            sp.push_back({(uintptr_t) dst[i], (uintptr_t) dst[i] + dst_bytes, true});
        }
        return sp;
    }
};

// The kernels' path for the DEVICE frames [first, first + count) of `a` and their outputs, and whether v is the lower pointer of the
// interleaved pairs (*swap).  The wide paths need, for EVERY one of these frames: width and y_stride multiples of 4 samples and y
// aligned to 4 samples (out16: and the output 16-byte aligned; rows4, the turning codes of nq_orient.hip: and height a multiple of
// 4), and either c_step 2 with u and v one sample apart in the same order, the lower one aligned to 4 samples and c_stride a multiple
// of 4 (interleaved: NV12, NV21, P010), or c_step 1 with u and v aligned to 2 samples and c_stride even (planar: I420, YV12, I010).
// Everything else takes the one-sample path.
template <typename S>
int plane_path(const PlaneFrames<S>& a, uint32_t* const* d_dst, int first, int count, bool out16, bool rows4, bool* swap) {
    const uintptr_t s4 = 4 * sizeof(S) - 1, s2 = 2 * sizeof(S) - 1;
    bool wide = a.width % 4 == 0 && a.y_stride % 4 == 0 && !(rows4 && a.height % 4);
    bool inter = a.c_step == 2 && a.c_stride % 4 == 0, planar = a.c_step == 1 && a.c_stride % 2 == 0;
    int order = 0;                                  // +1: u is the lower pointer of every frame so far, -1: v is
    for (int i = first; i < first + count; ++i) {
        const uintptr_t u = (uintptr_t) a.u[i], v = (uintptr_t) a.v[i];
        wide = wide && !((uintptr_t) a.y[i] & s4) && !(out16 && ((uintptr_t) d_dst[i] & 15));
        const int o = v == u + sizeof(S) ? 1 : u == v + sizeof(S) ? -1 : 0;
        inter = inter && o != 0 && (order == 0 || order == o) && !(std::min(u, v) & s4);
        if (o) order = o;
        planar = planar && !((u | v) & s2);
    }
    *swap = order < 0;
    return wide && inter ? YUV_WIDE_INTERLEAVED : wide && planar ? YUV_WIDE_PLANAR : YUV_BYTE;
}

// Where a frame's planes lie in the staging buffer of plane_host, in bytes: luma, the lower chroma span, the other one
struct PlanePlace { size_t y, lo, hi; bool joined; };

// ... for every frame of `a`, and the bytes they take together: per frame the luma span, then the chroma spans -- ONE span where u's
// and v's overlap or touch (the interleaved layouts, and planes that follow each other) -- each at a 16-byte boundary, which keeps
// what the wide paths need of a layout that has it
template <typename S> size_t plane_places(const PlaneFrames<S>& a, std::vector<PlanePlace>& at) {
    const size_t up16 = 15;
    const uintptr_t yb = a.y_span(), cb = a.c_span();
    at.resize(a.n);
    size_t total = 0;
    for (int i = 0; i < a.n; ++i) {
        const uintptr_t u = (uintptr_t) a.u[i], v = (uintptr_t) a.v[i], lo = std::min(u, v), hi = std::max(u, v);
        at[i].y = total; total += (yb + up16) & ~up16;
        at[i].joined = hi <= lo + cb;
        at[i].lo = total;
        if (at[i].joined) { at[i].hi = total + (hi - lo); total += (hi - lo + cb + up16) & ~up16; }
        else { total += (cb + up16) & ~up16; at[i].hi = total; total += (cb + up16) & ~up16; }
    }
    return total;
}

// The host form of a stage over YUV frames: the planes go up into d_in as plane_places lays them out, the outputs (out_px words each)
// are staged in d_out 16-byte aligned; device(frames, outputs) runs the device form on the staged copies; the outputs come back and
// are waited for.  On failure the stream is waited for too.
template <typename S, typename Device>
int plane_host(std::string& err, hipStream_t s, DevBuf<unsigned char>& d_in, DevBuf<uint32_t>& d_out, const PlaneFrames<S>& a,
               uint32_t* const* dst, size_t out_px, Device device) {
    const int n = a.n;
    const uintptr_t yb = a.y_span(), cb = a.c_span();
    std::vector<PlanePlace> at;
    const size_t total = plane_places(a, at), dpitch = (out_px + 3) & ~(size_t) 3;
    auto body = [&]() -> int {
        NQ_HIP_TO(err, d_in.reserve(total));
        NQ_HIP_TO(err, d_out.reserve(n * dpitch));
        std::vector<const S*> dy(n), du(n), dv(n);
        std::vector<uint32_t*> d_dst(n);
        unsigned char* base = d_in.p;
        for (int i = 0; i < n; ++i) {
            const bool u_low = a.u[i] <= a.v[i];
            const unsigned char* lo = reinterpret_cast<const unsigned char*>(u_low ? a.u[i] : a.v[i]);
            const unsigned char* hi = reinterpret_cast<const unsigned char*>(u_low ? a.v[i] : a.u[i]);
            dy[i] = reinterpret_cast<const S*>(base + at[i].y); d_dst[i] = d_out.p + i * dpitch;
            (u_low ? du : dv)[i] = reinterpret_cast<const S*>(base + at[i].lo);
            (u_low ? dv : du)[i] = reinterpret_cast<const S*>(base + at[i].hi);
            NQ_HIP_TO(err, hipMemcpyAsync(base + at[i].y, a.y[i], yb, hipMemcpyHostToDevice, s));
            if (at[i].joined) {
                NQ_HIP_TO(err, hipMemcpyAsync(base + at[i].lo, lo, (size_t) (hi - lo) + cb, hipMemcpyHostToDevice, s));
            } else {
                NQ_HIP_TO(err, hipMemcpyAsync(base + at[i].lo, lo, cb, hipMemcpyHostToDevice, s));
                NQ_HIP_TO(err, hipMemcpyAsync(base + at[i].hi, hi, cb, hipMemcpyHostToDevice, s));
            }
        }
        PlaneFrames<S> d = a;
        d.y = dy.data(); d.u = du.data(); d.v = dv.data();
        const int rc = device(d, d_dst.data());
        if (rc) return rc;
        for (int i = 0; i < n; ++i) NQ_HIP_TO(err, hipMemcpyAsync(dst[i], d_dst[i], out_px * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
        NQ_HIP_TO(err, hipStreamSynchronize(s));
        return NQ_OK;
    };
    const int rc = body();
    if (rc) (void) hipStreamSynchronize(s);
    return rc;
}

} // namespace

// ---- temporal hold (nq_hold.hip) ----
namespace {

// every argument of both forms, from the host arrays alone (no device work)
int hold_check(nq_handle* h, int n, const uint32_t* const* argb, uint16_t* const* index, uint32_t* const* out_argb, int width, int height,
               int threshold) {
    if (n < 1) NQ_FAIL(h, NQ_ERR_INVALID, "n = %d: at least one frame", n);
    if (width < 1 || width > 65535 || height < 1 || height > 65535) NQ_FAIL(h, NQ_ERR_INVALID, "%d x %d: sides must be 1..65535", width, height);
    if (threshold < 0 || threshold > 255) NQ_FAIL(h, NQ_ERR_INVALID, "threshold = %d: must be 0..255", threshold);
    if ((long long) n * width * height > 2147483647ll)
        NQ_FAIL(h, NQ_ERR_INVALID, "%d frames of %d x %d: more than 2^31 - 1 pixels", n, width, height);
    if (!argb || !index) NQ_FAIL(h, NQ_ERR_INVALID, "the array of frame / index pointers is NULL");
    for (int i = 0; i < n; ++i) {
        if (!argb[i] || ((uintptr_t) argb[i] & 3)) NQ_FAIL(h, NQ_ERR_INVALID, "frame %d: pixel pointer NULL or not 4-byte aligned", i);
        if (!index[i] || ((uintptr_t) index[i] & 1)) NQ_FAIL(h, NQ_ERR_INVALID, "frame %d: index pointer NULL or not 2-byte aligned", i);
        if (out_argb && (!out_argb[i] || ((uintptr_t) out_argb[i] & 3)))
            NQ_FAIL(h, NQ_ERR_INVALID, "frame %d: output pointer NULL or not 4-byte aligned", i);
    }
    return NQ_OK;
}

// nq_hold_frames_device after the checks: the pointer tables go up, one launch walks the sequence, the counters come back when wanted
int hold_device(nq_handle* h, int n, const uint32_t* const* d_argb, uint16_t* const* d_index, uint32_t* const* d_out_argb, int width,
                int height, int threshold, int64_t* out_held) {
    if (n == 1) {                                   // frame 0 is never written
        if (out_held) out_held[0] = 0;
        return NQ_OK;
    }
    std::vector<void*>& t = h->h_hold_ptrs;
    t.assign(3 * (size_t) n, nullptr);
    bool vec = true;                                // the 16-byte path needs every frame of every stream aligned to it
    for (int i = 0; i < n; ++i) {
        t[i] = const_cast<uint32_t*>(d_argb[i]); t[n + (size_t) i] = d_index[i];   // (the kernel reads the sources only)
        if (d_out_argb) t[2 * (size_t) n + i] = d_out_argb[i];
        vec = vec && !(((uintptr_t) d_argb[i] | (uintptr_t) d_index[i] | (uintptr_t) (d_out_argb ? d_out_argb[i] : nullptr)) & 15);
    }
    if (out_held) NQ_HIP(h, h->hold_held.reserve(n));
    const int rc = upload_table(h->err, h->stream, t, h->hold_ptrs);      // (with out_held == NULL the call returns with it only enqueued)
    if (rc) return rc;
    if (out_held) NQ_HIP(h, hipMemsetAsync(h->hold_held.p, 0, n * sizeof(unsigned long long), h->stream));
    launch_hold(reinterpret_cast<const unsigned* const*>(h->hold_ptrs.p), reinterpret_cast<unsigned short* const*>(h->hold_ptrs.p + n),
                d_out_argb ? reinterpret_cast<unsigned* const*>(h->hold_ptrs.p + 2 * (size_t) n) : nullptr, n, (long long) width * height,
                threshold, vec, out_held ? h->hold_held.p : nullptr, h->stream);
    NQ_HIP(h, launch_status());
    if (!out_held) return NQ_OK;
    static_assert(sizeof(int64_t) == sizeof(unsigned long long), "held counters");
    NQ_HIP(h, hipMemcpyAsync(out_held, h->hold_held.p, n * sizeof(int64_t), hipMemcpyDeviceToHost, h->stream));
    NQ_HIP(h, hipStreamSynchronize(h->stream));
    return NQ_OK;
}

} // namespace

extern "C" {

int nq_hold_frames_device(nq_handle* h, int n, const uint32_t* const* d_argb, uint16_t* const* d_index, uint32_t* const* d_out_argb,
                          int width, int height, int threshold, int64_t* out_held) {
    if (!h) return NQ_ERR_INVALID;
    int rc = hold_check(h, n, d_argb, d_index, d_out_argb, width, height, threshold);
    if (rc) return rc;
    rc = use_device(h);
    if (rc) return rc;
    return hold_device(h, n, d_argb, d_index, d_out_argb, width, height, threshold, out_held);
}

int nq_hold_frames(nq_handle* h, int n, const uint32_t* const* argb, uint16_t* const* index, uint32_t* const* out_argb, int width, int height,
                   int threshold, int64_t* out_held) {
    if (!h) return NQ_ERR_INVALID;
    int rc = hold_check(h, n, argb, index, out_argb, width, height, threshold);
    if (rc) return rc;
    rc = use_device(h);
    if (rc) return rc;
    if (n == 1) return hold_device(h, n, argb, index, out_argb, width, height, threshold, out_held);
    // frames lie `pitch` elements apart in the staging buffers, so that every one starts 16-byte aligned (the vector path)
    const size_t px = (size_t) width * height, pitch = (px + 7) & ~(size_t) 7;
    return host_form(h, [&]() -> int {
        NQ_HIP(h, h->d_in.reserve(n * pitch));
        NQ_HIP(h, h->d_out_index.reserve(n * pitch));
        if (out_argb) NQ_HIP(h, h->d_out_argb.reserve(n * pitch));
        std::vector<const uint32_t*> d_src(n);
        std::vector<uint16_t*> d_idx(n);
        std::vector<uint32_t*> d_out(n);
        for (int i = 0; i < n; ++i) {
            d_src[i] = h->d_in.p + i * pitch; d_idx[i] = h->d_out_index.p + i * pitch; d_out[i] = out_argb ? h->d_out_argb.p + i * pitch : nullptr;
            NQ_HIP(h, hipMemcpyAsync(h->d_in.p + i * pitch, argb[i], px * sizeof(uint32_t), hipMemcpyHostToDevice, h->stream));
            NQ_HIP(h, hipMemcpyAsync(d_idx[i], index[i], px * sizeof(uint16_t), hipMemcpyHostToDevice, h->stream));
            if (out_argb) NQ_HIP(h, hipMemcpyAsync(d_out[i], out_argb[i], px * sizeof(uint32_t), hipMemcpyHostToDevice, h->stream));
        }
        const int rc2 = hold_device(h, n, d_src.data(), d_idx.data(), out_argb ? d_out.data() : nullptr, width, height, threshold, out_held);
        if (rc2) return rc2;
        for (int i = 1; i < n; ++i) {
            NQ_HIP(h, hipMemcpyAsync(index[i], d_idx[i], px * sizeof(uint16_t), hipMemcpyDeviceToHost, h->stream));
            if (out_argb) NQ_HIP(h, hipMemcpyAsync(out_argb[i], d_out[i], px * sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream));
        }
        NQ_HIP(h, hipStreamSynchronize(h->stream));
        return NQ_OK;
    });
}

} // extern "C"

// ---- shot detection (nq_shots.hip) ----
namespace {

// the frames of every form, from the host arrays alone (no device work)
int sig_check(nq_handle* h, int n, const uint32_t* const* argb, int width, int height) {
    if (n < 1) NQ_FAIL(h, NQ_ERR_INVALID, "n = %d: at least one frame", n);
    if (width < 1 || width > 65535 || height < 1 || height > 65535) NQ_FAIL(h, NQ_ERR_INVALID, "%d x %d: sides must be 1..65535", width, height);
    if ((long long) n * width * height > 2147483647ll)
        NQ_FAIL(h, NQ_ERR_INVALID, "%d frames of %d x %d: more than 2^31 - 1 pixels", n, width, height);
    if (!argb) NQ_FAIL(h, NQ_ERR_INVALID, "the array of frame pointers is NULL");
    for (int i = 0; i < n; ++i)
        if (!argb[i] || ((uintptr_t) argb[i] & 3)) NQ_FAIL(h, NQ_ERR_INVALID, "frame %d: pixel pointer NULL or not 4-byte aligned", i);
    return NQ_OK;
}

// what the rule takes besides the signatures; false + the reason otherwise
bool shots_check_rule(int threshold_pm, int min_shot, const int32_t* out_starts, const int32_t* out_n_shots, char* why, size_t len) {
    if (threshold_pm < 0 || threshold_pm > 1000) { std::snprintf(why, len, "threshold_pm = %d: must be 0..1000", threshold_pm); return false; }
    if (min_shot < 1) { std::snprintf(why, len, "min_shot = %d: must be at least 1", min_shot); return false; }
    if (!out_starts || !out_n_shots) { std::snprintf(why, len, "out_starts / out_n_shots is NULL"); return false; }
    return true;
}

// floor(1000 max_c E_c / (255 npix)), E_c the 1-D earth mover's distance of channel c's histograms (include/nquant_abi.h)
int shots_score(const uint32_t* a, const uint32_t* b, int64_t npix) {
    int64_t worst = 0;
    for (int c = 0; c < 4; ++c) {
        int64_t cum = 0, e = 0;
        for (int v = 0; v < 255; ++v) {
            cum += (int64_t) a[c * 256 + v] - (int64_t) b[c * 256 + v];
            e += cum < 0 ? -cum : cum;
        }
        worst = std::max(worst, e);
    }
    return (int) (1000 * worst / (255 * npix));
}

// nq_shots_from_signatures: every check first, so that a rejected call has written nothing
int shots_rule(const uint32_t* sig, int n, int64_t npix, int threshold_pm, int min_shot, int32_t* out_starts, int32_t* out_n_shots,
               int32_t* out_scores, char* why, size_t len) {
    if (!shots_check_rule(threshold_pm, min_shot, out_starts, out_n_shots, why, len)) return NQ_ERR_INVALID;
    if (!sig) { std::snprintf(why, len, "sig is NULL"); return NQ_ERR_INVALID; }
    if (n < 1) { std::snprintf(why, len, "n = %d: at least one frame", n); return NQ_ERR_INVALID; }
    if (npix < 1 || npix > 2147483647ll) { std::snprintf(why, len, "npix = %lld: must be 1 .. 2^31 - 1", (long long) npix); return NQ_ERR_INVALID; }
    for (int i = 0; i < n; ++i)
        for (int c = 0; c < 4; ++c) {
            int64_t sum = 0;
            for (int v = 0; v < 256; ++v) sum += sig[(size_t) i * NQ_SIG_WORDS + c * 256 + v];
            if (sum != npix) {
                std::snprintf(why, len, "frame %d: channel %d of the signature sums to %lld, not to npix = %lld", i, c, (long long) sum, (long long) npix);
                return NQ_ERR_INVALID;
            }
        }
    int anchor = 0, shots = 1;
    out_starts[0] = 0;
    if (out_scores) out_scores[0] = 0;
    for (int i = 1; i < n; ++i) {
        const int score = shots_score(sig + (size_t) i * NQ_SIG_WORDS, sig + (size_t) anchor * NQ_SIG_WORDS, npix);
        if (out_scores) out_scores[i] = score;
        if (score > threshold_pm && i - anchor >= min_shot) { out_starts[shots++] = i; anchor = i; }
    }
    *out_n_shots = shots;
    return NQ_OK;
}

// nq_frame_signatures_device after the checks: the pointer table goes up, one launch counts the whole sequence, the counters come back
int signatures_device(nq_handle* h, int n, const uint32_t* const* d_argb, int width, int height, uint32_t* out_sig) {
    std::vector<const uint32_t*>& t = h->h_sig_ptrs;
    t.assign(d_argb, d_argb + n);
    bool vec = true;                                // the 16-byte path needs every frame aligned to it
    for (int i = 0; i < n; ++i) vec = vec && !((uintptr_t) d_argb[i] & 15);
    const size_t words = (size_t) n * NQ_SIG_WORDS;
    NQ_HIP(h, h->d_sig.reserve(words));
    const int rc = upload_table(h->err, h->stream, t, h->sig_ptrs);
    if (rc) return rc;
    NQ_HIP(h, hipMemsetAsync(h->d_sig.p, 0, words * sizeof(uint32_t), h->stream));
    launch_signatures(reinterpret_cast<const unsigned* const*>(h->sig_ptrs.p), n, (long long) width * height, vec, h->n_cus, h->d_sig.p, h->stream);
    NQ_HIP(h, launch_status());
    NQ_HIP(h, hipMemcpyAsync(out_sig, h->d_sig.p, words * sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream));
    NQ_HIP(h, hipStreamSynchronize(h->stream));
    return NQ_OK;
}

// nq_frame_signatures after the checks: the frames lie `pitch` elements apart in d_in, so that every one starts 16-byte aligned
int signatures_host(nq_handle* h, int n, const uint32_t* const* argb, int width, int height, uint32_t* out_sig) {
    const size_t px = (size_t) width * height, pitch = (px + 3) & ~(size_t) 3;
    return host_form(h, [&]() -> int {
        NQ_HIP(h, h->d_in.reserve(n * pitch));
        std::vector<const uint32_t*> d_src(n);
        for (int i = 0; i < n; ++i) {
            d_src[i] = h->d_in.p + i * pitch;
            NQ_HIP(h, hipMemcpyAsync(h->d_in.p + i * pitch, argb[i], px * sizeof(uint32_t), hipMemcpyHostToDevice, h->stream));
        }
        return signatures_device(h, n, d_src.data(), width, height, out_sig);
    });
}

// both forms of nq_frame_signatures / nq_detect_shots (out_sig null: detect, the signatures stay in the handle)
int shots_call(nq_handle* h, bool host, bool detect, int n, const uint32_t* const* argb, int width, int height, uint32_t* out_sig,
               int threshold_pm, int min_shot, int32_t* out_starts, int32_t* out_n_shots, int32_t* out_scores) {
    if (!h) return NQ_ERR_INVALID;
    int rc = sig_check(h, n, argb, width, height);
    if (rc) return rc;
    char why[256];
    if (detect && !shots_check_rule(threshold_pm, min_shot, out_starts, out_n_shots, why, sizeof why)) NQ_FAIL(h, NQ_ERR_INVALID, "%s", why);
    if (!detect && !out_sig) NQ_FAIL(h, NQ_ERR_INVALID, "out_sig is NULL");
    rc = use_device(h);
    if (rc) return rc;
    if (detect) {
        h->h_sig.resize((size_t) n * NQ_SIG_WORDS);
        out_sig = h->h_sig.data();
    }
    rc = host ? signatures_host(h, n, argb, width, height, out_sig) : signatures_device(h, n, argb, width, height, out_sig);
    if (rc || !detect) return rc;
    rc = shots_rule(out_sig, n, (int64_t) width * height, threshold_pm, min_shot, out_starts, out_n_shots, out_scores, why, sizeof why);
    if (rc) NQ_FAIL(h, rc, "%s", why);
    return NQ_OK;
}

} // namespace

extern "C" {

int nq_frame_signatures_device(nq_handle* h, int n, const uint32_t* const* d_argb, int width, int height, uint32_t* out_sig) {
    return shots_call(h, false, false, n, d_argb, width, height, out_sig, 0, 1, nullptr, nullptr, nullptr);
}

int nq_frame_signatures(nq_handle* h, int n, const uint32_t* const* argb, int width, int height, uint32_t* out_sig) {
    return shots_call(h, true, false, n, argb, width, height, out_sig, 0, 1, nullptr, nullptr, nullptr);
}

int nq_shots_from_signatures(const uint32_t* sig, int n, int64_t npix, int threshold_pm, int min_shot, int32_t* out_starts,
                             int32_t* out_n_shots, int32_t* out_scores) {
    char why[256];
    return shots_rule(sig, n, npix, threshold_pm, min_shot, out_starts, out_n_shots, out_scores, why, sizeof why);
}

int nq_detect_shots_device(nq_handle* h, int n, const uint32_t* const* d_argb, int width, int height, int threshold_pm, int min_shot,
                           int32_t* out_starts, int32_t* out_n_shots, int32_t* out_scores) {
    return shots_call(h, false, true, n, d_argb, width, height, nullptr, threshold_pm, min_shot, out_starts, out_n_shots, out_scores);
}

int nq_detect_shots(nq_handle* h, int n, const uint32_t* const* argb, int width, int height, int threshold_pm, int min_shot,
                    int32_t* out_starts, int32_t* out_n_shots, int32_t* out_scores) {
    return shots_call(h, true, true, n, argb, width, height, nullptr, threshold_pm, min_shot, out_starts, out_n_shots, out_scores);
}

} // extern "C"

// ---- palette refinement (nq_refine.hip) ----
extern "C" {

int nq_refine_palette_device(nq_handle* h, int n, const uint32_t* const* d_argb, const int32_t* widths, const int32_t* heights,
                             uint32_t* io_palette, int K, int iterations, int64_t* out_sse, int64_t* out_counts, int32_t* out_passes) {
    return refine_call(h, false, n, d_argb, widths, heights, io_palette, K, iterations, out_sse, out_counts, out_passes);
}

int nq_refine_palette(nq_handle* h, int n, const uint32_t* const* argb, const int32_t* widths, const int32_t* heights,
                      uint32_t* io_palette, int K, int iterations, int64_t* out_sse, int64_t* out_counts, int32_t* out_passes) {
    return refine_call(h, true, n, argb, widths, heights, io_palette, K, iterations, out_sse, out_counts, out_passes);
}

} // extern "C"

// ---- frame reduction (nq_resample.hip) ----
namespace {

// every argument of both forms, from the host arrays alone (no device work)
int resample_check(nq_handle* h, int n, const uint32_t* const* src, int src_width, int src_height, int crop_x, int crop_y, int crop_w,
                   int crop_h, uint32_t* const* dst, int dst_width, int dst_height, int flags) {
    if (n < 1) NQ_FAIL(h, NQ_ERR_INVALID, "n = %d: at least one frame", n);
    if (src_width < 1 || src_width > 65535 || src_height < 1 || src_height > 65535)
        NQ_FAIL(h, NQ_ERR_INVALID, "%d x %d: source sides must be 1..65535", src_width, src_height);
    const int rc = reduce_check(h->err, src_width, src_height, crop_x, crop_y, crop_w, crop_h, dst_width, dst_height, flags);
    if (rc) return rc;
    if ((long long) n * src_width * src_height > 2147483647ll)
        NQ_FAIL(h, NQ_ERR_INVALID, "%d frames of %d x %d: more than 2^31 - 1 pixels", n, src_width, src_height);
    if (!src || !dst) NQ_FAIL(h, NQ_ERR_INVALID, "the array of source / output pointers is NULL");
    for (int i = 0; i < n; ++i) {
        if (!src[i] || ((uintptr_t) src[i] & 3)) NQ_FAIL(h, NQ_ERR_INVALID, "frame %d: source pointer NULL or not 4-byte aligned", i);
        if (!dst[i] || ((uintptr_t) dst[i] & 3)) NQ_FAIL(h, NQ_ERR_INVALID, "frame %d: output pointer NULL or not 4-byte aligned", i);
    }
    std::vector<Span> spans;
    spans.reserve(2 * (size_t) n);
    const uintptr_t src_bytes = (uintptr_t) src_width * src_height * sizeof(uint32_t), dst_bytes = (uintptr_t) dst_width * dst_height * sizeof(uint32_t);
    for (int i = 0; i < n; ++i) {
        spans.push_back({(uintptr_t) src[i], (uintptr_t) src[i] + src_bytes, false});
        spans.push_back({(uintptr_t) dst[i], (uintptr_t) dst[i] + dst_bytes, true});
    }
    if (output_overlaps(spans)) NQ_FAIL(h, NQ_ERR_INVALID, "an output overlaps a source frame or another output");
    return NQ_OK;
}

// nq_resample_frames_device after the checks: the pointer tables go up, one launch reduces the sequence
int resample_device(nq_handle* h, int n, const uint32_t* const* d_src, int src_width, int crop_x, int crop_y, int crop_w, int crop_h,
                    uint32_t* const* d_dst, int dst_width, int dst_height, int flags) {
    std::vector<void*>& t = h->h_resample_ptrs;
    t.assign(2 * (size_t) n, nullptr);
    bool vec = src_width % 4 == 0;                  // the 16-byte path needs every row of every source aligned to it
    for (int i = 0; i < n; ++i) {
        t[i] = const_cast<uint32_t*>(d_src[i]); t[n + (size_t) i] = d_dst[i];     // (the kernel reads the sources only)
        vec = vec && !((uintptr_t) d_src[i] & 15);
    }
    const int rc = upload_table(h->err, h->stream, t, h->resample_ptrs);
    if (rc) return rc;
    launch_resample(reinterpret_cast<const unsigned* const*>(h->resample_ptrs.p), reinterpret_cast<unsigned* const*>(h->resample_ptrs.p + n), n,
                    src_width, crop_x, crop_y, crop_w, crop_h, dst_width, dst_height, (flags & NQ_RESAMPLE_LINEAR) != 0, vec, h->stream);
    NQ_HIP(h, launch_status());
    return NQ_OK;
}

} // namespace

extern "C" {

int nq_resample_frames_device(nq_handle* h, int n, const uint32_t* const* d_src, int src_width, int src_height, int crop_x, int crop_y,
                              int crop_w, int crop_h, uint32_t* const* d_dst, int dst_width, int dst_height, int flags) {
    if (!h) return NQ_ERR_INVALID;
    int rc = resample_check(h, n, d_src, src_width, src_height, crop_x, crop_y, crop_w, crop_h, d_dst, dst_width, dst_height, flags);
    if (rc) return rc;
    rc = use_device(h);
    if (rc) return rc;
    return resample_device(h, n, d_src, src_width, crop_x, crop_y, crop_w, crop_h, d_dst, dst_width, dst_height, flags);
}

int nq_resample_frames(nq_handle* h, int n, const uint32_t* const* src, int src_width, int src_height, int crop_x, int crop_y, int crop_w,
                       int crop_h, uint32_t* const* dst, int dst_width, int dst_height, int flags) {
    if (!h) return NQ_ERR_INVALID;
    int rc = resample_check(h, n, src, src_width, src_height, crop_x, crop_y, crop_w, crop_h, dst, dst_width, dst_height, flags);
    if (rc) return rc;
    rc = use_device(h);
    if (rc) return rc;
    return argb_host(h->err, h->stream, h->d_in, h->d_out_argb, n, src, (size_t) src_width * src_height, n, dst, (size_t) dst_width * dst_height,
                     [&](const uint32_t* const* d_src, uint32_t* const* d_dst) {
        return resample_device(h, n, d_src, src_width, crop_x, crop_y, crop_w, crop_h, d_dst, dst_width, dst_height, flags);
    });
}

} // extern "C"

// ---- YUV input (nq_yuv.hip) ----
namespace {

using YuvFrames = PlaneFrames<uint8_t>;

// floor(65536 e + 1/2) of the rationals of include/nquant_abi.h "YUV input", by flag word: {cy, crv, cgu, cgv, cbu, yo}
const YuvCoef YUV_COEF[4] = {
    {76309, 104597, 25675, 53279, 132201, 16},      // BT.601, limited range
    {76309, 117489, 13975, 34925, 138438, 16},      // NQ_YUV_BT709
    {65536, 91881, 22553, 46802, 116130, 0},        // NQ_YUV_FULL_RANGE
    {65536, 103206, 12276, 30679, 121609, 0},       // both
};

// every argument of the four entry points, from the host arrays alone (no device work).  nq_frames_from_yuv* pass the whole frame as
// crop and target, and flags 0.
int yuv_check(nq_handle* h, const YuvFrames& a, int crop_x, int crop_y, int crop_w, int crop_h, uint32_t* const* dst, int dst_width,
              int dst_height, int flags) {
    const int n = a.n;
    if (n < 1) NQ_FAIL(h, NQ_ERR_INVALID, "n = %d: at least one frame", n);
    if (a.width < 1 || a.width > 65535 || a.height < 1 || a.height > 65535)
        NQ_FAIL(h, NQ_ERR_INVALID, "%d x %d: source sides must be 1..65535", a.width, a.height);
    if (a.y_stride < a.width) NQ_FAIL(h, NQ_ERR_INVALID, "y_stride = %d: shorter than a row of %d pixels", a.y_stride, a.width);
    if (a.c_step != 1 && a.c_step != 2) NQ_FAIL(h, NQ_ERR_INVALID, "c_step = %d: must be 1 or 2", a.c_step);
    if (a.c_stride < a.c_step * ((a.width + 1) / 2 - 1) + 1)
        NQ_FAIL(h, NQ_ERR_INVALID, "c_stride = %d: shorter than a chroma row of %d samples %d apart", a.c_stride, (a.width + 1) / 2, a.c_step);
    if (a.flags & ~(NQ_YUV_BT709 | NQ_YUV_FULL_RANGE)) NQ_FAIL(h, NQ_ERR_INVALID, "yuv_flags = 0x%x: unknown bits", (unsigned) a.flags);
    const int rc = reduce_check(h->err, a.width, a.height, crop_x, crop_y, crop_w, crop_h, dst_width, dst_height, flags);
    if (rc) return rc;
    if ((long long) n * a.width * a.height > 2147483647ll)
        NQ_FAIL(h, NQ_ERR_INVALID, "%d frames of %d x %d: more than 2^31 - 1 pixels", n, a.width, a.height);
    if (!a.y || !a.u || !a.v || !dst) NQ_FAIL(h, NQ_ERR_INVALID, "an array of plane / output pointers is NULL");
    for (int i = 0; i < n; ++i) {
        if (!a.y[i] || !a.u[i] || !a.v[i]) NQ_FAIL(h, NQ_ERR_INVALID, "frame %d: a plane pointer is NULL", i);
        if (!dst[i] || ((uintptr_t) dst[i] & 3)) NQ_FAIL(h, NQ_ERR_INVALID, "frame %d: output pointer NULL or not 4-byte aligned", i);
    }
    std::vector<Span> spans = a.spans(dst, (uintptr_t) dst_width * dst_height * sizeof(uint32_t));
    if (output_overlaps(spans)) NQ_FAIL(h, NQ_ERR_INVALID, "an output overlaps a source plane or another output");
    return NQ_OK;
}

// The kernels' path for DEVICE frames `a` and outputs d_dst -- plane_path over the whole call -- and the pointer table on its way to
// the device.
int yuv_table(nq_handle* h, const YuvFrames& a, uint32_t* const* d_dst, bool out16, int* path, bool* swap, bool rows4 = false) {
    const int n = a.n;
    *path = plane_path(a, d_dst, 0, n, out16, rows4, swap);
    std::vector<const void*>& t = h->h_yuv_ptrs;
    t.assign(4 * (size_t) n, nullptr);
    for (int i = 0; i < n; ++i) {
        t[i] = a.y[i];
        t[n + (size_t) i] = *path == YUV_WIDE_INTERLEAVED ? std::min(a.u[i], a.v[i]) : a.u[i];
        t[2 * (size_t) n + i] = a.v[i];
        t[3 * (size_t) n + i] = d_dst[i];             // (the only pointers the kernels write through)
    }
    return upload_table(h->err, h->stream, t, h->yuv_ptrs);
}

// nq_frames_from_yuv_device after the checks: the pointer table goes up, one launch converts the sequence
int yuv_device(nq_handle* h, const YuvFrames& a, uint32_t* const* d_dst) {
    int path; bool swap;
    const int rc = yuv_table(h, a, d_dst, true, &path, &swap);
    if (rc) return rc;
    launch_yuv_argb(h->yuv_ptrs.p, a.n, a.width, a.height, a.y_stride, a.c_stride, a.c_step, path, swap, YUV_COEF[a.flags], h->stream);
    NQ_HIP(h, launch_status());
    return NQ_OK;
}

// nq_resample_frames_yuv_device after the checks: the pointer table goes up, one launch converts and reduces the sequence
int resample_yuv_device(nq_handle* h, const YuvFrames& a, int crop_x, int crop_y, int crop_w, int crop_h, uint32_t* const* d_dst,
                        int dst_width, int dst_height, int flags) {
    int path; bool swap;
    const int rc = yuv_table(h, a, d_dst, false, &path, &swap);
    if (rc) return rc;
    launch_resample_yuv(h->yuv_ptrs.p, a.n, a.y_stride, a.c_stride, a.c_step, path, swap, YUV_COEF[a.flags], crop_x, crop_y, crop_w,
                        crop_h, dst_width, dst_height, (flags & NQ_RESAMPLE_LINEAR) != 0, h->stream);
    NQ_HIP(h, launch_status());
    return NQ_OK;
}

// The host forms: plane_host with the handle's buffers (the planes in yuv_in, the outputs of out_px words each in d_out_argb)
template <typename Device>
int yuv_host(nq_handle* h, const YuvFrames& a, uint32_t* const* dst, size_t out_px, Device device) {
    return plane_host(h->err, h->stream, h->yuv_in, h->d_out_argb, a, dst, out_px, device);
}

} // namespace

extern "C" {

int nq_frames_from_yuv_device(nq_handle* h, int n, const uint8_t* const* d_y, const uint8_t* const* d_u, const uint8_t* const* d_v,
                              int width, int height, int y_stride, int c_stride, int c_step, int yuv_flags, uint32_t* const* d_dst) {
    if (!h) return NQ_ERR_INVALID;
    const YuvFrames a = {n, d_y, d_u, d_v, width, height, y_stride, c_stride, c_step, yuv_flags};
    int rc = yuv_check(h, a, 0, 0, width, height, d_dst, width, height, 0);
    if (rc) return rc;
    rc = use_device(h);
    if (rc) return rc;
    return yuv_device(h, a, d_dst);
}

int nq_frames_from_yuv(nq_handle* h, int n, const uint8_t* const* y, const uint8_t* const* u, const uint8_t* const* v,
                       int width, int height, int y_stride, int c_stride, int c_step, int yuv_flags, uint32_t* const* dst) {
    if (!h) return NQ_ERR_INVALID;
    const YuvFrames a = {n, y, u, v, width, height, y_stride, c_stride, c_step, yuv_flags};
    int rc = yuv_check(h, a, 0, 0, width, height, dst, width, height, 0);
    if (rc) return rc;
    rc = use_device(h);
    if (rc) return rc;
    return yuv_host(h, a, dst, (size_t) width * height, [&](const YuvFrames& d, uint32_t* const* d_dst) { return yuv_device(h, d, d_dst); });
}

int nq_resample_frames_yuv_device(nq_handle* h, int n, const uint8_t* const* d_y, const uint8_t* const* d_u, const uint8_t* const* d_v,
                                  int src_width, int src_height, int y_stride, int c_stride, int c_step, int yuv_flags,
                                  int crop_x, int crop_y, int crop_w, int crop_h,
                                  uint32_t* const* d_dst, int dst_width, int dst_height, int flags) {
    if (!h) return NQ_ERR_INVALID;
    const YuvFrames a = {n, d_y, d_u, d_v, src_width, src_height, y_stride, c_stride, c_step, yuv_flags};
    int rc = yuv_check(h, a, crop_x, crop_y, crop_w, crop_h, d_dst, dst_width, dst_height, flags);
    if (rc) return rc;
    rc = use_device(h);
    if (rc) return rc;
    return resample_yuv_device(h, a, crop_x, crop_y, crop_w, crop_h, d_dst, dst_width, dst_height, flags);
}

int nq_resample_frames_yuv(nq_handle* h, int n, const uint8_t* const* y, const uint8_t* const* u, const uint8_t* const* v,
                           int src_width, int src_height, int y_stride, int c_stride, int c_step, int yuv_flags,
                           int crop_x, int crop_y, int crop_w, int crop_h,
                           uint32_t* const* dst, int dst_width, int dst_height, int flags) {
    if (!h) return NQ_ERR_INVALID;
    const YuvFrames a = {n, y, u, v, src_width, src_height, y_stride, c_stride, c_step, yuv_flags};
    int rc = yuv_check(h, a, crop_x, crop_y, crop_w, crop_h, dst, dst_width, dst_height, flags);
    if (rc) return rc;
    rc = use_device(h);
    if (rc) return rc;
    return yuv_host(h, a, dst, (size_t) dst_width * dst_height, [&](const YuvFrames& d, uint32_t* const* d_dst) {
        return resample_yuv_device(h, d, crop_x, crop_y, crop_w, crop_h, d_dst, dst_width, dst_height, flags);
    });
}

} // extern "C"

// ---- orientation (nq_orient.hip) ----
namespace {

// The geometry of an oriented call, from its numbers alone: the code, the source sides, and -- reduce: for the reducing calls -- the
// crop against the ORIENTED frame.  On success the crop is mapped back into source coordinates and, for the turning codes, the
// target's sides are swapped: the reducer runs on the source with these, and orienting its result gives the call's (orienting
// commutes with the reducer: DESIGN.md 5h).  out(x, y) = src(sx, sy) with sx running with or against (fx) one oriented axis and sy
// with or against (fy) the other; codes 5..8 swap the axes.
int orient_geometry(nq_handle* h, int width, int height, int orientation, bool reduce, int* crop_x, int* crop_y, int* crop_w, int* crop_h,
                    int* dst_width, int* dst_height) {
    if (orientation < 1 || orientation > 8) NQ_FAIL(h, NQ_ERR_INVALID, "orientation = %d: must be 1..8 (EXIF)", orientation);
    if (width < 1 || width > 65535 || height < 1 || height > 65535)
        NQ_FAIL(h, NQ_ERR_INVALID, "%d x %d: source sides must be 1..65535", width, height);
    if (!reduce) return NQ_OK;
    const bool turn = orientation >= 5;
    const bool fx = orientation == 2 || orientation == 3 || orientation == 7 || orientation == 8;
    const bool fy = orientation == 3 || orientation == 4 || orientation == 6 || orientation == 7;
    const int ow = turn ? height : width, oh = turn ? width : height;
    const int cx = *crop_x, cy = *crop_y, cw = *crop_w, ch = *crop_h;
    if (cw < 1 || ch < 1 || cx < 0 || cy < 0 || cx > ow - cw || cy > oh - ch)
        NQ_FAIL(h, NQ_ERR_INVALID, "crop %d x %d at (%d, %d): empty or outside the oriented %d x %d frame", cw, ch, cx, cy, ow, oh);
    // along the source's columns lies the oriented y axis when the code turns, else the x axis
    const int a = turn ? cy : cx, al = turn ? ch : cw, b = turn ? cx : cy, bl = turn ? cw : ch;
    *crop_x = fx ? width - a - al : a; *crop_w = al;
    *crop_y = fy ? height - b - bl : b; *crop_h = bl;
    if (turn) std::swap(*dst_width, *dst_height);
    return NQ_OK;
}

// nq_orient_frames_device after the checks: the pointer tables go up, one launch orients the sequence
int orient_device(nq_handle* h, int n, const uint32_t* const* d_src, int width, int height, int orientation, uint32_t* const* d_dst) {
    std::vector<void*>& t = h->h_orient_ptrs;
    t.assign(2 * (size_t) n, nullptr);
    bool wide = width % 4 == 0 && !(orientation >= 5 && height % 4);     // the 16-byte path: loads along width, turned stores along height
    for (int i = 0; i < n; ++i) {
        t[i] = const_cast<uint32_t*>(d_src[i]); t[n + (size_t) i] = d_dst[i];     // (the kernel reads the sources only)
        wide = wide && !(((uintptr_t) d_src[i] | (uintptr_t) d_dst[i]) & 15);
    }
    const int rc = upload_table(h->err, h->stream, t, h->orient_ptrs);
    if (rc) return rc;
    launch_orient(reinterpret_cast<const unsigned* const*>(h->orient_ptrs.p), reinterpret_cast<unsigned* const*>(h->orient_ptrs.p + n), n, width,
                  height, orientation, wide, h->stream);
    NQ_HIP(h, launch_status());
    return NQ_OK;
}

// room for n reduced frames of px words in orient_tmp, each at a 16-byte boundary (growing the buffer frees the old one, which waits
// for the device)
int orient_room(nq_handle* h, int n, size_t px, std::vector<uint32_t*>& d_tmp) {
    const size_t pitch = (px + 3) & ~(size_t) 3;
    NQ_HIP(h, h->orient_tmp.reserve(n * pitch));
    d_tmp.resize(n);
    for (int i = 0; i < n; ++i) d_tmp[i] = h->orient_tmp.p + i * pitch;
    return NQ_OK;
}

// nq_resample_frames_oriented_device after the checks; crop and target are the SOURCE's (orient_geometry).  Code 1 is the reducer alone.
int resample_oriented_device(nq_handle* h, int n, const uint32_t* const* d_src, int src_width, int orientation, int crop_x, int crop_y,
                             int crop_w, int crop_h, uint32_t* const* d_dst, int dst_width, int dst_height, int flags) {
    if (orientation == 1) return resample_device(h, n, d_src, src_width, crop_x, crop_y, crop_w, crop_h, d_dst, dst_width, dst_height, flags);
    std::vector<uint32_t*> d_tmp;
    int rc = orient_room(h, n, (size_t) dst_width * dst_height, d_tmp);
    if (rc) return rc;
    rc = resample_device(h, n, d_src, src_width, crop_x, crop_y, crop_w, crop_h, d_tmp.data(), dst_width, dst_height, flags);
    if (rc) return rc;
    return orient_device(h, n, d_tmp.data(), dst_width, dst_height, orientation, d_dst);
}

// nq_frames_from_yuv_oriented_device after the checks: the pointer table goes up, one launch converts and orients the sequence
int yuv_orient_device(nq_handle* h, const YuvFrames& a, int orientation, uint32_t* const* d_dst) {
    int path; bool swap;
    const int rc = yuv_table(h, a, d_dst, true, &path, &swap, orientation >= 5);
    if (rc) return rc;
    launch_yuv_orient(h->yuv_ptrs.p, a.n, a.width, a.height, a.y_stride, a.c_stride, a.c_step, path, swap, YUV_COEF[a.flags], orientation,
                      h->stream);
    NQ_HIP(h, launch_status());
    return NQ_OK;
}

// nq_resample_frames_yuv_oriented_device after the checks; crop and target are the SOURCE's.  Code 1 is the fused reducer alone.
int resample_yuv_oriented_device(nq_handle* h, const YuvFrames& a, int orientation, int crop_x, int crop_y, int crop_w, int crop_h,
                                 uint32_t* const* d_dst, int dst_width, int dst_height, int flags) {
    if (orientation == 1) return resample_yuv_device(h, a, crop_x, crop_y, crop_w, crop_h, d_dst, dst_width, dst_height, flags);
    std::vector<uint32_t*> d_tmp;
    int rc = orient_room(h, a.n, (size_t) dst_width * dst_height, d_tmp);
    if (rc) return rc;
    rc = resample_yuv_device(h, a, crop_x, crop_y, crop_w, crop_h, d_tmp.data(), dst_width, dst_height, flags);
    if (rc) return rc;
    return orient_device(h, a.n, d_tmp.data(), dst_width, dst_height, orientation, d_dst);
}

// every argument of both forms of nq_orient_frames: resample_check's, with the whole frame as crop and target (a turned output
// holds as many words)
int orient_check(nq_handle* h, int n, const uint32_t* const* src, int width, int height, int orientation, uint32_t* const* dst) {
    const int rc = orient_geometry(h, width, height, orientation, false, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr);
    return rc ? rc : resample_check(h, n, src, width, height, 0, 0, width, height, dst, width, height, 0);
}

// ... of nq_resample_frames_oriented: on success crop and target are the source's
int resample_oriented_check(nq_handle* h, int n, const uint32_t* const* src, int width, int height, int orientation, int* crop_x, int* crop_y,
                            int* crop_w, int* crop_h, uint32_t* const* dst, int* dst_width, int* dst_height, int flags) {
    const int rc = orient_geometry(h, width, height, orientation, true, crop_x, crop_y, crop_w, crop_h, dst_width, dst_height);
    return rc ? rc : resample_check(h, n, src, width, height, *crop_x, *crop_y, *crop_w, *crop_h, dst, *dst_width, *dst_height, flags);
}

} // namespace

extern "C" {

int nq_orient_frames_device(nq_handle* h, int n, const uint32_t* const* d_src, int src_width, int src_height, int orientation,
                            uint32_t* const* d_dst) {
    if (!h) return NQ_ERR_INVALID;
    int rc = orient_check(h, n, d_src, src_width, src_height, orientation, d_dst);
    if (rc) return rc;
    rc = use_device(h);
    if (rc) return rc;
    return orient_device(h, n, d_src, src_width, src_height, orientation, d_dst);
}

int nq_orient_frames(nq_handle* h, int n, const uint32_t* const* src, int src_width, int src_height, int orientation, uint32_t* const* dst) {
    if (!h) return NQ_ERR_INVALID;
    int rc = orient_check(h, n, src, src_width, src_height, orientation, dst);
    if (rc) return rc;
    rc = use_device(h);
    if (rc) return rc;
    const size_t px = (size_t) src_width * src_height;
    return argb_host(h->err, h->stream, h->d_in, h->d_out_argb, n, src, px, n, dst, px, [&](const uint32_t* const* d_src, uint32_t* const* d_dst) {
        return orient_device(h, n, d_src, src_width, src_height, orientation, d_dst);
    });
}

int nq_resample_frames_oriented_device(nq_handle* h, int n, const uint32_t* const* d_src, int src_width, int src_height, int orientation,
                                       int crop_x, int crop_y, int crop_w, int crop_h, uint32_t* const* d_dst, int dst_width,
                                       int dst_height, int flags) {
    if (!h) return NQ_ERR_INVALID;
    int rc = resample_oriented_check(h, n, d_src, src_width, src_height, orientation, &crop_x, &crop_y, &crop_w, &crop_h, d_dst, &dst_width,
                                     &dst_height, flags);
    if (rc) return rc;
    rc = use_device(h);
    if (rc) return rc;
    return resample_oriented_device(h, n, d_src, src_width, orientation, crop_x, crop_y, crop_w, crop_h, d_dst, dst_width, dst_height, flags);
}

int nq_resample_frames_oriented(nq_handle* h, int n, const uint32_t* const* src, int src_width, int src_height, int orientation,
                                int crop_x, int crop_y, int crop_w, int crop_h, uint32_t* const* dst, int dst_width, int dst_height,
                                int flags) {
    if (!h) return NQ_ERR_INVALID;
    int rc = resample_oriented_check(h, n, src, src_width, src_height, orientation, &crop_x, &crop_y, &crop_w, &crop_h, dst, &dst_width,
                                     &dst_height, flags);
    if (rc) return rc;
    rc = use_device(h);
    if (rc) return rc;
    return argb_host(h->err, h->stream, h->d_in, h->d_out_argb, n, src, (size_t) src_width * src_height, n, dst, (size_t) dst_width * dst_height,
                     [&](const uint32_t* const* d_src, uint32_t* const* d_dst) {
        return resample_oriented_device(h, n, d_src, src_width, orientation, crop_x, crop_y, crop_w, crop_h, d_dst, dst_width, dst_height, flags);
    });
}

int nq_frames_from_yuv_oriented_device(nq_handle* h, int n, const uint8_t* const* d_y, const uint8_t* const* d_u, const uint8_t* const* d_v,
                                       int width, int height, int y_stride, int c_stride, int c_step, int yuv_flags, int orientation,
                                       uint32_t* const* d_dst) {
    if (!h) return NQ_ERR_INVALID;
    const YuvFrames a = {n, d_y, d_u, d_v, width, height, y_stride, c_stride, c_step, yuv_flags};
    int rc = orient_geometry(h, width, height, orientation, false, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr);
    if (!rc) rc = yuv_check(h, a, 0, 0, width, height, d_dst, width, height, 0);
    if (rc) return rc;
    rc = use_device(h);
    if (rc) return rc;
    return yuv_orient_device(h, a, orientation, d_dst);
}

int nq_frames_from_yuv_oriented(nq_handle* h, int n, const uint8_t* const* y, const uint8_t* const* u, const uint8_t* const* v,
                                int width, int height, int y_stride, int c_stride, int c_step, int yuv_flags, int orientation,
                                uint32_t* const* dst) {
    if (!h) return NQ_ERR_INVALID;
    const YuvFrames a = {n, y, u, v, width, height, y_stride, c_stride, c_step, yuv_flags};
    int rc = orient_geometry(h, width, height, orientation, false, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr);
    if (!rc) rc = yuv_check(h, a, 0, 0, width, height, dst, width, height, 0);
    if (rc) return rc;
    rc = use_device(h);
    if (rc) return rc;
    return yuv_host(h, a, dst, (size_t) width * height,
                    [&](const YuvFrames& d, uint32_t* const* d_dst) { return yuv_orient_device(h, d, orientation, d_dst); });
}

int nq_resample_frames_yuv_oriented_device(nq_handle* h, int n, const uint8_t* const* d_y, const uint8_t* const* d_u,
                                           const uint8_t* const* d_v, int src_width, int src_height, int y_stride, int c_stride, int c_step,
                                           int yuv_flags, int orientation, int crop_x, int crop_y, int crop_w, int crop_h,
                                           uint32_t* const* d_dst, int dst_width, int dst_height, int flags) {
    if (!h) return NQ_ERR_INVALID;
    const YuvFrames a = {n, d_y, d_u, d_v, src_width, src_height, y_stride, c_stride, c_step, yuv_flags};
    int rc = orient_geometry(h, src_width, src_height, orientation, true, &crop_x, &crop_y, &crop_w, &crop_h, &dst_width, &dst_height);
    if (!rc) rc = yuv_check(h, a, crop_x, crop_y, crop_w, crop_h, d_dst, dst_width, dst_height, flags);
    if (rc) return rc;
    rc = use_device(h);
    if (rc) return rc;
    return resample_yuv_oriented_device(h, a, orientation, crop_x, crop_y, crop_w, crop_h, d_dst, dst_width, dst_height, flags);
}

int nq_resample_frames_yuv_oriented(nq_handle* h, int n, const uint8_t* const* y, const uint8_t* const* u, const uint8_t* const* v,
                                    int src_width, int src_height, int y_stride, int c_stride, int c_step, int yuv_flags, int orientation,
                                    int crop_x, int crop_y, int crop_w, int crop_h, uint32_t* const* dst, int dst_width, int dst_height,
                                    int flags) {
    if (!h) return NQ_ERR_INVALID;
    const YuvFrames a = {n, y, u, v, src_width, src_height, y_stride, c_stride, c_step, yuv_flags};
    int rc = orient_geometry(h, src_width, src_height, orientation, true, &crop_x, &crop_y, &crop_w, &crop_h, &dst_width, &dst_height);
    if (!rc) rc = yuv_check(h, a, crop_x, crop_y, crop_w, crop_h, dst, dst_width, dst_height, flags);
    if (rc) return rc;
    rc = use_device(h);
    if (rc) return rc;
    return yuv_host(h, a, dst, (size_t) dst_width * dst_height, [&](const YuvFrames& d, uint32_t* const* d_dst) {
        return resample_yuv_oriented_device(h, d, orientation, crop_x, crop_y, crop_w, crop_h, d_dst, dst_width, dst_height, flags);
    });
}

} // extern "C"

// ---- ordered dither (nq_ordered.hip) ----
namespace {

// the frames and outputs of every form, from the host arrays alone (no device work): the sizes first, then the pointers
int ordered_check_frames(nq_handle* h, int n, const uint32_t* const* argb, const int32_t* widths, const int32_t* heights,
                         uint32_t* const* out_argb, uint16_t* const* out_index, int64_t* out_total) {
    if (n < 1) NQ_FAIL(h, NQ_ERR_INVALID, "n = %d: at least one frame", n);
    if (!argb || !widths || !heights) NQ_FAIL(h, NQ_ERR_INVALID, "the array of frame pointers, widths or heights is NULL");
    if (!out_index) NQ_FAIL(h, NQ_ERR_INVALID, "the array of index pointers is NULL");
    int64_t total = 0;
    for (int i = 0; i < n; ++i) {
        if (widths[i] < 1 || widths[i] > 65535 || heights[i] < 1 || heights[i] > 65535)
            NQ_FAIL(h, NQ_ERR_INVALID, "frame %d: %d x %d: sides must be 1..65535", i, widths[i], heights[i]);
        total += (int64_t) widths[i] * heights[i];
        if (total > 2147483647ll) NQ_FAIL(h, NQ_ERR_INVALID, "the sequence holds more than 2^31 - 1 pixels (frame %d)", i);
    }
    for (int i = 0; i < n; ++i) {
        if (!argb[i] || ((uintptr_t) argb[i] & 3)) NQ_FAIL(h, NQ_ERR_INVALID, "frame %d: pixel pointer NULL or not 4-byte aligned", i);
        if (!out_index[i] || ((uintptr_t) out_index[i] & 1)) NQ_FAIL(h, NQ_ERR_INVALID, "frame %d: index pointer NULL or not 2-byte aligned", i);
        if (out_argb && (!out_argb[i] || ((uintptr_t) out_argb[i] & 3)))
            NQ_FAIL(h, NQ_ERR_INVALID, "frame %d: output pointer NULL or not 4-byte aligned", i);
    }
    std::vector<Span> spans;
    spans.reserve(3 * (size_t) n);
    for (int i = 0; i < n; ++i) {
        const uintptr_t px = (uintptr_t) widths[i] * heights[i];
        spans.push_back({(uintptr_t) argb[i], (uintptr_t) argb[i] + px * sizeof(uint32_t), false});
        spans.push_back({(uintptr_t) out_index[i], (uintptr_t) out_index[i] + px * sizeof(uint16_t), true});
        if (out_argb) spans.push_back({(uintptr_t) out_argb[i], (uintptr_t) out_argb[i] + px * sizeof(uint32_t), true});
    }
    if (output_overlaps(spans)) NQ_FAIL(h, NQ_ERR_INVALID, "an output overlaps a source frame or another output");
    *out_total = total;
    return NQ_OK;
}

// every argument of both forms of nq_dither_ordered
int ordered_check(nq_handle* h, int n, const uint32_t* const* argb, const int32_t* widths, const int32_t* heights, const uint32_t* palette,
                  int K, int limit, uint32_t* const* out_argb, uint16_t* const* out_index, int64_t* out_total) {
    if (K < 1 || K > 256) NQ_FAIL(h, NQ_ERR_INVALID, "K = %d: must be 1..256", K);
    if (limit < 0 || limit > 255) NQ_FAIL(h, NQ_ERR_INVALID, "limit = %d: must be 0..255", limit);
    if (!palette) NQ_FAIL(h, NQ_ERR_INVALID, "palette is NULL");
    return ordered_check_frames(h, n, argb, widths, heights, out_argb, out_index, out_total);
}

// ... and of both forms of nq_convert_frames_ordered
int ordered_check_convert(nq_handle* h, int n, const uint32_t* const* argb, const int32_t* widths, const int32_t* heights, int nMaxColors,
                          int refine, int limit, uint32_t* const* out_argb, uint16_t* const* out_index, const uint32_t* out_palette,
                          const int32_t* out_K, int64_t* out_total) {
    if (nMaxColors < 1 || nMaxColors > 256) NQ_FAIL(h, NQ_ERR_INVALID, "nMaxColors = %d: must be 1..256", nMaxColors);
    if (refine < 0 || refine > 64) NQ_FAIL(h, NQ_ERR_INVALID, "refine = %d: must be 0..64", refine);
    if (limit < 0 || limit > 255) NQ_FAIL(h, NQ_ERR_INVALID, "limit = %d: must be 0..255", limit);
    if (!out_palette || !out_K) NQ_FAIL(h, NQ_ERR_INVALID, "out_palette or out_K is NULL");
    return ordered_check_frames(h, n, argb, widths, heights, out_argb, out_index, out_total);
}

// nq_dither_ordered_device after the checks: frame table and palette go up, one launch dithers the sequence, the statistics come back
// when wanted
int ordered_device(nq_handle* h, int n, const uint32_t* const* d_argb, const int32_t* widths, const int32_t* heights, int64_t total,
                   const uint32_t* palette, int K, int limit, uint32_t* const* d_out_argb, uint16_t* const* d_out_index, int64_t* out_stats) {
    std::vector<nq::OrderedFrame>& t = h->h_ordered_frames;
    t.resize(n);
    bool vec = true;                                // the four-pixel path: 16-byte sources and ARGB outputs, 8-byte index maps, every frame
    for (int i = 0; i < n; ++i) {
        t[i] = {reinterpret_cast<const unsigned*>(d_argb[i]), d_out_index[i], d_out_argb ? reinterpret_cast<unsigned*>(d_out_argb[i]) : nullptr,
                (long long) widths[i] * heights[i], widths[i], 0};
        vec = vec && !(((uintptr_t) d_argb[i] | (uintptr_t) (d_out_argb ? d_out_argb[i] : nullptr)) & 15) && !((uintptr_t) d_out_index[i] & 7);
    }
    std::vector<unsigned>& pal = h->h_ordered_pal;
    pal.assign(256, 0u);
    std::memcpy(pal.data(), palette, (size_t) K * sizeof(uint32_t));
    int T = -1;                                     // the first entry with alpha 0
    for (int k = K - 1; k >= 0; --k) if ((pal[k] >> 24) == 0) T = k;
    NQ_HIP(h, h->d_ordered_frames.reserve(n));
    NQ_HIP(h, h->d_ordered_pal.reserve(256));
    if (out_stats) NQ_HIP(h, h->d_ordered_stats.reserve(2 * (size_t) n));
    // (with out_stats == NULL the call returns with these uploads only enqueued: safe for the reason given at upload_table)
    NQ_HIP(h, hipMemcpyAsync(h->d_ordered_frames.p, t.data(), n * sizeof(nq::OrderedFrame), hipMemcpyHostToDevice, h->stream));
    NQ_HIP(h, hipMemcpyAsync(h->d_ordered_pal.p, pal.data(), 256 * sizeof(unsigned), hipMemcpyHostToDevice, h->stream));
    if (out_stats) NQ_HIP(h, hipMemsetAsync(h->d_ordered_stats.p, 0, 2 * (size_t) n * sizeof(unsigned long long), h->stream));
    launch_ordered(h->d_ordered_frames.p, n, (long long) total, vec, d_out_argb != nullptr, h->d_ordered_pal.p, K, T, limit,
                   out_stats ? h->d_ordered_stats.p : nullptr, h->stream);
    NQ_HIP(h, launch_status());
    if (!out_stats) return NQ_OK;
    static_assert(sizeof(int64_t) == sizeof(unsigned long long), "statistics");
    NQ_HIP(h, hipMemcpyAsync(out_stats, h->d_ordered_stats.p, 2 * (size_t) n * sizeof(int64_t), hipMemcpyDeviceToHost, h->stream));
    NQ_HIP(h, hipStreamSynchronize(h->stream));
    return NQ_OK;
}

// The host form of both calls: the frames go up into d_in, step(sources, ARGB outputs or null, index maps) runs on the device copies,
// index maps and outputs come back.  Frames lie a multiple of 4 elements apart in the staging buffers, so that every source and
// ARGB output starts 16-byte and every index map 8-byte aligned (the four-pixel path).
template <typename Step>
int ordered_host(nq_handle* h, int n, const uint32_t* const* argb, const int32_t* widths, const int32_t* heights, uint32_t* const* out_argb,
                 uint16_t* const* out_index, Step step) {
    return host_form(h, [&]() -> int {
        std::vector<size_t> at(n + 1, 0);
        for (int i = 0; i < n; ++i) at[i + 1] = at[i] + (((size_t) widths[i] * heights[i] + 3) & ~(size_t) 3);
        NQ_HIP(h, h->d_in.reserve(at[n]));
        NQ_HIP(h, h->d_out_index.reserve(at[n]));
        if (out_argb) NQ_HIP(h, h->d_out_argb.reserve(at[n]));
        std::vector<const uint32_t*> d_src(n);
        std::vector<uint16_t*> d_idx(n);
        std::vector<uint32_t*> d_out(n);
        for (int i = 0; i < n; ++i) {
            d_src[i] = h->d_in.p + at[i]; d_idx[i] = h->d_out_index.p + at[i]; d_out[i] = out_argb ? h->d_out_argb.p + at[i] : nullptr;
            NQ_HIP(h, hipMemcpyAsync(h->d_in.p + at[i], argb[i], (size_t) widths[i] * heights[i] * sizeof(uint32_t), hipMemcpyHostToDevice, h->stream));
        }
        const int rc = step(d_src.data(), out_argb ? d_out.data() : nullptr, d_idx.data());
        if (rc) return rc;
        for (int i = 0; i < n; ++i) {
            const size_t px = (size_t) widths[i] * heights[i];
            NQ_HIP(h, hipMemcpyAsync(out_index[i], d_idx[i], px * sizeof(uint16_t), hipMemcpyDeviceToHost, h->stream));
            if (out_argb) NQ_HIP(h, hipMemcpyAsync(out_argb[i], d_out[i], px * sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream));
        }
        NQ_HIP(h, hipStreamSynchronize(h->stream));
        return NQ_OK;
    });
}

// nq_convert_frames_ordered_device after the checks: the three calls it stands for, one after another
int ordered_convert_device(nq_handle* h, int n, const uint32_t* const* d_argb, const int32_t* widths, const int32_t* heights, int64_t total,
                           int nMaxColors, int refine, int limit, uint32_t* const* d_out_argb, uint16_t* const* d_out_index,
                           uint32_t* out_palette, int32_t* out_K) {
    int rc = nq_pnnquan_frames_device(h, n, d_argb, widths, heights, nMaxColors, out_palette, out_K);
    if (rc) return rc;
    const int K = *out_K;
    if (K < 1 || K > 256) NQ_FAIL(h, NQ_ERR_UNSUPPORTED, "the palette has %d entries: the ordered dither takes 1..256", K);
    if (refine > 0) {
        int64_t sse[65];
        int32_t passes = 0;
        rc = refine_device(h, n, d_argb, widths, heights, total, out_palette, K, refine, sse, nullptr, &passes);
        if (rc) return rc;
    }
    rc = ordered_device(h, n, d_argb, widths, heights, total, out_palette, K, limit, d_out_argb, d_out_index, nullptr);
    if (rc) return rc;
    NQ_HIP(h, hipStreamSynchronize(h->stream));
    return NQ_OK;
}

} // namespace

extern "C" {

int nq_dither_ordered_device(nq_handle* h, int n, const uint32_t* const* d_argb, const int32_t* widths, const int32_t* heights,
                             const uint32_t* palette, int K, int limit, uint32_t* const* d_out_argb, uint16_t* const* d_out_index,
                             int64_t* out_stats) {
    if (!h) return NQ_ERR_INVALID;
    int64_t total = 0;
    int rc = ordered_check(h, n, d_argb, widths, heights, palette, K, limit, d_out_argb, d_out_index, &total);
    if (rc) return rc;
    rc = use_device(h);
    if (rc) return rc;
    return ordered_device(h, n, d_argb, widths, heights, total, palette, K, limit, d_out_argb, d_out_index, out_stats);
}

int nq_dither_ordered(nq_handle* h, int n, const uint32_t* const* argb, const int32_t* widths, const int32_t* heights,
                      const uint32_t* palette, int K, int limit, uint32_t* const* out_argb, uint16_t* const* out_index, int64_t* out_stats) {
    if (!h) return NQ_ERR_INVALID;
    int64_t total = 0;
    int rc = ordered_check(h, n, argb, widths, heights, palette, K, limit, out_argb, out_index, &total);
    if (rc) return rc;
    rc = use_device(h);
    if (rc) return rc;
    return ordered_host(h, n, argb, widths, heights, out_argb, out_index, [&](auto in, auto out, auto index) {
        return ordered_device(h, n, in, widths, heights, total, palette, K, limit, out, index, out_stats);
    });
}

int nq_convert_frames_ordered_device(nq_handle* h, int n, const uint32_t* const* d_argb, const int32_t* widths, const int32_t* heights,
                                     int nMaxColors, int refine, int limit, uint32_t* const* d_out_argb, uint16_t* const* d_out_index,
                                     uint32_t* out_palette, int32_t* out_K) {
    if (!h) return NQ_ERR_INVALID;
    int64_t total = 0;
    int rc = ordered_check_convert(h, n, d_argb, widths, heights, nMaxColors, refine, limit, d_out_argb, d_out_index, out_palette, out_K, &total);
    if (rc) return rc;
    rc = use_device(h);
    if (rc) return rc;
    return ordered_convert_device(h, n, d_argb, widths, heights, total, nMaxColors, refine, limit, d_out_argb, d_out_index, out_palette, out_K);
}

int nq_convert_frames_ordered(nq_handle* h, int n, const uint32_t* const* argb, const int32_t* widths, const int32_t* heights,
                              int nMaxColors, int refine, int limit, uint32_t* const* out_argb, uint16_t* const* out_index,
                              uint32_t* out_palette, int32_t* out_K) {
    if (!h) return NQ_ERR_INVALID;
    int64_t total = 0;
    int rc = ordered_check_convert(h, n, argb, widths, heights, nMaxColors, refine, limit, out_argb, out_index, out_palette, out_K, &total);
    if (rc) return rc;
    rc = use_device(h);
    if (rc) return rc;
    return ordered_host(h, n, argb, widths, heights, out_argb, out_index, [&](auto in, auto out, auto index) {
        return ordered_convert_device(h, n, in, widths, heights, total, nMaxColors, refine, limit, out, index, out_palette, out_K);
    });
}

} // extern "C"

// ---- quality measurement (nq_compare.hip): stateless calls -- no handle, the error text goes to the thread's handle-free string ----
namespace {

// one call: n pairs; out[i] is an ARGB frame or, with `indexed`, a uint16 index map into palette[0 .. K)
struct CompareCall {
    int device, n;
    const uint32_t* const* src; const void* const* out;
    bool indexed; const uint32_t* palette; int K;
    const int32_t* widths; const int32_t* heights;
    int flags; int64_t* result;
};

// NQ_ERR_INVALID of the four entry points, before any device is touched (the pointers may be host or device addresses alike)
int compare_check(const CompareCall& c) {
    if (c.device < 0) NQ_CMP_FAIL(NQ_ERR_INVALID, "device = %d: a device ordinal is not negative", c.device);
    if (c.n < 1 || c.n > 65535) NQ_CMP_FAIL(NQ_ERR_INVALID, "n = %d: 1..65535 pairs of frames", c.n);
    if (c.flags & ~NQ_COMPARE_LINEAR) NQ_CMP_FAIL(NQ_ERR_INVALID, "flags = 0x%x: unknown bits", (unsigned) c.flags);
    if (c.indexed && (c.K < 1 || c.K > 256)) NQ_CMP_FAIL(NQ_ERR_INVALID, "K = %d: a palette has 1..256 entries", c.K);
    if (!c.src || !c.out || !c.widths || !c.heights) NQ_CMP_FAIL(NQ_ERR_INVALID, "an array of frame pointers or of sides is NULL");
    if (c.indexed && !c.palette) NQ_CMP_FAIL(NQ_ERR_INVALID, "palette is NULL");
    if (!c.result || ((uintptr_t) c.result & 7)) NQ_CMP_FAIL(NQ_ERR_INVALID, "result is NULL or not 8-byte aligned");
    const uintptr_t r0 = (uintptr_t) c.result, r1 = r0 + (uintptr_t) c.n * 16 * sizeof(int64_t);
    for (int i = 0; i < c.n; ++i) {
        const int w = c.widths[i], h = c.heights[i];
        if (w < 1 || w > 65535 || h < 1 || h > 65535) NQ_CMP_FAIL(NQ_ERR_INVALID, "frame %d: %d x %d: sides must be 1..65535", i, w, h);
        const uintptr_t px = (uintptr_t) w * (uintptr_t) h;
        if (px > 2147483647u) NQ_CMP_FAIL(NQ_ERR_INVALID, "frame %d: %d x %d: more than 2^31 - 1 pixels", i, w, h);
        const uintptr_t s0 = (uintptr_t) c.src[i], o0 = (uintptr_t) c.out[i], obytes = px * (c.indexed ? sizeof(uint16_t) : sizeof(uint32_t));
        if (!s0 || (s0 & 3)) NQ_CMP_FAIL(NQ_ERR_INVALID, "frame %d: source pointer NULL or not 4-byte aligned", i);
        if (!o0 || (o0 & (c.indexed ? 1 : 3)))
            NQ_CMP_FAIL(NQ_ERR_INVALID, "frame %d: %s pointer NULL or not %d-byte aligned", i, c.indexed ? "index map" : "output", c.indexed ? 2 : 4);
        if ((s0 < r1 && r0 < s0 + px * sizeof(uint32_t)) || (o0 < r1 && r0 < o0 + obytes))
            NQ_CMP_FAIL(NQ_ERR_INVALID, "frame %d: result overlaps the frame", i);
    }
    return NQ_OK;
}

int compare_use_device(int device) {
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0)
        NQ_CMP_FAIL(NQ_ERR_NO_DEVICE, "no HIP device available (libnquant_hip has no CPU fallback)");
    if (device >= count) NQ_CMP_FAIL(NQ_ERR_INVALID, "device ordinal out of range");
    NQ_CMP_HIP(hipSetDevice(device));
    return NQ_OK;
}

// after the checks: the result zeroed, then one launch per COMPARE_FRAMES_PER_LAUNCH pairs, all on s; nothing is allocated or awaited.
// c.result and the frames are device memory, *d_bad as launch_compare wants it.
int compare_device(const CompareCall& c, int* d_bad, hipStream_t s) {
    NQ_CMP_HIP(hipMemsetAsync(c.result, 0, (size_t) c.n * 16 * sizeof(int64_t), s));
    for (int first = 0; first < c.n; first += COMPARE_FRAMES_PER_LAUNCH) {
        const int count = std::min(c.n - first, (int) COMPARE_FRAMES_PER_LAUNCH);
        CompareLaunch a;
        std::memset(&a, 0, sizeof a);
        bool vec = true;                             // the 16-byte path needs every frame of the launch to allow it
        for (int i = 0; i < count; ++i) {
            a.frame[i] = {c.src[first + i], c.out[first + i], c.widths[first + i], c.heights[first + i], 0u, 0};
            vec = vec && c.widths[first + i] % 4 == 0 && !((uintptr_t) c.src[first + i] & 15) &&
                  !((uintptr_t) c.out[first + i] & (c.indexed ? 7 : 15));
        }
        a.result = reinterpret_cast<long long*>(c.result + 16 * (size_t) first);
        a.first = first;
        a.linear = (c.flags & NQ_COMPARE_LINEAR) != 0;
        launch_compare(a, count, vec, c.indexed, c.palette, c.K, d_bad, s);
    }
    NQ_CMP_HIP(launch_status());
    return NQ_OK;
}

// the host forms: frames and index maps uploaded to temporary buffers (every one on a 16-byte boundary), the device form, the
// results read back; everything is freed when the call returns
int compare_host(const CompareCall& c) {
    int rc = compare_check(c);
    if (rc) return rc;
    rc = compare_use_device(c.device);
    if (rc) return rc;
    DevBuf<uint32_t> d_px;
    DevBuf<int64_t> d_res;
    DevBuf<int> d_bad;
    std::vector<size_t> at(2 * (size_t) c.n);        // first word of src i, of out i
    size_t words = 0;
    for (int i = 0; i < c.n; ++i) {
        const size_t px = (size_t) c.widths[i] * c.heights[i];
        at[2 * (size_t) i] = words; words += (px + 3) & ~(size_t) 3;
        at[2 * (size_t) i + 1] = words; words += ((c.indexed ? (px + 1) / 2 : px) + 3) & ~(size_t) 3;
    }
    hipStream_t s = nullptr;
    int bad = INT_MAX;
    auto body = [&]() -> int {
        NQ_CMP_HIP(d_px.reserve(words));
        NQ_CMP_HIP(d_res.reserve(16 * (size_t) c.n));
        NQ_CMP_HIP(d_bad.reserve(1));
        std::vector<const uint32_t*> d_src(c.n);
        std::vector<const void*> d_out(c.n);
        for (int i = 0; i < c.n; ++i) {
            const size_t px = (size_t) c.widths[i] * c.heights[i];
            d_src[i] = d_px.p + at[2 * (size_t) i]; d_out[i] = d_px.p + at[2 * (size_t) i + 1];
            NQ_CMP_HIP(hipMemcpyAsync(d_px.p + at[2 * (size_t) i], c.src[i], px * sizeof(uint32_t), hipMemcpyHostToDevice, s));
            NQ_CMP_HIP(hipMemcpyAsync(d_px.p + at[2 * (size_t) i + 1], c.out[i], px * (c.indexed ? sizeof(uint16_t) : sizeof(uint32_t)),
                                      hipMemcpyHostToDevice, s));
        }
        NQ_CMP_HIP(hipMemcpyAsync(d_bad.p, &bad, sizeof bad, hipMemcpyHostToDevice, s));
        CompareCall d = c;
        d.src = d_src.data(); d.out = d_out.data(); d.result = d_res.p;
        const int rc2 = compare_device(d, d_bad.p, s);
        if (rc2) return rc2;
        NQ_CMP_HIP(hipMemcpyAsync(c.result, d_res.p, 16 * (size_t) c.n * sizeof(int64_t), hipMemcpyDeviceToHost, s));
        NQ_CMP_HIP(hipMemcpyAsync(&bad, d_bad.p, sizeof bad, hipMemcpyDeviceToHost, s));
        NQ_CMP_HIP(hipStreamSynchronize(s));
        return NQ_OK;
    };
    rc = body();
    if (rc) { (void) hipStreamSynchronize(s); return rc; }
    if (bad != INT_MAX) NQ_CMP_FAIL(NQ_ERR_INVALID, "frame %d: an index >= K = %d (it was read as the word 0)", bad, c.K);
    return NQ_OK;
}

int compare_device_form(const CompareCall& c, void* hip_stream) {
    int rc = compare_check(c);
    if (rc) return rc;
    rc = compare_use_device(c.device);
    if (rc) return rc;
    return compare_device(c, nullptr, (hipStream_t) hip_stream);
}

} // namespace

extern "C" {

int nq_compare_frames_device(int device, void* hip_stream, int n, const uint32_t* const* d_src, const uint32_t* const* d_out,
                             const int32_t* widths, const int32_t* heights, int flags, int64_t* d_result) {
    return compare_device_form({device, n, d_src, reinterpret_cast<const void* const*>(d_out), false, nullptr, 0, widths, heights, flags, d_result},
                               hip_stream);
}

int nq_compare_indexed_device(int device, void* hip_stream, int n, const uint32_t* const* d_src, const uint16_t* const* d_index,
                              const uint32_t* palette, int K, const int32_t* widths, const int32_t* heights, int flags, int64_t* d_result) {
    return compare_device_form({device, n, d_src, reinterpret_cast<const void* const*>(d_index), true, palette, K, widths, heights, flags, d_result},
                               hip_stream);
}

int nq_compare_frames(int device, int n, const uint32_t* const* src, const uint32_t* const* out, const int32_t* widths,
                      const int32_t* heights, int flags, int64_t* result) {
    return compare_host({device, n, src, reinterpret_cast<const void* const*>(out), false, nullptr, 0, widths, heights, flags, result});
}

int nq_compare_indexed(int device, int n, const uint32_t* const* src, const uint16_t* const* index, const uint32_t* palette, int K,
                       const int32_t* widths, const int32_t* heights, int flags, int64_t* result) {
    return compare_host({device, n, src, reinterpret_cast<const void* const*>(index), true, palette, K, widths, heights, flags, result});
}

} // extern "C"

// ---- WebP encoding (nq_webp.hip; include/nquant_abi.h "WebP encoding"): stateless calls like the quality measurement -- no handle, the
// error text goes to the thread's handle-free string; all scratch lives for the call only ----
namespace {

constexpr int kWebpMaxChain = 32768, kWebpGreen = 280, kWebpDist = 40;
// the bound's ingredients (DESIGN.md "WebP encoder"): the five code headers of a band; header, transform, colour table and the fixed
// bits of the main image; the entropy image's codes and one of its rows
constexpr long long kWebpHeadBits = 4640, kWebpTableBits = 30400, kWebpEntropyBits = 7700, kWebpEntropyRowBits = 64;
// RIFF header, VP8X, ANIM | ANMF header, VP8L header
constexpr long long kWebpFileLead = 12 + 18 + 14, kWebpFrameLead = 24 + 8;
const int kWebpClOrderHost[19] = {17, 18, 0, 1, 2, 3, 4, 5, 16, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15};

inline int webp_per(int K) { return K <= 2 ? 8 : K <= 4 ? 4 : K <= 16 ? 2 : 1; }
// p: a band is 2^p packed rows; 0: none fits a chain at this packed width
inline int webp_band_bits(int pw, int band_bits) {
    if (band_bits) return ((long long) pw << band_bits) <= kWebpMaxChain ? band_bits : 0;
    for (int p = 9; p >= 2; --p)
        if (((long long) pw << p) <= kWebpMaxChain) return p;
    return 0;
}
// most bytes of one frame's ANMF header and VP8L chunk, over every bundling the geometry allows; 0: it allows none
long long webp_frame_max(int w, int h, int band_bits) {
    long long worst = 0;
    for (int per = 1; per <= 8; per *= 2) {
        const int pw = (w + per - 1) / per, p = webp_band_bits(pw, band_bits);
        if (!p) continue;
        const long long nb = (h + (1 << p) - 1) >> p;
        const long long bits = kWebpTableBits + (nb > 1 ? kWebpEntropyBits + kWebpEntropyRowBits * nb : 0) + nb * kWebpHeadBits + 15ll * pw * h;
        worst = std::max(worst, (bits + 7) / 8);
    }
    return worst ? kWebpFrameLead + worst + 1 : 0;
}

// the arguments nq_webp_max_bytes takes; false + the reason otherwise
bool webp_check_shape(int n, int width, int height, int band_bits, char* why, size_t len) {
    if (n < 1 || n > 65535) { std::snprintf(why, len, "n = %d: 1..65535 frames", n); return false; }
    if (width < 1 || width > 16384 || height < 1 || height > 16384) {
        std::snprintf(why, len, "%d x %d: sides must be 1..16384", width, height); return false;
    }
    if (band_bits != 0 && (band_bits < 2 || band_bits > 9)) { std::snprintf(why, len, "band_bits = %d: must be 0 or 2..9", band_bits); return false; }
    if (!webp_frame_max(width, height, band_bits)) {
        std::snprintf(why, len, "width %d at band_bits = %d: no band of 2^p packed rows fits a chain of %d packed pixels", width, band_bits, kWebpMaxChain);
        return false;
    }
    return true;
}

// a bit string, first bit in bit 0 of word 0
struct WebpBits {
    std::vector<uint32_t> w;
    long long nb = 0;
    void put(uint32_t v, int b) {                    // b <= 32
        for (int done = 0; done < b;) {
            const int sh = (int) (nb & 31);
            if (!sh) w.push_back(0);
            const int take = std::min(32 - sh, b - done);
            w.back() |= (uint32_t) (((uint64_t) (v >> done) & ((1ull << take) - 1)) << sh);
            nb += take; done += take;
        }
    }
    void append(const WebpBits& o) {
        for (long long i = 0; i < o.nb; i += 32) put(o.w[(size_t) (i >> 5)], (int) std::min<long long>(32, o.nb - i));
    }
};

// build_code of nq_lz.inc on the host: lengths <= limit and the canonical codes, bit-reversed
void webp_build_code(const std::vector<unsigned>& freq, int limit, std::vector<int>& lens, std::vector<unsigned>& codes) {
    const int nsym = (int) freq.size();
    std::vector<std::pair<unsigned, int>> used;
    for (int s = 0; s < nsym; ++s)
        if (freq[s]) used.push_back({freq[s], s});
    std::sort(used.begin(), used.end());
    const int n = (int) used.size();
    lens.assign(nsym, 0);
    if (n <= 1) lens[n ? used[0].second : 0] = 1;
    else {
        std::vector<unsigned long long> W(2 * n - 1, 0);
        std::vector<int> parent(2 * n - 1, 0), depth(2 * n - 1, 0), cnt(limit + 1, 0);
        for (int i = 0; i < n; ++i) W[i] = used[i].first;
        int i = 0, j = n;
        for (int k = n; k < 2 * n - 1; ++k)
            for (int r = 0; r < 2; ++r) {
                int t;
                if (i < n && (j >= k || W[i] <= W[j])) t = i++; else t = j++;
                W[k] += W[t];
                parent[t] = k;
            }
        for (int t = 2 * n - 3; t >= 0; --t) {
            depth[t] = depth[parent[t]] + 1;
            if (t < n) cnt[std::min(depth[t], limit)]++;
        }
        unsigned long long total = 0;
        for (int l = 1; l <= limit; ++l) total += (unsigned long long) cnt[l] << (limit - l);
        for (; total > (1ull << limit); --total) {
            cnt[limit]--;
            int l = limit - 1;
            while (l > 1 && cnt[l] == 0) --l;
            cnt[l]--;
            cnt[l + 1] += 2;
        }
        int t = 0;
        for (int l = limit; l >= 1; --l)
            for (int c = cnt[l]; c > 0 && t < n; --c) lens[used[t++].second] = l;
    }
    std::vector<unsigned> count(limit + 2, 0), next(limit + 2, 0);
    for (int s = 0; s < nsym; ++s) count[lens[s]]++;
    count[0] = 0;
    unsigned code = 0;
    for (int l = 1; l <= limit; ++l) {
        code = (code + count[l - 1]) << 1;
        next[l] = code;
    }
    codes.assign(nsym, 0);
    for (int s = 0; s < nsym; ++s) {
        const int l = lens[s];
        if (!l) continue;
        unsigned c = next[l]++, rev = 0;
        for (int b = 0; b < l; ++b) rev |= ((c >> b) & 1u) << (l - 1 - b);
        codes[s] = rev;
    }
}

struct WebpCode {
    std::vector<int> len;
    std::vector<unsigned> code;
    void put(WebpBits& o, int s) const { o.put(code[s], len[s]); }
};

// emit_code of nq_webp.hip on the host: the prefix code of the symbols counted in freq, written to o
WebpCode webp_put_code(WebpBits& o, const std::vector<unsigned>& freq) {
    const int nsym = (int) freq.size();
    WebpCode c;
    int used = 0, only = 0;
    for (int s = nsym - 1; s >= 0; --s)
        if (freq[s]) { ++used; only = s; }
    if (used <= 1) {                                 // the simple form; the symbol costs no bits
        o.put(1, 1); o.put(0, 1);
        if (only < 2) { o.put(0, 1); o.put((uint32_t) only, 1); }
        else { o.put(1, 1); o.put((uint32_t) only & 255u, 8); }
        c.len.assign(nsym, 0); c.code.assign(nsym, 0);
        return c;
    }
    webp_build_code(freq, 15, c.len, c.code);
    std::vector<std::pair<int, int>> cls;            // code-length symbol, extra value
    std::vector<unsigned> cf(19, 0);
    auto put = [&](int sym, int extra) { cls.push_back({sym, extra}); cf[sym]++; };
    for (int i = 0; i < nsym;) {
        const int v = c.len[i];
        int r = 1;
        while (i + r < nsym && c.len[i + r] == v) ++r;
        i += r;
        if (v == 0) {
            while (r >= 11) { const int k = std::min(r, 138); put(18, k - 11); r -= k; }
            if (r >= 3) { put(17, r - 3); r = 0; }
        } else {
            put(v, 0); --r;
            while (r >= 3) { const int k = std::min(r, 6); put(16, k - 3); r -= k; }
        }
        for (; r > 0; --r) put(v, 0);
    }
    std::vector<int> cl;
    std::vector<unsigned> cc;
    webp_build_code(cf, 7, cl, cc);
    int ncl = 19;
    while (ncl > 4 && cl[kWebpClOrderHost[ncl - 1]] == 0) --ncl;
    o.put(0, 1); o.put((uint32_t) (ncl - 4), 4);
    for (int i = 0; i < ncl; ++i) o.put((uint32_t) cl[kWebpClOrderHost[i]], 3);
    o.put(0, 1);                                     // all lengths follow
    for (const auto& e : cls) {
        o.put(cc[e.first], cl[e.first]);
        o.put((uint32_t) e.second, e.first == 16 ? 2 : e.first == 17 ? 3 : e.first == 18 ? 7 : 0);
    }
    return c;
}

WebpCode webp_put_single(WebpBits& o, int symbol) {
    std::vector<unsigned> f(256, 0);
    f[symbol] = 1;
    return webp_put_code(o, f);
}

// {prefix symbol, extra bits, extra value} of a length or distance code v >= 1
inline void webp_prefix(unsigned v, int& sym, int& eb, unsigned& ev) {
    const unsigned d = v - 1;
    if (d < 4) { sym = (int) d; eb = 0; ev = 0; return; }
    int hb = 31;
    while (!((d >> hb) & 1u)) --hb;
    eb = hb - 1;
    sym = 2 * hb + (int) ((d >> eb) & 1u);
    ev = d & ((1u << eb) - 1u);
}

// the colour-indexing transform with its table: a K x 1 image of per-channel differences, all literals
void webp_color_table(WebpBits& o, const uint32_t* pal, int K) {
    static const int shift[4] = {8, 16, 0, 24};      // a pixel is coded green, red, blue, alpha
    std::vector<unsigned> f[4] = {std::vector<unsigned>(kWebpGreen, 0), std::vector<unsigned>(256, 0), std::vector<unsigned>(256, 0),
                                  std::vector<unsigned>(256, 0)};
    std::vector<uint8_t> px(4 * (size_t) K);
    for (int k = 0; k < K; ++k)
        for (int c = 0; c < 4; ++c) {
            const uint32_t prev = k ? pal[k - 1] : 0u;
            px[4 * (size_t) k + c] = (uint8_t) (((pal[k] >> shift[c]) & 255u) - ((prev >> shift[c]) & 255u));
            f[c][px[4 * (size_t) k + c]]++;
        }
    o.put(1, 1); o.put(3, 2); o.put((uint32_t) (K - 1), 8);
    o.put(0, 1);                                     // no colour cache
    WebpCode code[4];
    for (int c = 0; c < 4; ++c) code[c] = webp_put_code(o, f[c]);
    webp_put_code(o, std::vector<unsigned>(kWebpDist, 0));
    for (int k = 0; k < K; ++k)
        for (int c = 0; c < 4; ++c) code[c].put(o, px[4 * (size_t) k + c]);
    o.put(0, 1);                                     // no more transforms
}

// the entropy image, ew x eh: pixel (x, y) names group y.  Per row a literal, then, when it is wider than 1, one copy of length
// ew - 1 at distance 1.
void webp_entropy_image(WebpBits& o, int ew, int eh) {
    std::vector<unsigned> fg(kWebpGreen, 0), fr(256, 0), fd(kWebpDist, 0);
    int ls, lb, ds, db;
    unsigned le, de;
    webp_prefix((unsigned) std::max(ew - 1, 1), ls, lb, le);
    webp_prefix(1 + 120, ds, db, de);
    for (int y = 0; y < eh; ++y) {
        fg[y & 255]++; fr[y >> 8]++;
        if (ew > 1) { fg[256 + ls]++; fd[ds]++; }
    }
    o.put(0, 1);                                     // no colour cache
    const WebpCode g = webp_put_code(o, fg), r = webp_put_code(o, fr);
    webp_put_single(o, 0);
    webp_put_single(o, 255);
    const WebpCode d = webp_put_code(o, fd);
    for (int y = 0; y < eh; ++y) {
        g.put(o, y & 255); r.put(o, y >> 8);
        if (ew > 1) {
            g.put(o, 256 + ls); o.put(le, lb);
            d.put(o, ds); o.put(de, db);
        }
    }
}

struct WebpCall {
    int device, n;
    const uint16_t* const* index;
    int width, height;
    const uint32_t* palette; int K;
    const int32_t* delays_cs; int loop_count, band_bits, delta;
    uint8_t* out; int64_t cap; int64_t* out_size; int32_t* out_rects;
};

// NQ_ERR_INVALID of both entry points, before any device is touched (the maps may be host or device addresses alike)
int webp_check(const WebpCall& c) {
    char why[256];
    if (c.device < 0) NQ_CMP_FAIL(NQ_ERR_INVALID, "device = %d: a device ordinal is not negative", c.device);
    if (!webp_check_shape(c.n, c.width, c.height, c.band_bits, why, sizeof why)) NQ_CMP_FAIL(NQ_ERR_INVALID, "%s", why);
    if (c.K < 1 || c.K > 256) NQ_CMP_FAIL(NQ_ERR_INVALID, "K = %d: a palette has 1..256 entries", c.K);
    const int pw = (c.width + webp_per(c.K) - 1) / webp_per(c.K);
    if (!webp_band_bits(pw, c.band_bits))
        NQ_CMP_FAIL(NQ_ERR_INVALID, "packed width %d at band_bits = %d: a band of 2^p packed rows must fit %d packed pixels", pw, c.band_bits, kWebpMaxChain);
    if (c.delta != 0 && c.delta != 1) NQ_CMP_FAIL(NQ_ERR_INVALID, "delta = %d: must be 0 or 1", c.delta);
    if (c.loop_count < 0 || c.loop_count > 65535) NQ_CMP_FAIL(NQ_ERR_INVALID, "loop_count = %d: must be 0..65535 (0 = for ever)", c.loop_count);
    if (c.delays_cs)
        for (int i = 0; i < c.n; ++i)
            if (c.delays_cs[i] < 0 || c.delays_cs[i] > 65535) NQ_CMP_FAIL(NQ_ERR_INVALID, "frame %d: delay %d outside 0..65535", i, c.delays_cs[i]);
    if (!c.palette || !c.out_size) NQ_CMP_FAIL(NQ_ERR_INVALID, "palette / out_size is NULL");
    if (c.cap < 0 || (!c.out && c.cap > 0)) NQ_CMP_FAIL(NQ_ERR_INVALID, "out is NULL or cap < 0");
    if (!c.index) NQ_CMP_FAIL(NQ_ERR_INVALID, "index is NULL");
    for (int i = 0; i < c.n; ++i)
        if (!c.index[i] || ((uintptr_t) c.index[i] & 1)) NQ_CMP_FAIL(NQ_ERR_INVALID, "frame %d: index pointer NULL or not 2-byte aligned", i);
    return NQ_OK;
}

void webp_u24(std::vector<uint8_t>& b, uint32_t v) { for (int k = 0; k < 3; ++k) b.push_back((uint8_t) (v >> (8 * k))); }
void webp_u32(std::vector<uint8_t>& b, uint32_t v) { for (int k = 0; k < 4; ++k) b.push_back((uint8_t) (v >> (8 * k))); }
void webp_tag(std::vector<uint8_t>& b, const char* t) { b.insert(b.end(), t, t + 4); }

// after the checks, on device c.device: c.index are device maps; everything runs on s and is freed before the return
int webp_encode(const WebpCall& c, hipStream_t s) {
    const int n = c.n, W = c.width, H = c.height, K = c.K, per = webp_per(K);
    int cus = 0;
    NQ_CMP_HIP(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, c.device));
    // ---- rectangles: one difference pass over all frames, which also finds an index >= K anywhere ----
    std::vector<GifRect> rects(n, GifRect{0, 0, W, H});
    const bool diff = n > 1 && c.delta;
    if (diff) {
        DevBuf<const unsigned short*> d_ptrs;
        DevBuf<int> d_box;
        std::vector<int> box(4 * (size_t) (n - 1) + 1, 0);
        for (int i = 0; i < n - 1; ++i) { box[4 * i] = box[4 * i + 1] = INT_MAX; box[4 * i + 2] = box[4 * i + 3] = -1; }
        NQ_CMP_HIP(d_ptrs.reserve(n));
        NQ_CMP_HIP(d_box.reserve(box.size()));
        NQ_CMP_HIP(hipMemcpyAsync(d_ptrs.p, c.index, n * sizeof(*c.index), hipMemcpyHostToDevice, s));
        NQ_CMP_HIP(hipMemcpyAsync(d_box.p, box.data(), box.size() * sizeof(int), hipMemcpyHostToDevice, s));
        launch_gif_diff(d_ptrs.p, n, W, H, K, d_box.p, d_box.p + 4 * (size_t) (n - 1), s);
        NQ_CMP_HIP(launch_status());
        NQ_CMP_HIP(hipMemcpyAsync(box.data(), d_box.p, box.size() * sizeof(int), hipMemcpyDeviceToHost, s));
        NQ_CMP_HIP(hipStreamSynchronize(s));
        if (box[4 * (size_t) (n - 1)]) NQ_CMP_FAIL(NQ_ERR_INVALID, "an index map holds an index >= K = %d", K);
        for (int i = 1; i < n; ++i) {
            const int* b = &box[4 * (size_t) (i - 1)];
            GifRect& r = rects[i];
            if (b[2] < 0) r = {0, 0, 1, 1};             // nothing changed
            else {                                      // the container stores offsets halved: left and top go down to even
                const int x = b[0] & ~1, y = b[1] & ~1;
                r = {x, y, b[2] - x + 1, b[3] - y + 1};
            }
            if (r.x < 0 || r.y < 0 || r.w < 1 || r.h < 1 || r.x + r.w > W || r.y + r.h > H)
                NQ_CMP_FAIL(NQ_ERR_HIP, "frame %d: the difference pass returned the box %d %d %d %d", i, b[0], b[1], b[2], b[3]);
        }
    }
    // ---- the images, their chains, and the bits the host writes (they depend on the palette and the geometry only) ----
    bool alpha = false;
    for (int i = 0; i < K; ++i) alpha = alpha || (c.palette[i] >> 24) != 255;
    WebpBits table;
    webp_color_table(table, c.palette, K);
    std::vector<nq::WebpImage> img(n);
    std::vector<uint32_t> pre;
    long long chains = 0;
    int max_len = 1;
    for (int i = 0; i < n; ++i) {
        nq::WebpImage& F = img[i];
        const GifRect& r = rects[i];
        std::memset(&F, 0, sizeof F);
        F.index = c.index[i] + (size_t) r.y * W + r.x;
        F.width = r.w; F.height = r.h; F.pitch = W; F.K = K; F.per = per; F.pw = (r.w + per - 1) / per;
        const int p = webp_band_bits(F.pw, c.band_bits);             // (a rectangle is no wider than the frame: p exists)
        F.band_rows = 1 << p; F.nbands = (r.h + F.band_rows - 1) >> p;
        F.chain_base = chains; chains += F.nbands;
        max_len = std::max(max_len, F.pw * std::min(F.band_rows, r.h));
        WebpBits b;
        b.put(0x2F, 8); b.put((uint32_t) (r.w - 1), 14); b.put((uint32_t) (r.h - 1), 14); b.put(alpha ? 1 : 0, 1); b.put(0, 3);
        b.append(table);
        b.put(0, 1);                                                 // no colour cache
        if (F.nbands > 1) {
            b.put(1, 1); b.put((uint32_t) (p - 2), 3);
            webp_entropy_image(b, (F.pw + F.band_rows - 1) >> p, F.nbands);
        } else b.put(0, 1);
        F.pre_word = (long long) pre.size(); F.pre_bits = b.nb;
        pre.insert(pre.end(), b.w.begin(), b.w.end());
        pre.push_back(0); pre.push_back(0);                          // a reader may touch the word after the last bit
    }
    const long long cw = nq::webp_chain_words(max_len);
    const int grid = (int) std::min<long long>(chains, 4ll * std::max(cus, 1));
    DevBuf<nq::WebpImage> d_img;
    DevBuf<uint32_t> d_pre, d_words, d_tokens;
    DevBuf<unsigned long long> d_bits, d_off, d_res;
    DevBuf<int> d_bad;
    DevBuf<uint8_t> d_blob, d_file;
    NQ_CMP_HIP(d_img.reserve(n));
    NQ_CMP_HIP(d_pre.reserve(pre.size()));
    NQ_CMP_HIP(d_words.reserve((size_t) (chains * cw)));
    NQ_CMP_HIP(d_tokens.reserve((size_t) grid * max_len));
    NQ_CMP_HIP(d_bits.reserve(2 * (size_t) chains));
    NQ_CMP_HIP(d_off.reserve((size_t) n + 2 * (size_t) chains));
    NQ_CMP_HIP(d_res.reserve(n));
    NQ_CMP_HIP(d_bad.reserve(n));
    NQ_CMP_HIP(hipMemcpyAsync(d_img.p, img.data(), n * sizeof(nq::WebpImage), hipMemcpyHostToDevice, s));
    NQ_CMP_HIP(hipMemcpyAsync(d_pre.p, pre.data(), pre.size() * sizeof(uint32_t), hipMemcpyHostToDevice, s));
    NQ_CMP_HIP(hipMemsetAsync(d_bad.p, 0, n * sizeof(int), s));
    NQ_CMP_HIP(launch_webp_chains(d_img.p, n, chains, max_len, grid, d_words.p, d_bits.p, d_tokens.p, d_bad.p, s));
    launch_webp_scan(d_img.p, n, max_len, d_bits.p, d_off.p, d_res.p, s);
    NQ_CMP_HIP(launch_status());
    std::vector<unsigned long long> res(n);
    std::vector<int> bad(n);
    NQ_CMP_HIP(hipMemcpyAsync(res.data(), d_res.p, n * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
    NQ_CMP_HIP(hipMemcpyAsync(bad.data(), d_bad.p, n * sizeof(int), hipMemcpyDeviceToHost, s));
    NQ_CMP_HIP(hipStreamSynchronize(s));
    for (int i = 0; i < n; ++i)
        if (bad[i]) NQ_CMP_FAIL(NQ_ERR_INVALID, "frame %d: the index map holds an index >= K = %d", i, K);
    // ---- the container: every image's chunk headers in one blob, then the file is gathered ----
    std::vector<uint8_t> blob;
    long long total = 0;
    for (int i = 0; i < n; ++i) {
        nq::WebpImage& F = img[i];
        F.data_bytes = (long long) ((res[i] + 7) / 8);
        total += (i == 0 ? (n > 1 ? kWebpFileLead : 12) : 0) + (n > 1 ? kWebpFrameLead : 8) + F.data_bytes + (F.data_bytes & 1);
    }
    long long at = 0;
    for (int i = 0; i < n; ++i) {
        nq::WebpImage& F = img[i];
        const GifRect& r = rects[i];
        const size_t start = blob.size();
        const long long padded = F.data_bytes + (F.data_bytes & 1);
        if (i == 0) {
            webp_tag(blob, "RIFF"); webp_u32(blob, (uint32_t) (total - 8)); webp_tag(blob, "WEBP");
            if (n > 1) {
                webp_tag(blob, "VP8X"); webp_u32(blob, 10);
                blob.push_back((uint8_t) (0x02 | (alpha ? 0x10 : 0))); blob.push_back(0); blob.push_back(0); blob.push_back(0);
                webp_u24(blob, (uint32_t) (W - 1)); webp_u24(blob, (uint32_t) (H - 1));
                webp_tag(blob, "ANIM"); webp_u32(blob, 6); webp_u32(blob, 0);
                blob.push_back((uint8_t) c.loop_count); blob.push_back((uint8_t) (c.loop_count >> 8));
            }
        }
        if (n > 1) {
            webp_tag(blob, "ANMF"); webp_u32(blob, (uint32_t) (16 + 8 + padded));
            webp_u24(blob, (uint32_t) (r.x / 2)); webp_u24(blob, (uint32_t) (r.y / 2));
            webp_u24(blob, (uint32_t) (r.w - 1)); webp_u24(blob, (uint32_t) (r.h - 1));
            webp_u24(blob, 10u * (uint32_t) (c.delays_cs ? c.delays_cs[i] : 0));
            blob.push_back(0x02);                                    // do not blend, dispose none
        }
        webp_tag(blob, "VP8L"); webp_u32(blob, (uint32_t) F.data_bytes);
        F.prefix_off = (long long) start; F.prefix_len = (int) (blob.size() - start);
        F.file_off = at;
        at += F.prefix_len + padded;
    }
    if (at != total) NQ_CMP_FAIL(NQ_ERR_HIP, "the container's %lld bytes are not the %lld counted", at, total);
    if (total > 4294967295ll + 8) NQ_CMP_FAIL(NQ_ERR_INVALID, "the file's %lld bytes exceed what RIFF can hold", total);
    *c.out_size = total;
    if (c.cap < total) NQ_CMP_FAIL(NQ_ERR_INVALID, "cap = %lld bytes < the file's %lld", (long long) c.cap, total);
    NQ_CMP_HIP(d_blob.reserve(blob.size()));
    NQ_CMP_HIP(d_file.reserve((size_t) total));
    NQ_CMP_HIP(hipMemcpyAsync(d_blob.p, blob.data(), blob.size(), hipMemcpyHostToDevice, s));
    NQ_CMP_HIP(hipMemcpyAsync(d_img.p, img.data(), n * sizeof(nq::WebpImage), hipMemcpyHostToDevice, s));
    launch_webp_gather(d_img.p, n, max_len, d_words.p, d_pre.p, d_bits.p, d_off.p, d_blob.p, d_file.p, total, s);
    NQ_CMP_HIP(launch_status());
    NQ_CMP_HIP(hipMemcpyAsync(c.out, d_file.p, (size_t) total, hipMemcpyDeviceToHost, s));
    NQ_CMP_HIP(hipStreamSynchronize(s));
    if (c.out_rects)
        for (int i = 0; i < n; ++i) { c.out_rects[4 * i] = rects[i].x; c.out_rects[4 * i + 1] = rects[i].y; c.out_rects[4 * i + 2] = rects[i].w; c.out_rects[4 * i + 3] = rects[i].h; }
    return NQ_OK;
}

// the work of a call, then the stream drained whatever happened: the scratch is freed on return
int webp_run(const WebpCall& c, hipStream_t s) {
    const int rc = webp_encode(c, s);
    if (rc) (void) hipStreamSynchronize(s);
    return rc;
}

} // namespace

extern "C" {

int nq_webp_max_bytes(int n, int width, int height, int band_bits, int64_t* out_bytes) {
    char why[256];
    if (!out_bytes || !webp_check_shape(n, width, height, band_bits, why, sizeof why)) return NQ_ERR_INVALID;
    *out_bytes = kWebpFileLead + (long long) n * webp_frame_max(width, height, band_bits);
    return NQ_OK;
}

int nq_encode_webp_device(int device, void* hip_stream, int n, const uint16_t* const* d_index, int width, int height, const uint32_t* palette,
                          int K, const int32_t* delays_cs, int loop_count, int band_bits, int delta, uint8_t* out, int64_t cap, int64_t* out_size,
                          int32_t* out_rects) {
    const WebpCall c{device, n, d_index, width, height, palette, K, delays_cs, loop_count, band_bits, delta, out, cap, out_size, out_rects};
    int rc = webp_check(c);
    if (rc) return rc;
    rc = compare_use_device(device);
    if (rc) return rc;
    return webp_run(c, (hipStream_t) hip_stream);
}

int nq_encode_webp(int device, int n, const uint16_t* const* index, int width, int height, const uint32_t* palette, int K,
                   const int32_t* delays_cs, int loop_count, int band_bits, int delta, uint8_t* out, int64_t cap, int64_t* out_size,
                   int32_t* out_rects) {
    WebpCall c{device, n, index, width, height, palette, K, delays_cs, loop_count, band_bits, delta, out, cap, out_size, out_rects};
    int rc = webp_check(c);
    if (rc) return rc;
    rc = compare_use_device(device);
    if (rc) return rc;
    // the maps uploaded to one temporary buffer, every one at an even element
    const size_t px = (size_t) width * height, stride = (px + 1) & ~(size_t) 1;
    DevBuf<uint16_t> d_maps;
    NQ_CMP_HIP(d_maps.reserve(stride * n));
    std::vector<const uint16_t*> dev(n);
    hipStream_t s = nullptr;
    for (int i = 0; i < n; ++i) {
        dev[i] = d_maps.p + stride * i;
        const hipError_t e = hipMemcpyAsync(d_maps.p + stride * i, index[i], px * sizeof(uint16_t), hipMemcpyHostToDevice, s);
        if (e != hipSuccess) {
            (void) hipStreamSynchronize(s);
            NQ_CMP_FAIL(NQ_ERR_HIP, "upload of frame %d failed: %s", i, hipGetErrorString(e));
        }
    }
    c.index = dev.data();
    return webp_run(c, s);
}

} // extern "C"

// ---- 10-bit YUV input (nq_yuv16.hip; include/nquant_abi.h "10-bit YUV input"): stateless calls like the quality measurement -- no
// handle, the error text goes to the thread's handle-free string; the frames of a launch travel in its arguments, so the device forms
// allocate nothing and wait for nothing ----
namespace {

using Yuv16Frames = PlaneFrames<uint16_t>;

// floor(16384 e + 1/2) of the rationals of include/nquant_abi.h "10-bit YUV input", by matrix and range: {cy, crv, cgu, cgv, cbu, yo}
const YuvCoef YUV16_COEF[3][2] = {
    {{76590, 104982, 25769, 53475, 132687, 64}, {65584, 91949, 22570, 46836, 116215, 0}},       // BT.601: limited, full
    {{76590, 117921, 14027, 35053, 138947, 64}, {65584, 103282, 12285, 30701, 121698, 0}},      // NQ_YUV_BT709
    {{76590, 110418, 12322, 42783, 140879, 64}, {65584, 96710, 10792, 37472, 123390, 0}},       // NQ_YUV16_BT2020
};

constexpr int kYuv16Flags = NQ_YUV_BT709 | NQ_YUV_FULL_RANGE | NQ_YUV16_BT2020 | NQ_YUV16_MSB | NQ_YUV16_PQ | NQ_YUV16_HLG;

// every argument of the four entry points, from the host arrays alone (no device work).  nq_frames_from_yuv16* pass the whole frame
// as crop and target, and flags 0.
int yuv16_check(int device, const Yuv16Frames& a, int crop_x, int crop_y, int crop_w, int crop_h, uint32_t* const* dst, int dst_width,
                int dst_height, int flags) {
    const int n = a.n;
    if (n < 1 || n > 65535) NQ_CMP_FAIL(NQ_ERR_INVALID, "n = %d: 1..65535 frames", n);
    if (a.width < 1 || a.width > 65535 || a.height < 1 || a.height > 65535)
        NQ_CMP_FAIL(NQ_ERR_INVALID, "%d x %d: source sides must be 1..65535", a.width, a.height);
    if (a.y_stride < a.width) NQ_CMP_FAIL(NQ_ERR_INVALID, "y_stride = %d: shorter than a row of %d samples", a.y_stride, a.width);
    if (a.c_step != 1 && a.c_step != 2) NQ_CMP_FAIL(NQ_ERR_INVALID, "c_step = %d: must be 1 or 2", a.c_step);
    if (a.c_stride < a.c_step * ((a.width + 1) / 2 - 1) + 1)
        NQ_CMP_FAIL(NQ_ERR_INVALID, "c_stride = %d: shorter than a chroma row of %d samples %d apart", a.c_stride, (a.width + 1) / 2, a.c_step);
    if (a.flags & ~kYuv16Flags) NQ_CMP_FAIL(NQ_ERR_INVALID, "yuv16_flags = 0x%x: unknown bits", (unsigned) a.flags);
    if ((a.flags & NQ_YUV_BT709) && (a.flags & NQ_YUV16_BT2020)) NQ_CMP_FAIL(NQ_ERR_INVALID, "yuv16_flags = 0x%x: two matrices", (unsigned) a.flags);
    if ((a.flags & NQ_YUV16_PQ) && (a.flags & NQ_YUV16_HLG)) NQ_CMP_FAIL(NQ_ERR_INVALID, "yuv16_flags = 0x%x: two transfers", (unsigned) a.flags);
    if (device < 0) NQ_CMP_FAIL(NQ_ERR_INVALID, "device = %d: a device ordinal is not negative", device);
    if (!a.y || !a.u || !a.v || !dst) NQ_CMP_FAIL(NQ_ERR_INVALID, "an array of plane / output pointers is NULL");
    for (int i = 0; i < n; ++i) {
        if (!a.y[i] || !a.u[i] || !a.v[i]) NQ_CMP_FAIL(NQ_ERR_INVALID, "frame %d: a plane pointer is NULL", i);
        if (((uintptr_t) a.y[i] | (uintptr_t) a.u[i] | (uintptr_t) a.v[i]) & 1)
            NQ_CMP_FAIL(NQ_ERR_INVALID, "frame %d: a plane pointer is not 2-byte aligned", i);
        if (!dst[i] || ((uintptr_t) dst[i] & 3)) NQ_CMP_FAIL(NQ_ERR_INVALID, "frame %d: output pointer NULL or not 4-byte aligned", i);
    }
    if ((long long) n * a.width * a.height > 2147483647ll)
        NQ_CMP_FAIL(NQ_ERR_INVALID, "%d frames of %d x %d: more than 2^31 - 1 pixels", n, a.width, a.height);
    const int rc = reduce_check(g_create_error, a.width, a.height, crop_x, crop_y, crop_w, crop_h, dst_width, dst_height, flags);
    if (rc) return rc;
    std::vector<Span> spans = a.spans(dst, (uintptr_t) dst_width * dst_height * sizeof(uint32_t));
    if (output_overlaps(spans)) NQ_CMP_FAIL(NQ_ERR_INVALID, "an output overlaps a source plane or another output");
    return NQ_OK;
}

struct Yuv16Geometry { bool fused; int crop_x, crop_y, crop_w, crop_h, dst_width, dst_height, flags; };

// after the checks, for DEVICE frames `a` and outputs d_dst: one launch per YUV16_FRAMES_PER_LAUNCH frames, each with the path of its
// own frames (plane_path), all on s
int yuv16_launches(const Yuv16Frames& a, uint32_t* const* d_dst, const Yuv16Geometry& g, hipStream_t s) {
    const int matrix = (a.flags & NQ_YUV16_BT2020) ? 2 : (a.flags & NQ_YUV_BT709) ? 1 : 0;
    for (int first = 0; first < a.n; first += YUV16_FRAMES_PER_LAUNCH) {
        const int count = std::min(a.n - first, (int) YUV16_FRAMES_PER_LAUNCH);
        Yuv16Launch l;
        std::memset(&l, 0, sizeof l);
        bool swap;
        l.path = plane_path(a, d_dst, first, count, !g.fused, false, &swap);
        for (int i = 0; i < count; ++i) {
            const int j = first + i;
            l.frame[i] = {a.y[j], l.path == YUV_WIDE_INTERLEAVED ? std::min(a.u[j], a.v[j]) : a.u[j], a.v[j], d_dst[j]};
        }
        l.count = count;
        l.y_stride = a.y_stride; l.c_stride = a.c_stride; l.c_step = a.c_step;
        l.swap = swap ? 1 : 0;
        l.shift = (a.flags & NQ_YUV16_MSB) ? 6 : 0;
        l.transfer = (a.flags & NQ_YUV16_PQ) ? YUV16_PQ : (a.flags & NQ_YUV16_HLG) ? YUV16_HLG : YUV16_SDR;
        l.k = YUV16_COEF[matrix][(a.flags & NQ_YUV_FULL_RANGE) ? 1 : 0];
        if (g.fused)
            launch_resample_yuv16(l, g.crop_x, g.crop_y, g.crop_w, g.crop_h, g.dst_width, g.dst_height, (g.flags & NQ_RESAMPLE_LINEAR) != 0, s);
        else
            launch_yuv16_argb(l, a.width, a.height, s);
    }
    NQ_CMP_HIP(launch_status());
    return NQ_OK;
}

int yuv16_device_form(int device, const Yuv16Frames& a, uint32_t* const* d_dst, const Yuv16Geometry& g, void* hip_stream) {
    int rc = yuv16_check(device, a, g.crop_x, g.crop_y, g.crop_w, g.crop_h, d_dst, g.dst_width, g.dst_height, g.flags);
    if (rc) return rc;
    rc = compare_use_device(device);
    if (rc) return rc;
    return yuv16_launches(a, d_dst, g, (hipStream_t) hip_stream);
}

// The host forms: plane_host with temporary buffers on the null stream; everything is freed when the call returns.
int yuv16_host_form(int device, const Yuv16Frames& a, uint32_t* const* dst, const Yuv16Geometry& g) {
    int rc = yuv16_check(device, a, g.crop_x, g.crop_y, g.crop_w, g.crop_h, dst, g.dst_width, g.dst_height, g.flags);
    if (rc) return rc;
    rc = compare_use_device(device);
    if (rc) return rc;
    DevBuf<unsigned char> d_in;
    DevBuf<uint32_t> d_out;
    hipStream_t s = nullptr;
    return plane_host(g_create_error, s, d_in, d_out, a, dst, (size_t) g.dst_width * g.dst_height,
                      [&](const Yuv16Frames& d, uint32_t* const* d_dst) { return yuv16_launches(d, d_dst, g, s); });
}

} // namespace

extern "C" {

int nq_frames_from_yuv16_device(int device, void* hip_stream, int n, const uint16_t* const* d_y, const uint16_t* const* d_u,
                                const uint16_t* const* d_v, int width, int height, int y_stride, int c_stride, int c_step, int yuv16_flags,
                                uint32_t* const* d_dst) {
    return yuv16_device_form(device, {n, d_y, d_u, d_v, width, height, y_stride, c_stride, c_step, yuv16_flags}, d_dst,
                             {false, 0, 0, width, height, width, height, 0}, hip_stream);
}

int nq_frames_from_yuv16(int device, int n, const uint16_t* const* y, const uint16_t* const* u, const uint16_t* const* v, int width,
                         int height, int y_stride, int c_stride, int c_step, int yuv16_flags, uint32_t* const* dst) {
    return yuv16_host_form(device, {n, y, u, v, width, height, y_stride, c_stride, c_step, yuv16_flags}, dst,
                           {false, 0, 0, width, height, width, height, 0});
}

int nq_resample_frames_yuv16_device(int device, void* hip_stream, int n, const uint16_t* const* d_y, const uint16_t* const* d_u,
                                    const uint16_t* const* d_v, int src_width, int src_height, int y_stride, int c_stride, int c_step,
                                    int yuv16_flags, int crop_x, int crop_y, int crop_w, int crop_h, uint32_t* const* d_dst, int dst_width,
                                    int dst_height, int flags) {
    return yuv16_device_form(device, {n, d_y, d_u, d_v, src_width, src_height, y_stride, c_stride, c_step, yuv16_flags}, d_dst,
                             {true, crop_x, crop_y, crop_w, crop_h, dst_width, dst_height, flags}, hip_stream);
}

int nq_resample_frames_yuv16(int device, int n, const uint16_t* const* y, const uint16_t* const* u, const uint16_t* const* v, int src_width,
                             int src_height, int y_stride, int c_stride, int c_step, int yuv16_flags, int crop_x, int crop_y, int crop_w,
                             int crop_h, uint32_t* const* dst, int dst_width, int dst_height, int flags) {
    return yuv16_host_form(device, {n, y, u, v, src_width, src_height, y_stride, c_stride, c_step, yuv16_flags}, dst,
                           {true, crop_x, crop_y, crop_w, crop_h, dst_width, dst_height, flags});
}

} // extern "C"

// ---- retiming (nq_retime.hip; include/nquant_abi.h "retiming"): the plan is host arithmetic; the mix is a stateless call like the
// 10-bit YUV input -- no handle, the error text goes to the thread's handle-free string; the outputs of a launch and their windows
// travel in its arguments, so the device form allocates nothing and waits for nothing ----
namespace {

typedef unsigned __int128 rt_u128;

// R(x) = floor((x + 5000) / 10000): microseconds to the nearest centisecond, halves up
inline rt_u128 retime_cs(rt_u128 x) { return (x + 5000) / 10000; }

// every argument of both forms of nq_retime_frames, from the host arrays alone (no device work)
int retime_check(int device, int n, const uint32_t* const* src, int width, int height, int m, const int32_t* offset, const int32_t* source,
                 const uint32_t* weight, uint32_t* const* dst, int flags) {
    if (n < 1 || n > 65535) NQ_CMP_FAIL(NQ_ERR_INVALID, "n = %d: 1..65535 source frames", n);
    if (m < 1 || m > 65535) NQ_CMP_FAIL(NQ_ERR_INVALID, "m = %d: 1..65535 output frames", m);
    if (width < 1 || width > 65535 || height < 1 || height > 65535) NQ_CMP_FAIL(NQ_ERR_INVALID, "%d x %d: sides must be 1..65535", width, height);
    if ((long long) n * width * height > 2147483647ll || (long long) m * width * height > 2147483647ll)
        NQ_CMP_FAIL(NQ_ERR_INVALID, "%d sources / %d outputs of %d x %d: more than 2^31 - 1 pixels", n, m, width, height);
    if (flags & ~NQ_RETIME_LINEAR) NQ_CMP_FAIL(NQ_ERR_INVALID, "flags = 0x%x: unknown bits", (unsigned) flags);
    if (device < 0) NQ_CMP_FAIL(NQ_ERR_INVALID, "device = %d: a device ordinal is not negative", device);
    if (!src || !dst || !offset || !source || !weight) NQ_CMP_FAIL(NQ_ERR_INVALID, "an array of frame pointers or of the plan is NULL");
    for (int i = 0; i < n; ++i)
        if (!src[i] || ((uintptr_t) src[i] & 3)) NQ_CMP_FAIL(NQ_ERR_INVALID, "frame %d: source pointer NULL or not 4-byte aligned", i);
    for (int j = 0; j < m; ++j)
        if (!dst[j] || ((uintptr_t) dst[j] & 3)) NQ_CMP_FAIL(NQ_ERR_INVALID, "output %d: pointer NULL or not 4-byte aligned", j);
    if (offset[0] != 0) NQ_CMP_FAIL(NQ_ERR_INVALID, "offset[0] = %d: the pairs begin at 0", (int) offset[0]);
    for (int j = 0; j < m; ++j) {
        const long long len = (long long) offset[j + 1] - offset[j];
        if (len < 1 || len > NQ_RETIME_MAX_WINDOW)
            NQ_CMP_FAIL(NQ_ERR_INVALID, "output %d: a window of %lld pairs: 1..%d", j, len, NQ_RETIME_MAX_WINDOW);
        uint64_t W = 0;
        for (int k = offset[j]; k < offset[j + 1]; ++k) {
            if (source[k] < 0 || source[k] >= n) NQ_CMP_FAIL(NQ_ERR_INVALID, "pair %d: source %d is outside 0..%d", k, (int) source[k], n - 1);
            W += weight[k];
        }
        if (W < 1 || W > 2147483647ull) NQ_CMP_FAIL(NQ_ERR_INVALID, "output %d: its weights sum to %llu: 1 .. 2^31 - 1", j, (unsigned long long) W);
    }
    std::vector<Span> spans;
    spans.reserve((size_t) n + m);
    const uintptr_t bytes = (uintptr_t) width * height * sizeof(uint32_t);
    for (int i = 0; i < n; ++i) spans.push_back({(uintptr_t) src[i], (uintptr_t) src[i] + bytes, false});
    for (int j = 0; j < m; ++j) spans.push_back({(uintptr_t) dst[j], (uintptr_t) dst[j] + bytes, true});
    if (output_overlaps(spans)) NQ_CMP_FAIL(NQ_ERR_INVALID, "an output overlaps a source frame or another output");
    return NQ_OK;
}

// after the checks, for DEVICE frames: consecutive outputs are packed into a launch until one more would exceed
// RETIME_OUTPUTS_PER_LAUNCH outputs or RETIME_PAIRS_PER_LAUNCH pairs (a window has at most that many); all on s.  The 16-byte path
// needs every source and output pointer of the call aligned to it.
int retime_launches(int n, const uint32_t* const* d_src, int width, int height, int m, const int32_t* offset, const int32_t* source,
                    const uint32_t* weight, uint32_t* const* d_dst, int flags, hipStream_t s) {
    bool vec = true;
    for (int i = 0; i < n; ++i) vec = vec && !((uintptr_t) d_src[i] & 15);
    for (int j = 0; j < m; ++j) vec = vec && !((uintptr_t) d_dst[j] & 15);
    for (int j = 0; j < m;) {
        RetimeLaunch l;
        std::memset(&l, 0, sizeof l);
        int pairs = 0;
        while (j < m && l.count < RETIME_OUTPUTS_PER_LAUNCH && pairs + (offset[j + 1] - offset[j]) <= RETIME_PAIRS_PER_LAUNCH) {
            uint64_t W = 0;
            for (int k = offset[j]; k < offset[j + 1]; ++k, ++pairs) {
                l.src[pairs] = d_src[source[k]];
                l.weight[pairs] = weight[k];
                W += weight[k];
            }
            l.dst[l.count] = d_dst[j];
            l.W[l.count] = (unsigned) W;
            l.first[++l.count] = pairs;
            ++j;
        }
        launch_retime(l, (long long) width * height, (flags & NQ_RETIME_LINEAR) != 0, vec, s);
    }
    NQ_CMP_HIP(launch_status());
    return NQ_OK;
}

} // namespace

extern "C" {

int nq_retime_plan(int n, const int64_t* t_us, int64_t period_us, int64_t shutter_us, int32_t cap_m, int32_t cap_pairs, int32_t* out_m,
                   int32_t* out_pairs, int32_t* out_offset, int32_t* out_source, uint32_t* out_weight, int32_t* out_delays_cs) {
    if (n < 1) NQ_CMP_FAIL(NQ_ERR_INVALID, "n = %d: at least one frame", n);
    if (!t_us || !out_m || !out_pairs) NQ_CMP_FAIL(NQ_ERR_INVALID, "t_us, out_m or out_pairs is NULL");
    for (int i = 0; i < n; ++i)
        if (t_us[i + 1] <= t_us[i]) NQ_CMP_FAIL(NQ_ERR_INVALID, "t_us[%d] = %lld is not above t_us[%d] = %lld", i + 1, (long long) t_us[i + 1], i, (long long) t_us[i]);
    if (period_us < 1) NQ_CMP_FAIL(NQ_ERR_INVALID, "period_us = %lld: at least 1", (long long) period_us);
    if (shutter_us < 1 || shutter_us > period_us || shutter_us > 2147483647ll)
        NQ_CMP_FAIL(NQ_ERR_INVALID, "shutter_us = %lld: 1 .. min(period_us, 2^31 - 1)", (long long) shutter_us);
    // times relative to t_us[0]: exact in unsigned 64-bit whatever the signs (the true differences are below 2^64)
    auto rel = [&](int i) { return (uint64_t) t_us[i] - (uint64_t) t_us[0]; };
    const uint64_t D = rel(n), P = (uint64_t) period_us, H = (uint64_t) shutter_us;
    const rt_u128 m128 = std::max<rt_u128>(1, (2 * (rt_u128) D + P) / (2 * (rt_u128) P));
    if (m128 > 2147483647ull || D / P > 2147483647ull) NQ_CMP_FAIL(NQ_ERR_INVALID, "the clip is more than 2^31 - 1 periods long");
    const int64_t m = (int64_t) m128;
    // one walk over the outputs, twice: to count (and to see that every delay fits its word), then to write.  Source i is the one on
    // display at lo when r[i] <= lo < r[i + 1]; the windows ascend, so i never goes back.
    auto walk = [&](bool write) -> int64_t {
        int64_t pairs = 0;
        int i = 0;
        for (int64_t j = 0; j < m; ++j) {
            const uint64_t lo = (uint64_t) j * P;                                   // < D
            const uint64_t hi = (uint64_t) std::min<rt_u128>((rt_u128) lo + H, D);
            if (write) out_offset[j] = (int32_t) pairs;
            while (rel(i + 1) <= lo) ++i;
            for (int k = i; k < n && rel(k) < hi; ++k, ++pairs) {
                if (!write) continue;
                out_source[pairs] = k;
                out_weight[pairs] = (uint32_t) (std::min(rel(k + 1), hi) - std::max(rel(k), lo));
            }
            const rt_u128 d = retime_cs(j + 1 < m ? (rt_u128) (j + 1) * P : (rt_u128) D) - retime_cs((rt_u128) j * P);
            if (d > 2147483647ull) return -1;
            if (write) out_delays_cs[j] = (int32_t) d;
        }
        if (write) out_offset[m] = (int32_t) pairs;
        return pairs;
    };
    const int64_t pairs = walk(false);
    if (pairs < 0) NQ_CMP_FAIL(NQ_ERR_INVALID, "a delay is above 2^31 - 1 centiseconds");
    if (pairs > 2147483647ll) NQ_CMP_FAIL(NQ_ERR_INVALID, "more than 2^31 - 1 pairs");
    const bool count_only = cap_m == 0 && cap_pairs == 0 && !out_offset && !out_source && !out_weight && !out_delays_cs;
    if (!count_only && cap_m >= m && cap_pairs >= pairs && (!out_offset || !out_source || !out_weight || !out_delays_cs))
        NQ_CMP_FAIL(NQ_ERR_INVALID, "an output array is NULL");
    *out_m = (int32_t) m;
    *out_pairs = (int32_t) pairs;
    if (count_only) return NQ_OK;
    if (cap_m < m || cap_pairs < pairs)
        NQ_CMP_FAIL(NQ_ERR_INVALID, "the plan has %lld outputs and %lld pairs, the arrays hold %d and %d", (long long) m, (long long) pairs, (int) cap_m, (int) cap_pairs);
    walk(true);
    return NQ_OK;
}

int nq_retime_frames_device(int device, void* hip_stream, int n, const uint32_t* const* d_src, int width, int height, int m,
                            const int32_t* offset, const int32_t* source, const uint32_t* weight, uint32_t* const* d_dst, int flags) {
    int rc = retime_check(device, n, d_src, width, height, m, offset, source, weight, d_dst, flags);
    if (rc) return rc;
    rc = compare_use_device(device);
    if (rc) return rc;
    return retime_launches(n, d_src, width, height, m, offset, source, weight, d_dst, flags, (hipStream_t) hip_stream);
}

// The host form: argb_host with temporary buffers on the null stream; everything is freed when the call returns.
int nq_retime_frames(int device, int n, const uint32_t* const* src, int width, int height, int m, const int32_t* offset,
                     const int32_t* source, const uint32_t* weight, uint32_t* const* dst, int flags) {
    int rc = retime_check(device, n, src, width, height, m, offset, source, weight, dst, flags);
    if (rc) return rc;
    rc = compare_use_device(device);
    if (rc) return rc;
    const size_t px = (size_t) width * height;
    DevBuf<uint32_t> d_in, d_out;
    hipStream_t s = nullptr;
    return argb_host(g_create_error, s, d_in, d_out, n, src, px, m, dst, px, [&](const uint32_t* const* d_src, uint32_t* const* d_dst) {
        return retime_launches(n, d_src, width, height, m, offset, source, weight, d_dst, flags, s);
    });
}

} // extern "C"
