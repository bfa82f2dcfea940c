/*
 * nquant_abi.h -- C ABI of libnquant_hip.so: the MI355X (gfx950) implementation of the reference's
 * PnnQuantizer / PnnLABQuantizer hot path (mcychan/nQuant.android).
 *
 * NQ/ = nQuant.master/src/main/java/com/android/nQuant/ in the reference.
 * Every entry point names the reference interface it replaces.  Plain pointers and sizes only; "host"
 * entry points take host memory (what a JNI shim gets from GetPrimitiveArrayCritical on the Java int[]),
 * "_device" entry points take HIP device pointers (what bench.py / a resident pipeline hands over).
 *
 * Pixel format: 32-bit ARGB_8888, non-premultiplied, a = c>>>24, r = (c>>16)&255, g = (c>>8)&255, b = c&255,
 * row-major, index = x + y*width (NQ/PnnQuantizer.java:413-417, NQ/GilbertCurve.java:126).
 *
 * All functions return NQ_OK (0) or a negative nq_status; nq_last_error() gives the text.  A JNI shim maps a
 * non-zero status to the RuntimeException the reference app raises (app/.../MainActivity.java:205-208).
 * A handle mirrors ONE reference quantizer object: stateful, not re-entrant (NQ/PnnQuantizer.java:17-33);
 * distinct handles are independent.  There is no CPU fallback: every compute entry point fails with
 * NQ_ERR_NO_DEVICE when no HIP device is usable.
 */
#ifndef NQUANT_ABI_H
#define NQUANT_ABI_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NQ_ABI_VERSION 1

typedef struct nq_handle nq_handle;

enum nq_kind { NQ_KIND_RGB = 0,   /* PnnQuantizer      (NQ/PnnQuantizer.java)    */
               NQ_KIND_LAB = 1 }; /* PnnLABQuantizer   (NQ/PnnLABQuantizer.java) */

enum nq_mode {
    /* One error-diffusion chain over the whole image with the reference's bin-keyed first-come nearest cache
     * and ONE java.util.Random(seed) stream: bit-exact against the sequential oracle.  Runs on one GPU lane
     * (debug / small images).                                                                              */
    NQ_MODE_REFERENCE_SEQUENTIAL = 0,
    /* Production mode: independent gilbert curve + error queue + Random stream per tile, lookups with the
     * reference's cache-miss semantics; bit-exact against the oracle's tiled restatement.                   */
    NQ_MODE_PARALLEL_TILED = 1,
    /* No diffusion: out_index[i] = nearestColorIndex(palette, pixel[i]) evaluated per pixel (cache-miss
     * semantics): BASELINE.json's "dither off, bit-exact index" check.                                      */
    NQ_MODE_LOOKUP_ONLY = 2
};

enum nq_status {
    NQ_OK = 0,
    NQ_ERR_INVALID = -1,          /* bad argument */
    NQ_ERR_HIP = -2,              /* HIP runtime error (text in nq_last_error) */
    NQ_ERR_UNSUPPORTED = -3,      /* a reference branch this build does not run on the GPU yet */
    NQ_ERR_REFERENCE_THROWS = -4, /* the Java code would throw here (e.g. setAlphaComponent range) */
    NQ_ERR_NO_DEVICE = -5,
    NQ_ERR_TIME_LIMIT = -6        /* a merge loop ran into its wall-clock limit (slow / shared / time-sliced device): nothing was
                                   * wrong with its state -- call again, or raise NQ_OPT_MERGE_WALL_SECONDS.  Distinct from
                                   * NQ_ERR_UNSUPPORTED, which the loop's find_nn budget (maxbins^2/2 calls) or an empty heap report */
};

/* Scalars convert() derives and the later stages consume.  Same layout as the
 * CPU oracle's parameter struct (tests compare the two field by field). */
typedef struct nq_params {
    int32_t kind;
    int32_t nMaxColors;
    int32_t hasSemiTransparency;   /* NQ/PnnQuantizer.java:431 */
    int32_t transparentPixelIndex; /* m_transparentPixelIndex (:420), -1 = none */
    int32_t transparentColor;      /* m_transparentColor (:22,:422) */
    int32_t isNano;                /* NQ/PnnLABQuantizer.java:180 */
    int32_t texicab;               /* NQ/PnnLABQuantizer.java:219 */
    int32_t quan_rt;
    int32_t maxbins;
    int32_t paletteLength;
    double PR, PG, PB, PA;         /* NQ/PnnQuantizer.java:24,432-436,176-180 */
    double ratio;
    double weight;                 /* signed (negated for semi-transparent images, :396-397) */
    int64_t distinctColors;        /* LAB: pixelMap.size() after the histogram (0 when not needed) */
} nq_params;

/* ---- lifetime: replaces `new PnnQuantizer(fname)` / `new PnnLABQuantizer(fname)` (NQ/PnnQuantizer.java:35,
 *      NQ/PnnLABQuantizer.java:24) and garbage collection.  device = HIP device ordinal. ---- */
/* Threads and devices: a handle is NOT thread-safe (like the reference object); distinct handles are independent and
 * may be driven from different threads and live on different devices of one process -- all per-device state (constant tables,
 * kernel attributes) is set up per handle on the handle's device, nothing is cached per process. */
int nq_create(int kind, int device, nq_handle** out);
void nq_destroy(nq_handle* h);
const char* nq_last_error(const nq_handle* h);   /* h may be NULL: the thread's handle-free text -- the last error of nq_create or of a
                                                  * call that takes no handle (nq_compare_*) on this thread */
int nq_abi_version(void);
/* All work of the handle is enqueued on this hipStream_t (NULL = the default stream): a call's reads of its device inputs are ordered
 * after the work the caller has queued on that stream before the call, its writes before the work queued there afterwards; the
 * calls marked "asynchronous" return without waiting for either.  Host arrays a call takes (pointer tables, palettes) belong to the
 * caller again when the call returns.
 * Precondition: the handle's earlier work has completed (the caller has waited for the previous stream, or the last call was one
 * that returns when its results are there).  State the handle keeps on the device -- the uploaded palette, the candidate lists, the
 * cell boxes, the curve tables -- is ordered only against the stream it was written on; a switch while that work is still running
 * is undefined.  (tests/test_gpu_streams.py: parts A, C and D.) */
int nq_set_stream(nq_handle* h, void* hip_stream);
/* Tile of the PARALLEL_TILED decomposition; <= 0 (default) = automatic: 8x8 when that gives the GPU at least 131072
 * independent chains (images from about 2900^2 pixels), 4x4 below that -- for every form of the error queue (a tile chain of the
 * sorted-by-yDiff mode, K > 128 && weight >= .02, starts with its queue in the steady state instead of re-growing it per tile). */
int nq_set_tile(nq_handle* h, int tile_w, int tile_h);
/* One image tiled over GPUs: this handle's following nq_dither[_device] calls treat their pixel buffer as the rows
 * [y0, y0 + height) of an image of image_height rows -- tile random streams, the blue-noise phase and the position-dependent
 * gates (`bidx & 4095`, `pos % 2`) are those of the whole image, so the bands of an image equal the same rows of the single-GPU
 * PARALLEL_TILED result.  y0 (and every band's row count but the last) must be a multiple of the tile height; the automatic tile
 * follows the whole image.  (0, 0) = a whole image again.  Not for REFERENCE_SEQUENTIAL. */
int nq_set_band(nq_handle* h, int y0, int image_height);

/* Tuning switches that never change results.  NQ_OPT_CELL_LISTS (default 1): scan only the per-colour-cell candidate
 * lists in nearest/closestColorIndex (exact, csrc/nq_lists.inc); 0 = scan the whole palette like the reference. */
#define NQ_OPT_CELL_LISTS 1
/* NQ_OPT_FAST_DITHER (default 1): run the specialised dither kernel (csrc/nq_dither_fast.inc) where the configuration allows
 * it (LAB, 32 < K <= 256, no semi-transparency, DITHER_MAX 25, PARALLEL_TILED); 0 = the generic kernel everywhere.  Same results. */
#define NQ_OPT_FAST_DITHER 2
/* NQ_OPT_DITHER_CHAIN (default 0 = automatic): the specialised kernel first walks a wavefront's tiles without the error-diffusion chain
 * wherever ditherPixel replaces the accumulated colour by a colour of the source pixel (LAB, dither, saliencies, 2 * acceptedDiff > 100),
 * and starts over with the chain only when a step needs it (direct branch, second stage); 1 = every step runs the chain.  Same results.
 * 2 = that fused single-kernel light walk wherever it applies; 3 = the split form wherever it applies: a light kernel of its own (87
 * registers and, at 8x8 tiles, 32 KB of LDS: at least four wavefronts per SIMD) lists the TILES that need the chain, the full walk then runs over that list.  0 picks the split form in the finish
 * phase of nq_convert_batch[_device], where the chain pass of image i runs on a side stream beside the light kernel of image i + 1, and the
 * fused form in every other entry point.  4 = the split form with the light pass in its pixel form (gilbert_pixel_kernel: one lane per
 * pixel instead of one per tile, the draws of a tile's Random by jump-ahead) for power-of-two tiles of 16, 32 or 64 pixels, and exactly 3
 * for every other tile size; it counts as a split pass in every statistic.  0 takes 4 where it takes the split form. */
#define NQ_OPT_DITHER_CHAIN 4
/* NQ_OPT_MERGE_WALL_SECONDS (default 0 = automatic: 60 s + 1 ms per histogram bin and per merge loop sharing a compute unit with it):
 * seconds of residency after which a merge loop of this handle's calls gives up with NQ_ERR_TIME_LIMIT.  Every loop of the persistent
 * merge kernel is bounded; this bound only exists so that a corrupt heap cannot keep the GPU for hours. */
#define NQ_OPT_MERGE_WALL_SECONDS 3
int nq_set_option(nq_handle* h, int option, int value);
/* Diagnostics of the last dither pass: out_fast = 1 if the specialised kernel ran; out_failed_tiles = tiles it handed back to
 * the generic kernel (synchronises the handle's stream). */
int nq_get_dither_path(nq_handle* h, int32_t* out_fast, int32_t* out_failed_tiles);
/* Diagnostics, process-wide, cumulative: out3[0] = dither passes that took the split form (NQ_OPT_DITHER_CHAIN), out3[1] = those of them
 * whose chain pass went onto the side stream of a batch call, out3[2] = tiles their light kernels listed for the chain pass (the lengths
 * of the need lists).  A pass's need list lives in device memory: its length enters out3[2] when nq_get_dither_path is asked for the
 * hand-back count of that pass (the two counts are read back together), once per pass. */
int nq_get_dither_split_stats(int64_t* out3);
/* Diagnostics: length of every cell's candidate list of the last dither/lookup call (255 = full scan), 65536 bytes each. */
int nq_get_list_counts(nq_handle* h, uint8_t* closest_counts, uint8_t* nearest_counts);
/* Self-test hook of the branch-free CIEDE2000 evaluation inside find_nn (csrc/nq_device.h: ciede_terms_fast): for n pairs
 * {L1, A1, B1, L2, A2, B2} returns, as float bit patterns, out9[9 i + 0..3] = deltaL', deltaC', deltaH', R_T of the fast pass,
 * out9[9 i + 4..7] = the same from the literal functions, out9[9 i + 8] = 1 when the fast pass decided (else find_nn uses the
 * literal values).  Wherever it decided the two quadruples must be identical. */
int nq_selftest_ciede(nq_handle* h, const float* lab_pairs, int64_t n, uint32_t* out9);
/* Self-test hook of the specialised dither kernel's scalar shortcuts (csrc/nq_dither_fast.hip): one launch that calls the SAME device
 * functions as the dither kernel, with qa / qb / qc derived as in every dither launch, the constant tables of the dither launch and
 * PR, PG, PB, ratio of the handle's params (nq_set_params).  `which` selects the filter; n = number of elements evaluated (at most
 * 2^26 per call except for the counting forms).
 * Range modes take in = int64_t {first, count, a0, a1} (count must equal n) and enumerate first .. first + n - 1 on the device:
 *   TANH           element = float bit pattern x.  out[2 i] = bits of tanh_to_float(x), out[2 i + 1] = 1 when tanh_library decided.
 *   CLOSEST_ERR    element = |dr| << 16 | |dg| << 8 | |db|, a0 = sign mask (bit 2 / 1 / 0: dr / dg / db negative; d = entry - colour).
 *                  out[3 i] = the F fast_closest_step leaves in an empty tuple (closest[2] = closest[3] = INT_MAX, so a value near an
 *                  integer always takes the exact evaluation), out[3 i + 1] = bits of the float32 form e32, out[3 i + 2] = 1 when
 *                  closest_err_exact ran.
 *   NEXTINT        element = uu in [0, 2^31), the draw next(31) of nextInt(32767).  out[i] = folded r | accepted << 16.
 *   NEXTINT_COUNT  the same range against plain 64-bit C on the device (uu % 32767; rejected iff uu - r + 32766 >= 2^31).
 *                  out = four words: uint64 number of disagreements, uint64 first disagreeing uu (all ones: none).
 *   REM_COUNT      element = r << 15 | dsum in [0, 2^30); the pairs 0 <= r < 32767, 1 <= dsum <= r are compared with plain r % dsum.
 *                  out as NEXTINT_COUNT (first disagreeing element).
 *   YDIFF_RANGE    element = opaque colour 0xFF000000 | rgb as c1; a0 = c2; a1 = thresholds << 1 | gt, the thresholds (at most 32
 *                  doubles) follow the header.  out[3 i] = bits of the float32 yd, out[3 i + 1] = decision bit per threshold,
 *                  out[3 i + 2] = bit per threshold where the f64 path decided.
 *   LAB32, LAB64   element = rgb of an opaque colour.  out[3 i + 0..2] = bits of L, A, B of lab32_of / of RGB2LAB_fast.
 *   NEAR_D32       element = rgb of an opaque colour, a0 = palette index.  out[i] = bits of the float32 distance fast_nearest32 forms
 *                  against that entry of the palette the handle's last lookup or dither call put on the device (at most 256 entries).
 * Explicit modes take n records at `in`:
 *   CLOSEST_ERR_PAIRS  int32 {colour, palette entry}; out as CLOSEST_ERR.
 *   REM                int32 {r, dsum}; out[i] = the remainder fast_closest_pick uses.
 *   YDIFF              {int32 c1, c2, gt, 0; double thr}; out[3 i] = decision, out[3 i + 1] = bits of yd, out[3 i + 2] = f64 path decided.
 *   NEAR_D32_PAIRS     int32 {colour, palette index}; out as NEAR_D32.  An index past the palette is the caller's error (here and in
 *                      NEAR_SAFE only its low 8 bits are used, and an entry past the palette reads as the colour 0).
 *   TANH_BITS          uint32 float bit patterns; out as TANH.
 *   NEXTINT_LIST       int32 uu in [0, 2^31); out as NEXTINT.
 *   NEAR_SAFE          int32 {colour, ka | kb << 8}; out[i] = the index fast_nearest32 picks from the two-entry list {ka, kb} | safe << 16
 *                      (safe: the runner-up is more than 2 NQ_FAST_NEAR_EPS behind, so the exact scan is skipped).
 *   JUMP               int64 Random state s0 (48 bits); out[66 i + n], n = 0..64 = next(31) of the draw that follows n earlier draws, from the
 *                      jump table of the pixel-form light pass (state (A_{n+1} s0 + C_{n+1}) mod 2^48), | 1 << 31 when nextInt(32767) rejects
 *                      it; out[66 i + 65] = how many of the 65 differ from the draw after n sequential steps of the generator (0).
 * tests/test_gpu_fast_filters.py holds each against the oracle over its whole domain. */
#define NQ_FAST_ST_TANH 0
#define NQ_FAST_ST_CLOSEST_ERR 1
#define NQ_FAST_ST_CLOSEST_ERR_PAIRS 2
#define NQ_FAST_ST_NEXTINT 3
#define NQ_FAST_ST_NEXTINT_COUNT 4
#define NQ_FAST_ST_REM 5
#define NQ_FAST_ST_REM_COUNT 6
#define NQ_FAST_ST_YDIFF 7
#define NQ_FAST_ST_YDIFF_RANGE 8
#define NQ_FAST_ST_LAB32 9
#define NQ_FAST_ST_LAB64 10
#define NQ_FAST_ST_NEAR_D32 11
#define NQ_FAST_ST_NEAR_D32_PAIRS 12
#define NQ_FAST_ST_TANH_BITS 13
#define NQ_FAST_ST_NEXTINT_LIST 14
#define NQ_FAST_ST_NEAR_SAFE 15
#define NQ_FAST_ST_JUMP 16
#define NQ_FAST_ST_MODES 17
int nq_selftest_fast(nq_handle* h, int which, const void* in, int64_t n, uint32_t* out);
int nq_get_params(const nq_handle* h, nq_params* out);
int nq_set_params(nq_handle* h, const nq_params* in);

/* ---- the ditherers' own static entry points: the Ditherable is the handle (its kind and params answer
 *      getColorIndex / nearestColorIndex exactly as in nq_dither) ----
 * static int[] GilbertCurve.dither(width, height, pixels, palette, ditherable, saliencies, weight, dither)
 *      (NQ/GilbertCurve.java:367-373): saliencies may be NULL, weight is the SIGNED constructor argument (negative = the image has
 *      semi-transparent pixels, :60-61).  out_qpixels follows the reference (:278-279): ARGB when dither || K <= 32, palette
 *      indices otherwise; out_index (nullable) always receives the indices.
 * static int[] BlueNoise.dither(width, height, pixels, palette, ditherable, qPixels, weight) (NQ/BlueNoise.java:207-222):
 *      io_qpixels holds palette indices on entry (what GilbertCurve.dither returned for !dither && K > 32) and ARGB on return.
 * REFERENCE_SEQUENTIAL: nq_gilbert_dither starts from empty lookup caches and Random(rng_seed); nq_bluenoise_dither continues with
 * the caches and the random stream the previous call on the handle left behind, as the two calls inside dither() do. */
int nq_gilbert_dither(nq_handle* h, int width, int height, const uint32_t* pixels, const uint32_t* palette, int K,
                      const float* saliencies, double weight, int dither, int64_t rng_seed, int mode,
                      int32_t* out_qpixels, uint16_t* out_index);
int nq_bluenoise_dither(nq_handle* h, int width, int height, const uint32_t* pixels, const uint32_t* palette, int K,
                        int32_t* io_qpixels, float weight, int64_t rng_seed, int mode, uint16_t* out_index);

/* ---- Bitmap convert(int nMaxColors, boolean dither)  (NQ/PnnQuantizer.java:409-456) ----
 * out_argb  [w*h]  : the pixels of the returned Bitmap (always ARGB)
 * out_index [w*h]  : palette index chosen per pixel (nullable)
 * out_palette      : room for max(nMaxColors,2) entries;  *out_K = palette length
 * The input is never modified (the n<=2 rewrite of :424 is applied internally). */
int nq_convert(nq_handle* h, const uint32_t* argb, int width, int height, int nMaxColors, int dither,
               int64_t rng_seed, int mode,
               uint32_t* out_argb, uint16_t* out_index, uint32_t* out_palette, int32_t* out_K);
/* same, all pixel buffers in device memory (out_palette/out_K stay host); asynchronous on the handle's stream
 * except for the small palette-parameter readbacks. */
int nq_convert_device(nq_handle* h, const uint32_t* d_argb, int width, int height, int nMaxColors, int dither,
                      int64_t rng_seed, int mode,
                      uint32_t* d_out_argb, uint16_t* d_out_index, uint32_t* out_palette, int32_t* out_K);

/* ---- convert() of n quantizer objects in one call (the reference app converts one file per executor task,
 *      app/src/main/java/nQuant/android/MainActivity.java:190-214; a service converting many images hands them over
 *      together).  Results are identical to n separate nq_convert_device calls.  The merge loop of one image is a
 *      sequential chain that occupies one CU; here the n merge loops run side by side in ONE launch (one workgroup
 *      each), the other stages run image after image on the first handle's stream and share its per-pixel scratch.
 *      The stages in front of the merge loops run on up to eight internal streams; every one of them starts behind the work queued on
 *      the first handle's stream when the call is made, so inputs written asynchronously on that stream are read after their producer.
 *      hs[i] are distinct handles on one device (mixing kinds is allowed); all pointer arrays are host arrays of n
 *      device pointers; out_palettes[i * palette_stride ...] / out_K[i] receive palette i
 *      (palette_stride >= max(nMaxColors, 2)); d_out_index may be NULL.
 *      The dither passes of ALL n images run on the first handle's stream and read state of hs[i] (palette, candidate lists, curve
 *      tables): before the next call on any hs[i] that is set to ANOTHER stream, wait for the first handle's stream -- the
 *      precondition of nq_set_stream, with the batch's stream as hs[i]'s "previous stream". ---- */
int nq_convert_batch_device(nq_handle* const* hs, int n, const uint32_t* const* d_argb, const int32_t* widths,
                            const int32_t* heights, int nMaxColors, int dither, const int64_t* rng_seeds, int mode,
                            uint32_t* const* d_out_argb, uint16_t* const* d_out_index,
                            uint32_t* out_palettes, int32_t palette_stride, int32_t* out_K);

/* same with HOST buffers (what a JNI shim holds): host arrays of n host pointers.  Uploads run ahead of the per-image stages and
 * results are copied back while the next image is dithered, on a second stream; only the inputs (4 B/pixel) stay resident for
 * the batch.  Page-locked buffers (direct ByteBuffers registered with hipHostRegister, hipHostMalloc) make the copies
 * asynchronous; pageable memory works, the copies then block the calling thread.  out_index / out_index[i] may be NULL. */
int nq_convert_batch(nq_handle* const* hs, int n, const uint32_t* const* argb, const int32_t* widths,
                     const int32_t* heights, int nMaxColors, int dither, const int64_t* rng_seeds, int mode,
                     uint32_t* const* out_argb, uint16_t* const* out_index,
                     uint32_t* out_palettes, int32_t palette_stride, int32_t* out_K);

/* ---- one palette for a sequence of frames: an animated GIF's global colour table, a video shot, a set of images shown side by side.
 *      Frames 0..n-1 are ARGB_8888, row-major, each with its own width and height; pointer arrays are host arrays of n pointers.
 *  * Palette and params are what convert() computes for ONE image whose int[] is all the frames' pixels one after another (frame 0
 *    first): the alpha pre-scan (transparentPixelIndex is an index into that sequence, transparentColor the colour there), the
 *    histogram (LAB: the float32 per-bin sums run in sequence order), the few-colours early return of the LAB class
 *    (NQ/PnnLABQuantizer.java:193-206: the HashMap keySet of the sequence's distinct colours, first-occurrence order), quanFn / ratio /
 *    weight and the merge loop.  nq_params.distinctColors counts over the whole sequence.  The palette equals nq_pnnquan_device run on a
 *    concatenated copy of the frames, bit for bit -- but the frames are read in place, no copy is made.
 *  * Frame i's pixels are what nq_set_params(h, <those params>) followed by nq_dither_device(h, frame i, palette, K, dither,
 *    rng_seeds[i], mode, ...) returns: each frame is dithered as an image of its own (its own tiles and automatic tile size, saliency
 *    map and random streams); it shares the palette, the params and the BlueNoise weight.  All three modes are allowed.
 *  * The sequence may hold at most 2^31 - 1 pixels (one Java int[]); for the convert forms every frame has the per-image dither limits
 *    (side <= 65535, nMaxColors <= 8192).  Anything else returns NQ_ERR_INVALID before any device work is done.
 *  * n = 1 gives nq_convert_device's results in every output (palette, K, params, ARGB, index), the nMaxColors <= 2 rewrite included.
 *  RGB sums are integers, so for the RGB kind the order of the frames does not change the palette; for the LAB kind it does, and the
 *  sequence order above is the definition (not the band-order partial sums of nq_palette_from_histograms_device).
 *  nq_pnnquan_frames_device leaves the params in h, like nq_pnnquan: followed by nq_dither_device per frame it is the "palettegen /
 *  paletteuse" split -- a palette from some frames, applied to others.  nq_convert_frames_device: d_out_index and its entries may be
 *  NULL; all work runs on the handle's stream; if frame i fails its status is returned and nq_last_error names the frame.
 *  nq_get_stage_ms covers the whole call: prescan and histogram span all frames, `dither` runs from the first frame's dither pass to the
 *  last frame's end (the BlueNoise post-passes included; `bluenoise` is 0 for n > 1).  nq_convert_frames: the same with HOST buffers
 *  (all frames are uploaded, the device form runs, the results are copied back; out_index and its entries may be NULL). ---- */
int nq_pnnquan_frames_device(nq_handle* h, int n, const uint32_t* const* d_argb, const int32_t* widths, const int32_t* heights,
                             int nMaxColors, uint32_t* out_palette, int32_t* out_K);
int nq_convert_frames_device(nq_handle* h, int n, const uint32_t* const* d_argb, const int32_t* widths, const int32_t* heights,
                             int nMaxColors, int dither, const int64_t* rng_seeds, int mode,
                             uint32_t* const* d_out_argb, uint16_t* const* d_out_index,
                             uint32_t* out_palette, int32_t* out_K);
int nq_convert_frames(nq_handle* h, int n, const uint32_t* const* argb, const int32_t* widths, const int32_t* heights,
                      int nMaxColors, int dither, const int64_t* rng_seeds, int mode,
                      uint32_t* const* out_argb, uint16_t* const* out_index,
                      uint32_t* out_palette, int32_t* out_K);

/* ---- GIF encoding: palette index maps (what the convert calls write to out_index) to a GIF89a file, on the GPU.  Frames 0..n-1 are
 *      uint16 index maps, row-major, each with its own width and height; they share one global colour table, the K ARGB entries of
 *      `palette` (host memory).  The file is standard: every GIF decoder reads it.
 *  * Colour table: N = the smallest value in 0..7 with 2^(N+1) >= max(K, 2); 2^(N+1) RGB entries, zeros after entry K-1.  GIF has
 *    1-bit transparency: t = the first palette entry whose alpha is 0 (none: -1) is the transparent index; every other alpha
 *    value is dropped.  Screen: the largest width and height of the frames, background index t (t < 0: 0).
 *  * n > 1: a NETSCAPE2.0 loop block with loop_count (0 = for ever; -1 = no block, play once) and per frame a graphic control
 *    extension with delays_cs[i] (hundredths of a second; delays_cs NULL: 0) and disposal 2 (restore to background).  n = 1: an
 *    extension only when t >= 0.  Every frame sits at (0, 0).
 *  * LZW: the minimum code size is m = max(2, N + 1).  Each frame's indices are cut into segments of segment_pixels pixels (0: the
 *    default 16384; the last segment may be shorter) and every segment is one LZW chain with a fresh dictionary: the frame's first
 *    segment starts with a Clear code, every segment but the last ends with a Clear code, the last one with End-of-Information.  The
 *    chains run in parallel on the GPU.  A longer segment compresses a little better (1.02x the bytes of one chain over the whole
 *    frame at 16384 pixels on dithered content) and gives fewer chains.  The bit-exact definition: DESIGN.md "GIF encoder".
 *  * nq_gif_max_bytes: an upper bound of the file size for any content and any K (pure arithmetic, no device, no handle).
 *  * nq_encode_gif_device: index maps in DEVICE memory (2-byte aligned pointers suffice), everything else on the host.  The file is
 *    assembled in device memory and copied to `out` in one copy; *out_size = its size.  The call returns when `out` holds the file.
 *    h may be a handle of either kind (its stream, scratch and error text are used).  nq_encode_gif: the same with index maps in
 *    HOST memory (they are uploaded first).
 *  * NQ_ERR_INVALID before any device work: n < 1, a side outside 1..65535, K outside 1..256, segment_pixels < 0, loop_count
 *    outside -1..65535, a delay outside 0..65535, NULL or odd index pointers.  After the encoding: an index >= K, or cap smaller
 *    than the file (then *out_size holds the size and `out` is untouched).  The handle stays usable after any of these. ---- */
int nq_gif_max_bytes(int n, const int32_t* widths, const int32_t* heights, int K, int segment_pixels, int64_t* out_bytes);
int nq_encode_gif_device(nq_handle* h, int n, const uint16_t* const* d_index, const int32_t* widths, const int32_t* heights,
                         const uint32_t* palette, int K, const int32_t* delays_cs, int loop_count, int segment_pixels,
                         uint8_t* out, int64_t cap, int64_t* out_size);
int nq_encode_gif(nq_handle* h, int n, const uint16_t* const* index, const int32_t* widths, const int32_t* heights,
                  const uint32_t* palette, int K, const int32_t* delays_cs, int loop_count, int segment_pixels,
                  uint8_t* out, int64_t cap, int64_t* out_size);

/* ---- GIF encoding, delta mode: an animation whose frames store only what changed.  All n frames are width x height.  Frame 0 is
 *      written whole; frame i >= 1 is the bounding rectangle of the pixels where index map i differs from index map i - 1, and the
 *      unchanged pixels inside it are transparent.  Every frame has disposal 1 ("keep"), so the canvas after frame i - 1 is frame i - 1
 *      and a decoder composes frame i exactly.  What makes static regions repeat from frame to frame is the caller's business: with
 *      NQ_MODE_PARALLEL_TILED and equal seeds a tile whose input pixels did not change gives the same indices again.
 *  * n = 1: the file is byte for byte nq_encode_gif's, out_rects = {0, 0, width, height}.  The rest of this list is n > 1.
 *  * A palette entry with alpha 0 is NQ_ERR_INVALID before any device work: real transparency cannot be un-painted under "keep";
 *    use nq_encode_gif.  Other alpha values are dropped.
 *  * u, the "unchanged" index: u = K when K <= 255; none when K = 256, then frames are cropped only.  Kt = K + 1 when u exists, else K.
 *    N and m follow nq_encode_gif's rules applied to Kt.  Colour table as there (entry u is 0, 0, 0), background index 0, loop block
 *    as there.
 *  * Every frame has a graphic control extension: packed = 1 << 2 | (u exists), delays_cs[i], transparent index u (none: 0).
 *  * Frame i >= 1: D = the pixels with index_i != index_(i-1); the rectangle is D's bounding box, 1 x 1 at (0, 0) when D is empty.
 *    The body is the rectangle row-major: index_i, with every pixel outside D replaced by u when u exists.  The body is cut into
 *    segment_pixels segments and LZW-coded exactly as nq_encode_gif does with a frame.
 *  * nq_gif_max_bytes(n, widths, heights, 256, segment_pixels) with every width / height equal to width / height bounds the file:
 *    no rectangle is larger than its frame and Kt <= 256.
 *  * out_rects (NULL: not wanted): 4 ints per frame, x, y, w, h of its rectangle, written on success.
 *  * Checks, cap / *out_size and the two memory forms as for nq_encode_gif; an index >= K in any frame is reported after the
 *    difference pass.  The index maps are never written.  The handle stays usable after any error.
 *  The bit-exact definition and the kernels: DESIGN.md "GIF encoder, delta mode". ---- */
int nq_encode_gif_delta_device(nq_handle* h, int n, const uint16_t* const* d_index, int width, int height,
                               const uint32_t* palette, int K, const int32_t* delays_cs, int loop_count, int segment_pixels,
                               uint8_t* out, int64_t cap, int64_t* out_size, int32_t* out_rects);
int nq_encode_gif_delta(nq_handle* h, int n, const uint16_t* const* index, int width, int height,
                        const uint32_t* palette, int K, const int32_t* delays_cs, int loop_count, int segment_pixels,
                        uint8_t* out, int64_t cap, int64_t* out_size, int32_t* out_rects);

/* ---- GIF encoding, lossy mode: the four GIF calls above with one more argument, `lossy` (0..255), after segment_pixels.  What decides
 *      the size of a GIF once the still pixels are gone is how well the rest compresses, and a dithered index map is close to the worst
 *      case for LZW: neighbouring pixels flip between two or three near palette colours and almost no string repeats.  In lossy mode
 *      (gifsicle --lossy, gifski's quality) the encoder may, where the exact next index does not continue the current dictionary
 *      string, take a near colour that does: matches get longer, there are fewer codes.  The file is a standard GIF.
 *  * Everything about the file is as nq_encode_gif / nq_encode_gif_delta define it: header, colour table, extensions, rectangles, bodies,
 *    segmentation, Clear and End-of-Information placement, code widths, sub-blocks.  The one change is inside a segment's chain, at the
 *    step "is (pre, c) in the dictionary?" (pre: the code of the current string, c: the next pixel's index):
 *      rgb[i] = the 8-bit r, g, b of entry i of the Kt-entry colour table as written to the file (alpha is ignored; delta mode's
 *               entry u is 0, 0, 0);  T = the file's transparent index: t for the full-frame calls, u for delta mode, -1 when none
 *      (pre, c) is in the dictionary:  proceed as without lossy (the exact index always wins, also among duplicate colours)
 *      otherwise, when lossy > 0 and c != T:  the candidates are all c' in 0..Kt-1 with c' != c, c' != T, (pre, c') in the dictionary
 *               and max(|dr|, |dg|, |db|) <= lossy between rgb[c'] and rgb[c].  If there is one, take the c' with the smallest
 *               (dr^2 + dg^2 + db^2, c') in lexicographic order: pre = the code of (pre, c'), go on with the next pixel; this pixel
 *               decodes as c'
 *      no candidate:  exactly the miss of the lossless call: emit pre, add (pre, c) with the EXACT c (or Clear at 4096), pre = c
 *    A segment's first pixel is always exact.
 *  * lossy = 0 gives the bytes of the call without `lossy`, byte for byte.
 *  * Every decoded pixel is the source index or a colour within `lossy` per channel of the source index's colour.  The metric is that
 *    of nq_hold_frames' threshold, on purpose: the two knobs read alike.
 *  * A transparent pixel is never replaced, and no pixel is replaced by the transparent index.
 *  * Delta mode: rectangles and bodies come from the index maps as given, so out_rects equals the lossless call's, and the bound holds
 *    for the composed canvas: a kept pixel shows a colour within `lossy` of an index that has not changed since.
 *  * nq_gif_max_bytes bounds the file as before: a chain still emits at most one code per pixel.
 *  * lossy outside 0..255 is NQ_ERR_INVALID before any device work (*out_size and out_rects untouched).  All other checks, cap /
 *    *out_size, out_rects and the two memory forms are as for the counterparts; an index >= K is reported after the encoding.
 *  The kernel and why the exact c is what enters the dictionary: DESIGN.md 5b "lossy mode". ---- */
int nq_encode_gif_lossy_device(nq_handle* h, int n, const uint16_t* const* d_index, const int32_t* widths, const int32_t* heights,
                               const uint32_t* palette, int K, const int32_t* delays_cs, int loop_count, int segment_pixels, int lossy,
                               uint8_t* out, int64_t cap, int64_t* out_size);
int nq_encode_gif_lossy(nq_handle* h, int n, const uint16_t* const* index, const int32_t* widths, const int32_t* heights,
                        const uint32_t* palette, int K, const int32_t* delays_cs, int loop_count, int segment_pixels, int lossy,
                        uint8_t* out, int64_t cap, int64_t* out_size);
int nq_encode_gif_delta_lossy_device(nq_handle* h, int n, const uint16_t* const* d_index, int width, int height,
                                     const uint32_t* palette, int K, const int32_t* delays_cs, int loop_count, int segment_pixels, int lossy,
                                     uint8_t* out, int64_t cap, int64_t* out_size, int32_t* out_rects);
int nq_encode_gif_delta_lossy(nq_handle* h, int n, const uint16_t* const* index, int width, int height,
                              const uint32_t* palette, int K, const int32_t* delays_cs, int loop_count, int segment_pixels, int lossy,
                              uint8_t* out, int64_t cap, int64_t* out_size, int32_t* out_rects);

/* ---- GIF encoding, local colour tables: one palette per frame instead of one per file.  An animation with a scene cut, or a slide
 *      show of unrelated pictures, is not tied to 256 colours for its whole length: frames of one shot share a palette, the next shot
 *      brings its own.  The palettes use the layout nq_convert_batch returns and nq_encode_png takes: frame i has K[i] <= 256 ARGB
 *      entries at palettes[i * palette_stride] (host memory).  `lossy` is an argument of these calls from the start; 0 is lossless.
 *      Everything not restated here is as nq_encode_gif / nq_encode_gif_delta / "lossy mode" define it: segmentation, the chain
 *      listing, Clear and End-of-Information placement, sub-blocks, the NETSCAPE2.0 block, cap / *out_size, that the call returns
 *      when `out` holds the file, that the index maps are never written, the _device form with 2-byte aligned device pointers and the
 *      host form that uploads first.
 *  Full frames (nq_encode_gif_local):
 *  * "GIF89a", then the screen descriptor: the largest width and height, packed 0x70 (NO global table), background 0, aspect 0.  The
 *    loop block as before (n > 1 and loop_count >= 0).
 *  * Per frame i: N_i, m_i and t_i follow nq_encode_gif's rules applied to frame i's own K[i] and palette (t_i: its first entry
 *    with alpha 0, -1: none).
 *  * A graphic control extension when n > 1 or t_i >= 0: packed = (n > 1 ? 2 << 2 : 0) | (t_i >= 0), delays_cs[i], then t_i or 0.
 *  * The image descriptor at (0, 0) with packed 0x80 | N_i, then 2^(N_i+1) RGB entries (zeros after entry K[i] - 1), the byte m_i and
 *    the sub-blocks.
 *  * n = 1 is this same form.  It is NOT byte-equal to nq_encode_gif's file, which has a global table and no local one.
 *  Delta mode (nq_encode_gif_local_delta), all frames width x height:
 *  * rgb_i[j] = the 24-bit RGB of entry j of frame i's palette (alpha is not part of it).
 *  * n > 1: an alpha-0 entry in ANY frame's palette is NQ_ERR_INVALID before any device work, for delta mode's reason.
 *  * u_i = K[i] when K[i] <= 255; a frame with K[i] = 256 has no u_i and is cropped only.  Kt_i = K[i] + (u_i exists); N_i and m_i
 *    come from Kt_i; table entry u_i is 0, 0, 0.
 *  * Every frame, frame 0 included, uses Kt_i and has an extension: packed = 1 << 2 | (u_i exists), delays_cs[i], then u_i or 0.
 *  * Frame 0 is written whole.
 *  * Frame i >= 1: D = the pixels p with rgb_i[index_i[p]] != rgb_(i-1)[index_(i-1)[p]] -- "unchanged" is judged on the colour shown,
 *    not on the index, since index 7 of frame i and index 7 of frame i - 1 are unrelated once the tables differ.  The rectangle is D's
 *    bounding box, 1 x 1 at (0, 0) when D is empty.  The body is index_i over the rectangle, with the pixels outside D replaced by u_i
 *    where it exists.  With equal palettes in consecutive frames this is nq_encode_gif_delta's D, up to duplicate colours.
 *  * n = 1 is the full-frame local file, out_rects = {0, 0, width, height}.
 *  Lossy mode (both calls): the loop body of "lossy mode" per frame, with rgb = that frame's written table and Kt = that frame's Kt_i;
 *    T = t_i for full frames, u_i for delta mode, -1 when there is none.  Rectangles and bodies come from the maps and palettes as
 *    given, so out_rects does not depend on `lossy`.
 *  * nq_gif_local_max_bytes = nq_gif_max_bytes(n, widths, heights, 256, segment_pixels) + 768 * n bounds either file (delta mode: pass
 *    n copies of width / height): it drops one global table and adds at most one 768-byte table per frame.
 *  * NQ_ERR_INVALID before any device work, *out_size and out_rects untouched: nq_encode_gif's list (nq_encode_gif_delta's for delta
 *    mode), a K[i] outside 1..256, palette_stride smaller than a K[i], K or palettes NULL, lossy outside 0..255.  An index >= its own
 *    frame's K[i] is reported after the encoding (delta mode: after the difference pass, anywhere in any frame); nq_last_error names the
 *    frame.  The handle stays usable after every error.
 *  The kernels, and why no canvas is composed: DESIGN.md 5b "Local colour tables". ---- */
int nq_gif_local_max_bytes(int n, const int32_t* widths, const int32_t* heights, int segment_pixels, int64_t* out_bytes);
int nq_encode_gif_local_device(nq_handle* h, int n, const uint16_t* const* d_index, const int32_t* widths, const int32_t* heights,
                               const uint32_t* palettes, int32_t palette_stride, const int32_t* K, const int32_t* delays_cs, int loop_count,
                               int segment_pixels, int lossy, uint8_t* out, int64_t cap, int64_t* out_size);
int nq_encode_gif_local(nq_handle* h, int n, const uint16_t* const* index, const int32_t* widths, const int32_t* heights,
                        const uint32_t* palettes, int32_t palette_stride, const int32_t* K, const int32_t* delays_cs, int loop_count,
                        int segment_pixels, int lossy, uint8_t* out, int64_t cap, int64_t* out_size);
int nq_encode_gif_local_delta_device(nq_handle* h, int n, const uint16_t* const* d_index, int width, int height,
                                     const uint32_t* palettes, int32_t palette_stride, const int32_t* K, const int32_t* delays_cs,
                                     int loop_count, int segment_pixels, int lossy, uint8_t* out, int64_t cap, int64_t* out_size,
                                     int32_t* out_rects);
int nq_encode_gif_local_delta(nq_handle* h, int n, const uint16_t* const* index, int width, int height,
                              const uint32_t* palettes, int32_t palette_stride, const int32_t* K, const int32_t* delays_cs,
                              int loop_count, int segment_pixels, int lossy, uint8_t* out, int64_t cap, int64_t* out_size,
                              int32_t* out_rects);

/* ---- PNG encoding: palette index maps (what the convert calls write to out_index) to indexed PNG files, on the GPU.  One call encodes
 *      n independent images into n files (n = 1 is the plain case; a batch fills the chip).  Image i is a uint16 index map, row-major,
 *      widths[i] x heights[i], with its own K[i] <= 256 and its own palette: the K[i] ARGB entries at palettes[i * palette_stride]
 *      (host memory; the layout nq_convert_batch returns).  The files are standard: every PNG decoder reads them.
 *  * Chunks: IHDR (colour type 3, no interlace), PLTE (K RGB entries), tRNS only when some entry's alpha is not 255 (the alpha bytes of
 *    entries 0 .. the last such entry: all 8 bits of alpha are kept), one IDAT, IEND.
 *  * Bit depth d: the smallest of 1, 2, 4, 8 with 2^d >= max(K, 2).  Every scanline has filter type 0; its indices are packed most
 *    significant bits first and padded to a byte.  The raw stream is heights[i] * (1 + ceil(widths[i] * d / 8)) bytes.
 *  * IDAT holds a zlib stream (header 78 01, deflate data, Adler-32).  The raw stream is cut into segments of segment_bytes bytes (0:
 *    the default 32768; at most 65535; the last segment may be shorter).  Every segment is one chain that sees only its own bytes
 *    (no match reaches before its start) and emits one dynamic-Huffman block; BFINAL is set on the last.  The chains run in parallel
 *    on the GPU.  A longer segment compresses a little better and gives fewer chains: on a dithered 256-colour map the default gives
 *    0.997x the bytes of zlib level 1 and 1.05x those of level 6.  The bit-exact definition (hash, parse, code lengths): DESIGN.md
 *    "PNG encoder".
 *  * nq_png_max_bytes: an upper bound of the n files' total size for any content (pure arithmetic, no device, no handle); K NULL
 *    stands for 256 everywhere.
 *  * nq_encode_png_device: index maps in DEVICE memory (2-byte aligned pointers suffice), everything else on the host.  The files are
 *    assembled back to back in device memory and copied to `out` in one copy: file i is out[out_offsets[i] .. out_offsets[i + 1]).
 *    The call returns when `out` holds them.  h may be a handle of either kind (its stream, scratch and error text are used).
 *    nq_encode_png: the same with index maps in HOST memory (they are uploaded first).
 *  * NQ_ERR_INVALID before any device work: n < 1, a side outside 1..65535, a K outside 1..256, palette_stride smaller than a K,
 *    segment_bytes outside 0..65535, NULL or odd index pointers, an image whose size bound exceeds 2^31 - 1 bytes.  After the
 *    encoding: an index >= its image's K (nq_last_error names the image), or cap smaller than the files (then out_offsets[n] holds
 *    the size needed and `out` is untouched).  The handle stays usable after any of these. ---- */
int nq_png_max_bytes(int n, const int32_t* widths, const int32_t* heights, const int32_t* K, int segment_bytes, int64_t* out_bytes);
int nq_encode_png_device(nq_handle* h, int n, const uint16_t* const* d_index, const int32_t* widths, const int32_t* heights,
                         const uint32_t* palettes, int32_t palette_stride, const int32_t* K, int segment_bytes,
                         uint8_t* out, int64_t cap, int64_t* out_offsets);
int nq_encode_png(nq_handle* h, int n, const uint16_t* const* index, const int32_t* widths, const int32_t* heights,
                  const uint32_t* palettes, int32_t palette_stride, const int32_t* K, int segment_bytes,
                  uint8_t* out, int64_t cap, int64_t* out_offsets);

/* ---- APNG encoding: n index maps of one size over one palette to ONE animated PNG file whose frames store only what changed, with
 *      all 8 bits of the palette's alpha (what delta GIF cannot do: it refuses alpha 0 and drops every other alpha).  All n frames are
 *      width x height uint16 index maps over the K <= 256 ARGB entries of `palette` (what nq_convert_frames returns).  A frame's data
 *      is the zlib stream nq_encode_png writes, so the same chains encode it; every APNG decoder composes the file back to the frames,
 *      and a plain PNG decoder shows frame 0.
 *  * n = 1: the file is byte for byte nq_encode_png's (no acTL, no fcTL), out_rects = {0, 0, width, height}.  The rest is n > 1.
 *  * One mode per file, decided from the palette alone.  Mark mode: every alpha is 255 and K <= 255; then u = K is the "unchanged"
 *    index, Kt = K + 1, palette entry u is (0, 0, 0) with alpha 0, and frames >= 1 have blend_op 1 (OVER).  Crop mode otherwise: no
 *    u, Kt = K, every frame has blend_op 0 (SOURCE), which replaces the region whatever the alpha is.  (In mark mode the bit depth
 *    grows when K is 2, 4 or 16.)
 *  * Header: signature; IHDR (depth: the smallest of 1, 2, 4, 8 with 2^d >= max(Kt, 2); colour type 3); PLTE (Kt RGB entries); tRNS by
 *    nq_encode_png's rule applied to the Kt entries (mark mode: K bytes 255, then 0); acTL (num_frames = n, num_plays = loop_count,
 *    0 = for ever).
 *  * Frame i: fcTL {sequence_number, the rectangle's width, height, x, y, delay_num = delays_cs[i] (NULL: 0), delay_den = 100,
 *    dispose_op 0, blend_op as above (frame 0: always 0)}, then its data: frame 0 one IDAT, frame i >= 1 one fdAT (its sequence number,
 *    then the zlib stream).  fcTL and fdAT share one sequence counter that starts at 0.  IEND follows the last frame.
 *  * Rectangle: frame 0 whole.  Frame i >= 1: D = the pixels with index_i != index_(i-1); the rectangle is D's bounding box, 1 x 1 at
 *    (0, 0) when D is empty.  The body is the rectangle row-major: index_i, in mark mode with every pixel outside D replaced by u.
 *  * A frame's zlib stream is exactly what nq_encode_png puts into IDAT for an image that is the body, with Kt colours and the same
 *    segment_bytes: header 78 01, the raw stream (per row a filter byte 0, then the indices packed most significant bits first) cut
 *    into segments, one dynamic-Huffman chain each, BFINAL on the last, Adler-32.  The bodies are never materialised: the chains read
 *    the rectangle out of the two index maps.
 *  * nq_apng_max_bytes: an upper bound of the file size for any content and any K (pure arithmetic, no device, no handle): n times
 *    nq_png_max_bytes of one width x height image at K = 256, plus 58 bytes (acTL and frame 0's fcTL) -- no rectangle exceeds its
 *    frame, Kt <= 256, and a later frame's fcTL and sequence number are smaller than the still-image header it does not repeat.
 *  * out_rects (NULL: not wanted): 4 ints per frame, x, y, w, h of its rectangle, written on success.
 *  * nq_encode_apng_device: index maps in DEVICE memory (2-byte aligned pointers suffice; never written), everything else on the host;
 *    h may be a handle of either kind.  The file is assembled in device memory and copied to `out` in one copy; *out_size = its size.
 *    nq_encode_apng: the same with index maps in HOST memory (they are uploaded first).
 *  * NQ_ERR_INVALID before any device work (*out_size and out_rects stay untouched): n < 1, a side outside 1..65535, K outside
 *    1..256, segment_bytes outside 0..65535, loop_count < 0, a delay outside 0..65535, NULL or odd index pointers, a frame whose size
 *    bound (K = 256) exceeds 2^31 - 1 bytes.  After the encoding: an index >= K anywhere in any frame (n >= 2: reported after the
 *    difference pass, also outside the rectangle), or cap smaller than the file (then *out_size holds the size and `out` is
 *    untouched).  The handle stays usable after any of these.
 *  The bit-exact definition and the kernels: DESIGN.md "PNG encoder, animated (APNG)". ---- */
int nq_apng_max_bytes(int n, int width, int height, int segment_bytes, int64_t* out_bytes);
int nq_encode_apng_device(nq_handle* h, int n, const uint16_t* const* d_index, int width, int height,
                          const uint32_t* palette, int K, const int32_t* delays_cs, int loop_count, int segment_bytes,
                          uint8_t* out, int64_t cap, int64_t* out_size, int32_t* out_rects);
int nq_encode_apng(nq_handle* h, int n, const uint16_t* const* index, int width, int height,
                   const uint32_t* palette, int K, const int32_t* delays_cs, int loop_count, int segment_bytes,
                   uint8_t* out, int64_t cap, int64_t* out_size, int32_t* out_rects);

/* ---- temporal hold: what makes still regions of REAL footage repeat from frame to frame, so that the delta GIF and APNG encoders above
 *      find something to drop.  One least-significant bit of sensor or codec noise in a tile changes that tile's whole error-diffusion
 *      chain; after this pass a pixel whose SOURCE colour has not moved by more than `threshold` keeps the PALETTE INDEX (and the ARGB
 *      output) it had in the frame before (gifski, ffmpeg paletteuse diff_mode).  It runs between nq_convert_frames_device and the
 *      encoder, on the buffers those calls share; no palette is needed.
 *  * Inputs: n ARGB frames d_argb[i] (never written), their n uint16 index maps d_index[i] and, optionally, their n ARGB outputs
 *    d_out_argb[i], both updated in place; all are width x height.  threshold is 0..255.
 *  * For every pixel position p, independently of every other:
 *        anchor = argb[0][p]
 *        for i = 1 .. n-1:
 *            d = the largest |difference| of the four 8-bit channels (a, r, g, b) of argb[i][p] and anchor
 *            d <= threshold: index[i][p] = index[i-1][p], out_argb[i][p] = out_argb[i-1][p] (the values AFTER frame i-1 was processed),
 *                            held[i] += 1
 *            otherwise:      anchor = argb[i][p]; index[i][p] and out_argb[i][p] stay as they are
 *    The anchor moves only when a pixel is released: a slow fade accumulates until it exceeds the threshold and is then taken over, it
 *    never drifts without bound.  threshold 0 holds exactly the pixels whose source equals the anchor bit for bit.  Frame 0 is never
 *    written and held[0] = 0; n = 1 checks its arguments and does nothing else.  Nothing outside the n * width * height elements of
 *    each array is read or written.
 *  * The trade: a held pixel does not diffuse its quantisation error again -- it shows the colour it was given when its anchor was
 *    set, not the nearest rendering of its present source.  With a threshold near the noise floor (2..6) that is invisible and the
 *    background stops shimmering; a large threshold posterises slow gradients in time.
 *  * nq_hold_frames_device: the frames in DEVICE memory; pointer arrays are host arrays of n pointers.  Index pointers need 2-byte,
 *    ARGB pointers 4-byte alignment; when every pointer is 16-byte aligned the kernel moves 16 bytes per access, otherwise one pixel per
 *    access (same results).  No index map or output may overlap any other buffer of the call.  out_held (host, n values; NULL: not wanted) receives held[];
 *    the call returns when it is there.  With out_held == NULL the call is asynchronous on the handle's stream.  h may be a handle of
 *    either kind: its stream, scratch and error text are used, its params are neither read nor changed.
 *    nq_hold_frames: the same with HOST buffers (all frames are uploaded, the device form runs, index maps and outputs 1 .. n-1 are
 *    copied back).
 *  * NQ_ERR_INVALID before any device work, every buffer untouched: n < 1, a side outside 1..65535, threshold outside 0..255, a NULL
 *    pointer array or entry (d_out_argb may be NULL as a whole, not in part), an odd index pointer, an ARGB pointer that is not 4-byte
 *    aligned, n * width * height above 2^31 - 1.  The handle stays usable after any of these.
 *  The kernel: DESIGN.md 5b "temporal hold". ---- */
int nq_hold_frames_device(nq_handle* h, int n, const uint32_t* const* d_argb, uint16_t* const* d_index, uint32_t* const* d_out_argb,
                          int width, int height, int threshold, int64_t* out_held);
int nq_hold_frames(nq_handle* h, int n, const uint32_t* const* argb, uint16_t* const* index, uint32_t* const* out_argb,
                   int width, int height, int threshold, int64_t* out_held);

/* ---- shot detection: where an animation needs a new palette, i.e. the shot_starts the local-colour-table encoders above are fed
 *      (palette per shot).  The measure is on the COLOUR DISTRIBUTION of a frame, not on pixel positions: a pan over one scene keeps
 *      its palette.  All frames are width x height, ARGB_8888.
 *  * Signature of a frame: sig[c][v] = the number of pixels whose channel c has the value v; c = 0..3 for a, r, g, b (shifts 24, 16,
 *    8, 0), v = 0..255: NQ_SIG_WORDS = 1024 uint32 counts per frame, sig[256 c + v].  Channels are counted as stored (a pixel with
 *    alpha 0 still contributes its r, g, b); every row sig[c][.] sums to npix = width * height.
 *  * Score of two signatures A, B (per mille, 0..1000), all arithmetic in int64:
 *        E_c   = sum over v = 0..254 of | sum over t <= v of (A[c][t] - B[c][t]) |      the 1-D earth mover's distance, <= 255 npix
 *        score = floor(1000 * max_c E_c / (255 * npix))
 *    It is graded: a brightness shift of d levels scores d / 255.
 *  * Rule (an anchor, as in the temporal hold: it moves only when a shot ends):
 *        A = 0; starts = {0}; scores[0] = 0
 *        for i = 1 .. n-1:
 *            scores[i] = score(sig[i], sig[A])
 *            if scores[i] > threshold_pm and i - A >= min_shot: starts += {i}; A = i
 *    scores[i] is the value measured against the anchor in force BEFORE the decision.  Comparing with the shot's first frame makes a
 *    slow drift accumulate until it is taken as a cut; a cut suppressed by min_shot is taken late, when min_shot is reached, not lost.
 *    threshold_pm is 0..1000 (1000 never cuts), min_shot >= 1.
 *  * nq_frame_signatures_device: the frames in DEVICE memory, d_argb a host array of n device pointers (4-byte aligned; when every
 *    one is 16-byte aligned the kernel reads 16 bytes per access, same results); the frames are never written.  out_sig (HOST memory,
 *    n * NQ_SIG_WORDS words) is filled when the call returns.  nq_frame_signatures: the same with HOST frames (uploaded first).
 *    h may be a handle of either kind: its stream, scratch and error text are used, its params are neither read nor changed.
 *  * nq_shots_from_signatures: the rule above over n signatures of frames with npix pixels -- pure host arithmetic, no device and no
 *    handle.  out_starts (room for n entries) receives the shot starts, *out_n_shots how many there are, out_scores (n entries, or
 *    NULL: not wanted) the scores.  NQ_ERR_INVALID, outputs untouched: sig, out_starts or out_n_shots NULL, n < 1, npix outside
 *    1 .. 2^31 - 1, threshold_pm outside 0..1000, min_shot < 1, a row of a signature that does not sum to npix.
 *  * nq_detect_shots_device / nq_detect_shots: the signatures call followed by nq_shots_from_signatures; n = 1 gives starts = {0}.
 *  * NQ_ERR_INVALID before any device work, outputs untouched: n < 1, a side outside 1..65535, n * width * height above 2^31 - 1, a
 *    NULL pointer array or entry, an ARGB pointer that is not 4-byte aligned, threshold_pm outside 0..1000, min_shot < 1, NULL
 *    out_starts, out_n_shots or out_sig.  The handle stays usable after any of these.
 *  The kernel: DESIGN.md 5b "Shot detection". ---- */
#define NQ_SIG_WORDS 1024
int nq_frame_signatures_device(nq_handle* h, int n, const uint32_t* const* d_argb, int width, int height, uint32_t* out_sig);
int nq_frame_signatures(nq_handle* h, int n, const uint32_t* const* argb, int width, int height, uint32_t* out_sig);
int nq_shots_from_signatures(const uint32_t* sig, int n, int64_t npix, int threshold_pm, int min_shot,
                             int32_t* out_starts, int32_t* out_n_shots, int32_t* out_scores);
int nq_detect_shots_device(nq_handle* h, int n, const uint32_t* const* d_argb, int width, int height, int threshold_pm, int min_shot,
                           int32_t* out_starts, int32_t* out_n_shots, int32_t* out_scores);
int nq_detect_shots(nq_handle* h, int n, const uint32_t* const* argb, int width, int height, int threshold_pm, int min_shot,
                    int32_t* out_starts, int32_t* out_n_shots, int32_t* out_scores);

/* ---- palette refinement: k-means (Lloyd) passes over a palette, and the squared error of a palette against the pixels.  The PNN
 *      merge loop stops at a greedy merge; a few passes of "assign every pixel to its nearest entry, move every entry to the mean of
 *      its pixels" lower the error further.  Opt-in: no other entry point's results change.  All arithmetic is integer.
 *  * Inputs: n ARGB_8888 frames, each with its own width and height (as for nq_pnnquan_frames_device); a palette of K entries (1..256)
 *    in HOST memory, read and written; iterations in 0..64.
 *  * The channels of a colour are a, r, g, b (shifts 24, 16, 8, 0).  A pixel with a = 0 is NOT COUNTED: it takes part in nothing.  A
 *    palette entry with a = 0 is PINNED: no pixel is assigned to it and it never changes.  An entry that is not pinned is LIVE.  With
 *    no live entry, no pixel is counted.
 *  * d(p, c) = da^2 + dr^2 + dg^2 + db^2.  A counted pixel is assigned to the live entry with the smallest d; on a tie to the lowest
 *    index.
 *  * Passes:
 *        P_0 = the palette as given
 *        for j = 0 .. iterations:
 *            assignment pass under P_j:
 *                cnt[k]   = pixels assigned to k
 *                sum_c[k] = sum of their channel c, c in {r, g, b}
 *                sse[j]   = sum over the counted pixels of d(p, its entry)
 *            if j == iterations: stop
 *            update: for every live k with cnt[k] > 0 and c in {r, g, b}:
 *                        P_{j+1}[k].c = floor((2 * sum_c[k] + cnt[k]) / (2 * cnt[k]))          (the mean, half rounds up)
 *                    the alpha of an entry NEVER changes; empty and pinned entries stay as they are
 *            if P_{j+1} == P_j: sse[j+1 .. iterations] = sse[j]; stop
 *  * Outputs: io_palette = the last palette; out_sse: iterations + 1 values; out_counts: K values or NULL, cnt[] of the last
 *    assignment pass that ran; *out_passes: the number of assignment passes that ran.
 *  * iterations = 0 is a pure error measurement.  sse is non-increasing, exactly: the rounded mean is the integer minimiser of a
 *    cluster's squared error per channel, and re-assignment cannot raise the error.  Alpha is part of the distance, so pixels pick
 *    entries of like alpha; it is not part of the update, so an opaque palette stays opaque.  Integer sums make the result
 *    independent of the order of the additions: it is deterministic.  The metric is plain ARGB for both kinds of handle.
 *  * Limits: the sequence holds at most 2^31 - 1 pixels, so every per-entry sum is at most 255 * 2^31 and sse at most 260 100 * 2^31.
 *  * nq_refine_palette_device: the frames in DEVICE memory, d_argb a host array of n device pointers (4-byte aligned; when every one
 *    is 16-byte aligned the kernel reads 16 bytes per access, same results); the frames are never written.  nq_refine_palette: the
 *    same with HOST frames (uploaded first, each on a 16-byte boundary).  h may be a handle of either kind: its stream, scratch and
 *    error text are used, its params are neither read nor changed.
 *  * NQ_ERR_INVALID before any device work, every output untouched, the handle still usable: n < 1, a side outside 1..65535, more
 *    than 2^31 - 1 pixels in total, K outside 1..256, iterations outside 0..64, a NULL pointer array, a NULL entry, NULL io_palette,
 *    out_sse or out_passes, a frame pointer that is not 4-byte aligned.
 *  * nq_convert_frames_refined_device / nq_convert_frames_refined: nq_convert_frames[_device] with `refine` update passes between the
 *    palette and the dither: palette and params are nq_pnnquan_frames_device's, then the palette takes `refine` iterations of the
 *    passes above over the same frames, then every frame is dithered with the refined palette exactly as nq_convert_frames_device
 *    does it.  refine = 0 gives nq_convert_frames[_device]'s results in every output, bit for bit.  refine outside 0..64, and
 *    refine > 0 with nMaxColors > 256 or with a frame pointer that is not 4-byte aligned, are NQ_ERR_INVALID.
 *  The kernel: DESIGN.md 5d "Palette refinement". ---- */
int nq_refine_palette_device(nq_handle* h, int n, const uint32_t* const* d_argb, const int32_t* widths, const int32_t* heights,
                             uint32_t* io_palette, int K, int iterations,
                             int64_t* out_sse, int64_t* out_counts, int32_t* out_passes);
int nq_refine_palette(nq_handle* h, int n, const uint32_t* const* argb, const int32_t* widths, const int32_t* heights,
                      uint32_t* io_palette, int K, int iterations,
                      int64_t* out_sse, int64_t* out_counts, int32_t* out_passes);
int nq_convert_frames_refined_device(nq_handle* h, int n, const uint32_t* const* d_argb, const int32_t* widths, const int32_t* heights,
                                     int nMaxColors, int refine, int dither, const int64_t* rng_seeds, int mode,
                                     uint32_t* const* d_out_argb, uint16_t* const* d_out_index,
                                     uint32_t* out_palette, int32_t* out_K);
int nq_convert_frames_refined(nq_handle* h, int n, const uint32_t* const* argb, const int32_t* widths, const int32_t* heights,
                              int nMaxColors, int refine, int dither, const int64_t* rng_seeds, int mode,
                              uint32_t* const* out_argb, uint16_t* const* out_index,
                              uint32_t* out_palette, int32_t* out_K);

/* ---- frame reduction: crop a sequence of ARGB_8888 frames and area-average it down to the size of the file, in front of everything
 *      above (gifski --width, ffmpeg scale= before palettegen).  Averaging is in linear light (or, on request, in stored values), alpha
 *      is premultiplied while averaging, and all arithmetic is integer: the result is deterministic and can be restated bit for bit.
 *  * Inputs: n frames of src_width x src_height words, rows contiguous; a crop rectangle (crop_x, crop_y, crop_w, crop_h) inside each
 *    frame; a target size dst_width x dst_height with 1 <= dst_width <= crop_w and 1 <= dst_height <= crop_h (this is a reducer:
 *    enlarging is refused); flags: bit 0 is NQ_RESAMPLE_LINEAR.  Write cw, ch, dw, dh for the crop's and the target's sides.  All of
 *    the following are exact integers, unsigned 64-bit where sums are formed.
 *  * Table T[v], v = 0..255.  With NQ_RESAMPLE_LINEAR, T is the 256-entry table of include/nq_srgb_linear_16.inc:
 *    L[v] = floor(65535 f(v / 255) + 0.5), f the sRGB decoding function (c / 12.92 for c <= 0.04045, else ((c + 0.055) / 1.055)^2.4);
 *    strictly increasing, L[0..3] = 0, 20, 40, 60, L[254] = 64952, L[255] = 65535; the committed file is the normative one.  Without
 *    the flag T[v] = 257 v.
 *  * Weights.  Output column x covers [x cw, (x + 1) cw) on an axis where source column j of the crop covers [j dw, (j + 1) dw);
 *    wx(x, j) is the length of the overlap, nonzero for j = floor(x cw / dw) .. floor(((x + 1) cw - 1) / dw); the weights of one x sum
 *    to cw.  Every product is at most 65535^2 < 2^32 (an unsigned 32-bit word, not a signed one).  wy(y, i) likewise with ch, dh.
 *    W = cw ch.
 *  * Sums of output pixel (x, y) over its footprint, with a, r, g, b the channels of source pixel (crop_x + j, crop_y + i):
 *        S_a = sum of wx wy a            S_c = sum of wx wy T[c] a    for c = r, g, b        (S_c <= W 65535 255 < 2^56)
 *  * Output: S_a = 0 gives 0x00000000.  Otherwise A = floor((2 S_a + W) / (2 W)); per channel t = floor((2 S_c + S_a) / (2 S_a)) and
 *    the stored value is the smallest v with 2 t <= T[v] + T[v + 1], or 255 if there is none (the nearest table entry, ties to the
 *    smaller); the word is A << 24 | r << 16 | g << 8 | b.  A transparent source pixel contributes nothing to the colour.
 *    Consequences: with dw = cw and dh = ch the call copies the crop exactly for every pixel with a > 0 (a = 0 becomes 0), in both
 *    modes; opaque input gives A = 255 everywhere.
 *  * nq_resample_frames_device: d_src and d_dst are host arrays of n DEVICE pointers; the call is asynchronous on the handle's
 *    stream.  Sources are never written; nothing outside the n dw dh output words is written.  Pointers need 4-byte alignment; when
 *    every source pointer is 16-byte aligned and src_width is a multiple of 4 the kernel reads 16 bytes per access (any crop_x),
 *    otherwise one pixel per access, with the same results.  h may be a handle of either kind: its stream, scratch and error text are
 *    used, its params are neither read nor changed.
 *    nq_resample_frames: the same with HOST buffers (the frames are uploaded, the device form runs, the n outputs are copied back; the
 *    call returns when they are there).
 *  * NQ_ERR_INVALID before any device work, every buffer untouched, the handle still usable: n < 1, a source side outside 1..65535, a
 *    crop that is empty or leaves the frame, a target side < 1 or larger than the crop's, unknown flag bits, a NULL pointer array or
 *    entry, a pointer that is not 4-byte aligned, n src_width src_height above 2^31 - 1, an output that overlaps any source frame or
 *    another output.
 *  The kernel: DESIGN.md 5e "Frame reduction". ---- */
#define NQ_RESAMPLE_LINEAR 1
int nq_resample_frames_device(nq_handle* h, int n, const uint32_t* const* d_src, int src_width, int src_height,
                              int crop_x, int crop_y, int crop_w, int crop_h,
                              uint32_t* const* d_dst, int dst_width, int dst_height, int flags);
int nq_resample_frames(nq_handle* h, int n, const uint32_t* const* src, int src_width, int src_height,
                       int crop_x, int crop_y, int crop_w, int crop_h,
                       uint32_t* const* dst, int dst_width, int dst_height, int flags);

/* ---- YUV input: 8-bit YUV 4:2:0 frames (NV12, NV21, I420, YV12: what a hardware video decoder, Android's camera and MediaCodec
 *      write) in front of the frame path.  nq_frames_from_yuv* converts a sequence 1:1 to ARGB_8888 words; nq_resample_frames_yuv*
 *      converts and reduces it in one step, without the full-size ARGB frames ever existing.  All arithmetic is integer: the result
 *      is deterministic and can be restated bit for bit.
 *  * The frame: width x height, both 1..65535, and three byte pointers y, u, v.  Luma of pixel (x, y) is y[y * y_stride + x].  The
 *    chroma planes are cw2 = (width + 1) >> 1 by ch2 = (height + 1) >> 1 samples; the chroma of pixel (x, y) is
 *    u[(y >> 1) * c_stride + (x >> 1) * c_step], likewise v (sample replication).  c_step is 1 or 2.  This is Android's Image.Plane
 *    (buffer, rowStride, pixelStride).  The named layouts:
 *        NV12           u = uv, v = uv + 1     c_step 2
 *        NV21           v = vu, u = vu + 1     c_step 2
 *        I420 / YV12    two planes             c_step 1
 *    All n frames of a call share width, height, y_stride, c_stride, c_step and the flag word.
 *  * yuv_flags: NQ_YUV_BT709 = 1 (otherwise BT.601); NQ_YUV_FULL_RANGE = 2 (otherwise limited range: luma offset yo = 16; in full
 *    range yo = 0).
 *  * Coefficients: floor(65536 e + 1/2) of the exact rationals e below, with Kr, Kb = 0.299, 0.114 (BT.601) or 0.2126, 0.0722
 *    (BT.709), Kg = 1 - Kr - Kb, and sy = 255/219, sc = 255/224 in limited range, both 1 in full range:
 *        cy = sy    crv = sc 2 (1 - Kr)    cgu = sc 2 (1 - Kb) Kb / Kg    cgv = sc 2 (1 - Kr) Kr / Kg    cbu = sc 2 (1 - Kb)
 *                          cy      crv     cgu     cgv     cbu
 *        601 limited    76309   104597   25675   53279  132201
 *        601 full       65536    91881   22553   46802  116130
 *        709 limited    76309   117489   13975   34925  138438
 *        709 full       65536   103206   12276   30679  121609
 *  * Output, per pixel with its Y and its chroma sample U, V:
 *        R = clamp((cy (Y - yo) + crv (V - 128) + 32768) >> 16)
 *        G = clamp((cy (Y - yo) - cgu (U - 128) - cgv (V - 128) + 32768) >> 16)
 *        B = clamp((cy (Y - yo) + cbu (U - 128) + 32768) >> 16)
 *    >> is the arithmetic shift of a signed 32-bit value (a floor), clamp is to 0..255, the word is 0xFF << 24 | R << 16 | G << 8 | B.
 *    Every intermediate is below 3.6e7 in magnitude.  Each channel is within one level of round-half-up of the exact real formula
 *    (and differs from it at all in at most 5.2e-4 of the 2^24 triples); full-range grey (U = V = 128) is the identity; in limited
 *    range Y = 16 gives 0 and Y = 235 gives 255.
 *  * nq_frames_from_yuv_device: d_y, d_u, d_v, d_dst are host arrays of n DEVICE pointers; output i is width x height words, rows
 *    contiguous.  nq_resample_frames_yuv_device is DEFINED as that call followed by nq_resample_frames_device with the same crop,
 *    target and flags ("frame reduction"), bit for bit; output i is dst_width x dst_height words.  The chroma of crop pixel (j, i) is
 *    the frame's sample ((crop_x + j) >> 1, (crop_y + i) >> 1): an odd crop_x or crop_y shifts the pairing.  The alpha is 255
 *    everywhere.  Both calls are asynchronous on the handle's stream, never write the sources and write nothing outside the n
 *    outputs.  h may be a handle of either kind: its stream, scratch and error text are used, its params are neither read nor changed.
 *    Any plane pointers are accepted; outputs need 4-byte alignment.  When width, every y pointer and y_stride are multiples of 4 and
 *    the chroma is either interleaved (c_step 2, u and v one byte apart in the same order in every frame, the lower one and c_stride
 *    multiples of 4) or planar with u, v and c_stride even (and, 1:1, every output is 16-byte aligned), the kernels load 4 luma bytes
 *    per access and store 16; otherwise one pixel per access, with the same results.
 *    nq_frames_from_yuv / nq_resample_frames_yuv: the same with HOST buffers.  Per frame the luma span ((height - 1) y_stride + width
 *    bytes) and the chroma spans ((ch2 - 1) c_stride + (cw2 - 1) c_step + 1 bytes each) are uploaded -- one span where u's and v's
 *    overlap or touch, as in the interleaved layouts --, the device form runs, the n outputs are copied back; the call returns when
 *    they are there.
 *  * NQ_ERR_INVALID before any device work, every buffer untouched, the handle still usable: n < 1, a side outside 1..65535,
 *    y_stride < width, c_step not 1 or 2, c_stride < c_step (cw2 - 1) + 1, unknown bits in either flag word, a NULL pointer array or
 *    entry, an output pointer that is not 4-byte aligned, n width height above 2^31 - 1, the crop and target errors of
 *    nq_resample_frames, an output that overlaps a source span or another output.
 *  The kernels: DESIGN.md 5g "YUV input". ---- */
#define NQ_YUV_BT709 1
#define NQ_YUV_FULL_RANGE 2
int nq_frames_from_yuv_device(nq_handle* h, int n, const uint8_t* const* d_y, const uint8_t* const* d_u, const uint8_t* const* d_v,
                              int width, int height, int y_stride, int c_stride, int c_step, int yuv_flags, uint32_t* const* d_dst);
int nq_frames_from_yuv(nq_handle* h, int n, const uint8_t* const* y, const uint8_t* const* u, const uint8_t* const* v,
                       int width, int height, int y_stride, int c_stride, int c_step, int yuv_flags, uint32_t* const* dst);
int nq_resample_frames_yuv_device(nq_handle* h, int n, const uint8_t* const* d_y, const uint8_t* const* d_u, const uint8_t* const* d_v,
                                  int src_width, int src_height, int y_stride, int c_stride, int c_step, int yuv_flags,
                                  int crop_x, int crop_y, int crop_w, int crop_h,
                                  uint32_t* const* d_dst, int dst_width, int dst_height, int flags);
int nq_resample_frames_yuv(nq_handle* h, int n, const uint8_t* const* y, const uint8_t* const* u, const uint8_t* const* v,
                           int src_width, int src_height, int y_stride, int c_stride, int c_step, int yuv_flags,
                           int crop_x, int crop_y, int crop_w, int crop_h,
                           uint32_t* const* dst, int dst_width, int dst_height, int flags);

/* ---- orientation: turn and mirror a frame sequence (ffmpeg transpose / autorotate; Android's sensorOrientation and MediaCodec's
 *      KEY_ROTATION).  A camera or a decoder writes frames in sensor orientation; these calls bring them upright on the device, as
 *      ARGB words or straight from the YUV planes, alone or together with the reducer.  Words are moved, never changed.
 *  * orientation is 1..8 with EXIF's meaning.  Source frame: W x H, pixel src(x, y).
 *        code   output   out(x, y) =             name
 *         1     W x H    src(x, y)               identity
 *         2     W x H    src(W-1-x, y)           mirror left-right
 *         3     W x H    src(W-1-x, H-1-y)       180 degrees
 *         4     W x H    src(x, H-1-y)           mirror top-bottom
 *         5     H x W    src(y, x)               transpose
 *         6     H x W    src(y, H-1-x)           90 degrees clockwise
 *         7     H x W    src(W-1-y, H-1-x)       transverse
 *         8     H x W    src(W-1-y, x)           270 degrees clockwise
 *    A clip with rotation r (clockwise, to be applied for display) takes 1, 6, 3, 8 for r = 0, 90, 180, 270; mirrored left-right
 *    afterwards 2, 5, 4, 7.
 *  * nq_orient_frames_device: n frames of src_width x src_height words, rows contiguous; output i holds the oriented frame, rows
 *    contiguous (src_height words per row for codes 5..8).
 *    nq_frames_from_yuv_oriented_device  IS  nq_frames_from_yuv_device, then nq_orient_frames_device, without the unturned ARGB frames
 *    ever existing.  The chroma sample of a pixel is that of its SOURCE coordinates.
 *    nq_resample_frames_oriented_device  IS  nq_orient_frames_device, then nq_resample_frames_device: the crop and the target are
 *    given in oriented (as displayed) coordinates.
 *    nq_resample_frames_yuv_oriented_device  IS  convert, then orient, then reduce.
 *    All three bit for bit.  The reducing calls map the crop back into the source, reduce there into handle scratch and orient the
 *    small result: the overlap weights of "frame reduction" are symmetric under the reflection of an axis, swapping the axes swaps wx
 *    and wy in a product, and the sums are integers, so orienting commutes with the reducer exactly.
 *  * The _device forms take host arrays of n DEVICE pointers and are asynchronous on the handle's stream; sources are never written
 *    and nothing outside the n outputs is written.  h may be a handle of either kind: its stream, scratch and error text are used,
 *    its params are neither read nor changed.  Pointers to words need 4-byte alignment.  nq_orient_frames_device moves 16 bytes per
 *    access when every source and output is 16-byte aligned, src_width is a multiple of 4 and, for codes 5..8, so is src_height;
 *    nq_frames_from_yuv_oriented_device when nq_frames_from_yuv_device would and, for codes 5..8, height is a multiple of 4;
 *    otherwise one word (one pixel) per access, with the same results.
 *    The forms without _device: the same with HOST buffers (upload, the device form, the n outputs copied back; the call returns
 *    when they are there).
 *  * NQ_ERR_INVALID before any device work, every buffer untouched, the handle still usable: orientation outside 1..8; every error
 *    of the calls the definition names, the crop being checked against the ORIENTED frame; an output that overlaps a source or
 *    another output (in-place use included).
 *  The kernels: DESIGN.md 5h "Orientation". ---- */
int nq_orient_frames_device(nq_handle* h, int n, const uint32_t* const* d_src, int src_width, int src_height, int orientation,
                            uint32_t* const* d_dst);
int nq_orient_frames(nq_handle* h, int n, const uint32_t* const* src, int src_width, int src_height, int orientation,
                     uint32_t* const* dst);
int nq_frames_from_yuv_oriented_device(nq_handle* h, int n, const uint8_t* const* d_y, const uint8_t* const* d_u,
                                       const uint8_t* const* d_v, int width, int height, int y_stride, int c_stride, int c_step,
                                       int yuv_flags, int orientation, uint32_t* const* d_dst);
int nq_frames_from_yuv_oriented(nq_handle* h, int n, const uint8_t* const* y, const uint8_t* const* u, const uint8_t* const* v,
                                int width, int height, int y_stride, int c_stride, int c_step, int yuv_flags, int orientation,
                                uint32_t* const* dst);
int nq_resample_frames_oriented_device(nq_handle* h, int n, const uint32_t* const* d_src, int src_width, int src_height,
                                       int orientation, int crop_x, int crop_y, int crop_w, int crop_h,
                                       uint32_t* const* d_dst, int dst_width, int dst_height, int flags);
int nq_resample_frames_oriented(nq_handle* h, int n, const uint32_t* const* src, int src_width, int src_height,
                                int orientation, int crop_x, int crop_y, int crop_w, int crop_h,
                                uint32_t* const* dst, int dst_width, int dst_height, int flags);
int nq_resample_frames_yuv_oriented_device(nq_handle* h, int n, const uint8_t* const* d_y, const uint8_t* const* d_u,
                                           const uint8_t* const* d_v, int src_width, int src_height, int y_stride, int c_stride,
                                           int c_step, int yuv_flags, int orientation,
                                           int crop_x, int crop_y, int crop_w, int crop_h,
                                           uint32_t* const* d_dst, int dst_width, int dst_height, int flags);
int nq_resample_frames_yuv_oriented(nq_handle* h, int n, const uint8_t* const* y, const uint8_t* const* u, const uint8_t* const* v,
                                    int src_width, int src_height, int y_stride, int c_stride, int c_step, int yuv_flags,
                                    int orientation, int crop_x, int crop_y, int crop_w, int crop_h,
                                    uint32_t* const* dst, int dst_width, int dst_height, int flags);

/* ---- ordered dither: a positional dither for frame sequences (ffmpeg paletteuse=dither=bayer, ImageMagick -ordered-dither).  The
 *      index of a pixel depends on its colour, its coordinates and the palette only -- not on any other pixel, as in the Gilbert-curve
 *      error diffusion of the convert calls.  An unchanged pixel gives an unchanged index in every frame, at any tile size, with no
 *      seeds, and the pattern is stationary in time.  It is the positional form of what the reference's closestColorIndex does with
 *      Random: choose between the two closest entries in proportion to where the pixel lies between them.  Opt-in: no other entry
 *      point's results change.  All arithmetic is integer.
 *  * Inputs: n ARGB_8888 frames, each with its own width and height (as for nq_convert_frames); a palette of K entries (1..256) in
 *    HOST memory, only read; limit in 0..255.
 *  * Terms as in "palette refinement": the channels of a colour are a, r, g, b (shifts 24, 16, 8, 0);
 *    d(p, c) = da^2 + dr^2 + dg^2 + db^2; a palette entry with a != 0 is LIVE; T = the first entry with a = 0, or -1 when there is none.
 *  * A pixel with a = 0 while T >= 0 gets index T and is NOT COUNTED in the statistics.  Every other pixel is COUNTED:
 *        with no live entry it gets index T (T = 0 then);
 *        otherwise, over the live entries j, key(j) = (d(p, P[j]) << 8) | j
 *            i1 = the j of the smallest key
 *            i2 = the j of the smallest key among the live j != i1 (there is none when one entry is live)
 *            d1, d2 = their distances, D = d2 - d1 >= 0
 *  * Mask: m = mask[(y & 63) * 64 + (x & 63)] + 128, in 0..255, with mask the 4096 signed bytes of include/nq_blue_noise_64x64.inc
 *    (every value -128..127 occurs exactly 16 times) and x, y the pixel's column and row in its own frame.  The same mask is used in
 *    every frame.
 *  * Choice: the pixel takes i2 iff ALL of
 *        limit > 0;  i2 exists;
 *        the largest |difference| of the four channels of P[i1] and P[i2] is <= limit;
 *        (255 - 2 m) * den > 256 * D,   den = d(P[i1], P[i2]);
 *    otherwise it takes i1.
 *  * Why that inequality: with num = (p - P[i1]).(P[i2] - P[i1]) and t = num / den, the position of p's projection on the segment
 *    from P[i1] to P[i2] (t <= 1/2, since i1 is the nearer), D = den - 2 num.  The inequality is therefore t > (2 m + 1) / 512: i2 is
 *    chosen at a share t of the positions.  A pixel beyond i1 (t <= 0) never takes i2; duplicate entries (den = 0) are never mixed;
 *    every product stays below 2^31 (|255 - 2 m| <= 255, den and D <= 260 100).
 *  * Outputs: out_index[i][p] = the entry taken; out_argb[i][p] (optional) = the palette word of that entry.
 *    out_stats (optional, HOST memory, 2 n int64 values): stats[2 i] = the counted pixels of frame i that took i2,
 *    stats[2 i + 1] = the sum over frame i's counted pixels of d(p, the entry taken).  Integer sums: deterministic.
 *  * Consequences: limit = 0 is the plain nearest entry (the assignment of "palette refinement").  Every pixel shows i1, or an entry
 *    within `limit` per channel of i1: the metric of the temporal hold's threshold and the GIF encoders' lossy mode, on purpose.
 *    Equal pixels at equal coordinates give equal indices, whatever else is in the frames.
 *  * What it does not do: a source pixel that moves by one level can still flip an index near a threshold, so noisy footage still wants
 *    the temporal hold.
 *  * nq_dither_ordered_device: the frames and outputs in DEVICE memory; d_argb, d_out_argb, d_out_index are host arrays of n device
 *    pointers.  d_out_argb may be NULL as a whole (no ARGB output), d_out_index may not.  ARGB pointers need 4-byte, index pointers
 *    2-byte alignment; when every source and ARGB output is 16-byte and every index map 8-byte aligned the kernel handles four pixels
 *    per access, otherwise one (same results).  The sources are never written and nothing outside the n * width * height elements of
 *    any output is written.  With out_stats == NULL the call is asynchronous on the handle's stream; otherwise it returns when the
 *    statistics are there.  h may be a handle of either kind: its stream, scratch and error text are used, its params are neither
 *    read nor changed.  nq_dither_ordered: the same with HOST buffers (the frames are uploaded, the device form runs, index maps and
 *    outputs are copied back).
 *  * nq_convert_frames_ordered_device / nq_convert_frames_ordered: (1) palette and params of nq_pnnquan_frames_device (out_palette
 *    has room for max(nMaxColors, 2) entries), (2) `refine` passes of nq_refine_palette_device over the same frames (0: none), (3) the
 *    call above with that palette and no statistics.  The results equal those three calls made one after another.  The call returns
 *    when the outputs are written.
 *  * NQ_ERR_INVALID before any device work, every buffer untouched, the handle still usable: n < 1, a side outside 1..65535, more
 *    than 2^31 - 1 pixels in total, K outside 1..256, limit outside 0..255, in the convert forms nMaxColors outside 1..256 or refine
 *    outside 0..64, a NULL pointer array, entry, palette (out_palette, out_K) or index array, an ARGB pointer that is not 4-byte
 *    aligned, an index pointer that is not 2-byte aligned, an output that overlaps a source frame or another output.  A NULL handle
 *    is refused the same way.
 *  The kernel: DESIGN.md 5f "Ordered dither". ---- */
int nq_dither_ordered_device(nq_handle* h, int n, const uint32_t* const* d_argb, const int32_t* widths, const int32_t* heights,
                             const uint32_t* palette, int K, int limit,
                             uint32_t* const* d_out_argb, uint16_t* const* d_out_index, int64_t* out_stats);
int nq_dither_ordered(nq_handle* h, int n, const uint32_t* const* argb, const int32_t* widths, const int32_t* heights,
                      const uint32_t* palette, int K, int limit,
                      uint32_t* const* out_argb, uint16_t* const* out_index, int64_t* out_stats);
int nq_convert_frames_ordered_device(nq_handle* h, int n, const uint32_t* const* d_argb, const int32_t* widths, const int32_t* heights,
                                     int nMaxColors, int refine, int limit,
                                     uint32_t* const* d_out_argb, uint16_t* const* d_out_index,
                                     uint32_t* out_palette, int32_t* out_K);
int nq_convert_frames_ordered(nq_handle* h, int n, const uint32_t* const* argb, const int32_t* widths, const int32_t* heights,
                              int nMaxColors, int refine, int limit,
                              uint32_t* const* out_argb, uint16_t* const* out_index,
                              uint32_t* out_palette, int32_t* out_K);

/* ---- quality measurement: what a conversion did to the picture.  n pairs of frames -- the source and the output of any of the calls
 *      above -- are compared in one streaming pass on the device: the per-pixel squared error (dither raises it), the error of the
 *      8 x 8 block means in linear light (dither is there to lower it) and SSIM on luma over the same blocks (pngquant and gifski
 *      --quality; the reference has no such step).  All arithmetic is integer: the result is deterministic and can be restated bit for bit.
 *      These calls take NO handle: they are pure functions of their arguments and keep no state, so they take the device ordinal (and
 *      the device forms a hipStream_t) directly.
 *  * Inputs: n pairs of frames; pair i is widths[i] x heights[i].  src and out are ARGB_8888 words, channels a, r, g, b at shifts 24,
 *    16, 8, 0.  flags: bit 0 is NQ_COMPARE_LINEAR; unknown bits are refused.
 *  * Per frame 16 signed 64-bit slots.  All of the following are exact integers, signed 64-bit where sums are formed.
 *  * Seen colour: a pixel with a = 0 has r = g = b = 0 for everything below.  Alpha is a channel of its own.
 *  * Per pixel: sse_c += (s_c - o_c)^2 for c = a, r, g, b; maxdiff = the largest |s_c - o_c| over pixels and channels.
 *  * Blocks: the frame is tiled with 8 x 8 blocks anchored at (0, 0); edge blocks are partial; N = the pixels of a block, 1..64.
 *  * Table T[v]: with NQ_COMPARE_LINEAR the table of include/nq_srgb_linear_16.inc (the normative copy the reducer uses); without the
 *    flag T[v] = 257 v.
 *  * Block means.  Premultiplied 16-bit values P_a = 257 a and P_c = floor((T[c] a + 127) / 255) for c = r, g, b; block sums S_c over
 *    src and S'_c over out; means m = floor((2 S + N) / (2 N)) and m' likewise; lf_c += (m - m')^2.
 *  * Luma: y = (77 r + 150 g + 29 b + 128) >> 8, y* = floor((y a + 127) / 255).  Per block over y* of src (x) and out (y): Sx, Sy, Sxx,
 *    Syy, Sxy.
 *  * SSIM per block:
 *        C1 = floor((65025 N^2 + 5000) / 10000)          C2 = floor((585225 N^2 + 5000) / 10000)
 *        A1 = 2 Sx Sy + C1                               B1 = Sx^2 + Sy^2 + C1
 *        A2 = 2 (N Sxy - Sx Sy) + C2                     B2 = N (Sxx + Syy) - Sx^2 - Sy^2 + C2
 *        l = floor(32768 A1 / B1)     cs = floor(32768 A2 / B2)     q = floor(l cs / 32768)
 *    floor rounds toward minus infinity; A2, and so cs and q, can be negative.  ssim += q; deficit = the largest 32768 - q over the
 *    blocks.
 *  * Bounds: every term A1, B1, |A2|, B2 is below 2^30 (Sx <= 64 * 255, Sxx <= 64 * 255^2), so 32768 A is below 2^45; B1, B2 >= C1 > 0;
 *    0 <= l <= 32768, |cs| <= 32768 (Cauchy-Schwarz), -32768 <= q <= 32768, 0 <= deficit <= 65536.
 *  * Slots:   0 pixels   1 blocks   2..5 sse a, r, g, b   6 maxdiff   7..10 lf a, r, g, b   11 ssim   12 deficit   13..15 0
 *    Identical frames give zeros everywhere except slots 0, 1 and 11; slot 11 is then 32768 x blocks.
 *  * Limits: a side is 1..65535, a frame holds at most 2^31 - 1 pixels, n is 1..65535.  So pixels < 2^31, blocks <= 2^26,
 *    sse <= 255^2 (2^31 - 1) < 2^47, maxdiff <= 255, lf <= 65535^2 2^26 < 2^58, |ssim| <= 2^15 2^26 = 2^41.
 *  * What the slots mean (formed by the caller, in floating point; nquant.android_amd.compare.Quality):
 *        psnr        = 10 log10(65025 * 3 * pixels / (sse_r + sse_g + sse_b)), infinite at 0
 *        lf_psnr     = 10 log10(65535^2 * 3 * blocks / (lf_r + lf_g + lf_b)), infinite at 0
 *        ssim        = slot 11 / (32768 * blocks)
 *        worst_block = 1 - deficit / 32768
 *        max_diff    = slot 6
 *    Over a sequence the slots add, slots 6 and 12 take the maximum.
 *  * Indexed form: out is a uint16_t index map plus a palette of K entries, K in 1..256, in HOST memory; the output word is
 *    palette[index].  An index >= K reads as the word 0; nq_compare_indexed then returns NQ_ERR_INVALID after the run, with every slot
 *    written (as the encoders report it).  nq_compare_indexed_device waits for nothing and so cannot report it: there such an index
 *    only reads as the word 0.
 *  * Device forms: d_src, d_out / d_index are host arrays of n DEVICE pointers, d_result 16 n slots in DEVICE memory.  The call is
 *    asynchronous on hip_stream (NULL = the default stream) of device `device`, ordered against it like a handle's calls are against
 *    the handle's stream; it allocates no device memory and waits for nothing; the pointer tables, the sides and the palette belong
 *    to the caller again on return.  Frames need 4-byte alignment, index maps 2-byte; groups of 16 consecutive pairs share a
 *    launch, and where every pointer of a group is 16-byte aligned (index maps: 8-byte) and every width a multiple of 4 the kernel reads
 *    16 bytes per access, otherwise one pixel per access, with the same results.  Frames are never written; nothing but the 16 n
 *    slots is.
 *  * Host forms: the same with HOST frames and a host result (uploaded to temporary buffers, the device form, the 16 n slots copied
 *    back); they return when the results are there, with everything freed: nq_get_device_bytes is the same before and after.
 *  * Errors: status as elsewhere; the text is the thread's handle-free one, nq_last_error(NULL).  NQ_ERR_INVALID comes first, before
 *    any device is touched, with every output untouched: n outside 1..65535, a side outside 1..65535, a frame above 2^31 - 1 pixels,
 *    unknown flag bits, K outside 1..256, a negative device, a NULL table, entry, palette or result, a frame pointer that is not
 *    4-byte aligned (2-byte for an index map), a result that is not 8-byte aligned, a result that overlaps a frame.  Then
 *    NQ_ERR_NO_DEVICE (no usable device; a device ordinal past the last one is NQ_ERR_INVALID), or NQ_ERR_HIP.
 *  The kernel: DESIGN.md 5k "Quality measurement". ---- */
#define NQ_COMPARE_LINEAR 1
int nq_compare_frames_device(int device, void* hip_stream, int n, const uint32_t* const* d_src, const uint32_t* const* d_out,
                             const int32_t* widths, const int32_t* heights, int flags, int64_t* d_result);
int nq_compare_indexed_device(int device, void* hip_stream, int n, const uint32_t* const* d_src, const uint16_t* const* d_index,
                              const uint32_t* palette, int K, const int32_t* widths, const int32_t* heights, int flags, int64_t* d_result);
int nq_compare_frames(int device, int n, const uint32_t* const* src, const uint32_t* const* out,
                      const int32_t* widths, const int32_t* heights, int flags, int64_t* result);
int nq_compare_indexed(int device, int n, const uint32_t* const* src, const uint16_t* const* index, const uint32_t* palette, int K,
                       const int32_t* widths, const int32_t* heights, int flags, int64_t* result);

/* ---- WebP encoding: n index maps of one size over one palette to ONE lossless WebP file (VP8L): a still image for n = 1, an
 *      animation whose frames store only what changed for n > 1, with all 8 bits of the palette's alpha.  All n frames are width x height
 *      uint16 index maps over the K <= 256 ARGB entries of `palette` (what nq_convert_frames returns).  The calls take no handle: a
 *      device ordinal and, in the device form, a stream, like the quality measurement above.
 *  * n = 1: `RIFF` size `WEBP`, one `VP8L` chunk, padded to even.  out_rects = {0, 0, width, height}.
 *  * n > 1: `RIFF` size `WEBP`; `VP8X` (flags 0x02 = animation, | 0x10 when any palette alpha != 255; three zero bytes; width - 1 and
 *    height - 1 as 24 bits, little-endian like every number of the container); `ANIM` (background 0, loop_count as 16 bits, 0 = for
 *    ever); n `ANMF` chunks: x / 2, y / 2, w - 1, h - 1 of the rectangle as 24 bits each, the duration 10 * delays_cs[i] ms (NULL: 0)
 *    as 24 bits, the flags byte 0x02 (do not blend, dispose none), then the rectangle's `VP8L` chunk.
 *  * Rectangle: frame 0 whole.  delta = 0: every frame whole.  delta = 1: frame i >= 1 is the bounding box of the pixels with
 *    index_i != index_(i-1), its left and top rounded DOWN to even (the container stores them halved); 1 x 1 at (0, 0) when nothing
 *    differs.  The rectangle holds frame i's own indices and replaces what was there whatever the alpha is: no mark index, no mode.
 *    It is read in place from the frame's map.  n = 1 ignores delta.
 *  * A VP8L chunk (bits go into bytes least significant first; prefix codes are canonical and go most significant bit first):
 *    byte 0x2f; 14 bits w - 1; 14 bits h - 1; 1 bit "alpha used" (any palette alpha != 255); 3 bits 0.  One transform: bit 1, type 3
 *    (colour indexing), 8 bits K - 1, the colour table as a K x 1 image (cache bit 0, five prefix codes, K pixels: each entry the
 *    per-channel difference to the entry before it mod 256, coded green, red, blue, alpha; all literals); bit 0.  Indices are
 *    bundled 8 / 4 / 2 / 1 per packed pixel at K <= 2 / <= 4 / <= 16 / more, index x in bits (x mod per) * (8 / per) of packed pixel
 *    x / per (LOW bits first); pw = ceil(w / per).  Main image: cache bit 0; with more than one band the bit 1, 3 bits p - 2 and the
 *    entropy image (cache bit 0, five codes, ceil(pw / 2^p) x ceil(h / 2^p) pixels, pixel (x, y) = group y: green y & 255, red
 *    y >> 8; per row a literal and, when wider than 1, one copy of length ew - 1 at distance 1), else the bit 0; then five prefix
 *    codes per group, group after group; then all pixels.
 *  * Bands: a band is 2^p packed rows and one chain: it sees only its own packed pixels, has its own five codes and is encoded by
 *    one wavefront.  band_bits = 0 selects the largest p in 2..9 with pw * 2^p <= 32768 (per rectangle); an explicit 2..9 must
 *    satisfy that for the whole frame.  A frame with pw * 4 > 32768 (wider than 8192 packed pixels, larger than anything this
 *    project measures) is refused.
 *  * A band's tokens are those of nq_encode_png's chains on the band's packed pixels (greedy, hash of 3, matches 3..258).  A literal
 *    is the green code of the packed pixel (red, blue and alpha are one-symbol codes: 0 bits).  A copy is green symbol 256 +
 *    prefix(length), its extra bits, the distance symbol prefix(distance + 120), its extra bits -- distance + 120 steps over the 120
 *    codes of the format's 2-D neighbourhood map.  A code with at most one used symbol is written in the simple form and costs
 *    no bits in the data; every other code in the normal form with all its lengths (runs through the symbols 16, 17, 18).  Lengths
 *    are limited to 15 by nq_encode_png's rule.
 *  * nq_webp_max_bytes: an upper bound of the file size for any content and any K (pure arithmetic, no device): 44 bytes, and per
 *    frame 33 bytes + ceil(bits / 8), bits = 30400 (header, transform, colour table) + [more than one band: 7700 + 64 per band]
 *    + 4640 per band + 15 per packed pixel, the largest over the four bundlings the geometry allows.  Derived in DESIGN.md.
 *  * out_rects (NULL: not wanted): 4 ints per frame, x, y, w, h of its rectangle, written on success.
 *  * nq_encode_webp_device: index maps in DEVICE memory of `device` (2-byte aligned pointers suffice; never written), d_index itself
 *    and everything else on the host.  The call works on hip_stream (NULL = the default stream), allocates its scratch, frees it
 *    before it returns, and returns when `out` holds the file: nq_get_device_bytes is the same before and after.
 *    nq_encode_webp: the same with index maps in HOST memory (they are uploaded first).
 *  * Errors: status as elsewhere; the text is the thread's handle-free one, nq_last_error(NULL).  NQ_ERR_INVALID before any device
 *    work (*out_size, out and out_rects stay untouched): n outside 1..65535, a side outside 1..16384, K outside 1..256, a delay or
 *    loop_count outside 0..65535, delta not 0 / 1, band_bits not 0 / 2..9 or too large for the width, a NULL or odd index pointer, a
 *    NULL table, palette or out_size, out NULL with cap > 0, cap < 0, a negative device.  Then NQ_ERR_NO_DEVICE (no usable device; a
 *    device ordinal past the last one is NQ_ERR_INVALID) or NQ_ERR_HIP.  After the encoding, NQ_ERR_INVALID: an index >= K anywhere
 *    in any frame (delta mode: also outside the rectangle), or cap smaller than the file (then *out_size holds the size and `out`
 *    is untouched).
 *  There is no Java method for this stage.  The bit-exact definition, the bound and the kernels: DESIGN.md "WebP encoder". ---- */
int nq_webp_max_bytes(int n, int width, int height, int band_bits, int64_t* out_bytes);
int nq_encode_webp_device(int device, void* hip_stream, int n, const uint16_t* const* d_index, int width, int height,
                          const uint32_t* palette, int K, const int32_t* delays_cs, int loop_count, int band_bits, int delta,
                          uint8_t* out, int64_t cap, int64_t* out_size, int32_t* out_rects);
int nq_encode_webp(int device, int n, const uint16_t* const* index, int width, int height,
                   const uint32_t* palette, int K, const int32_t* delays_cs, int loop_count, int band_bits, int delta,
                   uint8_t* out, int64_t cap, int64_t* out_size, int32_t* out_rects);

/* ---- 10-bit YUV input: 10-bit YUV 4:2:0 frames in 16-bit words (P010: what a 10-bit MediaCodec hands out as COLOR_FormatYUVP010
 *      and the camera as ImageFormat.YCBCR_P010; I010: the planar form) in front of the frame path, in SDR, PQ (SMPTE ST 2084) or HLG
 *      (BT.2100).  nq_frames_from_yuv16* converts a sequence 1:1 to ARGB_8888 words (8-bit sRGB); nq_resample_frames_yuv16* converts
 *      and reduces it in one step, without the full-size ARGB frames ever existing.  All arithmetic is integer and two committed
 *      tables: the result is deterministic and can be restated bit for bit (tests/yuv16_ref.py).  The calls take NO handle: a device
 *      ordinal and, in the device forms, a stream, as nq_compare_* do; the error text is the thread's, nq_last_error(NULL).
 *  * The frame: the geometry of "YUV input" with every stride and step counted in 16-bit SAMPLES.  width x height, both 1..65535, and
 *    three pointers to 16-bit little-endian words y, u, v.  Luma of pixel (x, y) is y[y * y_stride + x]; the chroma planes are
 *    cw2 = (width + 1) >> 1 by ch2 = (height + 1) >> 1 samples, and the chroma of pixel (x, y) is
 *    u[(y >> 1) * c_stride + (x >> 1) * c_step], likewise v (sample replication).  c_step is 1 (planar) or 2 (interleaved):
 *        P010                     u = uv, v = uv + 1     c_step 2
 *        P010, v first            v = vu, u = vu + 1     c_step 2
 *        I010 / YV12 at 10 bits   two planes             c_step 1
 *    All n frames of a call share width, height, y_stride, c_stride, c_step and the flag word.
 *  * yuv16_flags:
 *        NQ_YUV_BT709        1   the BT.709 matrix (BT.601 when no matrix bit is set)
 *        NQ_YUV_FULL_RANGE   2   full range (otherwise limited range)
 *        NQ_YUV16_BT2020     4   the BT.2020 non-constant-luminance matrix, Kr = 0.2627, Kb = 0.0593; exclusive with bit 1
 *        NQ_YUV16_MSB        8   sample = word >> 6 (P010); otherwise sample = word & 1023 (I010).  The other 6 bits are ignored.
 *        NQ_YUV16_PQ        16   PQ transfer; exclusive with HLG
 *        NQ_YUV16_HLG       32   HLG transfer; exclusive with PQ
 *    Neither transfer bit: SDR.
 *  * Step 1, every mode: R'G'B' on a 12-bit scale.  yo = 64 in limited range, 0 in full range; the chroma centre is 512.
 *    Coefficients: floor(16384 e + 1/2) of the rationals e of "YUV input" (cy = sy, crv = sc 2 (1 - Kr), cgu = sc 2 (1 - Kb) Kb / Kg,
 *    cgv = sc 2 (1 - Kr) Kr / Kg, cbu = sc 2 (1 - Kb)) with sy = 4095/876 and sc = 4095/896 in limited range, both 4095/1023 in full
 *    range:
 *                          cy      crv     cgu     cgv     cbu
 *        601 limited     76590   104982   25769   53475  132687
 *        601 full        65584    91949   22570   46836  116215
 *        709 limited     76590   117921   14027   35053  138947
 *        709 full        65584   103282   12285   30701  121698
 *        2020 limited    76590   110418   12322   42783  140879
 *        2020 full       65584    96710   10792   37472  123390
 *        R' = clamp((cy (Y - yo) + crv (V - 512) + 8192) >> 14, 0, 4095)
 *        G' = clamp((cy (Y - yo) - cgu (U - 512) - cgv (V - 512) + 8192) >> 14, 0, 4095)
 *        B' = clamp((cy (Y - yo) + cbu (U - 512) + 8192) >> 14, 0, 4095)
 *    >> is the arithmetic shift of a signed 32-bit value (a floor).  Every intermediate is below 1.6e8 in magnitude.
 *  * Step 2, SDR: channel = (c' * 255 + 2047) / 4095 (integer division).  DEVIATION: there is no gamut change, with the BT.2020
 *    matrix too -- wide-gamut SDR comes out with its primaries read as BT.709's.  Each channel is within one level of round-half-up
 *    of the exact real formula.
 *  * Step 2, PQ / HLG: through the two tables of the transfer in include/nq_hdr_luts.inc (normative; tools/make_hdr_luts.py wrote it).
 *      - E[4096], unsigned 16 bit: the 12-bit signal to linear light with 8192 = reference white.
 *          PQ   min(65535, floor(8192 * 10000 * pq_eotf(i / 4095) / 203 + 1/2)): the ST 2084 EOTF with 203 nits for white
 *               (BT.2408); it saturates near 1624 nits.
 *          HLG  floor(8192 * h(i / 4095) / h(0.75) + 1/2), h the inverse OETF of BT.2100: h(x) = x^2 / 3 for x <= 1/2, otherwise
 *               (exp((x - c) / a) + b) / 12 with a = 0.17883277, b = 0.28466892, c = 0.55991073.  System gamma 1: no OOTF.
 *      - Gamut, BT.2020 -> BT.709 at 2^12: l_c = clamp((row . (E[R'], E[G'], E[B']) + 2048) >> 12, 0, 65535) with the rows
 *          r: (6801, -2407, -298)    g: (-510, 4640, -34)    b: (-75, -412, 4583)
 *        Each row sums to 4096: grey stays grey.  Every term stays below 4.5e8 in magnitude: signed 32 bits suffice.
 *      - O[1280], unsigned 8 bit: the per-channel tone curve and the sRGB encoding behind one logarithmic index.  For l < 256
 *        idx = l; otherwise, with e = 31 - clz(l), idx = 256 + 128 (e - 8) + ((l >> (e - 7)) & 127).  The representative of an index
 *        is l itself below 256, otherwise the bucket's lower bound plus half its width, 2^(e - 8).
 *        O[idx] = floor(255 s(t(x / 8192)) + 1/2) with t(x) = min(1, x (1 + x / p^2) / (1 + x)) (extended Reinhard; p = 65535 / 8192
 *        for PQ, E_HLG[4095] / 8192 for HLG) and s the sRGB encoding function.  The bucketed O stays within 0.68 of a level of the
 *        unbucketed curve over all 65536 inputs.
 *    The matrix bit is honoured as given; PQ and HLG footage carries BT.2020 (NQ_YUV16_BT2020), and the gamut rows assume it.
 *  * The word is 0xFF << 24 | R << 16 | G << 8 | B in every mode.
 *  * nq_frames_from_yuv16_device: d_y, d_u, d_v, d_dst are host arrays of n DEVICE pointers; output i is width x height words, rows
 *    contiguous.  nq_resample_frames_yuv16_device is DEFINED as that call followed by nq_resample_frames_device with the same crop,
 *    target and flags ("frame reduction"), bit for bit; output i is dst_width x dst_height words; it needs no scratch.  The chroma of
 *    crop pixel (j, i) is the frame's sample ((crop_x + j) >> 1, (crop_y + i) >> 1).  For sideways footage reduce first and turn the
 *    small result with nq_orient_frames: exact, because orientation moves words and the reducer is symmetric ("orientation").
 *    Both calls are asynchronous on hip_stream (NULL: the default stream) of `device`; the frames of a launch travel in its arguments,
 *    16 to a launch, so the calls allocate nothing and wait for nothing.  They never write the sources and write nothing outside the n
 *    outputs.  Sample pointers need 2-byte alignment, outputs 4-byte alignment.  When width is a multiple of 4, every y pointer is
 *    8-byte aligned, y_stride is a multiple of 4 and the chroma is either interleaved (c_step 2, u and v one sample apart in the same
 *    order in every frame of a launch, the lower one 8-byte aligned and c_stride a multiple of 4) or planar with u and v 4-byte aligned
 *    and c_stride even (and, 1:1, every output is 16-byte aligned), the kernels load 8 luma bytes per access and store 16; otherwise
 *    one pixel per access, with the same results.
 *    nq_frames_from_yuv16 / nq_resample_frames_yuv16: the same with HOST buffers.  Per frame the luma span and the chroma spans are
 *    uploaded -- one span where u's and v's overlap or touch --, the device form runs, the n outputs are copied back and every
 *    temporary buffer is freed; the call returns when the outputs are there.  nq_get_device_bytes is the same before and after.
 *  * NQ_ERR_INVALID before any device is touched, every buffer untouched: n outside 1..65535, a side outside 1..65535,
 *    y_stride < width, c_step not 1 or 2, c_stride < c_step (cw2 - 1) + 1, unknown bits in either flag word, both matrix bits, both
 *    transfer bits, a negative device, a NULL pointer array or entry, a sample pointer that is not 2-byte aligned, an output pointer
 *    that is not 4-byte aligned, n width height above 2^31 - 1, the crop and target errors of nq_resample_frames, an output that
 *    overlaps a source span or another output.  Then NQ_ERR_NO_DEVICE (no usable device; a device ordinal past the last one is
 *    NQ_ERR_INVALID) or NQ_ERR_HIP.
 *  Out of scope: 12-bit samples, 4:2:2 and 4:4:4, Dolby Vision and HDR10+ metadata.  The kernels: DESIGN.md 5g2 "10-bit YUV input". ---- */
#define NQ_YUV16_BT2020 4
#define NQ_YUV16_MSB 8
#define NQ_YUV16_PQ 16
#define NQ_YUV16_HLG 32
int nq_frames_from_yuv16_device(int device, void* hip_stream, int n, const uint16_t* const* d_y, const uint16_t* const* d_u,
                                const uint16_t* const* d_v, int width, int height, int y_stride, int c_stride, int c_step,
                                int yuv16_flags, uint32_t* const* d_dst);
int nq_frames_from_yuv16(int device, int n, const uint16_t* const* y, const uint16_t* const* u, const uint16_t* const* v,
                         int width, int height, int y_stride, int c_stride, int c_step, int yuv16_flags, uint32_t* const* dst);
int nq_resample_frames_yuv16_device(int device, void* hip_stream, int n, const uint16_t* const* d_y, const uint16_t* const* d_u,
                                    const uint16_t* const* d_v, int src_width, int src_height, int y_stride, int c_stride, int c_step,
                                    int yuv16_flags, int crop_x, int crop_y, int crop_w, int crop_h,
                                    uint32_t* const* d_dst, int dst_width, int dst_height, int flags);
int nq_resample_frames_yuv16(int device, int n, const uint16_t* const* y, const uint16_t* const* u, const uint16_t* const* v,
                             int src_width, int src_height, int y_stride, int c_stride, int c_step, int yuv16_flags,
                             int crop_x, int crop_y, int crop_w, int crop_h,
                             uint32_t* const* dst, int dst_width, int dst_height, int flags);

/* ---- retiming: timestamps in, blended frames and their delays out (ffmpeg fps / framerate / tmix).  A phone records 30, 60 or 120
 *      frames per second at a variable rate; a GIF is shown at 10 to 20 on a centisecond grid.  nq_retime_plan turns the source's
 *      timestamps into output frames, each the weighted mean of a window of sources, and into the delays_cs every encoder above takes;
 *      nq_retime_frames* forms the means: exact overlap weights, linear light through the table of "frame reduction", alpha
 *      premultiplied, one rounding at the end -- that call's footprint sum with time in place of x and y.  All integers, so the result
 *      can be restated bit for bit (tests/retime_ref.py).  None of the calls takes a handle; the error text is nq_last_error(NULL).
 *  * nq_retime_plan (host arithmetic; no device): t_us holds n + 1 strictly increasing values in microseconds
 *    (MediaCodec.BufferInfo.presentationTimeUs); source frame i is on display during [t[i], t[i + 1]), t[n] is the end of the clip,
 *    D = t[n] - t[0].  period_us >= 1 is the output frame's duration, shutter_us in 1 .. min(period_us, 2^31 - 1) the part of it that
 *    gathers light.  m = max(1, floor((2 D + period) / (2 period))) output frames: every one stands for at least half a period, and
 *    (m - 1) period < D.
 *      - The window of output j is [o_j, min(o_j + shutter, t[n])) with o_j = t[0] + j period; its length W_j is >= 1.  w(j, i) is the
 *        length of its overlap with source i's interval; the intervals tile [t[0], t[n]), so the weights of one j sum to W_j exactly.
 *      - The plan is in CSR form: out_offset has m + 1 entries, the pairs of output j are offset[j] .. offset[j + 1] - 1, with
 *        out_source[k] ascending and out_weight[k] >= 1.  shutter <= period keeps the windows disjoint: pairs <= n + m - 1.
 *      - out_delays_cs[j] = R(e_(j+1)) - R(e_j) with e_j = j period for j < m, e_m = D and R(x) = floor((x + 5000) / 10000): every
 *        delay is >= 0 and within one centisecond of its interval, and they sum to R(D): no drift (15 fps gives 7, 6, 7, ...).
 *      - shutter = 1 picks the frame on display at o_j.
 *    *out_m and *out_pairs receive the counts.  With cap_m = cap_pairs = 0 and the four arrays NULL the call only counts; otherwise
 *    the arrays hold cap_m + 1, cap_pairs, cap_pairs and cap_m entries, and a cap that is too small is NQ_ERR_INVALID with the counts
 *    written.  NQ_ERR_INVALID with nothing written: n < 1, NULL t_us, out_m or out_pairs, timestamps not strictly increasing,
 *    period < 1, shutter out of range, m or D / period above 2^31 - 1, a delay above 2^31 - 1, a NULL array where it is needed.
 *  * nq_retime_frames_device takes ANY plan, not only one of nq_retime_plan's (a crossfade is a plan too): n sources and m outputs of
 *    width x height words, rows contiguous; every source[k] in 0 .. n - 1 (indices may repeat and need not be consecutive); each
 *    output has 1 .. NQ_RETIME_MAX_WINDOW pairs; weights may be 0; W_j, the sum of output j's weights, is in 1 .. 2^31 - 1.  flags:
 *    bit 0 is NQ_RETIME_LINEAR.  Per output pixel, with T the table of "frame reduction" (that of include/nq_srgb_linear_16.inc with
 *    the flag, 257 v without) and a, r, g, b the channels of the pixel in source[k]:
 *        S_a = sum of w a            S_c = sum of w a T[c]    for c = r, g, b        (S_c < 2^31 255 65535 < 2^55; unsigned 64-bit)
 *    S_a = 0 gives 0x00000000.  Otherwise A = floor((2 S_a + W_j) / (2 W_j)); per channel t = floor((2 S_c + S_a) / (2 S_a)) and the
 *    stored value is the nearest table entry, ties to the smaller, as in "frame reduction"; the word is A << 24 | r << 16 | g << 8 | b.
 *    Consequences: a window that lies in one source copies it exactly for every pixel with a > 0 (a = 0 becomes 0), in both modes; a
 *    transparent source pixel contributes nothing to the colour; opaque input gives A = 255.
 *    d_src and d_dst are host arrays of n and m DEVICE pointers; offset, source and weight are host arrays, and all five may be freed
 *    when the call returns.  The call is asynchronous on hip_stream (NULL: the default stream) of `device`: frame pointers and weights
 *    travel in the kernel arguments -- consecutive outputs are packed into a launch until one more would exceed 16 outputs or 64
 *    pairs --, so it allocates nothing and waits for nothing.  Sources are never written; nothing outside the m outputs is written.
 *    Pointers need 4-byte alignment; when every source and output pointer is 16-byte aligned the kernel moves 16 bytes per access,
 *    otherwise one pixel, with the same results.
 *    nq_retime_frames: the same with HOST buffers (every source is uploaded on a 16-byte boundary, the device form runs, the m outputs
 *    are copied back, every temporary buffer is freed; the call returns when the outputs are there).
 *  * NQ_ERR_INVALID before any device is touched, every buffer untouched: n or m outside 1..65535, a side outside 1..65535,
 *    n width height or m width height above 2^31 - 1, unknown flag bits, a negative device, a NULL array or entry, a pointer that is
 *    not 4-byte aligned, offsets that do not start at 0 or do not ascend, a window that is empty or longer than
 *    NQ_RETIME_MAX_WINDOW pairs, a source index out of range, W_j outside 1 .. 2^31 - 1, an output that overlaps a source or another
 *    output.  Then NQ_ERR_NO_DEVICE (no usable device; a device ordinal past the last one is NQ_ERR_INVALID) or NQ_ERR_HIP.
 *  Out of scope: fusing the temporal sum into the spatial reducers (a 3-D box with one rounding is a different result), motion-
 *  compensated interpolation, dropping near-duplicate frames, windows over more than 64 frames.  The kernel: DESIGN.md 5e2 "Retiming". ---- */
#define NQ_RETIME_LINEAR 1
#define NQ_RETIME_MAX_WINDOW 64
int nq_retime_plan(int n, const int64_t* t_us, int64_t period_us, int64_t shutter_us, int32_t cap_m, int32_t cap_pairs,
                   int32_t* out_m, int32_t* out_pairs, int32_t* out_offset, int32_t* out_source, uint32_t* out_weight,
                   int32_t* out_delays_cs);
int nq_retime_frames_device(int device, void* hip_stream, int n, const uint32_t* const* d_src, int width, int height,
                            int m, const int32_t* offset, const int32_t* source, const uint32_t* weight,
                            uint32_t* const* d_dst, int flags);
int nq_retime_frames(int device, int n, const uint32_t* const* src, int width, int height,
                     int m, const int32_t* offset, const int32_t* source, const uint32_t* weight,
                     uint32_t* const* dst, int flags);

/* ---- Integer[] pnnquan(int[] pixels, int nMaxColors) incl. the alpha pre-scan of convert()
 *      (NQ/PnnQuantizer.java:410-436,134-267; NQ/PnnLABQuantizer.java:131-327) ---- */
int nq_pnnquan(nq_handle* h, const uint32_t* argb, int width, int height, int nMaxColors,
               uint32_t* out_palette, int32_t* out_K);
int nq_pnnquan_device(nq_handle* h, const uint32_t* d_argb, int width, int height, int nMaxColors,
                      uint32_t* out_palette, int32_t* out_K);

/* ---- int[] dither(cPixels, palette, width, height, dither) of the quantizer object
 *      (RGB NQ/PnnQuantizer.java:393-407, LAB NQ/PnnLABQuantizer.java:493-522): GilbertCurve.dither
 *      (NQ/GilbertCurve.java:367-373) followed, for !dither && K>32, by BlueNoise.dither
 *      (NQ/BlueNoise.java:207-222).  Uses the handle's params (from nq_pnnquan or nq_set_params). ---- */
int nq_dither(nq_handle* h, const uint32_t* argb, int width, int height, const uint32_t* palette, int K,
              int dither, int64_t rng_seed, int mode, uint32_t* out_argb, uint16_t* out_index);
int nq_dither_device(nq_handle* h, const uint32_t* d_argb, int width, int height, const uint32_t* palette, int K,
                     int dither, int64_t rng_seed, int mode, uint32_t* d_out_argb, uint16_t* d_out_index);

/* ---- Ditherable.nearestColorIndex on a cache miss (NQ/Ditherable.java:3-7;
 *      RGB NQ/PnnQuantizer.java:269-311, LAB NQ/PnnLABQuantizer.java:330-404): pure per colour. ---- */
int nq_nearest_index(nq_handle* h, const uint32_t* palette, int K, const uint32_t* colors, int64_t M,
                     int16_t* out_index);
/* ---- the closest[4] = {idx1, idx2, (int)err1, (int)err2} tuple of closestColorIndex
 *      (RGB NQ/PnnQuantizer.java:320-363, LAB NQ/PnnLABQuantizer.java:413-464); {-1,-1,-1,-1} where the
 *      reference returns through nearestColorIndex first (alpha <= alphaThreshold). ---- */
int nq_closest_tuple(nq_handle* h, const uint32_t* palette, int K, const uint32_t* colors, int64_t M,
                     int32_t* out_closest4);

/* ---- split pipeline for an image tiled over several GPUs: each rank scans its band, the
 *      caller reduces the partial histograms between ranks (RCCL via torch.distributed), every rank then
 *      builds the same palette and dithers its own band.  Buffers are device memory. ---- */
/* pass 1 over a band: alpha pre-scan partials.  d_scan3 = int64[3]: {max global index of an alpha==0 pixel or -1,
 * its colour, count of pixels with 0xF < alpha < 0xE0}; index_offset = global index of the band's first pixel.
 * Reduce across ranks: [0] max (carry [1] of the winner), [2] sum; then nq_set_scan(). */
int nq_band_scan_device(nq_handle* h, const uint32_t* d_argb, int64_t n_pixels, int64_t index_offset,
                        int nMaxColors, int64_t* d_scan3);
int nq_set_scan(nq_handle* h, int nMaxColors, int64_t transparent_index, uint32_t transparent_color,
                int64_t semi_count);
/* pass 2 over a band: partial histogram, NQ_HIST_STRIDE doubles per bin x 65536 bins:
 * {count, sum0, sum1, sum2, sum3} (RGB: a,r,g,b integer sums; LAB: float32 running sums of alpha,L,A,B of
 * the band in pixel order, widened). */
#define NQ_HIST_BINS 65536
#define NQ_HIST_STRIDE 5
int nq_band_histogram_device(nq_handle* h, const uint32_t* d_argb, int64_t n_pixels, double* d_hist);
/* palette from per-band histograms laid out [n_bands][65536][5] (already gathered on this rank); band partials
 * are added in band order (float32 for LAB, exactly as a sequential pass over band-ordered partial sums). */
int nq_palette_from_histograms_device(nq_handle* h, const double* d_hists, int n_bands, int nMaxColors,
                                      uint32_t* out_palette, int32_t* out_K);

/* few-colours early return of the LAB class (NQ/PnnLABQuantizer.java:193-206) in the split pipeline: when the gathered histograms
 * hold <= nMaxColors occupied bins, every rank lists the distinct colours of its band as the histogram sees them (alpha <= 15 ->
 * transparent colour; needs nq_set_scan first) in first-occurrence order -- *out_count = how many there are, out_colors filled
 * when *out_count <= cap -- the caller concatenates the lists in band order, drops repeats, and hands the image-wide list to
 * every rank with nq_set_distinct (count < 0 = "more than nMaxColors": no early return).  nq_palette_from_histograms_device then takes the
 * same early return as a single GPU would. */
int nq_band_distinct_device(nq_handle* h, const uint32_t* d_argb, int64_t n_pixels, int cap, int64_t* out_count,
                            uint32_t* out_colors);
/* The list belongs to the image of the last nq_set_scan: nq_set_scan forgets it, so every image's round hands over its own (or, with
 * <= nMaxColors occupied bins and none handed over, ends with NQ_ERR_UNSUPPORTED). */
int nq_set_distinct(nq_handle* h, int64_t count, const uint32_t* colors);

/* Image-wide distinct-colour count of a banded LAB run (it sets the BlueNoise weight of convert(n, false),
 * NQ/PnnLABQuantizer.java:511-515, and lives in nq_params.distinctColors): every rank marks the opaque colours of its band in
 * d_presence (2^24 bytes, one per RGB value; the caller zeroes it once and may pass the same table for several bands) and gets
 * the band's non-opaque colours (after the alpha <= 15 substitution; needs nq_set_scan first) as a list -- *out_other_count = -1
 * when there are more than cap_other (<= 131072).  The caller combines the tables by byte-wise MAX (an all-reduce), counts their
 * non-zero bytes, adds the size of the union of the lists and stores the sum with nq_set_params. */
int nq_band_color_presence_device(nq_handle* h, const uint32_t* d_argb, int64_t n_pixels, uint8_t* d_presence, int cap_other,
                                  int64_t* out_other_count, uint32_t* out_other);

/* Wall-clock of the stages of the last nq_convert*_ call on this handle, milliseconds, measured with HIP
 * events on the handle's stream: {prescan, histogram, nn_init, merge, palette_fill, dither, bluenoise, total}.
 * Batch entry points: an event record costs the GPU ~3 us of queue time, so only the first SIXTEEN handles of a batch record all
 * eight boundaries; for the others {prescan, histogram, nn_init, merge, palette_fill, bluenoise} are reported as -1 (not recorded),
 * `dither` is the per-pixel pass as for every handle, and `total` spans from the start of the image's pre-scan to the END OF THE
 * DITHER PASS -- it leaves out the BlueNoise post-pass of convert(n, false).  nq_get_batch_phase_ms gives the amortised phases.
 * `dither` in a batch call whose dither passes take the split form (NQ_OPT_DITHER_CHAIN): the span ends behind the LIGHT kernel on the
 * launch stream; the image's chain pass and hand-back pass run on a side stream beside the next image and are not inside it (their
 * time shows in the finish phase of nq_get_batch_phase_ms, which waits for them).  Everywhere else it is the whole per-pixel pass.
 * `palette_fill` in nq_convert_batch_device with the finish phase's prep stream (NQ_FINISH_PREP): the image's candidate lists, Lab table
 * and saliency map are built on that stream beside the light kernels of the images in front of it, and the boundary between
 * `palette_fill` and `dither` is recorded on the launch stream behind its wait for them -- `palette_fill` then holds only what the launch
 * stream still waited of the list build, and `dither` stays the light kernel alone (slower there than by itself: it shares the GPU). */
#define NQ_N_STAGES 8
int nq_get_stage_ms(const nq_handle* h, float* out8);
/* Counters of the last merge loop (diagnostics), 16 values: {find_nn calls, merges, 100 MHz ticks inside find_nn, ticks in
 * the sequential heap/merge section, live-list rebuilds, find_nn list overflows, candidates evaluated exactly, ticks in
 * the bound pass, ticks in the exact pass, ticks in the replay, 64-candidate chunks visited, chunks that ran the level-1
 * bound, chunks that ran the tight bound, chunks that listed a candidate, aborted flag, ticks of the seed round inside the bound pass}. */
int nq_get_merge_stats(const nq_handle* h, int64_t* out16);
/* Counters of the last merge loop's TEAM (csrc/nq_merge.inc: a merge loop that has CUs to spare -- a single image, a batch of up to 128 -- runs as a master
 * workgroup plus 1 - 7 helper workgroups that evaluate find_nn speculatively for the bins that will surface next), 16 values:
 * {work records published, helper results used in place of an own find_nn, waits for a result that timed out, 100 MHz ticks spent
 * waiting, helpers per loop, 1 if the loop was still speculating at its end, bin-info cache hits for the heap top, results used that were
 * computed for a merge before it happened ("virtual merge"), then the control thread's 100 MHz ticks in heap sifts / in merges / fetching the heap top's bin, the deleted nodes
 * popped, ticks in the find_nn epilogues, ticks spent choosing work records, results a helper declined (RGB), times the loop gave up
 * on its helpers for a while}.  Diagnostics. */
int nq_get_team_stats(const nq_handle* h, int64_t* out16);
/* Which merge kernel the last merge launch ran for THIS handle's job (a host-side record, no device traffic): *out_threads = the
 * workgroup-size code as NQ_MERGE_THREADS spells it -- 512, 256, 128, or 127 for the dense 128-thread variant (csrc/nq_kernels.hip:
 * chosen from the number of merge jobs of the whole call) --, *out_helpers = helper workgroups per loop of the handle's kind in that
 * launch (0 unless 512 threads).  Both are 0 when the handle's last palette needed no merge loop (few colours, nMaxColors <= 2) or
 * none has run yet.  Diagnostics. */
int nq_get_merge_variant(const nq_handle* h, int32_t* out_threads, int32_t* out_helpers);
/* Phases of the last nq_convert_batch[_device] call, as seen by its FIRST handle: HIP-event spans on the launch stream, ms:
 * {every image's pre-scan + histogram + initial find_nn pass, the merge launch (all merge loops side by side + palette fill),
 *  every image's palette read-back + candidate lists + dither pass, whole call}.  Divided by the batch size these are the
 * amortised per-image times (the per-handle stage times of nq_get_stage_ms are event spans that include queueing behind the
 * other images of the batch). */
int nq_get_batch_phase_ms(const nq_handle* h0, float* out4);
/* Bytes of device memory the library holds in THIS PROCESS, over all handles: every grow-only workspace buffer, the curve tables
 * and the batch rings, counted where they are allocated and freed (a host-side counter, no device traffic; hipMalloc's own rounding
 * is not included).  A handle's buffers only grow, so the count is constant once every call of a workload has run once; nq_destroy
 * gives back everything nq_create and the handle's calls took.  Curve tables: shapes up to 32 x 32 are kept for the handle's life,
 * of the larger ones (the whole image of REFERENCE_SEQUENTIAL) at most four, the most recent one per shape slot of a dither pass
 * (tile, right column, bottom row, corner; csrc/nq_abi.cpp: get_path).
 * (tests/test_gpu_handle_lifecycle.py, part D.)  Diagnostics. */
int nq_get_device_bytes(int64_t* out);

#ifdef __cplusplus
}
#endif
#endif /* NQUANT_ABI_H */
