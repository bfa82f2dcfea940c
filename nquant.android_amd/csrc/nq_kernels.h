// nq_kernels.h -- host-callable launchers of the gfx950 kernels (defined in nq_kernels.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace nq {

// scalars of the quantizer object that the per-pixel code needs
struct DevParams {
    int kind;              // 0 RGB, 1 LAB
    int K;                 // palette.length
    int hasSemi;           // hasSemiTransparency
    int hasAlpha;          // m_transparentPixelIndex > -1
    int transparentColor;  // m_transparentColor
    int isNano;            // NQ/PnnLABQuantizer.java:180
    int binKeyed;          // nearest cache keyed by histogram bin (LAB: isNano; RGB: !(weight > .015))
    int nMaxColors;
    int rewriteA0;         // nMaxColors <= 2: pixels with alpha == 0 read as m_transparentColor (NQ/PnnQuantizer.java:424)
    int pad;
    double PR, PG, PB, PA, ratio, weight;   // weight signed
};

// scalars the GilbertCurve constructor derives (NQ/GilbertCurve.java:50-112) + initWeights tables (:336-354),
// evaluated once on the host (control plane) and handed to the kernel by value
struct GilbertConsts {
    int margin, thresold, DITHER_MAX, ditherMax, sortedByYDiff, hasAlphaW, dither;
    int hasSaliencies;      // saliencies != null
    int salSubst;           // saliency computed from the alpha-substituted pixel (pnnquan path, nMaxColors < 128)
    float beta;
    double weightAbs;       // the field `weight` (abs value, :61)
    float weights[25];      // initWeights(DITHER_MAX) (non-sorted mode)
    float w1[1], w3[3], w7[7], w15[15]; // initWeights(1|3|7|15) (sorted mode growth 1 -> 3 -> 7 -> 15 -> 31)
};

struct TileGeom {
    int width, height;
    int tile_w, tile_h, tiles_x, tiles_y;
    // visiting order of each tile shape: 0 interior, 1 right edge, 2 bottom edge, 3 corner; entries (dx | dy << 16)
    const uint32_t* path[4];
    int path_len[4];
    int shape_w[4], shape_h[4];
    // a row band of a larger image (one image tiled over GPUs): the band starts at image row y_origin (a multiple of
    // tile_h) and its first tile is tile number tile_base of the whole image.  Pixel buffers are band-local; the tile's random
    // stream, the blue-noise phase (x, y), the `bidx & 4095` gates and the pixel position handed to the lookups are those of the
    // whole image, so that the bands of an image equal the same rows of the single-GPU result.  0 / 0 for a whole image.
    int y_origin, tile_base;
};

void upload_tables(const double gamma[256], double exp1_5, double exp1_75, hipStream_t s);        // nq_kernels.hip's copy
void upload_tables_fast(const double gamma[256], double exp1_5, double exp1_75, hipStream_t s);   // nq_dither_fast.hip's copy

// candidate lists per 5-6-5 colour cell (nq_lists.inc); null pointers = full palette scans
struct ListsView {
    const unsigned char* closest; const unsigned char* closestCount;
    const unsigned char* nearest; const unsigned char* nearestCount;
};
// wA..wB: total weight of da^2, dr^2, dg^2, db^2 in closestColorIndex's err; nearest: also build the nearestColorIndex lists
void launch_cell_lab_box(float* d_box /* [65536][6] */, hipStream_t s);
// a saliency map to build beside the LAB candidate lists (the three passes are independent; one launch, nq_dither.inc build_lab_lists_kernel)
struct SalJob { const int* pixels; long long N; float* out; long long vec4; int salSubst; int blocks; };
// d_sal_pixels != null: the saliency map of these N pixels is wanted too -- returns true when it went into the same launch (LAB with
// nearest lists), false when the caller has to launch_saliency itself.
// d_packed / d_failed (nullable): the LAB launch also writes the packed records of launch_pack_lists (both lists must be in use) and
// zeroes d_failed[0], the hand-back count of launch_gilbert_fast; *folded says whether it did -- false: the caller launches
// launch_pack_lists itself and launch_gilbert_fast clears the count.  With d_packed the LAB launch also leaves the palette's Lab behind the
// packed records (NQ_LAB_TABLE_BYTES at d_packed + NQ_PACKED_BYTES: 256 x {L, A, B, 0} of RGB2LAB, zero from entry K on) for
// launch_gilbert_fast's d_lab, so the table lives and travels with the records of its palette
constexpr size_t NQ_PACKED_BYTES = (size_t) 65536 * 64, NQ_LAB_TABLE_BYTES = 256 * 16;
bool launch_build_lists(const DevParams& P, const int* d_palette, double wA, double wR, double wG, double wB, bool nearest,
                        const float* d_box, unsigned char* d_closest, unsigned char* d_closestCount, unsigned char* d_nearest,
                        unsigned char* d_nearestCount, hipStream_t s, const int* d_sal_pixels = nullptr, int64_t N = 0, float* d_sal_out = nullptr,
                        int salSubst = 0, void* d_packed = nullptr, int* d_failed = nullptr, bool* folded = nullptr);
void launch_saliency(const DevParams& P, int salSubst, const int* d_pixels, int64_t N, float* d_out, hipStream_t s);

void launch_nearest_index(const DevParams& P, const int* d_palette, const ListsView& lv, const int* d_colors, int64_t M, short* d_out, hipStream_t s);
void launch_closest_tuple(const DevParams& P, const int* d_palette, const ListsView& lv, const int* d_colors, int64_t M, int* d_out4, hipStream_t s);
// LOOKUP_ONLY: index (+ARGB) of nearestColorIndex(pixel) for every pixel
void launch_lookup_only(const DevParams& P, const int* d_palette, const ListsView& lv, const int* d_pixels, int64_t N,
                        unsigned short* d_index, int* d_argb, hipStream_t s);

// GilbertCurve.dither over every tile; writes indices (always) and ARGB (when d_argb != nullptr)
void launch_gilbert(const DevParams& P, const GilbertConsts& G, const TileGeom& T, const ListsView& lv, const int* d_pixels,
                    const float* d_saliency, const int* d_palette, short* d_binCache, long long seed, int sequential,
                    long long* d_rng_state, unsigned short* d_index, int* d_argb,
                    // REFERENCE_SEQUENTIAL + LAB only (else null): log of the colours / palette entries getLab() sees during the pass
                    int* d_log, int* d_log_count, unsigned char* d_seen, int log_cap,
                    // nullable: {count, tile indices...} -- walk only these tiles (the ones gilbert_fast_kernel handed back)
                    const int* d_tile_list, hipStream_t s);
// nq_dither_fast.hip: the specialised kernel for 32 < K <= 256, no semi-transparency, DITHER_MAX 25, tiled: PnnLABQuantizer, and
// PnnQuantizer with dither = true on images without transparency
bool gilbert_fast_eligible(const DevParams& P, const GilbertConsts& G, const TileGeom& T, const ListsView& lv);
// chain_mode: how the launches that can do without the error chain in most steps (gilbert_fast_split_eligible) run
enum { FAST_CHAIN_FUSED = 0,      // one kernel: a wavefront walks without the chain and starts over with it when a lane needs it
       FAST_CHAIN_ALWAYS = 1,     // NQ_OPT_DITHER_CHAIN = 1: no light walk, every step runs the error chain
       FAST_CHAIN_SPLIT = 2,      // gilbert_light_kernel (87 registers, four or more wavefronts per SIMD; per-tile need list), then the full walk over the listed tiles
       FAST_CHAIN_PIXEL = 3 };    // the split form with gilbert_pixel_kernel (one lane per pixel, the draws by jump-ahead) as its light pass where the tile
                                  // size allows (gilbert_pixel_eligible), with gilbert_light_kernel elsewhere
bool gilbert_fast_split_eligible(const DevParams& P, const GilbertConsts& G);
bool gilbert_pixel_eligible(const TileGeom& T);       // power-of-two tiles of 16, 32 or 64 pixels
// d_failed points at word 1 of an int[2 + 2 * tiles] block: d_failed[-1] = the need count of the split form, d_failed[0] = the hand-back
// count, d_failed[1 .. tiles] the tiles handed back, d_failed[1 + tiles ..] the need list.  chain_stream (split form only, nullable): the chain
// pass goes onto that stream behind chain_gate, recorded on s after the light kernel; the caller orders what follows (the generic kernel over
// the hand-back list must run behind the chain pass).  d_lab (nullable): the Lab table a folded launch_build_lists wrote for this palette;
// without it the pixel-form light pass converts the palette in every workgroup
hipError_t launch_gilbert_fast(const DevParams& P, const GilbertConsts& G, const TileGeom& T, const ListsView& lv, const int* d_pixels,
                               const float* d_saliency, const int* d_palette, long long seed, unsigned short* d_index, int* d_argb,
                               int* d_failed, void* d_packed /* 65536 x 64 bytes */, hipStream_t s,
                               bool failed_cleared = false /* d_failed[-1..0] were zeroed by the launch_build_lists in front of this call */,
                               int chain_mode = FAST_CHAIN_FUSED, hipStream_t chain_stream = nullptr, hipEvent_t chain_gate = nullptr,
                               const void* d_lab = nullptr);
bool fast_lookup_eligible(const DevParams& P, const ListsView& lv);
bool fast_pack_wanted(const DevParams& P, const ListsView& lv);     // the packed records are needed (LAB lookups, or the RGB dither kernel)
// packs the two lists of every colour cell into the 32-byte records (+ continuations) the specialised kernels read; must follow
// launch_build_lists on the same stream whenever fast_lookup_eligible() holds
void launch_pack_lists(const ListsView& lv, void* d_packed, hipStream_t s);
void launch_fast_nearest_index(const DevParams& P, const ListsView& lv, const int* d_palette, void* d_packed, const int* d_colors, int64_t M,
                               short* d_out, hipStream_t s);
void launch_fast_closest_tuple(const DevParams& P, const ListsView& lv, const int* d_palette, void* d_packed, const int* d_colors, int64_t M,
                               int* d_out4, hipStream_t s);
// d_todo: unsigned[N + 1] scratch (the pixels the float32 pass leaves to the exact pass)
void launch_fast_lookup_only(const DevParams& P, const ListsView& lv, const int* d_palette, void* d_packed, const int* d_pixels, int64_t N,
                             unsigned short* d_index, int* d_argb, unsigned* d_todo, hipStream_t s);
void launch_fast_bluenoise(const DevParams& P, const ListsView& lv, const int* d_palette, void* d_packed, const int* d_pixels, int width, int height,
                           int y_origin, float weight, long long seed, unsigned short* d_index, int* d_argb, hipStream_t s);
// nq_selftest_fast (include/nquant_abi.h): mode `which` (NQ_FAST_ST_*) of the dither kernel's filters over the range
// [first, first + n) or over n explicit records at d_in; a0 / a1: the mode's own arguments; d_palette: P.K entries (null when P.K == 0)
void launch_fast_selftest(const DevParams& P, const int* d_palette, int which, const void* d_in, int64_t first, int64_t n, int64_t a0, int64_t a1,
                          unsigned* d_out, hipStream_t s);
// BlueNoise.dither post-pass (NQ/BlueNoise.java:207-222); in-place on d_index, writes d_argb
void launch_bluenoise(const DevParams& P, const int* d_palette, const ListsView& lv, const int* d_pixels, int width, int height,
                      int y_origin /* band start row in the whole image, 0 otherwise */,
                      float weight, long long seed, int sequential, short* d_binCache, long long* d_rng_state,
                      unsigned short* d_index, int* d_argb, hipStream_t s);

// ---- palette build (nq_palette.inc) ----
struct Bins {
    float* f[4];
    double* d[4];
    float* cnt;
    float* err;
    int* nn;
    int* tm;
    int* mtm;
};
struct HistParams { int hasSemi, hasTransp, transparentColor, rewriteTransparent; };
struct NNParams {
    int kind, hasSemi, texicab;
    double ratio, PR, PG, PB, PA;
    int pgLessThanCoeff;
    double rgbTheta;            // RGB scans: assumed cap of the running error = rgbTheta x error after the seed blocks (>= 1; checked, see nq_merge.inc)
};
struct SortWorkspace {
    unsigned short *keys_a, *keys_b; // (unused since the histogram sorts packed {bin, rest-of-pixel} words; may be null)
    int *vals_a, *vals_b;            // [n] each: the packed words before / after the sort
    void* tmp; size_t tmp_bytes;
    unsigned *seg_start, *seg_end;   // [65536] each, contiguous (seg_end = seg_start + 65536), followed by the occupied-bin counter (seg_end[65536])
                                     // and, 64 words further, the list of the occupied bins [65536] and that of the fat bins [1024]
};
size_t sort_temp_bytes(int64_t n);
size_t sort32_temp_bytes(int64_t n, bool pairs);
// (d_pixels == nullptr: keys_a / idx_a already hold the substituted colours and indices, launch_frames_pass FRAMES_SUBST)
void launch_distinct(const int* d_pixels, int64_t n, int transparentColor, unsigned* keys_a, unsigned* keys_b, unsigned* idx_a,
                     unsigned* idx_b, void* tmp, size_t tmp_bytes, unsigned long long* d_out, void* d_heads, unsigned cap, hipStream_t s);
// colours present in a band: opaque ones mark d_bytes[rgb] (2^24 bytes, NOT cleared here: bands accumulate), the others enter the set
void launch_color_presence(const int* d_pixels, int64_t n, int transparentColor, unsigned char* d_bytes, unsigned* d_set, unsigned slots,
                           unsigned* d_counters, hipStream_t s);
void launch_ciede_selftest(const float* d_pairs /* n x 6 */, int64_t n, unsigned* d_out /* n x 9 */, hipStream_t s);
void launch_prescan(const int* d_pixels, int64_t n, int64_t index_offset, long long* d_scan3, hipStream_t s);
// pre-scan + the histogram's packed sort words (5-6-5 keys, default transparent colour) in one read of the image; false: not
// applicable (n not a multiple of 4 / unaligned buffers) and nothing was launched.  The words are valid only if the scan then
// reports no alpha == 0 pixel and no semi-transparency and nMaxColors >= 64 (launch_histogram(..., words_ready = true)).
// d_occ_count (nullable): the occupied-bin counters of the SortWorkspace this image's launch_histogram will use (seg_end + 65536), cleared
// by the same kernel -- launch_histogram(..., words_ready = true, occ_cleared = true) then issues no fill for them
bool launch_front(const int* d_pixels, int64_t n, long long* d_scan3, int* d_words /* SortWorkspace::vals_a */, int defaultTransparent,
                  unsigned* d_occ_count, hipStream_t s);
// ---- the same passes over a sequence of frames read in place (nq_palette.inc frames_kernel): frame f's pixel i has the global index
// offset + i; the work list holds (frame, chunk) items of at most NQ_FRAME_CHUNK pixels, none crossing a frame boundary ----
struct FrameDesc { const int* pixels; long long n; long long offset; };
struct FrameChunk { int frame; int count; long long begin; };     // pixels [begin, begin + count) of frame `frame`
#define NQ_FRAME_CHUNK 16384
enum { FRAMES_SCAN = 0, FRAMES_FRONT = 1, FRAMES_KEYS = 2, FRAMES_SUBST = 3 };
// FRAMES_SCAN: launch_prescan's result in d_scan3 (global indices); FRAMES_FRONT: the same + launch_front's speculative words in d_words
// (color = the default transparent colour); FRAMES_KEYS: bin_keys_kernel's words (color = m_transparentColor, keyfmt as launch_histogram's);
// FRAMES_SUBST: subst_colors_kernel's keys in d_words and global indices in d_idx (nullable)
void launch_frames_pass(int op, const FrameDesc* d_frames, int n_frames, const FrameChunk* d_items, int n_items, long long* d_scan3,
                        unsigned* d_words, unsigned* d_idx, int color, int keyfmt, hipStream_t s);
void launch_histogram(int kind, const int* d_pixels, int64_t n, const HistParams& hp, const SortWorkspace& ws,
                      double* d_hist, hipStream_t s, bool words_ready = false, bool occ_cleared = false);
// d_blockcnt: int[64] scratch (occupied bins per 1024-bin slice)
void launch_compact(int kind, const double* d_hists, int n_bands, const Bins& B, int* d_maxbins, int* d_blockcnt, hipStream_t s);
void launch_quanfn(float* d_cnt, int maxbins, int fn, hipStream_t s);
// d_box: float[1024 * 8] scratch (LAB: bounding boxes of the blocks of 64 consecutive bins)
// d_init_cand: int[65536 * 128 * 2 + 65536] scratch of the LAB kind (candidate lists between the bound and the exact kernel); may be null for RGB
void launch_find_nn_init(const NNParams& np, const Bins& B, int maxbins, float* d_box, int* d_init_cand, hipStream_t s);
// One merge loop (P9).  heap: int[2*(65536+2)] (ids, then float keys); live3: int[3*65536] (two live lists + position index);
// scan_f: float[2*10*65536 + 256] (LAB uses 2 x 6 x 65536, RGB 2 x 10 x 65536; a scan may read 63 records past the live list), scan_i: int[2*65536] (LAB scan arrays, two generations); stats: long long[16] (see merge_kernel)
struct MergeJob {
    NNParams np;
    Bins B;
    int maxbins, extbins;
    int* heap; int* live3; float* scan_f; int* scan_i;
    float* scan_box;            // float[1024 * 8]: bounding boxes of the 64-position blocks of the LAB scan arrays
    long long* stats;
    int plen; int* palette; int* status;   // P10 runs at the end of the merge workgroup: palette[plen], status |= 1 where Java throws
    // merge teams (launch_merge decides): 256 u64 of zeroed device memory per job for the work records / results of the helpers
    unsigned long long* team; int helpers;
    long long wall_ticks;       // watchdog: the loop stops (stats[14] = 2) after this many 100 MHz ticks of residency
};
// d_jobs: n jobs of one kind in device memory, one workgroup per job.  n_in_flight = merge loops expected to run at the same
// time on the device (the whole batch), n_cus = compute units of the handle's device (hipDeviceAttributeMultiprocessorCount: 256 on an
// unpartitioned MI355X): <= n_cus -> 512-thread workgroups, one per CU; <= 2 n_cus -> 256 threads, two per CU; more -> 128 threads, four
// per CU.  helpers > 0 (either kind, 512-thread variant only; every job's `team` area zeroed and `helpers` set to
// the same number): the grid holds 1 + helpers workgroups per job (merge teams, nq_merge.inc).  Returns the first HIP error of the
// attribute call / launch.  out_variant (nullable; untouched when n <= 0): {the workgroup-size code as NQ_MERGE_THREADS spells it -- 512, 256,
// 128, or 127 for the dense variant --, helper workgroups per job} of the kernel that was launched.
hipError_t launch_merge(int kind, const MergeJob* d_jobs, int n, int n_in_flight, int n_cus, int helpers, hipStream_t s, int* out_variant = nullptr);
// after launch_merge on the same stream, one workgroup per job: slot j of d_out (slot_words 64-bit words each, >= 37 + (plen + 1) / 2)
// receives the 37 words behind job j's `stats` ([36] = its status word) and, from word 37 on, its palette[plen]
void launch_merge_readback(const MergeJob* d_jobs, int n, long long* d_out, long long slot_words, hipStream_t s);
// helpers launch_merge would use for n jobs of one kind when n_in_flight loops share a device of n_cus compute units (0..7;
// NQ_MERGE_HELPERS overrides).  Sized on THIS call's jobs: merge launches of other handles / threads on the same device are not
// counted -- correctness does not depend on it (every wait of a team is bounded, nq_merge.inc), only the speed-up does.
int merge_team_helpers(int n_jobs, int n_in_flight, int n_cus);
// first error of a hipFuncSetAttribute issued by a launch_* function on this thread since the last call (hipSuccess: none); cleared
hipError_t take_launch_error();

// ---- GIF encoding (nq_gif.hip): frame f's indices are cut into segments of seg_len pixels (the last one shorter), segment s of the
// frame is chain seg_base + s of the call and writes its bit string to words[word_base + s * seg_words ...] (seg_words: the worst case
// of one segment + 1); file_off .. stream_len place the frame in the file (filled in after the bit lengths are known) ----
struct GifFrame {
    const unsigned short* index;   // 2-byte aligned
    long long npix, seg_base, nseg, word_base, seg_words;
    int seg_len, prefix_len;       // prefix: the bytes in front of the frame's sub-blocks (file header for frame 0, extension, descriptor, m)
    long long file_off, prefix_off, data_bytes, stream_len;     // stream: the sub-blocks and their terminator
};
// seg_bits[g]: bit length of chain g; *d_bad = 1 when an index >= K was met (zeroed by the caller)
// lossy > 0 ("GIF encoding, lossy mode"): d_rgb = the file's colour table, 256 entries 0x00RRGGBB (zeros from entry K on), T = its
// transparent index or -1; lossy == 0 runs the lossless chains and reads neither
void launch_gif_lzw(const GifFrame* d_frames, int n_frames, long long n_segs, int K, int m, unsigned* d_words, unsigned long long* d_seg_bits,
                    unsigned long long* d_bad, const unsigned* d_rgb, int T, int lossy, hipStream_t s);
void launch_gif_scan(const GifFrame* d_frames, int n_frames, const unsigned long long* d_seg_bits, unsigned long long* d_seg_off,
                     unsigned long long* d_frame_bits, hipStream_t s);
// the whole file (total bytes): frame prefixes from d_blob, sub-block stream of every frame, trailer
void launch_gif_gather(const GifFrame* d_frames, int n_frames, const unsigned* d_words, const unsigned long long* d_seg_bits,
                       const unsigned long long* d_seg_off, const unsigned char* d_blob, unsigned char* d_file, long long total, hipStream_t s);

// ---- GIF delta mode (nq_gif.hip): n frames of one size W x H.  Frame f >= 1 is compared with frame f - 1; its body is the changed
// pixels' bounding rectangle, row-major, with the unchanged pixels replaced by the index u (u < 0: kept) ----
struct GifDelta {
    const unsigned short* cur;     // frame f and frame f - 1, 2-byte aligned
    const unsigned short* prev;
    unsigned short* body;          // 16-byte aligned, room for w * h rounded up to a multiple of 8 elements
    int x, y, w, h;                // the rectangle, inside the frame
};
// box[4 * (f - 1) ..] = {min x, min y, max x, max y} of the pixels where frame f differs from frame f - 1, reduced with atomic min /
// max into what the caller put there ({INT_MAX, INT_MAX, -1, -1}); *d_bad = 1 when an index >= K was met in any frame (n >= 2)
void launch_gif_diff(const unsigned short* const* d_index, int n_frames, int W, int H, int K, int* d_box, int* d_bad, hipStream_t s);
// bodies of the n_bodies rectangles in d_delta (max_area: the largest w * h among them)
void launch_gif_body(const GifDelta* d_delta, int n_bodies, int W, int u, long long max_area, hipStream_t s);

// ---- GIF local colour tables (nq_gif.hip; "GIF encoding, local colour tables"): one record per frame, what the launches above take
// per call.  The record holds its table (not an offset to it), so a chain finds everything behind one pointer ----
struct GifLocal {
    int K;                         // the frame's palette entries: what an index of the caller's map is checked against
    int Kt;                        // entries of the written table (delta mode: K + 1 when u exists): what a chain checks against
    int m;                         // minimum code size, from Kt
    int T;                         // the index the lossy step leaves alone and delta bodies mark unchanged pixels with (t or u); -1: none
    unsigned rgb[256];             // the written table, 0x00RRGGBB, zeros from entry K on
};
// launch_gif_lzw with K, m, T and the colour table taken per chain from d_local[frame of the chain].  *d_bad: the caller puts ~0 there;
// a chain that meets an index >= its frame's Kt lowers it to the frame's number
void launch_gif_lzw_local(const GifFrame* d_frames, int n_frames, long long n_segs, const GifLocal* d_local, unsigned* d_words,
                          unsigned long long* d_seg_bits, unsigned long long* d_bad, int lossy, hipStream_t s);
// launch_gif_diff by colour: pixel p of frame f differs when d_local[f].rgb[index_f[p]] != d_local[f - 1].rgb[index_(f-1)[p]].  *d_bad: the
// caller puts INT_MAX there; it is lowered to the number of a frame that holds an index >= its own K
void launch_gif_diff_local(const unsigned short* const* d_index, int n_frames, int W, int H, const GifLocal* d_local, int* d_box, int* d_bad,
                           hipStream_t s);
// launch_gif_body by colour: body b is frame b + 1 against frame b, unchanged pixels replaced by d_local[b + 1].T where that is >= 0
void launch_gif_body_local(const GifDelta* d_delta, int n_bodies, int W, const GifLocal* d_local, long long max_area, hipStream_t s);

// ---- PNG encoding (nq_png.hip): image i's raw stream (per row a filter byte 0 + the indices packed at `depth` bits) is cut into
// segments of seg_len bytes (the last one shorter); segment s of the image is chain seg_base + s of the call and writes its deflate
// block to words[word_base + s * seg_words ...].  An image is width x height pixels whose rows lie `pitch` elements apart, so it may be
// a rectangle inside a larger map (index points at its first pixel); with `prev` set (the same rectangle of another map of that
// pitch) a pixel equal to prev's is packed as the index u instead.  file_off .. crc_base place the image's data chunk in the output
// (filled in after the bit lengths are known): prefix (everything in front of the deflate data, from the blob: for a still image
// signature .. IDAT header + zlib header), data_bytes of deflate data, Adler-32, the chunk's CRC, and the IEND chunk when `iend` is
// set.  The CRC covers the last crc_lead bytes of the prefix (chunk type .. zlib header: 6 for IDAT, 10 for an APNG frame's fdAT with
// its sequence number), the data and the Adler-32.  Several images may so make up one file (an APNG: one per frame). ----
struct PngImage {
    const unsigned short* index;   // 2-byte aligned
    const unsigned short* prev;    // NULL: every pixel is packed as it is
    int width, height, pitch, K, depth, u, row_bytes, seg_len, prefix_len, crc_lead, iend;
    long long raw_len, seg_base, nseg, word_base, seg_words;
    long long file_off, prefix_off, data_bytes, crc_base;      // crc_base: first of the image's 128-byte pieces in png_crc_kernel
};
// LDS bytes a chain keeps for a segment of seg_len bytes (zero padding for the match compare, 16-byte granule)
inline int png_buf_bytes(int seg_len) { return (seg_len + 16 + 15) & ~15; }
// dynamic LDS of one chain (= one workgroup of 64) at this largest segment length
size_t png_deflate_lds_bytes(int max_seg_len);
// `grid` chains at a time; rect: some image of the call has prev set or pitch != width (then the kernel that honours them runs;
// without it every image is a whole map and the still-image kernel runs); d_tokens: grid * max_seg_len words; seg_bits[g] / seg_adler[g]: bit length and Adler-32 partial
// (A | B << 32) of chain g; *d_bad = 1 when an index >= its image's K was met (zeroed by the caller)
hipError_t launch_png_deflate(const PngImage* d_images, int n_images, long long n_segs, int max_seg_len, int grid, bool rect, unsigned* d_words,
                              unsigned long long* d_seg_bits, unsigned long long* d_seg_adler, unsigned* d_tokens, unsigned long long* d_bad,
                              hipStream_t s);
// d_res[2 i] = image i's deflate bit length, d_res[2 i + 1] = the Adler-32 of its raw stream
void launch_png_scan(const PngImage* d_images, int n_images, const unsigned long long* d_seg_bits, const unsigned long long* d_seg_adler,
                     unsigned long long* d_seg_off, unsigned long long* d_res, hipStream_t s);
// all files (total bytes) and the data chunks' CRCs (d_crc[n_images], zeroed by the caller; n_crc_chunks 128-byte pieces over all images)
void launch_png_gather(const PngImage* d_images, int n_images, const unsigned* d_words, const unsigned long long* d_seg_bits,
                       const unsigned long long* d_seg_off, const unsigned long long* d_res, const unsigned char* d_blob, unsigned char* d_file,
                       long long total, long long n_crc_chunks, unsigned* d_crc, hipStream_t s);

// ---- WebP encoding (nq_webp.hip): an image is one VP8L bit string: a frame, or the rectangle of a frame (rows `pitch` elements
// apart, index points at its first pixel).  `per` indices make one packed pixel, pw packed pixels a row; band b (band_rows packed rows,
// the last one shorter) is chain chain_base + b of the call.  Chain c writes two bit strings: its five code headers to
// words[c * chain_words ...] and its pixel data to words[c * chain_words + WEBP_HEAD_WORDS ...]; bits[2 c] and bits[2 c + 1] are their
// lengths.  The image's bit string is the host's pre_bits bits (d_pre[pre_word ...]: header, transform, colour table, entropy image),
// the headers in band order, the data in band order: 1 + 2 nbands segments, whose offsets are d_off[image + 2 chain_base ...].
// file_off .. data_bytes place the image in the file once the lengths are known: prefix_len bytes of the blob (container chunk
// headers), data_bytes of the bit string, a zero byte when data_bytes is odd. ----
struct WebpImage {
    const unsigned short* index;   // 2-byte aligned
    int width, height, pitch, K, per, pw, band_rows, nbands, prefix_len;
    long long chain_base, pre_word, pre_bits;
    long long file_off, prefix_off, data_bytes;
};
constexpr int WEBP_HEAD_WORDS = 148;       // 4640 bits of code headers at most (DESIGN.md "WebP encoder"), and the words a reader may touch past them
// words of a chain at this largest chain length: the headers, at most 15 bits per packed pixel, and the words a reader may touch past them
inline long long webp_chain_words(int max_len) { return WEBP_HEAD_WORDS + (15ll * max_len + 31) / 32 + 2; }
// dynamic LDS of one chain (= one workgroup of 64) at this largest chain length (<= 32768)
size_t webp_chain_lds_bytes(int max_len);
// `grid` chains at a time; d_tokens: grid * max_len words; d_bad[image] = 1 when an index >= K was met (zeroed by the caller)
hipError_t launch_webp_chains(const WebpImage* d_images, int n_images, long long n_chains, int max_len, int grid, unsigned* d_words,
                              unsigned long long* d_bits, unsigned* d_tokens, int* d_bad, hipStream_t s);
// d_off: the segments' bit offsets inside their image; d_res[image] = the image's bit length
void launch_webp_scan(const WebpImage* d_images, int n_images, int max_len, const unsigned long long* d_bits, unsigned long long* d_off,
                      unsigned long long* d_res, hipStream_t s);
// the file (total bytes) from the placed images
void launch_webp_gather(const WebpImage* d_images, int n_images, int max_len, const unsigned* d_words, const unsigned* d_pre,
                        const unsigned long long* d_bits, const unsigned long long* d_off, const unsigned char* d_blob, unsigned char* d_file,
                        long long total, hipStream_t s);

// ---- temporal hold (nq_hold.hip): d_src / d_idx / d_out are device arrays of n frame pointers (npix elements per frame; d_out null: no
// ARGB stream), d_held n counters the caller zeroed (null: not counted).  Frames 1 .. n - 1 of idx (and out) are updated in place in one
// launch.  vec: the 16-byte path -- the caller has checked that EVERY frame pointer of every stream is 16-byte aligned; otherwise the
// one-pixel-per-thread path, which needs 2-byte (idx) and 4-byte (src, out) alignment only.  No idx / out frame may overlap another frame. ----
void launch_hold(const unsigned* const* d_src, unsigned short* const* d_idx, unsigned* const* d_out, int n, long long npix, int threshold,
                 bool vec, unsigned long long* d_held, hipStream_t s);

// ---- shot detection (nq_shots.hip): d_frames is a device array of n frame pointers (npix ARGB pixels per frame, never written), d_sig
// n * 1024 counters the caller zeroed: d_sig[1024 i + 256 c + v] += pixels of frame i whose channel c (a, r, g, b) is v, in one launch.
// vec: the 16-byte path -- the caller has checked that EVERY frame pointer is 16-byte aligned; otherwise one pixel per access (4-byte
// alignment).  cus: compute units of the device (sizes the grid). ----
void launch_signatures(const unsigned* const* d_frames, int n, long long npix, bool vec, int cus, unsigned* d_sig, hipStream_t s);

// ---- palette refinement (nq_refine.hip): d_frames is a device array of n frames (never written), `total` the pixels of the sequence.
// d_state holds REFINE_STATE_WORDS 64-bit words the caller uploaded: everything 0 but the K palette entries (32 bits each) from
// REFINE_PALETTE on.  Enqueues the iterations + 1 assignment passes with their update steps; afterwards the words from REFINE_DONE on
// hold the call's results.  vec: the 16-byte path -- the caller has checked that EVERY frame pointer is 16-byte aligned; otherwise one
// pixel per access (4-byte alignment).  cus: compute units of the device (sizes the grid).  K is 1..256, iterations 0..64. ----
struct RefineFrame { const unsigned* pixels; long long npix; };
enum {
    REFINE_ACC = 0,                         // [256][4] sums of the running pass: pixels, r, g, b per entry
    REFINE_SSE_ACC = 1024,                  // ... and its squared error
    REFINE_DONE = 1025,                     // 1: an update changed nothing, the later passes return at once
    REFINE_PASSES = 1026,                   // assignment passes that ran
    REFINE_SSE_OUT = 1027,                  // sse[0 .. 64]
    REFINE_COUNTS = REFINE_SSE_OUT + 65,    // cnt[] of the last assignment pass that ran
    REFINE_PALETTE = REFINE_COUNTS + 256,   // 256 entries of 32 bits
    REFINE_STATE_WORDS = REFINE_PALETTE + 128
};
void launch_refine(const RefineFrame* d_frames, int n, long long total, bool vec, int cus, int K, int iterations, unsigned long long* d_state,
                   hipStream_t s);

// ---- frame reduction (nq_resample.hip): d_src / d_dst are device arrays of n frame pointers (src_width pixels per source row, never
// written; dst_width * dst_height pixels per output).  The crop (crop_x, crop_y, crop_w, crop_h) of every source is area-averaged to
// dst_width x dst_height (1 <= dst <= crop on both sides) in one launch, by the integer rule of include/nquant_abi.h "frame reduction";
// linear: through the sRGB table, else in stored values.  vec: the 16-byte path -- the caller has checked that EVERY source pointer is
// 16-byte aligned and src_width is a multiple of 4; otherwise one pixel per access (4-byte alignment).  Outputs need 4-byte alignment. ----
void launch_resample(const unsigned* const* d_src, unsigned* const* d_dst, int n, int src_width, int crop_x, int crop_y, int crop_w,
                     int crop_h, int dst_width, int dst_height, bool linear, bool vec, hipStream_t s);

// ---- YUV 4:2:0 input (nq_yuv.hip; include/nquant_abi.h "YUV input"): d_tab is a device array of 4 n pointers -- the frames' y, u, v
// planes (bytes, never written) and their outputs (ARGB words), n each.  Luma of pixel (x, y) is y[y * y_stride + x], its chroma
// u / v[(y >> 1) * c_stride + (x >> 1) * c_step]; k: the coefficients of the call's flag word.  path: YUV_BYTE takes any pointers and
// strides.  The wide paths -- the caller has checked for EVERY frame: width a multiple of 4, y and y_stride multiples of 4, and
// YUV_WIDE_INTERLEAVED: c_step 2, the two chroma pointers one byte apart, the lower one (it goes into the u slot of the table; swap:
// it is v's, the same for every frame) and c_stride multiples of 4; YUV_WIDE_PLANAR: c_step 1, u, v and c_stride even.
// launch_yuv_argb converts 1:1 into tight width x height outputs; its wide paths also need every output 16-byte aligned.
// launch_resample_yuv is launch_resample on the converted frames, bit for bit, without forming them (outputs: 4-byte alignment). ----
enum { YUV_BYTE = 0, YUV_WIDE_INTERLEAVED = 1, YUV_WIDE_PLANAR = 2 };
struct YuvCoef { int cy, crv, cgu, cgv, cbu, yo; };
void launch_yuv_argb(const void* const* d_tab, int n, int width, int height, int y_stride, int c_stride, int c_step, int path, bool swap,
                     const YuvCoef& k, hipStream_t s);
void launch_resample_yuv(const void* const* d_tab, int n, int y_stride, int c_stride, int c_step, int path, bool swap, const YuvCoef& k,
                         int crop_x, int crop_y, int crop_w, int crop_h, int dst_width, int dst_height, bool linear, hipStream_t s);

// ---- orientation (nq_orient.hip; include/nquant_abi.h "orientation"): every frame of width x height is turned / mirrored by the
// EXIF code `orientation` (1..8, checked by the caller) into a tight output of width x height (codes 1..4) or height x width
// (codes 5..8) words, in one launch.  launch_orient: d_src / d_dst are device arrays of n frame pointers (sources never written).
// wide: the 16-byte path -- the caller has checked that EVERY pointer is 16-byte aligned, width is a multiple of 4 and, for codes
// 5..8, so is height; otherwise one word per access (4-byte alignment).  launch_yuv_orient is launch_yuv_argb followed by
// launch_orient, bit for bit, without forming the unturned frames: d_tab and the other arguments as for launch_yuv_argb; its wide
// paths need what launch_yuv_argb's need and, for codes 5..8, height a multiple of 4. ----
void launch_orient(const unsigned* const* d_src, unsigned* const* d_dst, int n, int width, int height, int orientation, bool wide,
                   hipStream_t s);
void launch_yuv_orient(const void* const* d_tab, int n, int width, int height, int y_stride, int c_stride, int c_step, int path, bool swap,
                       const YuvCoef& k, int orientation, hipStream_t s);

// ---- ordered dither (nq_ordered.hip): d_frames is a device array of n frames, `total` the pixels of the sequence (sizes the grid),
// d_palette the K entries (1..256) in device memory, T the first entry with alpha 0 or -1, limit 0..255.  One launch writes every
// frame's index map and, with out, its ARGB output (then every frame's `argb` is set); d_stats: 2 n sums the caller zeroed, {pixels
// that took the second entry, squared error} per frame, or null.  vec: the four-pixel path -- the caller has checked that EVERY source
// and ARGB output is 16-byte and every index map 8-byte aligned; otherwise one pixel per access (4-byte / 2-byte alignment).  The
// sources are never written; no output may overlap a source or another output. ----
struct OrderedFrame { const unsigned* pixels; unsigned short* index; unsigned* argb; long long npix; int width; int pad; };
void launch_ordered(const OrderedFrame* d_frames, int n, long long total, bool vec, bool out, const unsigned* d_palette, int K, int T, int limit,
                    unsigned long long* d_stats, hipStream_t s);

// ---- quality measurement (nq_compare.hip; include/nquant_abi.h "quality measurement"): `count` pairs of frames (1 ..
// COMPARE_FRAMES_PER_LAUNCH) go to the kernel BY VALUE, so a launch needs no table in device memory.  frame[i].out is an ARGB frame or,
// with `indexed`, a uint16 index map into `palette` (K entries in HOST memory, 1..256; copied into the launch).  result: 16 64-bit
// slots per frame of the launch, in device memory, zeroed by the caller on the same stream; `first`: the number of frame[0] in the
// call, for *d_bad (device, may be null): the caller puts INT_MAX there, it is lowered to the number of a frame that holds an index
// >= K.  vec: the 16-byte path -- the caller has checked for EVERY frame of the launch: src (and an ARGB out) 16-byte aligned, an index
// map 8-byte aligned, width a multiple of 4; otherwise one pixel per access (4-byte / 2-byte alignment).  Sides are 1..65535.  Nothing
// but the result slots (and *d_bad) is written.  compare_grid: workgroups a frame of this size gets (tests count with it). ----
constexpr int COMPARE_FRAMES_PER_LAUNCH = 16;
struct CompareFrame { const void* src; const void* out; int width, height; unsigned strips_x_rcp; int pad; };   // strips_x_rcp: launch_compare's
struct CompareLaunch { CompareFrame frame[COMPARE_FRAMES_PER_LAUNCH]; long long* result; int first; int linear; };
int compare_grid(int width, int height);
void launch_compare(const CompareLaunch& a, int count, bool vec, bool indexed, const unsigned* palette, int K, int* d_bad, hipStream_t s);

// ---- 10-bit YUV 4:2:0 input (nq_yuv16.hip; include/nquant_abi.h "10-bit YUV input"): `count` frames (1 .. YUV16_FRAMES_PER_LAUNCH) go
// to the kernel BY VALUE, so a launch needs no table in device memory.  Planes hold 16-bit words; strides and the chroma step count
// samples.  A sample is (word >> shift) & 1023 (shift 6: the high ten bits, 0: the low ten).  k: the 2^14 coefficients of the flag
// word; transfer: YUV16_SDR, YUV16_PQ or YUV16_HLG (the tables of include/nq_hdr_luts.inc).  path: YUV_BYTE takes any (2-byte aligned)
// pointers and strides, one pixel per access.  The wide paths -- the caller has checked for EVERY frame of the launch: width a multiple
// of 4, y 8-byte aligned and y_stride a multiple of 4, and YUV_WIDE_INTERLEAVED: c_step 2, the two chroma pointers one sample apart,
// the lower one (it goes into the u slot; swap: it is v's) 8-byte aligned and c_stride a multiple of 4; YUV_WIDE_PLANAR: c_step 1, u
// and v 4-byte aligned, c_stride even.  launch_yuv16_argb converts 1:1 into tight width x height outputs; its wide paths also need
// every output 16-byte aligned.  launch_resample_yuv16 is launch_resample on the converted frames, bit for bit, without forming them
// (outputs: 4-byte alignment).  Nothing but the outputs is written. ----
constexpr int YUV16_FRAMES_PER_LAUNCH = 16;
enum { YUV16_SDR = 0, YUV16_PQ = 1, YUV16_HLG = 2 };
struct Yuv16Frame { const void* y; const void* u; const void* v; void* dst; };
struct Yuv16Launch {
    Yuv16Frame frame[YUV16_FRAMES_PER_LAUNCH];
    int count, y_stride, c_stride, c_step, path, swap, shift, transfer;
    YuvCoef k;
};
void launch_yuv16_argb(const Yuv16Launch& a, int width, int height, hipStream_t s);
void launch_resample_yuv16(const Yuv16Launch& a, int crop_x, int crop_y, int crop_w, int crop_h, int dst_width, int dst_height, bool linear,
                           hipStream_t s);

// ---- retiming (nq_retime.hip; include/nquant_abi.h "retiming"): `count` consecutive outputs (1 .. RETIME_OUTPUTS_PER_LAUNCH) with
// their windows, at most RETIME_PAIRS_PER_LAUNCH (source, weight) pairs in all, go to the kernel BY VALUE, so a launch needs no table
// in device memory.  Output o of the launch is dst[o]; its pairs are first[o] .. first[o + 1] - 1 (1..64 of them), pair k reads frame
// src[k] with weight weight[k]; W[o] is the sum of its weights (1 .. 2^31 - 1).  Every frame is px words.  vec: the 16-byte path -- the
// caller has checked that EVERY src and dst of the launch is 16-byte aligned; otherwise one pixel per access (4-byte alignment).  The
// sources are never written; nothing but the px words of each output is. ----
constexpr int RETIME_OUTPUTS_PER_LAUNCH = 16;
constexpr int RETIME_PAIRS_PER_LAUNCH = 64;
struct RetimeLaunch {
    const void* src[RETIME_PAIRS_PER_LAUNCH];
    void* dst[RETIME_OUTPUTS_PER_LAUNCH];
    unsigned weight[RETIME_PAIRS_PER_LAUNCH];
    unsigned W[RETIME_OUTPUTS_PER_LAUNCH];
    int first[RETIME_OUTPUTS_PER_LAUNCH + 1];
    int count;
};
void launch_retime(const RetimeLaunch& a, long long px, bool linear, bool vec, hipStream_t s);

} // namespace nq
