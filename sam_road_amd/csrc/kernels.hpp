// Host-side launch interface of the HIP kernels (internal; the public surface is include/samroad_hip.h).
#pragma once
#include <mutex>

#include "common.hpp"
#include "scene_pad_piece.hpp"
#include "scene_group_piece.hpp"
#include "scene_bands_piece.hpp"
#include "scene_scale_piece.hpp"
#include "mask_clean_piece.hpp"
#include "scene_nodata_piece.hpp"
#include "scene_aoi_piece.hpp"
#include "scene_float_piece.hpp"
#include "graph_raster_piece.hpp"
#include "edge_support_piece.hpp"
#include "road_width_piece.hpp"
#include "graph_clean_piece.hpp"
#include "geotiff_piece.hpp"

namespace srh {

// hipFuncSetAttribute (the > 64 KiB dynamic-LDS opt-in) is per device and per kernel.  run(fn) calls fn once per device ordinal of the
// process; the device's bit is published only AFTER fn returned true, under the mutex, so a second host thread on the same device can
// never launch before the opt-in has happened, and a failed opt-in is retried (and reported) by the next launch.
struct OncePerDevice {
    std::mutex mu;
    unsigned long long done = 0;
    template <class F> bool run(F&& fn) {
        int dev = 0;
        if (hipGetDevice(&dev) != hipSuccess) return false;
        const unsigned long long bit = 1ull << (dev & 63);
        std::lock_guard<std::mutex> lk(mu);
        if (done & bit) return true;
        if (!fn()) return false;
        done |= bit;
        return true;
    }
};

// gemm_z192's persistent tile-order tables (device memory).  Owned by the caller's context: one slab, allocated at the first z192
// launch of the context and freed with it; at most SLOTS shapes, least recently used replaced (gemm_z192.hip).  A table is computed
// on the host and uploaded with a stream-ordered copy: no host synchronisation in the launch path (first use of a shape included).
struct ZTileTables {
    static constexpr int SLOTS = 32, SLOT_TILES = 8192;
    struct Key { int M = 0, N = 0, lda = 0, ldw = 0, ldc = 0, blocked = 0; };
    std::mutex mu;
    int* slab = nullptr;
    int* host = nullptr;                      // pinned image of the slab: the source of the asynchronous uploads (must outlive them)
    Key key[SLOTS];
    unsigned long long stamp[SLOTS] = {}, clock = 0;
    hipStream_t used_on[SLOTS] = {};          // the stream a slot's table was uploaded on
    hipEvent_t ready[SLOTS] = {};             // recorded behind a slot's upload: the first launch from another stream waits for it
    static constexpr int SEEN = 4;
    hipStream_t seen[SLOTS][SEEN] = {};       // other streams that have waited for the upload already: a one-time dependency per stream
    bool settled[SLOTS] = {};                 // the upload is known to be complete: no stream has to wait any more
    bool shared[SLOTS] = {};                  // launched from more than the upload stream: replacing the slot drains the device
    int used = 0, n_cu = 0;
    const int* get(int M, int N, int lda, int ldw, int ldc, int blocked, hipStream_t stream, int* ntiles_out);
    void release();
    size_t device_bytes() const { return slab ? (size_t)SLOTS * SLOT_TILES * 4 * sizeof(int) : 0; }
};

struct GemmParams {
    const f16* A = nullptr; int lda = 0;       // activations [M,K] row-major fp16
    const f16* W = nullptr; int ldw = 0;       // weights     [N,K] row-major fp16
    int M = 0, N = 0, K = 0;
    const float* bias = nullptr;               // [N]
    const float* resid = nullptr; int ldr = 0; // f32 [M,N], may alias out_f32 (in-place residual)
    const float* pos = nullptr; int pos_rows = 1;  // f32 [pos_rows,N], row m % pos_rows
    float* out_f32 = nullptr; int ldc = 0;
    f16* out_f16 = nullptr; int ldc16 = 0;
    int act = 0;                               // 0 none, 1 exact-erf GELU, 2 ReLU (applied after bias)
    int conv_S = 0, conv_C = 0;                // >0: implicit 3x3 conv over [B,S,S,C]
    int tile_gr = 0, prio_mode = 0;            // probe builds only (tools/probes/gemm_q192.hip: SRH_Q192_GR / SRH_Q192_PRIO)
    unsigned long long* dbg = nullptr;         // probe builds only: per-workgroup shader-clock ticks (gemm_z192 schedule variants, gemm_q192 segments)
    int variant = 0;                           // probe builds only: kernel / ablation selection by number (launch_gemm_probe_variant, gemm.hip); 0 in the product
    // split-K for layers with too few 128x128 tiles to fill the chip (small M: ViT-L / ViT-H at 256 px): splitk workgroups
    // per tile write f32 partials to split_ws [splitk, M, N]; a second kernel sums them in a fixed order (deterministic)
    // and applies bias / residual / activation.  0 / 1 = off.
    int splitk = 0; float* split_ws = nullptr;
    int defer_reduce = 0;                      // split-K only: leave the partials in split_ws, the caller's next LayerNorm pass sums them (NormParams::slices)
    // gemm_z192 only: A / OUT16 in the blocked-16 layout (1 KiB blocks of 32 rows x 16 columns, the two 16-byte chunks of a row
    // chunk-major: element (m, n) at ((m/32)*(cols/16) + n/16)*1024 + ((n%16)/8)*512 + (m%32)*16 + (n%8)*2; lda / ldc16 still
    // name the logical row length).  Used for the MLP's hidden activation between fc1 and fc2 (see tools/kgen/gemm_z192_gen.py).
    int a_blocked16 = 0, out_blocked16 = 0;
    ZTileTables* ztab = nullptr;               // gemm_z192's tile tables: the context's (ctx.hpp gemm() sets it; without it the layer takes the generic kernels)
};
int launch_gemm(const GemmParams& p, hipStream_t s);
int gemm_splitk_factor(const GemmParams& p);   // what launch_gemm would use if a workspace were provided (1 = no split)
// hand-scheduled persistent 256 x 192 kernel with the deferred epilogue (gemm_z192.hip, body generated by tools/kgen/gemm_z192_gen.py):
// fp16 output, bias, act none / GELU, no residual / pos-embed; `preferred` = supported and enough tiles to occupy the chip
bool z192_supported(const GemmParams& p);
bool z192_preferred(const GemmParams& p);
int launch_gemm_z192(const GemmParams& p, hipStream_t s, int var = 0);   // var: schedule variant, probe builds only
#ifdef SRH_TUNING      // probe builds (tools/probes/): z192's predecessor kept for A/B runs, and the generated schedule variants
bool q192_supported(const GemmParams& p);
int launch_gemm_q192(const GemmParams& p, hipStream_t s, int ablation = 0);
int z192_var_count();
int z192_var_out_blocked(int var);     // 1: this schedule variant writes the blocked-16 layout (the caller sets out_blocked16)
#endif

// Row LayerNorm (biased variance) f32 [M,D] -> fp16 and/or f32; gamma == nullptr => cast only.
struct NormParams {
    const float* x = nullptr; int M = 0, D = 0;
    int x_period = 0;                          // > 0: x has x_period rows and row m reads row m % x_period (pos_embed as block 0's initial residual)
    const float* gamma = nullptr; const float* beta = nullptr; float eps = 1e-6f;
    int act = 0;                               // 1: GELU after affine
    f16* out_f16 = nullptr; float* out_f32 = nullptr;
    // optional fused residual add: x' = x + delta16 (fp16 [M,D], a GEMM's deferred-epilogue output) is what gets
    // normalised, and is written back to x_out (may alias x) when x_out != nullptr
    const f16* delta16 = nullptr; float* x_out = nullptr;
    // optional second branch output folded AFTER the first: x' = (x + delta16) + delta16b (needs delta16)
    const f16* delta16b = nullptr;
    // optional split-K partials of the preceding GEMM (GemmParams::defer_reduce) folded instead of a reduce pass:
    // x' = x + ((slice 0 + slice 1 + ...) + slice_bias), the sums in splitk_reduce_kernel's order (same bits); excludes delta16
    const float* slices = nullptr; int nslices = 0; size_t slice_stride = 0; const float* slice_bias = nullptr;
    // optional non-finite sentinel (gamma != nullptr only): a row whose variance is not finite — an Inf / NaN in x or in a folded
    // branch output, i.e. an fp16 overflow upstream — sets nf[nf_tag] = 1.  The pass reads every branch output anyway: one compare per row.
    unsigned* nf = nullptr; int nf_tag = 0;
};
int launch_layernorm(const NormParams& p, hipStream_t s);

// Tile batcher + pixel normalise + patch im2col (K1/K2 prologue).
struct PatchParams {
    const void* src = nullptr;   // f32 [B,P,P,3] tiles (scene_W == 0) or u8/f32 scene [H,W,3]
    int src_is_u8 = 0;
    int B = 0, P = 0;
    int scene_W = 0;             // >0: crop tiles out of a resident scene of this width (= row pitch in pixels) at tile_xy;
                                 // every tile must lie inside the scene (the height is not needed to address it)
    const int* tile_xy = nullptr;  // device [B,2] (x0,y0)
    f16* out = nullptr;          // [B*(P/16)^2, 768] with k = ky*48 + kx*3 + c
};
int launch_patch_im2col(const PatchParams& p, hipStream_t s);

// Windowed / global attention with rel-pos bias; pad tokens are real keys with k = b_k, v = b_v.
struct AttnParams {
    const f16* qkv = nullptr; int ld = 0;   // [tokens, 3*D]: q | k | v, each head-major
    const f16* table_h = nullptr;           // [2*win-1, hd] fp16 rel-pos tables: the kernels derive the bias from the unscaled q
    const f16* table_w = nullptr;
    const f16* bias_qkv = nullptr;          // [3*D] fp16 (pad-token k / v rows)
    f16* out = nullptr; int ldo = 0;        // [tokens, D]
    int B = 0, S = 0, heads = 0, hd = 0, win = 0;  // win == S => global
    float scale = 0.125f;
    int ablate = 0;                         // probe builds (SRH_TUNING): ablation / kernel selection, see tools/probes/attn_win_probe.hip
    unsigned hx_order[16] = {};             // attention_hdx.hip only, filled by its launcher: workgroup slot -> (window << 1 | query part), heaviest first
    void* scratch = nullptr;                // probe builds: >= ATTN_SCRATCH_BYTES of device memory nobody reads (the persistent windowed experiment's waves without a result store there) + the phase counters
};
constexpr size_t ATTN_SCRATCH_BYTES = 512 * 128;
int launch_attention(const AttnParams& p, hipStream_t s);
// tools/probes/attention_g64.hip (probe builds only): the generated-asm global attention for 32 x 32 tokens, head dim 64
bool attention_g64_supported(const AttnParams& p);
int launch_attention_g64(const AttnParams& p, hipStream_t s);
// attention_hdx.hip: MFMA attention for head dim 80 on 14x14 windows / the 16x16 global window (ViT-H at 256 px)
bool attention_hdx_supported(const AttnParams& p);
int launch_attention_hdx(const AttnParams& p, hipStream_t s);

// The whole map_decoder in one kernel (decoder.hip decode_fused_kernel; reference model.py:286-295, :445-446 / :490-494):
// ConvT(256->128) + LayerNorm2d + GELU + ConvT(128->64) + GELU + ConvT(64->32) + GELU + ConvT(32->2) + sigmoid + NHWC scatter
struct DecodeFusedParams {
    const f16* emb16 = nullptr;  // [B*S*S, 256] the neck's output (fp16 copy), token-major
    const char* frags = nullptr; // packed MFMA A fragments (pack_host.hpp pack_decoder_fused)
    const float* prm = nullptr;  // biases, LayerNorm2d affine, the last layer's f32 weights
    int B = 0, S = 0;
    float* logits = nullptr;     // nullable [B,P,P,2]
    float* scores = nullptr;     // nullable [B,P,P,2]
    unsigned* nf = nullptr; int nf_tag = 0;   // non-finite sentinel of the LayerNorm2d (NormParams::nf)
};
int launch_decode_fused(const DecodeFusedParams& p, hipStream_t s);

// Scene canvases -> u8 masks (divide by analytic coverage count, x255, truncate; uncovered -> 0).
struct SceneNormParams {
    const float* canvas_kp = nullptr; const float* canvas_road = nullptr;
    const float* counter = nullptr;  // f32 [H,W] coverage count
    uint8_t* kp_u8 = nullptr; uint8_t* road_u8 = nullptr; int n = 0;
};
int launch_scene_normalise(const SceneNormParams& p, hipStream_t s);
// scene_H * scene_W <= INT_MAX (the C ABI checks it): a pixel index fits an int, byte offsets are 64-bit
int launch_scene_count(float* counter, int scene_H, int scene_W, const int* tile_xy, int n_tiles, int P, hipStream_t s);
int launch_scene_add(const float* scores, int B, int P, const int* tile_xy, float* kp, float* road, int scene_H, int scene_W,
                     hipStream_t s);
// Validity mask of a scene (scene_valid.hip): valid u8 [H,W], non-zero = valid.  Valid pixels per tile (int32 [n_tiles]; -1 for a tile
// outside the scene; P a multiple of 16, else -2), nodata -> fill colour in place, and the normalise that also zeroes nodata pixels.
int launch_tile_valid_count(const uint8_t* valid, int scene_H, int scene_W, const int* tile_xy, int n_tiles, int P, int* counts, hipStream_t s);
int launch_scene_fill_invalid(uint8_t* scene, const uint8_t* valid, int scene_H, int scene_W, int fill_r, int fill_g, int fill_b, hipStream_t s);
int launch_scene_normalise_valid(const SceneNormParams& p, const uint8_t* valid, hipStream_t s);
// Window-weighted fusion (scene_window.hip): profile f32 [P] on the device, weight of a tile at a pixel = profile[lx] * profile[ly].
// canvas += w * score for one batch (terms in tile order, one fma each), and weight sum + normalise in one kernel (valid nullable).
int launch_scene_add_window(const float* scores, int B, int P, const int* tile_xy, const float* profile, float* kp, float* road, int scene_H,
                            int scene_W, hipStream_t s);
int launch_scene_normalise_window(const float* kp, const float* road, int scene_H, int scene_W, const int* tile_xy, int n_tiles, int P,
                                  const float* profile, const uint8_t* valid, uint8_t* kp_u8, uint8_t* road_u8, hipStream_t s);
// Test-time augmentation (scene_tta.hip), orient = 1..7 (0 = id runs neither): the A matrix launch_patch_im2col writes
// for the oriented crop of every tile, bit for bit (u8 scene of scene_H rows only), and the scores [B,P,P,2] of oriented tiles brought
// back to the scene frame (a permutation of float2 values; in != out).
int launch_patch_im2col_oriented(const PatchParams& p, int scene_H, int orient, hipStream_t s);
int launch_scores_unorient(const float* in, int B, int P, int orient, float* out, hipStream_t s);
// Scene border padding (scene_pad.hip; ScenePadParams in scene_pad_piece.hpp): dst = src padded by reflection, edge
// replication or a constant colour, u8 rows of 3 bytes (the scene) or 1 byte (the mask) per pixel; -2 for parameters outside their range.
int launch_scene_pad(const ScenePadParams& p, hipStream_t s);
// Scene groups (scene_group.hip; SceneGroupParams and the table in scene_group_piece.hpp): the stack of a group's padded
// scenes from one ragged source buffer, and every scene's window of the stack's two u8 masks into two ragged outputs (kp / road: the
// same table and sizes, C = 1).  The table is on the device and has been checked on the host (group_table_ok); -2 for bad parameters.
int launch_scene_group_pack(const SceneGroupParams& p, hipStream_t s);
int launch_scene_group_crop(const SceneGroupParams& kp, const SceneGroupParams& road, hipStream_t s);
// 16-bit and multi-band scenes (scene_bands.hip; SceneBandsParams in scene_bands_piece.hpp): the exact histogram of the
// three selected bands (hist u32 [3, levels], zeroed by the launch itself) and dst u8 [n,3] = the tables gathered at the selected bands;
// -2 for parameters outside their range.
int launch_scene_bands_hist(const SceneBandsParams& p, hipStream_t s);
int launch_scene_bands_apply(const SceneBandsParams& p, hipStream_t s);
// Scene resampling (scene_scale.hip; SceneScaleParams in scene_scale_piece.hpp): dst = src resampled by two per-axis tap
// tables, the weighted sum with one rounding or the validity rule; -2 for parameters outside their range.
int launch_scene_resample(const SceneScaleParams& p, hipStream_t s);
// Connected-component filter of u8 masks, in place (mask_clean.hip; MaskCleanParams and the table in mask_clean_piece.hpp):
// step 0 .. 4 = init, merge, flatten, statistics, apply — five launches per call, none of which waits for another workgroup.  The table
// is on the device and has been checked on the host (mask_clean_table_ok); -2 for bad parameters.
int launch_mask_clean(const MaskCleanParams& p, int step, hipStream_t s);
// Validity mask from a nodata value (scene_nodata.hip; the parameters in scene_nodata_piece.hpp): the per-pixel match of a
// raw u8 / u16 scene against per-band ranges, and the Chebyshev dilation of n u8 images described by a device table that has been checked
// on the host (grow_table_ok; max_blocks = grow_max_blocks); -2 for bad parameters.
int launch_scene_nodata_match(const SceneNodataParams& p, hipStream_t s);
int launch_scene_nodata_grow(const SceneGrowParams& p, long max_blocks, hipStream_t s);
// Validity mask from the polygons of an area of interest (scene_aoi.hip; the parameters in scene_aoi_piece.hpp): the even-odd
// fill of include / exclude polygons given as a device table of edges that has been checked on the host (aoi_table_ok); -2 for bad
// parameters.
int launch_scene_aoi_fill(const SceneAoiParams& p, hipStream_t s);
// Float32 scenes (scene_float.hip; SceneFloatParams in scene_float_piece.hpp): the validity mask by rule 1, the exact
// histograms of the ordered keys (pass 1 over key >> 16, with targets pass 2 over key & 0xffff; zeroed by the launch itself) and dst u8
// [n,3] = the level of every selected value among 255 threshold keys; -2 for parameters outside their range.
int launch_scene_float_valid(const SceneFloatParams& p, hipStream_t s);
int launch_scene_float_hist(const SceneFloatParams& p, hipStream_t s);
int launch_scene_float_apply(const SceneFloatParams& p, hipStream_t s);
// The road graph as a raster (graph_raster.hip; the parameters in graph_raster_piece.hpp).  The class map is three launches
// that the caller orders on one stream: clear (always), edges (E > 0), nodes (N > 0 and a mark); the tables are on the device and have
// been checked on the host (gr_tables_ok).  composite: the scene with the classes in colour.  compare: four counts (counts_zero in front)
// and the optional diff image in one pass.  -2 for bad parameters.
int launch_graph_clear(const GraphRasterParams& p, hipStream_t s);
int launch_graph_edges(const GraphRasterParams& p, hipStream_t s);
int launch_graph_nodes(const GraphRasterParams& p, hipStream_t s);
int launch_graph_composite(const GraphCompositeParams& p, hipStream_t s);
int launch_graph_counts_zero(const GraphCompareParams& p, hipStream_t s);
int launch_graph_compare(const GraphCompareParams& p, hipStream_t s);
// The road-mask evidence under every edge (edge_support.hip; the parameters in edge_support_piece.hpp): one launch, a wave
// per edge, four int32 per edge.  E >= 1; the tables are on the device and have been checked on the host (gr_tables_ok).  -2 for bad parameters.
int launch_graph_edge_stats(const EdgeStatsParams& p, hipStream_t s);
// The capped squared distance map of a thresholded mask (road_width.hip; the parameters in road_width_piece.hpp): pass 0
// the column pass (mask -> g), pass 1 the row pass (g -> d2), one launch each.  -2 for bad parameters.
int launch_road_dist(const RoadDistParams& p, int pass, hipStream_t s);
// The six width statistics of every edge over its centre line: one launch, 16 lanes per edge, eight int32 per edge.  E >= 1; the tables
// are on the device and have been checked on the host (gr_tables_ok).  -2 for bad parameters.
int launch_graph_edge_widths(const EdgeWidthParams& p, hipStream_t s);
// Spur and small-component pruning of the graph (graph_clean.hip; the parameters in graph_clean_piece.hpp): step 0 .. 4 of a
// pass — init, edges, chains, sums, decide — one launch each.  E >= 1; the tables are on the device and have been checked on the host
// (gr_tables_ok).  -2 for bad parameters.
int launch_graph_clean(const GraphCleanParams& p, int step, hipStream_t s);

// A GeoTIFF's decompressed segments -> the raster (scene_tiff.hip; the parameters in geotiff_piece.hpp).  One launch.
int launch_tiff_assemble(const TiffParams& p, hipStream_t s);

// Bilinear sampler (F.grid_sample, align_corners=False, zeros) on channels-last embeddings.
struct SampleParams {
    const float* emb = nullptr;    // [B,h,w,C] channels-last f32
    const void* points = nullptr; int points_i64 = 0;  // [B,N,2] (x,y) pixels, int64 or f32
    int B = 0, N = 0, h = 0, w = 0, C = 0; float patch = 512.f;
    f16* out_f16 = nullptr; float* out_f32 = nullptr;   // [B*N, C]
    const int* point_tile = nullptr;                     // ragged rows (srh_toponet_ragged): the embedding tile of every point, instead of point / N
    int n_tiles = 0;                                     // with point_tile: tiles in emb (indices are clamped into [0, n_tiles))
};
int launch_sample(const SampleParams& p, hipStream_t s);

// TopoNet helpers.
struct PairGatherParams {
    const f16* pf = nullptr;        // relu(feature_proj) [B*N,128] fp16
    const void* points = nullptr; int points_i64 = 0;
    const void* pairs = nullptr; int pairs_i64 = 0;   // [B,Ns,K,2]
    int B = 0, N = 0, Ns = 0, Kp = 0; int zero_offset = 0;
    long index_base = 0;                                 // subtracted from every pair index (a chunk of a longer flat row list, srh_toponet_ragged)
    // ragged rows (srh_toponet_ragged): every pair must name two rows of this launch that sample the same tile (point_tile equal); no
    // python-style wrap, and a pair that breaks this sets *bad (the host-mapped sentinel, NF_PAIRS) instead of gathering another row
    const int* point_tile = nullptr; unsigned* bad = nullptr;
    f16* out = nullptr; int ld = 0;  // [B*Ns*K, ld>=258] = src | tgt | dx dy | 0...
};
int launch_pair_gather(const PairGatherParams& p, hipStream_t s);

// fused TopoNet trunk (topo_fused.hip): pair rows -> logits / scores
struct TopoFusedParams {
    // K = pairs per sequence (MAX_NEIGHBOR_QUERIES, 1..64): sequence s owns pair rows, valid bytes and outputs s*K .. s*K+K-1
    const f16* pair = nullptr; int ld_pair = 320;     // [nseq*K, ld_pair] gathered pair rows (src | tgt | dx dy | 0)
    const uint8_t* valid = nullptr;                   // [nseq, K], byte-addressed
    const char* stream = nullptr;                     // packed MFMA fragments (pack_host.hpp pack_topo_fused)
    const float* params = nullptr;                    // biases, LayerNorm affine, output_proj
    int nlayers = 3, nseq = 0, K = 16;
    float* logits = nullptr; float* scores = nullptr; // [nseq*K], nullable
};
int launch_topo_fused(const TopoFusedParams& p, hipStream_t s);

// ---- SAM MaskDecoder branch (sam_decoder.hip; reference model.py:260-282, :426-443) ----------------------------------------
struct SdLinearParams {                  // y[r,n] = act((x[r,:] + xadd[r % add_rows,:]) . W[n,:] + b[n]); f32, token side
    const float* x = nullptr; int ldx = 0; const float* xadd = nullptr; int add_rows = 1;
    const float* W = nullptr; const float* b = nullptr; int rows = 0, N = 0, K = 0, act = 0;
    float* y = nullptr; int ldy = 0;
};
int launch_sd_add_channel(const float* emb, const float* vec, float* out_f32, f16* out_f16, size_t rows, hipStream_t s);
int launch_sd_tok_linear(const SdLinearParams& p, hipStream_t s);
int launch_sd_tok_ln(const float* x, const float* resid, const float* g, const float* b, float* y, int rows, hipStream_t s);
int launch_sd_tok_selfattn(const float* q, const float* k, const float* v, float* out, int B, hipStream_t s);
int launch_sd_t2i_attn(const float* q, const f16* K, const f16* V, float* out, int B, int HW, hipStream_t s);
int launch_sd_i2t_attn(const f16* Q, const float* k, const float* v, f16* out, int B, int HW, hipStream_t s);
int launch_sd_ln64_gelu(const float* x, const float* g, const float* b, f16* y, size_t rows, hipStream_t s);
int launch_sd_mask(const f16* up, const float* hyper, float* low, int B, int S, hipStream_t s);
int launch_sd_upsample(const float* low, float* logits, float* scores, int B, int L, int P, hipStream_t s);

}  // namespace srh
