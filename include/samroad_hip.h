/*
 * samroad_hip.h — C ABI of libsamroad_hip.so: the MI355X (gfx950) implementation of sam_road's
 * tiled-inference hot path.  Plain C types only (no torch, no C++ in the signatures).
 *
 * This is the drop-in boundary of SURVEY.md §8(b).  The reference has no FFI of its own for this
 * path (it is pure Python on torch.nn); each entry point below names the reference interface it
 * replaces (file:line under the reference repository) and INTEGRATION.md shows the ctypes binding a
 * sam_road maintainer would add behind `SAMRoad`.
 *
 * Conventions
 *   - every function returns 0 on success or a negative srh_status; srh_last_error(ctx) has text;
 *   - all data pointers are DEVICE pointers on the ctx's device unless documented as host;
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream); calls are asynchronous on
 *     that stream; nothing is retained past return except by srh_weights_pack (which copies);
 *   - the callee allocates nothing in hot calls except growing the ctx-owned workspace the first
 *     time a larger batch is seen;
 *   - image embeddings cross this ABI CHANNELS-LAST: [B, h, w, 256] f32 (the Python shim returns a
 *     permuted view with the reference's logical shape [B, 256, h, w]).
 */
#ifndef SAMROAD_HIP_H
#define SAMROAD_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SRH_ABI_VERSION 11

typedef enum {
    SRH_OK = 0,
    SRH_ERR_BAD_ARG = -1,      /* null pointer, bad dtype code, bad shape */
    SRH_ERR_UNSUPPORTED = -2,  /* configuration not built (e.g. head_dim other than 64 / 80) */
    SRH_ERR_HIP = -3,          /* HIP runtime error (text in srh_last_error) */
    SRH_ERR_MISSING_WEIGHT = -4,
    SRH_ERR_NO_DEVICE = -5,
    SRH_ERR_NONFINITE = -6     /* ABI 8: a LayerNorm pass of an EARLIER call on this context read an Inf / NaN (fp16 overflow upstream) */
    /* ABI 9: an earlier srh_toponet_ragged call's pair outside its row's tile is reported the same lazy way, as SRH_ERR_BAD_ARG */
} srh_status;

typedef enum { SRH_F32 = 0, SRH_F16 = 1, SRH_U8 = 2, SRH_I32 = 3, SRH_I64 = 4, SRH_U16 = 5 /* scene bands only */ } srh_dtype;

typedef struct srh_ctx srh_ctx;          /* per (process, device): workspace + error state */
typedef struct srh_weights srh_weights;  /* packed, device-resident, immutable model weights */

/* Architecture, mirrors SAMRoad.__init__ (model.py:197-258, :283-300). */
typedef struct {
    int32_t embed_dim;          /* 768 / 1024 / 1280 */
    int32_t depth;              /* 12 / 24 / 32 */
    int32_t num_heads;          /* 12 / 16 / 16 */
    int32_t patch_size;         /* config.PATCH_SIZE: tile side in pixels, a multiple of 16 from 128 to 1024 */
    int32_t n_global;           /* number of entries used in global_attn_indexes */
    int32_t global_attn_indexes[8];
    int32_t window_size;        /* 14 */
    int32_t toponet_version;    /* 0 'normal' (and 'no_tgt_features', App. D.7), 1 'no_offset', 2 'no_transformer' */
    int32_t use_sam_decoder;    /* config.USE_SAM_DECODER (model.py:260-282): 0 = naive map_decoder, 1 = SAM PromptEncoder + MaskDecoder */
} srh_model_cfg;

/* One state_dict entry (SURVEY.md Appendix A names), f32, contiguous. */
typedef struct {
    const char* name;
    const void* data;           /* host pointer, or device pointer if on_device != 0 */
    int32_t on_device;
    int32_t ndim;
    int64_t shape[4];
} srh_named_tensor;

int srh_abi_version(void);
/* 16 hex digits: sha256 over the sources (csrc, this header, compiler flags) the library was built from.  The Python shim,
 * __graft_entry__.build() / smoke() and bench.py compare it with the hash of the sources in the tree, so a stale prebuilt
 * library is rebuilt or refused instead of silently measured (the reference has no counterpart: it is interpreted). */
const char* srh_build_id(void);

/* lifetime ------------------------------------------------------------------------------------ */
int srh_ctx_create(int device, srh_ctx** out);
void srh_ctx_destroy(srh_ctx* ctx);
const char* srh_last_error(const srh_ctx* ctx);
/* ABI 8 — non-finite sentinel.  Inter-kernel activations are fp16; a checkpoint whose activations overflow would come out as silently
 * wrong masks (the reference's own guards, inferencer.py:206 NaN -> -100 and :219 assert 0 <= score <= 1, only see TopoNet's output).
 * Every LayerNorm pass of the encoder / neck / map_decoder reads each branch output anyway and flags a row whose variance is not finite
 * (flags live in host-mapped memory: nothing is copied or synchronised in the hot loop).  The condition is reported LAZILY as
 * SRH_ERR_NONFINITE — by the next srh_encode_decode / srh_scene_pass1 on the context, or by srh_ctx_check — with srh_last_error naming
 * the first stage that saw it ("encoder block 7, norm2 ..."); reporting clears it.  synchronize != 0: wait for `stream` first (the
 * answer then covers every call issued so far); 0: only what has already completed. */
int srh_ctx_check(srh_ctx* ctx, void* stream, int synchronize);
/* Lanes (two entries added to ABI 11; the version number is unchanged because nothing that existed changed).  srh_encode_decode and the
 * srh_scene_pass1* calls can run the encoder of a batch as TWO half-batch chains of the same kernels — tiles [0, B/2) on the caller's
 * stream, tiles [B/2, B) on one stream the context owns — joined before the neck; tiles never interact in the encoder, so the outputs
 * are those of one chain bit for bit, and the caller still sees one stream (outputs ordered on it, the input free to be overwritten on
 * it right after the call; no additional device memory).  mode 0 = auto (the default): two lanes when B is even, profiling is off and a
 * HALF batch still runs the patch embed and every block GEMM on the persistent 256 x 192 kernel with enough tiles (ViT-B, B/2 *
 * (patch_size/16)^2 >= 8192: B >= 16 at 512 px, B >= 4 at 1024 px); 1 = always one lane; 2 = two lanes whenever B is even and profiling
 * is off (for tests at small shapes; no promise about speed).  While srh_profile_enable is on every call runs one lane.
 * srh_ctx_last_lanes: how many lanes the last such call ran (1 before any). */
int srh_ctx_set_lanes(srh_ctx* ctx, int mode);
int srh_ctx_last_lanes(const srh_ctx* ctx);

/* Packs `net.load_state_dict(ckpt["state_dict"])` + `net.to(device)` (inferencer.py:250-254):
 * fp16 MFMA operand copies of every matmul weight (conv kernels re-ordered to the GEMM K order),
 * f32 biases / LayerNorm affine / pos_embed, fp16 rel_pos tables. */
int srh_weights_pack(srh_ctx* ctx, const srh_model_cfg* cfg, const srh_named_tensor* tensors, int n,
                     srh_weights** out);
void srh_weights_free(srh_weights* w);

/* Multi-GPU weight distribution (north_star: "RCCL broadcast of weights over xGMI"; the reference is single-process,
 * inferencer.py:243-254).  The packed arena is position-independent and its layout depends on srh_model_cfg alone, so ONE
 * rank packs a checkpoint and the others receive the packed fp16/f32 bytes device-to-device — no state_dict travels, no rank
 * but the first reads the checkpoint or re-packs.  srh_weights_export: *bytes = size of the packed arena; with dst != NULL
 * (device pointer, `capacity` bytes) the arena is copied there.  srh_weights_import: builds a weights object for `cfg` from
 * such a copy (device pointer; SRH_ERR_BAD_ARG if `bytes` is not what `cfg` packs to). */
int srh_weights_export(srh_ctx* ctx, const srh_weights* w, void* dst, size_t capacity, size_t* bytes);
int srh_weights_import(srh_ctx* ctx, const srh_model_cfg* cfg, const void* src, size_t bytes, srh_weights** out);

/* model ----------------------------------------------------------------------------------------- */

/* SAMRoad.infer_masks_and_img_features (model.py:459-495; body shared with forward :420-446):
 * rgb [B,P,P,3] channels-last, values 0..255, dtype SRH_F32 or SRH_U8
 *   -> mask_logits (nullable) / mask_scores (nullable) [B,P,P,2] f32, embeddings [B,h,w,256] f32. */
int srh_encode_decode(srh_ctx* ctx, const srh_weights* w, const void* rgb, int rgb_dtype, int B,
                      float* mask_logits, float* mask_scores, float* embeddings, void* stream);

/* SAMRoad.infer_toponet (model.py:498-508) = BilinearSampler (:29-58) + TopoNet (:61-148).
 * embeddings [B,h,w,256] f32 channels-last; points [B,N,2] (x,y) SRH_I64 or SRH_F32;
 * pairs [B,Ns,K,2] SRH_I64 or SRH_I32; valid [B,Ns,K] u8 (bool).
 * ABI 10: K = MAX_NEIGHBOR_QUERIES may be 1 to 64 (it had to be 16); any other K is SRH_ERR_UNSUPPORTED.
 *   -> logits (nullable) / scores (nullable) [B,Ns,K] f32. */
int srh_toponet(srh_ctx* ctx, const srh_weights* w, const float* embeddings, const void* points,
                int points_dtype, const void* pairs, int pairs_dtype, const uint8_t* valid, int B, int N,
                int Ns, int K, float* logits, float* scores, void* stream);

/* infer_toponet over the query rows of MANY tiles at once, unpadded (pass 2 of infer_one_img, inferencer.py:179-207: the reference
 * pads every batch of INFER_BATCH_SIZE tiles to its longest tile, graph_collate_fn-style; every row is scored on its own, so the
 * padding rows are pure waste — 68 k padded rows for 48 k real ones on a CityScale scene).  Rows = the concatenated per-tile point
 * lists; embeddings [n_tiles,h,w,256]; points f32 [R,2] tile-local (x,y); point_tile i32 [R] = index of the row's tile in
 * `embeddings` (clamped into [0, n_tiles)); pairs i32 [R,K,2] = (row, target row) into the flat list; valid u8 [R,K]; scores f32
 * [R,K] out.  srh_pass2_pack_ragged builds these.
 * ABI 8: tile_offsets (HOST pointer, int64 [n_tiles + 1], nullable) = the first row of every tile, from 0 to R.  With it the rows are
 * scored in chunks of whole tiles of at most 16 384 x 16 pairs (rows x K; same bits: rows are independent and a pair only names rows
 * of its own tile), so the context's workspace is bounded like the reference's INFER_BATCH_SIZE batches instead of growing with the
 * scene; without it the call is one launch and refuses more than 65 536 x 16 pairs.
 * ABI 10: K may be 1 to 64 (it had to be 16); any other K is SRH_ERR_UNSUPPORTED.  The bounds above count pairs, so they are the
 * 16 384 / 65 536 rows of ABI 8 at K = 16.
 * ABI 9: both indices of every pair must be rows in [0, R) whose point_tile equals the source row's (no python-style wrap of a
 * negative index).  The pair gather checks this on the device; a pair that breaks it makes the call's scores invalid and is reported
 * like the non-finite sentinel — SRH_ERR_BAD_ARG from srh_ctx_check or the next srh_encode_decode / srh_scene_pass1 on the context —
 * instead of silently gathering another row (a chunk would otherwise wrap or clamp it into an unrelated row of its own). */
int srh_toponet_ragged(srh_ctx* ctx, const srh_weights* w, const float* embeddings, int n_tiles, const float* points,
                       const int32_t* point_tile, const int32_t* pairs, const uint8_t* valid, int64_t R, int K,
                       const int64_t* tile_offsets, float* scores, void* stream);

/* scene level (pass 1 of infer_one_img, inferencer.py:79-110) ------------------------------------ */

/* Tile batcher + model + mask fusion: crops n_tiles PxP tiles at tile_xy[(x0,y0)] (device int32)
 * out of a resident u8 scene [S,S,3], runs them in batches of B, accumulates mask scores into the
 * two f32 canvases [S,S] (caller zero-initialises) in the reference's sequential tile order, and
 * writes every tile's embeddings to embeddings_all [n_tiles,h,w,256]. */
int srh_scene_pass1(srh_ctx* ctx, const srh_weights* w, const uint8_t* scene, int S, const int32_t* tile_xy,
                    int n_tiles, int B, float* canvas_kp, float* canvas_road, float* embeddings_all,
                    void* stream);

/* canvas / coverage-count * 255 -> u8 (truncation; uncovered border -> 0), inferencer.py:106-110. */
int srh_scene_normalise(srh_ctx* ctx, const float* canvas_kp, const float* canvas_road, int S,
                        const int32_t* tile_xy, int n_tiles, int P, uint8_t* kp_u8, uint8_t* road_u8,
                        void* stream);

/* ABI 11: rectangular scenes.  The same two calls for a scene u8 [H,W,3] (row pitch W pixels, no padding) with canvases f32 [H,W] and
 * masks u8 [H,W]; H and W are independent, each >= PATCH_SIZE, and H * W <= 2^31 - 1 pixels (SRH_ERR_BAD_ARG otherwise).  Tiles stay
 * PATCH_SIZE squares, and every tile is computed by the kernels that compute it for a square scene: srh_scene_pass1(S) and
 * srh_scene_normalise(S) ARE the H = W = S case of this code.  tile_xy is a device array the host cannot read without a
 * synchronisation, so it is a PRECONDITION (as it always was for the square calls) that every tile lies inside the scene:
 * 0 <= x0 <= W - P and 0 <= y0 <= H - P.  The tile list may have any length (no n x n grid is assumed); pixels no tile covers
 * keep their canvas value and come out of the normalise as 0. */
int srh_scene_pass1_hw(srh_ctx* ctx, const srh_weights* w, const uint8_t* scene, int H, int W, const int32_t* tile_xy,
                       int n_tiles, int B, float* canvas_kp, float* canvas_road, float* embeddings_all,
                       void* stream);
int srh_scene_normalise_hw(srh_ctx* ctx, const float* canvas_kp, const float* canvas_road, int H, int W,
                           const int32_t* tile_xy, int n_tiles, int P, uint8_t* kp_u8, uint8_t* road_u8,
                           void* stream);

/* Scenes with a per-pixel validity mask (nodata).  Three additive entries; the ABI number stays 11 because nothing existing changes.
 * valid = device u8 [H,W], row pitch W, non-zero = valid pixel.  A scene without a mask calls none of them.
 *
 * srh_scene_tile_valid: counts[t] = number of valid pixels inside the PxP tile at tile_xy[t] = (x0, y0) (device int32 [n_tiles]; exact,
 *   one workgroup per tile, no atomics).  P must be a multiple of 16, at least 32 (every PATCH_SIZE is); H, W >= P and H * W <= 2^31 - 1, else
 *   SRH_ERR_BAD_ARG.  Every tile must lie inside the scene, as for srh_scene_pass1_hw; a tile that does not is not read and counts -1.
 *   The call touches no workspace of the context, so it may be issued on another stream than the context's compute stream.
 * srh_scene_fill_invalid: scene[y][x] = (fill_r, fill_g, fill_b) wherever valid[y][x] == 0, in place on the device u8 [H,W,3] scene;
 *   valid pixels keep their values (a group of four pixels that holds an invalid one is stored back whole, so the scene must not be read
 *   by other work while the call runs).  fill_* outside 0..255 and H * W > 2^31 - 1 are SRH_ERR_BAD_ARG; no tile size enters this call.
 * srh_scene_normalise_valid_hw: srh_scene_normalise_hw whose masks are also 0 on every invalid pixel; for valid pixels the same
 *   arithmetic, so an all-valid mask gives the bytes of srh_scene_normalise_hw. */
int srh_scene_tile_valid(srh_ctx* ctx, const uint8_t* valid, int H, int W, const int32_t* tile_xy, int n_tiles, int P,
                         int32_t* counts, void* stream);
int srh_scene_fill_invalid(srh_ctx* ctx, uint8_t* scene, const uint8_t* valid, int H, int W, int fill_r, int fill_g,
                           int fill_b, void* stream);
int srh_scene_normalise_valid_hw(srh_ctx* ctx, const float* canvas_kp, const float* canvas_road, int H, int W,
                                 const int32_t* tile_xy, int n_tiles, int P, const uint8_t* valid, uint8_t* kp_u8,
                                 uint8_t* road_u8, void* stream);

/* Window-weighted fusion of overlapping tiles (config key FUSE_WINDOW; an extension, the reference fuses with a uniform mean).  Three
 * additive entries; the ABI number stays 11 because nothing existing changes, and a scene without a window calls none of them.
 * profile = device f32 [P], every value finite and in [2^-20, 2^20] (the caller checks it: the host cannot read the array here).  The
 * weight of tile t at scene pixel (x, y) is w = profile[x - x0_t] * profile[y - y0_t], one f32 product.
 *
 * srh_scene_pass1_window_hw: srh_scene_pass1_hw whose canvases receive canvas = fma(w, score, canvas) per covering tile, in tile order
 *   (deterministic, no atomics, independent of B).  Same encoder and decoder launches, same embeddings, same preconditions and
 *   SRH_ERR_BAD_ARG cases as srh_scene_pass1_hw; the tile size is the model's PATCH_SIZE, so profile must hold that many values.
 * srh_scene_normalise_window_hw: u8 = trunc((canvas / Wsum) * 255) with Wsum = the f32 sum of w over ALL n_tiles tiles in list order;
 *   0 where no tile covers the pixel and, with valid != NULL (u8 [H,W], non-zero = valid), where the pixel is invalid.  An all-ones
 *   profile gives the bytes of srh_scene_normalise_hw / srh_scene_normalise_valid_hw.  P must be a tile size (a multiple of 16 from 128
 *   to 1024) and H * W <= 2^31 - 1, else SRH_ERR_BAD_ARG.
 * srh_op_scene_fuse_window (test-only): the weighted add of pass 1 applied to caller-supplied scores f32 [n,P,P,2], all n tiles in
 *   one launch; H, W >= P, every tile inside the scene. */
int srh_scene_pass1_window_hw(srh_ctx* ctx, const srh_weights* w, const uint8_t* scene, int H, int W, const int32_t* tile_xy,
                              int n_tiles, int B, const float* profile, float* canvas_kp, float* canvas_road,
                              float* embeddings_all, void* stream);
int srh_scene_normalise_window_hw(srh_ctx* ctx, const float* canvas_kp, const float* canvas_road, int H, int W,
                                  const int32_t* tile_xy, int n_tiles, int P, const float* profile, const uint8_t* valid,
                                  uint8_t* kp_u8, uint8_t* road_u8, void* stream);
int srh_op_scene_fuse_window(srh_ctx* ctx, const float* scores, int n, int P, const int32_t* tile_xy, const float* profile,
                             float* canvas_kp, float* canvas_road, int H, int W, void* stream);

/* Test-time augmentation over the 8 orientations of a tile (config key TTA; an extension).  Additive entries; the ABI
 * number stays 11 because nothing existing changes, and a scene without TTA calls none of them.  An orientation code acts on a P x P
 * tile T[row, col]:  0 id  1 flip_h T[:, ::-1]  2 flip_v T[::-1, :]  3 rot180  4 transpose  5 rot90 (np.rot90(T, 1))  6 rot270
 * (np.rot90(T, 3))  7 anti_transpose T[::-1, ::-1] transposed.
 *
 * srh_scene_pass1_tta_hw: srh_scene_pass1_hw (profile == NULL) or srh_scene_pass1_window_hw (profile = device f32 [P]) run once per
 *   orientation, in the order of orients (HOST array of k codes), each time over the WHOLE tile list: the crop of a tile is oriented,
 *   encoded and decoded, its score tile is brought back with the inverse orientation and added by the same add kernel, so the
 *   summation order is (orientation, tile) and independent of B.  embeddings_all receives the embeddings of orientation id, bit for bit
 *   those of a call without TTA; the others go to a workspace of the context.  The canvases are to be normalised with the tile list
 *   repeated k times.  The preconditions and SRH_ERR_BAD_ARG cases of srh_scene_pass1_hw, and SRH_ERR_BAD_ARG (nothing is launched)
 *   unless 1 <= k <= 8, every code <= 7, no code twice and orients[0] == 0.  k == 1 makes exactly the launches of the entry it extends.
 * srh_op_patch_im2col (test-only): the GEMM A matrix f16 [n (P/16)^2, 768] of pass 1's crop + normalise + im2col for n tiles of a u8
 *   scene in one orientation; orient 0 is the launch of every scene without TTA.  P a tile size, H, W >= P, n <= 65535.
 * srh_op_scores_unorient (test-only): scores f32 [n,P,P,2] of oriented tiles -> the scene frame, a permutation of bit patterns;
 *   scores_out must not be scores_in.  orient 0 copies. */
int srh_scene_pass1_tta_hw(srh_ctx* ctx, const srh_weights* w, const uint8_t* scene, int H, int W, const int32_t* tile_xy,
                           int n_tiles, int B, const uint8_t* orients, int k, const float* profile, float* canvas_kp,
                           float* canvas_road, float* embeddings_all, void* stream);
int srh_op_patch_im2col(srh_ctx* ctx, const uint8_t* scene_u8, int H, int W, const int32_t* tile_xy, int n, int P, int orient,
                        void* out_f16, void* stream);
int srh_op_scores_unorient(srh_ctx* ctx, const float* scores_in, int n, int P, int orient, float* scores_out, void* stream);

/* Scene border padding (config key SCENE_PAD; an extension).  One additive entry; the ABI number stays 11 because nothing
 * existing changes, and a scene without the key does not call it.
 *
 * srh_scene_pad: dst u8 [H + top + bottom, W + left + right, C] = src u8 [H, W, C] (both on the device, dense rows, any byte address, not
 *   overlapping) with the four borders added: pixel (Y, X) of dst holds pixel (f(Y - top, H), f(X - left, W)) of src, where for an axis of n
 *   pixels SRH_PAD_REFLECT folds i with period T = 2 (n - 1): i mod T if that is below n, else T - (i mod T) (n = 1: always 0) — numpy's
 *   pad mode "reflect" for any pad width; SRH_PAD_EDGE clamps i to [0, n - 1]; SRH_PAD_CONSTANT takes fill_rgb (HOST array of three ints,
 *   C = 1 uses the first) wherever i falls outside [0, n).  Every byte of dst is written exactly once and nothing else is.  C must be 3
 *   (a scene) or 1 (a validity mask), the pads >= 0, mode one of the three, H, W >= 1, H * W and the padded size <= 2^31 - 1 pixels and,
 *   where fill_rgb is given, its values 0..255 (it may be NULL unless mode is SRH_PAD_CONSTANT): else SRH_ERR_BAD_ARG and nothing is
 *   launched.  The call touches no workspace of the context. */
#define SRH_PAD_REFLECT 0
#define SRH_PAD_EDGE 1
#define SRH_PAD_CONSTANT 2
int srh_scene_pad(srh_ctx* ctx, const uint8_t* src, int H, int W, int C, int top, int bottom, int left, int right, int mode,
                  const int32_t* fill_rgb, uint8_t* dst, void* stream);

/* Scene groups (config key SCENE_GROUP; an extension): the tiles of several small scenes run as one pass 1 over a vertical
 * stack of their (padded) images.  Two additive entries; the ABI number stays 11 because nothing existing changes, and a run without
 * the key calls neither.
 *
 * The table has one row of eight int64 per scene k: { off, H, W, top, left, Hv, Wv, row0 }.  H x W is the real scene, Hv x Wv >= (H + top)
 * x (W + left) its virtual (padded) size, row0 the stack row it starts at: row0[0] = 0, row0[k + 1] = row0[k] + Hv[k], sum Hv = Ha, every
 * Wv <= Wa.  off is the byte offset of the scene's block in the ragged buffer of THAT call.  The table is passed twice: table_host is read
 * and validated by the entry before anything is launched, table_dev — the same n * 8 values on the device, uploaded by the caller — is
 * what the kernel reads.  The entry cannot compare the two; a table_dev that differs from table_host is undefined behaviour.
 *
 * srh_scene_group_pack: dst u8 [Ha, Wa, C] on the device, every byte written exactly once and nothing else: stack pixel (row0 + Y, X)
 *   with X < Wv holds pixel (f(Y - top, H), f(X - left, W)) of the scene's block src + off (u8 [H, W, C], dense rows, any byte address) by
 *   the rule and the modes of srh_scene_pad; columns X >= Wv hold 0.  src_bytes: the size of the ragged buffer; every block must lie
 *   inside it (blocks may repeat or leave gaps).  fill_rgb as for srh_scene_pad.
 * srh_scene_group_crop: for every scene the window [row0 + top : row0 + top + H, left : left + W] of the two u8 [Ha, Wa] masks kp and
 *   road -> the dense H x W blocks out_kp + off and out_road + off.  The blocks must tile [0, out_bytes) in table order with no gap
 *   (off[0] = 0, off[k + 1] = off[k] + H W, the last one ending at out_bytes), so every output byte is written exactly once.
 * Both: SRH_ERR_BAD_ARG, and nothing is launched, unless the pointers are non-null, n >= 1, C is 1 or 3, mode one of the three, every
 *   row of table_host is consistent as above with H, W >= 1 and pads >= 0, the blocks lie inside src_bytes / tile out_bytes, and Ha * Wa
 *   <= 2^31 - 1.  Neither touches a workspace of the context.  Profiler rows: scene_group_pack, scene_group_crop. */
int srh_scene_group_pack(srh_ctx* ctx, const uint8_t* src, int64_t src_bytes, const int64_t* table_host, const int64_t* table_dev, int n,
                         int C, int Ha, int Wa, int mode, const int32_t* fill_rgb, uint8_t* dst, void* stream);
int srh_scene_group_crop(srh_ctx* ctx, const uint8_t* kp, const uint8_t* road, int Ha, int Wa, const int64_t* table_host,
                         const int64_t* table_dev, int n, uint8_t* out_kp, uint8_t* out_road, int64_t out_bytes, void* stream);

/* 16-bit and multi-band scenes (config key SCENE_BANDS; an extension): band selection and a radiometric lookup table on
 * the device, in front of everything above.  Two additive entries and one dtype code (SRH_U16); the ABI number stays 11 because nothing
 * existing changes, and a run without the key calls neither.
 *
 * Both see the source as n_pixels pixels of C elements, dense, on the device: src_dtype SRH_U8 (levels = 256; any byte address) or
 * SRH_U16 (levels = 65536; any 2-byte-aligned address), 1 <= C <= 16, 1 <= n_pixels <= 2^31 - 1.  They know nothing of rows: a scene
 * and the ragged buffer of a scene group are the same to them.  select: HOST array of three ints in 0 .. C - 1 (repeats allowed), the
 * source band of output channel 0, 1, 2.  The source is not written.
 *
 *   hist: u32 [3, levels] on the device, zeroed by the call itself; on return hist[b][v] is the exact number of counted pixels whose
 *     band select[b] holds v.  valid: u8 [n_pixels] on the device, 0 = the pixel is not counted, or NULL = every pixel is.  Integer
 *     adds: the result does not depend on scheduling.
 *   apply: dst u8 [n_pixels, 3] on the device (any byte address, not overlapping src), byte 3 i + b = lut[b][src[i][select[b]]] with
 *     lut u8 [3, levels] on the device.  Every byte of dst is written exactly once and nothing else is.
 * SRH_ERR_BAD_ARG, and nothing is launched, for a null pointer (valid excepted), another dtype, C or n_pixels outside their range, a
 * select entry outside 0 .. C - 1 or a misaligned u16 source.  Neither touches a workspace of the context.  Profiler rows:
 * scene_bands_hist, scene_bands_apply. */
int srh_scene_bands_hist(srh_ctx* ctx, const void* src, int src_dtype, int64_t n_pixels, int C, const int32_t* select,
                         const uint8_t* valid, uint32_t* hist, void* stream);
int srh_scene_bands_apply(srh_ctx* ctx, const void* src, int src_dtype, int64_t n_pixels, int C, const int32_t* select,
                          const uint8_t* lut, uint8_t* dst, void* stream);

/* Scenes at another ground resolution (config key SCENE_SCALE; an extension): the scene is resampled on the device in
 * front of pass 1 and the masks are resampled back behind it.  One additive entry; the ABI number stays 11 because nothing existing
 * changes, and a run without the key does not call it.
 *
 * srh_scene_resample: dst u8 [Ho, Wo, C] from src u8 [H, W, C] (both on the device, dense rows, any byte address, not overlapping), C = 3
 *   (a scene) or 1 (a mask).  Each axis has a table on the device: start int32 [n_out] and weights u8 [n_out, T] whose rows sum to D; tap
 *   t of output j reads input clamp(start[j] + t, 0, n_in - 1).  The tables state the rule (sam_road_amd/resample.py builds them: area
 *   averaging down, bilinear up); the entry evaluates them exactly, in integers:
 *     mode 0: dst = (sum_y sum_x wy wx src + (Dy Dx) / 2) / (Dy Dx) per channel — one rounding;
 *     mode 1: src is a validity mask and dst = 1 iff every tap whose weights are non-zero on both axes is non-zero, else 0.
 *   zero_where: u8 [Ho, Wo] on the device or NULL; where it is 0, dst is 0.  The source is not written, every byte of dst is written
 *   exactly once and nothing else is.  Every tap index is clamped where it is used, so no table content leads outside src.
 *   block_h x block_w: the outputs one workgroup produces (1..256 each).  win_h x win_w: the source window, in rows and pixels, it may
 *   stage in LDS for the separable form of mode 0 — win_h * (round16(win_w C + 15) + 2 block_w C) bytes, at most 64 KiB; a block
 *   whose taps span more, and every block of mode 1, gathers each output's taps from src instead (the same bytes).  0 x 0: no LDS at
 *   all (the direct form).
 *   SRH_ERR_BAD_ARG, and nothing is launched, unless the pointers (zero_where excepted) are non-null, C is 1 or 3, mode 0 or 1, H, W,
 *   Ho, Wo >= 1 with H * W and Ho * Wo <= 2^31 - 1, 1 <= Ty, Tx <= 32, 1 <= Dy, Dx <= 32 and the block / window are as above.  The call
 *   touches no workspace of the context.  Profiler row: scene_resample. */
int srh_scene_resample(srh_ctx* ctx, const uint8_t* src, int H, int W, int C, uint8_t* dst, int Ho, int Wo, const int32_t* start_y,
                       const uint8_t* weights_y, int Ty, int Dy, const int32_t* start_x, const uint8_t* weights_x, int Tx, int Dx, int mode,
                       const uint8_t* zero_where, int block_h, int block_w, int win_h, int win_w, void* stream);

/* Small mask components dropped on the device (config key MASK_CLEAN; an extension): a connected-component filter of the
 * u8 masks between the normalise step and the download.  One additive entry; the ABI number stays 11 because nothing existing changes,
 * and a run without the key does not call it.
 *
 * srh_mask_clean: filters n u8 images IN PLACE.  Image k is a dense H_k x W_k block at byte offset OFF_k of buf (buf_bytes bytes on the
 *   device, any byte address).  A pixel is foreground iff its level is >= T_ON_k; the components are the connected components of the
 *   foreground under `connectivity` (8 or 4) inside the image — nothing connects two images, however their blocks lie; a component
 *   stays iff its pixel count is >= MIN_AREA_k and its highest level is >= T_PEAK_k; the pixels of the others become 0 and every other
 *   byte of buf is untouched (sam_road_amd/mask_clean.py states the rule: mask_clean_ref).
 *   The table, int64 [n, 8], is given twice, as for srh_scene_group_pack: table_host is validated, table_dev is what the kernels read.
 *   Row k: {OFF, H, W, T_ON, MIN_AREA, T_PEAK, BASE, SEG0}, BASE = sum of H W and SEG0 = sum of H ceil(W / 64) over the rows before k.
 *   parent, area, peak: int32 [ws_pixels] each on the device, the CALLER's — the entry touches no workspace of the context; their
 *   content on entry does not matter and is undefined afterwards.
 *   Five launches per call whatever the images hold (init, merge, flatten, statistics, apply: label equivalence with a union-find in
 *   global memory).  No workgroup waits for another, nothing is read back and the host does not wait.
 *   SRH_ERR_BAD_ARG, and nothing is launched, for a null pointer, a connectivity other than 4 or 8, a workspace that is not 4-byte
 *   aligned, n outside 1 .. 4096, or a host table in which a block has H or W < 1, leaves buf or overlaps another block, T_ON or T_PEAK
 *   lies outside 0 .. 256, MIN_AREA is < 1, BASE or SEG0 is not the running sum, or the pixels of all images exceed ws_pixels or
 *   2^31 - 1.  Every pixel and neighbour access of the kernels is bounded by the row's H and W.  Profiler rows: mask_clean_init,
 *   mask_clean_merge, mask_clean_flatten, mask_clean_stats, mask_clean_apply. */
int srh_mask_clean(srh_ctx* ctx, uint8_t* buf, int64_t buf_bytes, const int64_t* table_host, const int64_t* table_dev, int n,
                   int connectivity, int32_t* parent, int32_t* area, int32_t* peak, int64_t ws_pixels, void* stream);

/* The validity mask from a nodata VALUE (config key SCENE_NODATA; an extension): which pixels of the raw scene hold the
 * value, and that set grown by r pixels, on the device right behind the upload.  (The area rule in between is srh_mask_clean as it is.)
 * Two additive entries; the ABI number stays 11 because nothing existing changes, and a run without the key calls neither.
 *
 * srh_scene_nodata_match: the source is n_pixels pixels of C elements, dense, on the device: src_dtype SRH_U8 (any byte address) or
 *   SRH_U16 (any 2-byte-aligned address), 1 <= C <= 16, 1 <= n_pixels <= 2^31 - 1.  It knows nothing of rows: a scene and the ragged
 *   buffer of a scene group are the same to it.  lo, hi: HOST arrays of C ints in 0 .. 65535; band c hits iff lo[c] <= element <=
 *   hi[c] (lo > hi: never).  match: SRH_NODATA_ALL = every band hits, SRH_NODATA_ANY = at least one does.  and_with: u8 [n_pixels] on
 *   the device or NULL; invert: 0 / 1.  out u8 [n_pixels] on the device (any byte address, overlapping neither src nor and_with):
 *   out[i] = (invert ? !hit : hit) & (and_with ? and_with[i] != 0 : 1), 0 or 1.  The source is read and never written, every byte of
 *   out is written exactly once and nothing else is.  No atomics, no LDS.
 * srh_scene_nodata_grow: n images, image k a dense H_k x W_k u8 block at byte offset OFF_k of src AND of dst (and of and_with, if
 *   given), each buffer `bytes` bytes on the device, src and dst not overlapping.  g[y, x] = 1 iff a pixel of the image within
 *   Chebyshev distance r of (y, x) is non-zero in src — nothing outside the image counts, and nothing connects two images; dst =
 *   (invert ? !g : g) & (and_with ? and_with != 0 : 1).  1 <= r <= 16.  The table, int64 [n, 8], is given twice, as for srh_mask_clean:
 *   table_host is validated, table_dev is what the kernel reads.  Row k: {OFF, H, W, ...}; columns 3 .. 7 are not read, so a
 *   srh_mask_clean table serves as it is.  Every byte of every block of dst is written exactly once and nothing else is.
 * SRH_ERR_BAD_ARG, and nothing is launched, for a null pointer (and_with excepted), another dtype, C, n_pixels, match, invert or r
 * outside their range, a bound outside 0 .. 65535, a misaligned u16 source, out overlapping src or and_with, src and dst of the grow
 * overlapping, n outside 1 .. 4096, or a host table in which a block has H or W < 1, leaves the buffers, overlaps another block, or
 * the pixels exceed 2^31 - 1.  Neither touches a workspace of the context.  Profiler rows: scene_nodata_match, scene_nodata_grow. */
#define SRH_NODATA_ALL 0
#define SRH_NODATA_ANY 1
int srh_scene_nodata_match(srh_ctx* ctx, const void* src, int src_dtype, int64_t n_pixels, int C, const int32_t* lo, const int32_t* hi,
                           int match, const uint8_t* and_with, int invert, uint8_t* out, void* stream);
int srh_scene_nodata_grow(srh_ctx* ctx, const uint8_t* src, uint8_t* dst, int64_t bytes, const int64_t* table_host,
                          const int64_t* table_dev, int n, int r, const uint8_t* and_with, int invert, void* stream);

/* The validity mask from the POLYGONS of an area of interest (config key SCENE_AOI; an extension): the even-odd fill of
 * include and exclude polygons on the device, right behind the upload.  One additive entry; the ABI number stays 11 because nothing
 * existing changes, and a run without the key does not call it.  (The buffer step is srh_scene_nodata_grow as it is, its invert flag
 * doing the shrink.)
 *
 * srh_scene_aoi_fill: edges int32 [E, 4], rows {y0, x0, y1, x1} in 1/256 px of the pixel-corner frame (pixel (r, c) covers [r, r + 1) x
 *   [c, c + 1)), every edge oriented y0 < y1, horizontal edges left out; polys int32 [n_include + n_exclude + 1], polygon k owns edges
 *   polys[k] .. polys[k + 1], the include polygons first.  Both tables are given twice, as srh_mask_clean takes its table: the host
 *   copy is validated, the device copy (edges 16-byte aligned) is what the kernel reads, and it is never written.  An edge crosses row
 *   y iff y0 <= 256 y + 128 < y1 and then toggles every pixel of the row from column max(0, ceil(((x0 - 128) dy + (256 y + 128 - y0)
 *   dx) / (256 dy))) on; a pixel is inside a polygon iff its toggles are odd.  aoi = (n_include ? inside any include polygon : 1) & not
 *   inside any exclude polygon.  and_with: u8 [H, W] on the device or NULL; invert: 0 / 1.  out u8 [H, W] on the device, any byte
 *   address: out[i] = (invert ? !aoi : aoi) & (and_with ? and_with[i] != 0 : 1), 0 or 1.  Every byte of out is written exactly once and
 *   nothing else is.  One launch, no global atomics, no workspace of the context, nothing read back; the result does not depend on
 *   scheduling.
 * SRH_ERR_BAD_ARG, and nothing is launched, for a null pointer (and_with excepted), H or W < 1 or H W > 2^31 - 1, n_include or
 * n_exclude < 0 or more than SRH_AOI_MAX_POLYGONS together, offsets that are not a running sum from 0 to at most SRH_AOI_MAX_EDGES, an
 * edge with y0 >= y1, a coordinate outside +-2^28, invert outside 0 / 1, a misaligned device edge table, or out overlapping and_with.
 * Profiler row: scene_aoi_fill. */
#define SRH_AOI_MAX_POLYGONS 64
#define SRH_AOI_MAX_EDGES 16384
int srh_scene_aoi_fill(srh_ctx* ctx, const int32_t* edges_host, const int32_t* edges_dev, const int32_t* polys_host, const int32_t* polys_dev,
                       int n_include, int n_exclude, int H, int W, const uint8_t* and_with, int invert, uint8_t* out, void* stream);

/* Float32 scenes (config key SCENE_FLOAT; an extension): a float32 scene of 1 to 16 bands becomes the u8 [n, 3] scene and
 * its validity mask on the device, right behind the upload.  Three additive entries; the ABI number stays 11 because nothing existing
 * changes, and a run without the key calls none of them.  A float is read as its 32-bit pattern b and compared through the ordered key:
 * b = 0x80000000 reads as 0 (-0.0 is +0.0); key = ~b if the sign bit is set, else b | 0x80000000.  Integer compares only.
 *
 * Common: src f32 [n_pixels, C] on the device at any 4-byte-aligned address, 1 <= C <= 16, 1 <= n_pixels <= 2^31 - 1; select: a HOST
 * array of three band indices in 0 .. C - 1.  The source is read (the selected bands only) and never written.  No entry knows of rows.
 * srh_scene_float_valid: valid_out u8 [n_pixels] on the device (any byte address, overlapping neither src nor valid_in): 1 iff every
 *   selected band is finite (exponent field not 0xff), has none of the n_nodata (0 .. 4) keys of the HOST array nodata_keys (NULL allowed
 *   for 0), with log = 1 has a key above that of zero, and valid_in (u8 [n_pixels] on the device, or NULL) is non-zero there; else 0.
 *   Every byte of valid_out is written exactly once and nothing else is.  No atomics, no LDS.
 * srh_scene_float_hist: exact counts over the pixels whose valid byte (u8 [n_pixels] on the device, required) is non-zero.  targets NULL
 *   (n_targets 0), pass 1: hist u32 [3, 65536], hist[b][v] = the pixels with key(band select[b]) >> 16 == v.  Otherwise pass 2: targets is
 *   a HOST array u32 [n_targets, 2] of (band, prefix) pairs, 1 <= n_targets <= 6, and hist u32 [n_targets, 65536] with hist[t][v] = the
 *   pixels with key(band) >> 16 == prefix and key(band) & 0xffff == v.  hist is on the device, 4-byte aligned, zeroed by the call itself.
 *   Integer adds only: the counts are exact and do not depend on scheduling.
 * srh_scene_float_apply: dst u8 [n_pixels, 3] on the device (any byte address, overlapping neither src nor valid): byte 3 i + b = the
 *   number of j < 255 with thresholds[b][j] <= key(src[i][select[b]]) where valid[i] != 0, else 0.  thresholds: u32 [3, 256] on the device,
 *   4-byte aligned, every row ascending, entry 255 = 0xffffffff.  Every byte of dst is written exactly once and nothing else is.  3 KiB
 *   of LDS, no atomics.
 * SRH_ERR_BAD_ARG, and nothing is launched, for a null pointer (valid_in, nodata_keys with n_nodata 0 and targets with n_targets 0
 * excepted), C or n_pixels outside their range, a select entry or a target's band outside 0 .. C - 1, a prefix above 65535, n_nodata
 * outside 0 .. 4, n_targets outside 0 .. 6, log outside 0 / 1, a source that is not 4-byte aligned, a misaligned hist or threshold table,
 * or an output overlapping an input.  None touches a workspace of the context.  Profiler rows: scene_float_valid, scene_float_hist,
 * scene_float_apply. */
int srh_scene_float_valid(srh_ctx* ctx, const void* src, int64_t n_pixels, int C, const int32_t* select, const uint32_t* nodata_keys,
                          int n_nodata, int log, const uint8_t* valid_in, uint8_t* valid_out, void* stream);
int srh_scene_float_hist(srh_ctx* ctx, const void* src, int64_t n_pixels, int C, const int32_t* select, const uint8_t* valid,
                         const uint32_t* targets, int n_targets, uint32_t* hist, void* stream);
int srh_scene_float_apply(srh_ctx* ctx, const void* src, int64_t n_pixels, int C, const int32_t* select, const uint8_t* valid,
                          const uint32_t* thresholds, uint8_t* dst, void* stream);

/* The road graph as a raster (config key GRAPH_RASTER; an extension): the OUTPUT side.  The reference draws the graph
 * over the scene with cv2.line / cv2.circle on the host (triage.py:8-35, inferencer.py:324-329) and carries, commented out, the pixel
 * comparison with the ground truth (triage.py:38-71, inferencer.py:305-322); cv2's bytes are not reproduced, the rule is the integer one
 * of sam_road_amd/graph_raster.py.  Three additive entries; the ABI number stays 11 because nothing existing changes, and a run
 * without the key calls none of them.  None touches a workspace of the context and nothing is read back.
 *
 * srh_graph_raster: nodes int32 [N, 2] (row, col) and edges int32 [E, 2] (indices into nodes), each given twice as srh_scene_aoi_fill
 *   takes its tables: the host copy is validated, the device copy (4-byte aligned) is what the kernels read, and it is never written.  A
 *   pixel is the point at its integer coordinates.  For an edge a -> b of width t: d = b - a, p = x - a, u = p.d, L = d.d; x is covered
 *   iff 4 p.p <= t^2 when L = 0 or u <= 0, 4 |p - d|^2 <= t^2 when u >= L, else 4 (p x d)^2 <= t^2 L — the pixels within t / 2 of the
 *   segment.  A node mark covers the pixels with Chebyshev distance <= r (SRH_GRAPH_MARK_SQUARE) or p.p <= r^2 (SRH_GRAPH_MARK_DISC) of
 *   the node; SRH_GRAPH_MARK_NONE draws none.  out u8 [H, W] on the device, any byte address: node_value on a node mark, else edge_value
 *   on an edge, else 0 (the class map: edge_value 1, node_value 2).  Nodes may lie outside the image; everything is clipped.  N = 0 and
 *   E = 0 are ordinary (the tables may then be NULL).  Every byte of out is defined after the call and nothing else is written: a clear,
 *   then one wave per edge, then one wave per node, ordered by the stream; writers of one launch store the same byte, so the result does
 *   not depend on scheduling.  No atomics.
 * srh_graph_composite: cls u8 [H, W] and img u8 [H, W, 3] or NULL on the device; three HOST colours of three ints 0 .. 255.  out u8
 *   [H, W, 3] on the device, any byte address: node_rgb where cls >= 2, edge_rgb where cls == 1, else img (background_rgb without one).
 * srh_graph_compare: four class maps u8 [H, W] (non-zero = covered), valid u8 [H, W] or NULL, img u8 [H, W, 3] or NULL, on the device.
 *   counts: four uint64 on the device, 8-byte aligned, written by the call: over the pixels with valid != 0 (all without valid)
 *   {#(pred_thin), #(pred_thin & !gt_wide), #(gt_thin), #(gt_thin & !pred_wide)} — integer sums, the same numbers in any order.  diff u8
 *   [H, W, 3] on the device or NULL, written in the same pass: img (black without one) with red (255, 0, 0) on a counted missed pixel,
 *   else blue (0, 0, 255) on a counted false positive.
 * SRH_ERR_BAD_ARG, and nothing is launched, for a null pointer (the tables of an empty graph, img, valid and diff excepted), a negative
 * count, H or W < 1 or H W > 2^31 - 1, t outside 1 .. 255, an unknown mark, r outside 0 .. 127, a class value outside 1 .. 255, a
 * coordinate outside +-2^28, an edge index outside [0, N), an edge spanning more than SRH_GRAPH_MAX_SPAN pixels on an axis (with it every
 * product of the rule stays inside 64 bits), a colour outside 0 .. 255, a misaligned device table or counts, or an output overlapping an
 * input.  Profiler rows: graph_clear, graph_edges, graph_nodes, graph_composite, graph_counts_zero, graph_compare. */
#define SRH_GRAPH_MAX_SPAN 16383
#define SRH_GRAPH_MARK_NONE 0
#define SRH_GRAPH_MARK_SQUARE 1
#define SRH_GRAPH_MARK_DISC 2
int srh_graph_raster(srh_ctx* ctx, const int32_t* nodes_host, const int32_t* nodes_dev, int N, const int32_t* edges_host,
                     const int32_t* edges_dev, int E, int H, int W, int t, int mark, int r, int edge_value, int node_value, uint8_t* out,
                     void* stream);
int srh_graph_composite(srh_ctx* ctx, const uint8_t* cls, const uint8_t* img, int H, int W, const int32_t* background_rgb,
                        const int32_t* edge_rgb, const int32_t* node_rgb, uint8_t* out, void* stream);
int srh_graph_compare(srh_ctx* ctx, const uint8_t* pred_thin, const uint8_t* pred_wide, const uint8_t* gt_thin, const uint8_t* gt_wide,
                      const uint8_t* valid, const uint8_t* img, int H, int W, uint64_t* counts, uint8_t* diff, void* stream);

/* The road-mask evidence under every edge of a graph (config key EDGE_SUPPORT; an extension): the graph-domain post-check.
 * The reference has none: its graph leaves as the votes produced it.  One additive entry; the ABI number stays 11 because nothing
 * existing changes, and a run without the key does not call it.  It touches no workspace of the context and nothing is read back.
 *
 * Tables as srh_graph_raster takes them: nodes int32 [N, 2] (row, col) and edges int32 [E, 2], each given twice — the host copy is
 * validated, the device copy (4-byte aligned) is what the kernel reads, and it is never written.  The covered set C_e of edge e is the
 * set of pixels of [0, H) x [0, W) that srh_graph_raster's rule covers for this edge alone at width t.  mask u8 [H, W] and valid u8
 * [H, W] or NULL on the device.  out int32 [E, 4] on the device, 16-byte aligned, per edge
 *   {n = |C_e|, s = sum of mask over C_e, n_on = #(mask > on_level in C_e), n_invalid = #(valid == 0 in C_e), 0 without valid}
 * — integer sums, the same numbers in any order; n < 6.0e6 and 255 n < 2^31 for every edge the tables admit.  An edge wholly outside
 * the image gives {0, 0, 0, 0}.  Every element of out is defined after the call and nothing else is written: one launch, a wave per
 * edge, one 16-byte store per edge, no atomics.  E = 0 is SRH_OK and launches nothing (mask and out may then be NULL).
 * SRH_ERR_BAD_ARG, and nothing is launched, for every condition srh_graph_raster refuses (a null table of a non-empty graph, a negative
 * count, H or W < 1 or H W > 2^31 - 1, t outside 1 .. 255, a coordinate outside +-2^28, an edge index outside [0, N), an edge spanning
 * more than SRH_GRAPH_MAX_SPAN pixels on an axis, a misaligned device table), on_level outside 0 .. 255, a null mask or out with E > 0,
 * an out that is not 16-byte aligned, or an out overlapping an input.  Profiler row: graph_edge_stats. */
int srh_graph_edge_stats(srh_ctx* ctx, const int32_t* nodes_host, const int32_t* nodes_dev, int N, const int32_t* edges_host,
                         const int32_t* edges_dev, int E, int H, int W, int t, const uint8_t* mask, const uint8_t* valid, int on_level,
                         int32_t* out, void* stream);

/* The road width under every edge of a graph (config key ROAD_WIDTH; an extension).  Two additive entries; the ABI number
 * stays 11 because nothing existing changes, and a run without the key calls neither.  Nothing is read back.
 *
 * srh_road_dist: the capped squared Euclidean distance map of a thresholded mask.  mask u8 [H, W] on the device; F = {mask > on_level};
 * d2_out u16 [H, W] on the device, 8-BYTE ALIGNED (pixel i of the flat image lies at d2_out + i; the row pass stores four pixels of the
 * flat index as one 8-byte word):
 *   d2_out[x] = 0 for x outside F, else min(R^2, min over the pixels y OF THE IMAGE outside F of |x - y|^2)
 * — pixels outside the image are not background.  R is 1 .. SRH_ROAD_MAX_RADIUS, so R^2 fits 16 bits.  Exact integers: it equals
 * road_dist_ref of sam_road_amd/road_width.py.  Two launches whatever the mask holds (a column pass into H W bytes of the context's
 * workspace, a row pass out of it; the entry holds a lock of the context from the workspace's growth to the second launch, so it may
 * be called from several threads), no atomics, no workgroup waits for another.  Every element of d2_out is defined after the call and
 * nothing else is written.  SRH_ERR_BAD_ARG, and nothing is launched, for a null argument, H or W < 1 or H W > 2^31 - 1, on_level
 * outside 0 .. 255, R outside 1 .. 254, a d2_out that is not 8-byte aligned or overlaps the mask.  Profiler rows: road_dist_cols,
 * road_dist_rows.
 *
 * srh_graph_edge_widths: tables as srh_graph_edge_stats takes them; the covered set C_e of edge e is that entry's at t = 1, the
 * 8-connected centre line.  d2 u16 [H, W] on the device (2-byte aligned), the map of srh_road_dist at the same R.  out int32 [E, 8] on
 * the device, 16-byte aligned, per edge
 *   {n = |C_e|, n_in = #(d2 > 0), s_q = sum of floor(16 sqrt(d2)), n_cap = #(d2 == R^2), d2_min over the pixels with d2 > 0 (0 when
 *    n_in = 0), d2_max, 0, 0}
 * — n <= 46343 and s_q <= 4064 n < 2^31 for every edge the tables admit.  An edge wholly outside the image gives eight zeros.  One
 * launch, 16 lanes per edge, two 16-byte stores per edge, no atomics.  E = 0 is SRH_OK and launches nothing (d2 and out may then be
 * NULL).  SRH_ERR_BAD_ARG, and nothing is launched, for every condition srh_graph_edge_stats refuses of its tables, H and W, R outside
 * 1 .. 254, a null d2 or out with E > 0, a misaligned d2 or out, or an out overlapping an input.  Profiler row: graph_edge_widths. */
#define SRH_ROAD_MAX_RADIUS 254
int srh_road_dist(srh_ctx* ctx, const uint8_t* mask, int H, int W, int on_level, int R, uint16_t* d2_out, void* stream);
int srh_graph_edge_widths(srh_ctx* ctx, const int32_t* nodes_host, const int32_t* nodes_dev, int N, const int32_t* edges_host,
                          const int32_t* edges_dev, int E, int H, int W, const uint16_t* d2, int R, int32_t* out, void* stream);

/* Spur and small-component pruning of a graph and its chains (config key GRAPH_CLEAN; an extension).  One additive entry;
 * the ABI number stays 11 because nothing existing changes, and a run without the key does not call it.  Nothing is read back.
 *
 * Tables as srh_graph_edge_stats takes them (the host copy is validated, the 4-byte aligned device copy is read and never written), N and
 * E at most SRH_GRAPH_CLEAN_MAX_ITEMS = 2^26.  The graph is a multigraph: self-loops and parallel edges count as they stand.  The rule is
 * that of sam_road_amd/graph_clean.py, in integers: len_q(e) = floor(16 sqrt(dr^2 + dc^2)); a chain is a class of live edges under "share
 * a node of degree exactly 2", its id the smallest edge index; a component's id is its smallest node index.  In each of `rounds` rounds
 * (1 .. SRH_GRAPH_CLEAN_MAX_ROUNDS), all at once on the graph the round before left, a live edge is dropped if its chain has one end of
 * degree 1, one of degree >= 3 and a 64-bit length sum < spur_q (a spur), or if its component's 64-bit length sum is < comp_q; a
 * threshold of 0 is not stated and its test never holds.  spur_q, comp_q: ceil(16 s), ceil(16 c) for thresholds in pixels.
 *   state_out u8 [E] on the device: 0 kept, else 4 * round + 1 (spur) + 2 (small component)
 *   out int32 [E, 4] on the device, 16-byte aligned: {chain, component, min(chain length, 2^31 - 1), min(component length, 2^31 - 1)} of
 *       one more pass over the kept graph, ids in the indices given; {-1, -1, 0, 0} for a dropped edge
 * Every element of both is defined after the call and nothing else of the caller's is written.  Integer sums: the same numbers in any
 * order.  5 (rounds + 1) launches whatever the graph holds — init, edges, chains, sums, decide per pass — over a workspace of the context
 * of 24 N + 25 E bytes that grows on demand; the entry holds a lock of the context from the workspace's growth to the last launch and a
 * call waits on the device for the call before it, so it may be called from several threads on several streams.  E = 0 is SRH_OK and
 * launches nothing (state_out and out may then be NULL).  SRH_ERR_BAD_ARG, and nothing is launched, for every condition
 * srh_graph_edge_stats refuses of its tables, N or E above 2^26, rounds outside 1 .. 8, a negative threshold, a null state_out or out
 * with E > 0, an out that is not 16-byte aligned, or an output overlapping an input, the other output or the workspace.  Profiler rows:
 * graph_clean_init, graph_clean_edges, graph_clean_chains, graph_clean_sums, graph_clean_decide. */
#define SRH_GRAPH_CLEAN_MAX_ROUNDS 8
#define SRH_GRAPH_CLEAN_MAX_ITEMS (1 << 26)
int srh_graph_clean(srh_ctx* ctx, const int32_t* nodes_host, const int32_t* nodes_dev, int N, const int32_t* edges_host,
                    const int32_t* edges_dev, int E, int64_t spur_q, int64_t comp_q, int rounds, uint8_t* state_out, int32_t* out,
                    void* stream);

/* GeoTIFF scenes (config key GEOTIFF; an extension).  Two additive entries, srh_tiff_assemble here and the host entry
 * srh_tiff_lzw_decode below; the ABI number stays 11 because nothing existing changes, and a run without the key calls neither.
 *
 * srh_tiff_assemble: the DECOMPRESSED strips or tiles of a TIFF, as the file holds them, -> the raster out [H, W, C] on the device, samples
 * of dtype SRH_U8, SRH_U16 or SRH_F32 (moved as bit patterns) in native byte order.  flat: flat_bytes bytes on the device, 16-byte
 * aligned.  The table, int64 [n_seg, 7], is given twice, as for srh_mask_clean: table_host is validated and sizes the launch, table_dev is
 * what the kernel reads.  Row k: {OFF, BYTES, ROW0, COL0, ROWS, COLS, BAND}: the segment lies at flat + OFF (a multiple of 16) and covers
 * rows ROW0 .. ROW0 + ROWS - 1 and columns COL0 .. COL0 + COLS - 1 — those outside the raster are padding and are never stored; BAND -1:
 * ROWS x COLS pixels of C interleaved samples, BAND b: ROWS x COLS samples of band b.  BYTES = ROWS x COLS x (C or 1) x sample size.
 * predictor 1: none; 2 (SRH_U8, SRH_U16): every sample is the wrapping difference to the sample of the same band one pixel to the left in
 * the segment's row; 3 (SRH_F32): TIFF Technical Note 3, the row's four byte planes, most significant first, differenced bytewise with
 * stride C (1 for a band segment) over the whole row.  big_endian 1: the samples of predictor 1 and 2 are byte-swapped first.
 * One launch whatever the file holds: a workgroup per row of a segment, an exact parallel prefix sum in wrapping integers (shuffles in a
 * wave, LDS across waves, fixed-size chunks with a carried total: LDS does not depend on W), 16-byte stores where a chunky row's
 * alignment allows, no atomics, nothing read back.  The pixels no segment covers are not written.  It equals tiff_read_ref of
 * sam_road_amd/geotiff.py bit for bit.  SRH_ERR_BAD_ARG, and nothing is launched, for a null argument, H or W < 1 or H W > 2^31 - 1, C
 * outside 1 .. 16, another dtype, a predictor that does not go with the dtype, n_seg < 1, a misaligned flat, out or device table, an out
 * that overlaps an input, or a host table in which a segment leaves flat or starts outside the raster, OFF is no multiple of 16, BAND
 * lies outside -1 .. C - 1 or BYTES is not the product above.  Profiler row: tiff_assemble. */
int srh_tiff_assemble(srh_ctx* ctx, const uint8_t* flat, int64_t flat_bytes, const int64_t* table_host, const int64_t* table_dev, int n_seg,
                      void* out, int H, int W, int C, int dtype, int predictor, int big_endian, void* stream);

/* op level(used by the parity tests to localise a failure; same kernels as above) ----------------- */

/* out = act(A[M,K] W[N,K]^T + bias) (+resid); A,W fp16; N%128==0, K%64==0. act: 0/1 GELU/2 ReLU. */
int srh_op_gemm(srh_ctx* ctx, const void* A_f16, const void* W_f16, const float* bias, const float* resid,
                int M, int N, int K, int act, float* out_f32, void* out_f16, void* stream);
/* The same with the operand layouts the model uses between fc1 and fc2 of a ViT block (reference model.py:245-258 through the SAM
 * fork's MLPBlock: lin2(act(lin1(x)))): the MLP's hidden activation is kept in the BLOCKED-16 layout — 1 KiB blocks of 32 rows x 16
 * columns, element (m, n) at fp16 index ((m/32)*(cols/16) + n/16)*512 + ((n%16)/8)*256 + (m%32)*8 + n%8.  flags: SRH_GEMM_A_BLOCKED16
 * = A_f16 is in that layout, SRH_GEMM_OUT_BLOCKED16 = out_f16 is written in it.  Only the persistent 256x192 kernel understands the
 * layout: M % 256 == 0, N % 192 == 0, K % 768 == 0, >= 128 tiles, a bias, fp16 output only, (A blocked, act 0) or (out blocked, act 1
 * GELU); anything else returns SRH_ERR_UNSUPPORTED.  flags == 0 is srh_op_gemm. */
#define SRH_GEMM_A_BLOCKED16 1
#define SRH_GEMM_OUT_BLOCKED16 2
int srh_op_gemm_ex(srh_ctx* ctx, const void* A_f16, const void* W_f16, const float* bias, const float* resid,
                   int M, int N, int K, int act, float* out_f32, void* out_f16, int flags, void* stream);
/* Device bytes the context owns right now (activation / scene / TopoNet workspaces, the GEMM tile-table slab): grows only when a larger
 * batch is first seen, flat in steady state — what tests/test_gpu_ops.py::test_ctx_memory_is_flat_over_batch_sizes watches. */
size_t srh_ctx_device_bytes(const srh_ctx* ctx);
/* 3x3 pad-1 conv over channels-last [B,S,S,C] as implicit GEMM; W_f16 [N, 9*C] (k = tap*C + c). */
int srh_op_conv3x3(srh_ctx* ctx, const void* A_f16, const void* W_f16, int B, int S, int C, int N,
                   float* out_f32, void* stream);
int srh_op_layernorm(srh_ctx* ctx, const float* x, const float* gamma, const float* beta, float eps, int M,
                     int D, int gelu, float* out_f32, void* out_f16, void* stream);
/* The residual-stream passes (test-only; additive, the ABI stays 11).  The encoder keeps the residual stream x in f32 and folds the
 * residual adds of a ViT block (reference model.py:245-258 builds the SAM fork's ImageEncoderViT: Block.forward's x = shortcut + attn(..)
 * and x = x + mlp(norm2(x)), ImageEncoderViT.forward's x = patch_embed(x) + pos_embed; run at model.py:424 / :469) into the LayerNorm
 * pass that reads x next.  srh_op_layernorm_ex launches that pass with the parameter patterns srh_encode_decode produces (api_model.hip
 * encode_batch: block_ln, fold_pending and the neck's cast), every optional member 0 / NULL being srh_op_layernorm:
 *   delta16            x' = x + delta16 (fp16 [M,D]: proj, fc2 or the patch embedding when the persistent 256x192 GEMM wrote it) —
 *                      Block.forward's residual adds; block_ln with one branch pending;
 *   delta16 + delta16b x' = (x + delta16) + delta16b, the order in which Block.forward adds attention then MLP — the next block's norm1
 *                      when both branch GEMMs of a block took the 256x192 kernel (encode_batch's defer_x, ViT-B at large batch);
 *   x_period > 0       x has x_period rows and row m reads row m % x_period: pos_embed [S*S, D] as block 0's initial residual,
 *                      x' = pos_embed[token] + delta16 (the patch embedding) — block_ln while x_is_pos;
 *   slices             x' = ((slice 0 + slice 1 + ...) + slice_bias) + x over nslices f32 [M,D] partials slice_stride ELEMENTS apart:
 *                      the split-K partials of a deferred fc2 (srh_op_gemm_partials), in the reduce pass's order — ViT-L / ViT-H at
 *                      256 px; D = 1024 / 1280 only, not together with delta16, slice_bias required (else SRH_ERR_UNSUPPORTED);
 *   x_out              where x' is written ([M,D] f32; may be x itself when x_period == 0) — block_ln's write_x; NULL: x' is only normalised;
 *   gamma == NULL      cast-only: out_f16 = fp16(x') — the neck's first pass over the last block's output (no sentinel in this mode);
 *   nf_tag             -1: no sentinel; 0 .. 63: a row of x' whose variance is not finite sets the context's flag nf_tag, which
 *                      srh_ctx_check reports as SRH_ERR_NONFINITE naming encoder block nf_tag / 2, norm1 (even) / norm2 (odd).
 * SRH_ERR_BAD_ARG: delta16b without delta16, nf_tag outside -1 .. 63.  SRH_ERR_UNSUPPORTED: D not one of 128 / 256 / 768 / 1024 / 1280
 * and the slices cases above.  Nothing is launched in either case. */
typedef struct {
    const float* x; int32_t M, D, x_period;
    const float* gamma; const float* beta; float eps; int32_t gelu;
    const void* delta16; const void* delta16b; float* x_out;
    const float* slices; int32_t nslices; size_t slice_stride; const float* slice_bias;
    int32_t nf_tag;
    float* out_f32; void* out_f16;
} srh_op_norm_args;
int srh_op_layernorm_ex(srh_ctx* ctx, const srh_op_norm_args* args, void* stream);
/* The GEMM as a block's deferred fc2 runs it (encode_batch's branch_gemm with defer_reduce; Block.forward's mlp lin2): split-K into the
 * context's workspace, no reduce pass.  *partials = that workspace (device, f32 [*nslices, M, N], slice stride M * N, valid until the
 * next GEMM on the context), to be folded with `bias` by srh_op_layernorm_ex's slices.  SRH_ERR_UNSUPPORTED, nothing launched, for a
 * shape the dispatch runs without split-K. */
int srh_op_gemm_partials(srh_ctx* ctx, const void* A_f16, const void* W_f16, const float* bias, int M, int N, int K,
                         const float** partials, int* nslices, void* stream);
/* out_f32 = A W^T + bias + pos[m % pos_rows] (pos f32 [pos_rows, N]): the patch embedding plus pos_embed in the GEMM epilogue
 * (ImageEncoderViT.forward), as encode_batch runs it whenever the 256x192 kernel is not preferred for that layer. */
int srh_op_gemm_pos(srh_ctx* ctx, const void* A_f16, const void* W_f16, const float* bias, const float* pos, int pos_rows,
                    int M, int N, int K, float* out_f32, void* stream);
/* SAM attention on a fused qkv tensor [B*S*S, 3*heads*64] fp16: rel-pos tables [2*win-1, 64] fp16,
 * qkv bias fp16 [3*heads*64] (pad-key rows), win = 14 (windowed) or S (global). out fp16 [B*S*S, heads*64]. */
int srh_op_attention(srh_ctx* ctx, const void* qkv_f16, const void* relpos_h_f16, const void* relpos_w_f16,
                     const void* bias_qkv_f16, int B, int S, int heads, int win, void* out_f16, void* stream);
/* The same with the head dim as an argument: 64 (ViT-B / ViT-L) or 80 (ViT-H, toponet_vith_256.yaml;
 * windows of 14 on any S, or the 16x16 global window).  Tables [2*win-1, head_dim], scale head_dim^-0.5
 * (segment_anything Attention.__init__, model.py:245-258 instantiates it with the checkpoint's dims). */
int srh_op_attention_hd(srh_ctx* ctx, const void* qkv_f16, const void* relpos_h_f16, const void* relpos_w_f16,
                        const void* bias_qkv_f16, int B, int S, int heads, int head_dim, int win,
                        void* out_f16, void* stream);

/* The heads after the encoder (test-only; the launches and parameters of srh_encode_decode / srh_toponet):
 *   srh_op_map_decoder: the fused map_decoder of `w` (naive decoder, S = patch_size / 16) on a neck output emb_f16 [B*S*S, 256] fp16
 *     -> mask_logits / mask_scores [B,P,P,2] f32, both nullable;
 *   srh_op_sample: BilinearSampler over emb_f32 [n_tiles,h,w,C] channels-last (C % 4 == 0) at points [B,N,2] (SRH_F32 / SRH_I64) in
 *     pixels of a `patch`-px tile; point_tile i32 [B*N] (nullable: point i samples tile i / N, B <= n_tiles; else clamped into
 *     [0, n_tiles)) -> out_f32 / out_f16 [B*N, C] (at least one);
 *   srh_op_pair_gather: pair rows [B*Ns*K, ld] fp16 = src | tgt features of pf_f16 [B*N,128] | dx dy (0 with zero_offset) | 0, pairs
 *     [B,Ns,K,2] (SRH_I32 / SRH_I64) minus index_base; a negative index wraps python-style only when index_base == 0;
 *   srh_op_topo_trunk (additive, the ABI stays 11): the fused TopoNet trunk of `w` alone (pair_proj, the encoder layers of its
 *     TOPONET_VERSION, output_proj, sigmoid: srh_toponet's last launch and its parameter block) on pair rows pair_f16 [nseq*K, ld] fp16
 *     (16-byte aligned; ld >= 320, ld % 8 == 0; columns 258 .. 319 are read against zero weights and must be finite) and valid u8
 *     [nseq, K] (4-byte aligned; any non-zero byte counts) -> logits / scores f32 [nseq*K], both nullable.  SRH_ERR_BAD_ARG for a bad ld,
 *     a null or misaligned input; SRH_ERR_UNSUPPORTED for K outside 1 .. 64; nseq == 0 is a no-op.  Nothing is launched in these cases.
 *   srh_op_sam_decoder (additive, the ABI stays 11): the SAM MaskDecoder branch of `w` alone (USE_SAM_DECODER: the launch sequence
 *     srh_encode_decode runs after the neck, the same function) on a neck output emb_f32 [B*S*S, 256] f32, token-major -> mask_logits /
 *     mask_scores [B,P,P,2] f32, and two intermediates copied out of the context's workspace on the same stream: tokens_out [B,4,256]
 *     (the IoU token and the three mask tokens after norm_final_attn) and low_res [B,2,4S,4S] (the logits of mask tokens 1 and 2 before
 *     the bilinear x4 upsample).  All four outputs are nullable; with none it is a no-op.  SRH_ERR_UNSUPPORTED for weights packed without
 *     use_sam_decoder, SRH_ERR_BAD_ARG for a null ctx / weights / input or B <= 0; nothing is launched in these cases. */
int srh_op_map_decoder(srh_ctx* ctx, const srh_weights* w, const void* emb_f16, int B, float* mask_logits, float* mask_scores, void* stream);
int srh_op_sample(srh_ctx* ctx, const float* emb_f32, int n_tiles, int h, int w, int C, const void* points, int points_dtype,
                  const int32_t* point_tile, int B, int N, float patch, float* out_f32, void* out_f16, void* stream);
int srh_op_pair_gather(srh_ctx* ctx, const void* pf_f16, const void* points, int points_dtype, const void* pairs, int pairs_dtype,
                       int B, int N, int Ns, int K, int zero_offset, int64_t index_base, void* out_f16, int ld, void* stream);
int srh_op_topo_trunk(srh_ctx* ctx, const srh_weights* w, const void* pair_f16, int ld, const uint8_t* valid, int nseq, int K,
                      float* logits, float* scores, void* stream);
int srh_op_sam_decoder(srh_ctx* ctx, const srh_weights* w, const float* emb_f32, int B, float* mask_logits, float* mask_scores,
                       float* tokens_out, float* low_res, void* stream);

/* profiling --------------------------------------------------------------------------------------- */

/* When enabled, every kernel launch made by this ctx is bracketed by HIP events on the launch
 * stream.  srh_profile_read synchronises, then returns per-class totals since the last enable. */
typedef struct {
    char name[32];
    int64_t launches;
    double ms;          /* summed GPU time of the launches */
    double flops;       /* algorithmic FLOPs (2*M*N*K for GEMMs; q.k + p.v for attention), else 0 */
    double bytes;       /* algorithmic HBM bytes for bandwidth-bound classes, else 0 */
} srh_profile_row;
int srh_profile_enable(srh_ctx* ctx, int on);
int srh_profile_read(srh_ctx* ctx, srh_profile_row* rows, int max_rows, int* n_rows);
/* Calibration of the above: what an event pair around ONE launch adds beyond the time the kernel's waves run — median over 32
 * launches of a kernel that spins for exactly 50 us of the 100 MHz wall clock, minus those 50 us (dispatch, completion and the
 * marker packets; rocprofv3 counts most of it as kernel duration as well).  bench.py reports it next to its event-timed classes. */
int srh_profile_overhead(srh_ctx* ctx, void* stream, double* ms_per_launch);

/* ---- host-side geometry between the two GPU passes (no device work, callable without a GPU) ---------------
 * Greedy radius NMS of reference graph_utils.py:572-591 (nms_points), the step that turns the fused masks into
 * graph points (graph_extraction.py:130-139).  Candidates are given ALREADY in the reference's processing order
 * (np.argsort(scores)[::-1], computed by the caller so numpy's tie order is kept): xy int32 [n,2] (x,y),
 * force[i] = (score_i > 1.0).  Writes kept[i] in {0,1}.  Exact integer arithmetic, identical result to the
 * reference's KDTree loop. */
int srh_nms_points_host(const int32_t* xy, const uint8_t* force, int64_t n, int32_t radius, uint8_t* kept);

/* Pass-2 query builder for all tiles of a scene (reference inferencer.py:148-176: per-tile rtree box query + scipy
 * KDTree.query(k = K+1, distance_upper_bound = R)).  pts int64 [n,2] (x,y) graph points; boxes int32 [n_tiles,4]
 * (x0,y0,x1,y1), closed.  srh_pass2_count writes the number of points per tile; the caller builds
 * offsets = exclusive prefix sum and allocates ids [total] and knn [total,K]; srh_pass2_fill writes, per tile, the point
 * ids in ascending order and each point's K nearest other points of the tile (distance strictly < radius, ascending by
 * (distance, index); -1 = missing).  Where distances alone do not determine scipy's answer — the K-th and (K+1)-th neighbour
 * equidistant, or a point coinciding with the source — the row is decided exactly as `scipy.spatial.KDTree(tile points)
 * .query(p, k = K+1, distance_upper_bound = radius)[1:]` decides it (same kd-tree, traversal and heaps restated in
 * csrc/kdtree_emul.hpp; scipy 1.15) and comes in scipy's output order; ambiguous [total] marks those rows (information
 * only: nothing is left for the caller to recompute); local (nullable) int64 [total,2] receives every row's tile-local (x, y) =
 * point - (x0, y0), the coordinates TopoNet samples at (inferencer.py:151). */
int srh_pass2_count(const int64_t* pts, int64_t n, const int32_t* boxes, int32_t n_tiles, int64_t* counts);
int srh_pass2_fill(const int64_t* pts, int64_t n, const int32_t* boxes, int32_t n_tiles, int32_t K, int64_t radius,
                   const int64_t* offsets, int64_t* ids, int32_t* knn, uint8_t* ambiguous, int64_t* local, int32_t n_threads);

/* `scipy.spatial.KDTree(points, leafsize).query(queries, k, distance_upper_bound=r)` (the reference's kNN, inferencer.py:156-160)
 * restated for 2-D points, INCLUDING how scipy breaks ties between equidistant points: points f64 [n,2], queries f64 [nq,2] ->
 * out_idx i32 [nq,k] in scipy's output order (n where fewer than k points lie within r); tree_indices (nullable) i32 [n]
 * receives scipy's `tree.indices` permutation.  Host code; what srh_pass2_fill uses for tied cut-offs. */
int srh_kdtree_knn_host(const double* points, int64_t n, int32_t leafsize, const double* queries, int64_t nq, int32_t k,
                        double distance_upper_bound, int32_t* out_idx, int32_t* tree_indices);

/* Candidate pixels of a fused u8 mask: reference graph_extraction.py:24-28 (`np.where(mask > threshold)` and the scores
 * there), row-major order.  xy int64 [capacity,2] (x, y) and scores u8 [capacity] receive the candidates and *n their number;
 * if capacity is too small (or xy = scores = NULL) only *n is written (SRH_ERR_BAD_ARG in the former case): call again with
 * capacity >= *n.  n_threads worker threads scan bands of rows (count, prefix, write). */
int srh_mask_candidates(const uint8_t* mask, int32_t H, int32_t W, float threshold, int64_t* xy, uint8_t* scores,
                        int64_t capacity, int64_t* n, int32_t n_threads);

/* The last of the three nms_points calls of graph_extraction.py:130-139 together with the gathers in front of it: candidates =
 * [xy_a[ord_a]; xy_b[ord_b]] (keypoint, then road candidates, each in its np.argsort(scores)[::-1] order), visited in `order`
 * (np.argsort of the priorities [1]*na + [0]*nb, reversed — computed by the caller with numpy so that the tie order is the
 * reference's), no candidate forced; greedy radius suppression as srh_nms_points_host.  out_xy int64 [na+nb,2] receives the kept
 * points (x, y) in visiting order, *n_out their number. */
int srh_nms_merge_points(const int64_t* xy_a, const int64_t* ord_a, int64_t na, const int64_t* xy_b, const int64_t* ord_b, int64_t nb,
                         const int64_t* order, int32_t radius, int64_t* out_xy, int64_t* n_out);

/* Votes of one TopoNet batch in the reference's visiting order (inferencer.py:206-221: tile, source point, neighbour slot):
 * scores [nb, n_max, K] f32 host (NaN already replaced by -100), offsets [nb+1] rows of these tiles in ids / knn (the
 * srh_pass2_fill layout).  Appends keys[*count] = ids[src] * n_points + ids[tgt] and the float64 score, advances *count;
 * SRH_ERR_BAD_ARG if a valid pair's score is outside [0, 1] (the reference's assert, inferencer.py:219). */
int srh_pass2_votes(const float* scores, int32_t nb, int64_t n_max, int32_t K, const int64_t* offsets, const int64_t* ids,
                    const int32_t* knn, int64_t n_points, int64_t* keys, double* votes, int64_t capacity, int64_t* count);

/* Padded collate of one TopoNet batch (reference inferencer.py:179-185) from the flat arrays of srh_pass2_fill: tile b of the
 * batch owns rows offsets[b] .. offsets[b+1] of local [*,2] and knn [*,K]; writes points f32 [nb,n_max,2], pairs i32
 * [nb,n_max,K,2] (source row, target row — the source itself where invalid) and valid u8 [nb,n_max,K], zero beyond a tile's rows. */
int srh_pass2_pack(const int64_t* offsets, const int64_t* local, const int32_t* knn, int32_t nb, int64_t n_max, int32_t K,
                   float* points, int32_t* pairs, uint8_t* valid);
/* The unpadded collate for srh_toponet_ragged: rows keep their position in the flat query arrays (numbered from offsets[0]), pairs
 * index the flat list, point_tile[r] = the row's tile counted from the first tile of the range. */
int srh_pass2_pack_ragged(const int64_t* offsets, const int64_t* local, const int32_t* knn, int32_t n_tiles, int32_t K,
                          float* points, int32_t* pairs, uint8_t* valid, int32_t* point_tile);

/* Directed edge votes of pass 2 (reference inferencer.py:209-221: dict of score sums / counts keyed by (src, tgt), filled in
 * tile / point / slot order).  keys[i] = src * n_points + tgt, scores[i] in that visiting order.  Writes the unique keys in
 * ascending order with their float64 sums — accumulated in the reference's order, hence bit-identical to its loop — and
 * counts; out_first (nullable) receives the index i of each key's first vote, i.e. its insertion position in the reference's
 * dict, which fixes the order of the pred_edges list (inferencer.py:224-228); out arrays have capacity n. */
int srh_edge_vote_accumulate(const int64_t* keys, const double* scores, int64_t n, int64_t* out_keys, double* out_sums,
                             double* out_counts, int64_t* out_first, int64_t* n_unique);
/* The same with n_threads worker threads: the key space is cut into contiguous ranges of equal vote counts (one stable
 * partition pass), each sorted and accumulated by its own thread; identical outputs, bit for bit. */
int srh_edge_vote_accumulate_mt(const int64_t* keys, const double* scores, int64_t n, int64_t* out_keys, double* out_sums,
                                double* out_counts, int64_t* out_first, int64_t* n_unique, int32_t n_threads);

/* srh_pass2_votes + srh_edge_vote_accumulate in one pass over the query rows, without materialising the votes (reference
 * inferencer.py:206-228).  scores[b] = f32 [batch_nb[b], batch_n_max[b], K] host scores (NaN -> -100 done) of the tiles
 * batch_tile0[b] .. batch_tile0[b] + batch_nb[b] (indices into offsets [n_tiles+1]; ids / knn = the srh_pass2_fill layout; a tile
 * outside every batch must be empty).  Rows are grouped by source point and each point's votes are added, in the reference's
 * visiting order, into a table of its targets: same unique keys (ascending), float64 sums, counts and first-vote positions as the
 * two-call path, bit for bit.  capacity = number of non-negative knn entries always suffices.  SRH_ERR_BAD_ARG if a valid pair's
 * score is outside [0, 1] (the reference's assert, inferencer.py:219). */
int srh_pass2_vote_sums(const float* const* scores, const int32_t* batch_tile0, const int32_t* batch_nb, const int64_t* batch_n_max,
                        int32_t n_batches, int32_t K, const int64_t* offsets, int32_t n_tiles, const int64_t* ids, const int32_t* knn,
                        int64_t n_points, int64_t* out_keys, double* out_sums, double* out_counts, int64_t* out_first,
                        int64_t capacity, int64_t* n_unique, int32_t n_threads);

/* Edge list from the vote sums (reference inferencer.py:224-228): the (src, tgt) pairs whose mean score sums / max(counts, 1)
 * exceeds the threshold, in the insertion order of the reference's dict (ascending first-vote position; `first` values are
 * distinct).  out_edges int64 [n,2]; *n_edges their number. */
int srh_votes_to_edges(const int64_t* keys, const double* sums, const double* counts, const int64_t* first, int64_t n,
                       int64_t n_points, double threshold, int64_t* out_edges, int64_t* n_edges);

/* The LZW segments of a TIFF (config key GEOTIFF), decoded on host threads: codes most significant bit first, 9 to 12
 * bits, the width growing one code early, 256 = clear, 257 = end, as every current writer emits them.  Segment k is src[in_off[k] ..
 * in_off[k] + in_bytes[k]) and must decode to exactly out_bytes[k] bytes, written at dst + out_off[k]; n_threads workers take segments
 * from a shared counter.  Whatever a stream holds, nothing is read outside its input and nothing written outside its output.  Returns
 * 0, or k + 1 for the lowest k whose stream is damaged or holds fewer or more bytes (the other segments are decoded all the same), or
 * SRH_ERR_BAD_ARG for a null pointer, a negative size or a segment that leaves src or dst.  No device work. */
int srh_tiff_lzw_decode(const uint8_t* src, int64_t src_bytes, const int64_t* in_off, const int64_t* in_bytes, int64_t n, uint8_t* dst,
                        int64_t dst_bytes, const int64_t* out_off, const int64_t* out_bytes, int32_t n_threads);

#ifdef __cplusplus
}
#endif
#endif /* SAMROAD_HIP_H */
