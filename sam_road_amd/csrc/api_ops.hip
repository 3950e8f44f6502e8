// C ABI, test-only op-level entries (srh_op_*): single launchers on caller-supplied buffers.  Where the model path builds a parameter
// block through a ctx.hpp builder, the entry here uses the same one.
#include "ctx.hpp"

// ---- op level ------------------------------------------------------------------------------------------------
extern "C" int srh_op_gemm_ex(srh_ctx* c, const void* A, const void* W, const float* bias, const float* resid, int M,
                              int N, int K, int act, float* out_f32, void* out_f16, int flags, void* stream) {
    if (!c || !A || !W) return fail(c, SRH_ERR_BAD_ARG, "srh_op_gemm: null argument");
    if (flags & ~(SRH_GEMM_A_BLOCKED16 | SRH_GEMM_OUT_BLOCKED16)) return fail(c, SRH_ERR_BAD_ARG, "srh_op_gemm_ex: unknown flag");
    hipSetDevice(c->device);
    GemmParams g = gemm_nt((const f16*)A, (const f16*)W, M, N, K);
    g.bias = bias; g.resid = resid; g.ldr = N; g.act = act;
    g.out_f32 = out_f32; g.ldc = N; g.out_f16 = (f16*)out_f16; g.ldc16 = N;
    g.a_blocked16 = (flags & SRH_GEMM_A_BLOCKED16) != 0; g.out_blocked16 = (flags & SRH_GEMM_OUT_BLOCKED16) != 0;
    return gemm(c, "gemm_op", g, (hipStream_t)stream);
}

extern "C" int srh_op_gemm(srh_ctx* c, const void* A, const void* W, const float* bias, const float* resid, int M,
                           int N, int K, int act, float* out_f32, void* out_f16, void* stream) {
    return srh_op_gemm_ex(c, A, W, bias, resid, M, N, K, act, out_f32, out_f16, 0, stream);
}

extern "C" int srh_op_conv3x3(srh_ctx* c, const void* A, const void* W, int B, int S, int C, int N, float* out_f32,
                              void* stream) {
    if (!c || !A || !W || !out_f32) return fail(c, SRH_ERR_BAD_ARG, "srh_op_conv3x3: null argument");
    hipSetDevice(c->device);
    GemmParams g = gemm_nt((const f16*)A, (const f16*)W, B * S * S, N, 9 * C);
    g.lda = C; g.conv_S = S; g.conv_C = C; g.out_f32 = out_f32; g.ldc = N;
    return gemm(c, "gemm_op", g, (hipStream_t)stream);
}

extern "C" int srh_op_layernorm(srh_ctx* c, const float* x, const float* gamma, const float* beta, float eps, int M,
                                int D, int gelu, float* out_f32, void* out_f16, void* stream) {
    if (!c || !x) return fail(c, SRH_ERR_BAD_ARG, "srh_op_layernorm: null argument");
    hipSetDevice(c->device);
    NormParams ln;
    ln.x = x; ln.M = M; ln.D = D; ln.gamma = gamma; ln.beta = beta; ln.eps = eps; ln.act = gelu;
    ln.out_f32 = out_f32; ln.out_f16 = (f16*)out_f16;
    hipStream_t s = (hipStream_t)stream;
    TRYK(c, "layernorm", 0, 0, s, launch_layernorm(ln, s));
    return 0;
}

// The residual-stream passes at op level: the NormParams patterns of encode_batch's block_ln / fold_pending / neck cast, and the two
// GEMM modes that feed them (branch_gemm's deferred split-K, the patch embedding's f32 + pos epilogue), on caller-supplied buffers.
extern "C" int srh_op_layernorm_ex(srh_ctx* c, const srh_op_norm_args* a, void* stream) {
    if (!c || !a || !a->x) return fail(c, SRH_ERR_BAD_ARG, "srh_op_layernorm_ex: null argument");
    if (a->delta16b && !a->delta16) return fail(c, SRH_ERR_BAD_ARG, "srh_op_layernorm_ex: delta16b needs delta16 (it is folded after it)");
    if (a->nf_tag < -1 || a->nf_tag >= NF_NECK) return fail(c, SRH_ERR_BAD_ARG, "srh_op_layernorm_ex: nf_tag must be -1 (no sentinel) or 0 to 63");
    if (a->M < 0 || a->x_period < 0 || a->nslices < 0) return fail(c, SRH_ERR_BAD_ARG, "srh_op_layernorm_ex: bad sizes");
    hipSetDevice(c->device);
    NormParams ln;
    ln.x = a->x; ln.M = a->M; ln.D = a->D; ln.x_period = a->x_period;
    ln.gamma = a->gamma; ln.beta = a->beta; ln.eps = a->eps; ln.act = a->gelu;
    ln.delta16 = (const f16*)a->delta16; ln.delta16b = (const f16*)a->delta16b; ln.x_out = a->x_out;
    ln.slices = a->slices; ln.nslices = a->nslices; ln.slice_stride = a->slice_stride; ln.slice_bias = a->slice_bias;
    if (a->nf_tag >= 0) { ln.nf = c->nf_dev; ln.nf_tag = a->nf_tag; }
    ln.out_f32 = a->out_f32; ln.out_f16 = (f16*)a->out_f16;
    hipStream_t s = (hipStream_t)stream;
    TRYK(c, "layernorm", 0, 0, s, launch_layernorm(ln, s));
    return 0;
}

extern "C" int srh_op_gemm_partials(srh_ctx* c, const void* A, const void* W, const float* bias, int M, int N, int K,
                                    const float** partials, int* nslices, void* stream) {
    if (!c || !A || !W || !partials || !nslices) return fail(c, SRH_ERR_BAD_ARG, "srh_op_gemm_partials: null argument");
    *partials = nullptr; *nslices = 0;
    hipSetDevice(c->device);
    GemmParams g = gemm_nt((const f16*)A, (const f16*)W, M, N, K);   // branch_gemm's gp: f32 in-place residual epilogue, which the deferred reduce leaves to the caller
    g.bias = bias;
    g.resid = c->x.as<float>(); g.ldr = N; g.out_f32 = c->x.as<float>(); g.ldc = N;   // named, never touched: the partials are the only output
    const int sk = gemm_splitk_factor(g);         // what gemm() splits by
    if (sk <= 1) return fail(c, SRH_ERR_UNSUPPORTED, "srh_op_gemm_partials: this shape runs without split-K");
    g.defer_reduce = 1;
    TRY(gemm(c, "gemm_op", g, (hipStream_t)stream));
    *partials = c->split_ws.as<float>(); *nslices = sk;
    return 0;
}

extern "C" int srh_op_gemm_pos(srh_ctx* c, const void* A, const void* W, const float* bias, const float* pos, int pos_rows,
                               int M, int N, int K, float* out_f32, void* stream) {
    if (!c || !A || !W || !pos || !out_f32) return fail(c, SRH_ERR_BAD_ARG, "srh_op_gemm_pos: null argument");
    if (pos_rows <= 0) return fail(c, SRH_ERR_BAD_ARG, "srh_op_gemm_pos: pos_rows must be positive");
    hipSetDevice(c->device);
    GemmParams g = gemm_nt((const f16*)A, (const f16*)W, M, N, K);
    g.bias = bias; g.pos = pos; g.pos_rows = pos_rows; g.out_f32 = out_f32; g.ldc = N;
    return gemm(c, "gemm_op", g, (hipStream_t)stream);
}

// The heads after the encoder at op level: the same launchers, with the parameter blocks of the model path (encode_batch, toponet_impl:
// the builders of ctx.hpp), on caller-supplied inputs.
extern "C" int srh_op_map_decoder(srh_ctx* c, const srh_weights* w, const void* emb_f16, int B, float* mask_logits, float* mask_scores,
                                  void* stream) {
    if (!c || !w || !emb_f16 || B <= 0) return fail(c, SRH_ERR_BAD_ARG, "srh_op_map_decoder: bad argument");
    if (w->cfg.use_sam_decoder || !w->dec_frags) return fail(c, SRH_ERR_UNSUPPORTED, "srh_op_map_decoder: the weights have no naive map_decoder");
    if (!mask_logits && !mask_scores) return 0;
    hipSetDevice(c->device);
    hipStream_t s = (hipStream_t)stream;
    const DecodeFusedParams dp = decode_params(c, w, (const f16*)emb_f16, B, mask_logits, mask_scores);
    TRYK(c, "map_decoder", 0, 0, s, launch_decode_fused(dp, s));
    return 0;
}

// The SAM MaskDecoder branch alone: encode_batch's sam_decode() on a caller-supplied neck output, plus two of its intermediates copied
// out of the workspace behind it on the same stream (the queries after norm_final_attn, sd_mask's low-res logits before the upsample).
extern "C" int srh_op_sam_decoder(srh_ctx* c, const srh_weights* w, const float* emb_f32, int B, float* mask_logits, float* mask_scores,
                                  float* tokens_out, float* low_res, void* stream) {
    if (!c || !w || !emb_f32 || B <= 0) return fail(c, SRH_ERR_BAD_ARG, "srh_op_sam_decoder: bad argument");
    if (!w->cfg.use_sam_decoder) return fail(c, SRH_ERR_UNSUPPORTED, "srh_op_sam_decoder: the weights were packed without use_sam_decoder");
    if (!mask_logits && !mask_scores && !tokens_out && !low_res) return 0;
    hipSetDevice(c->device);
    hipStream_t s = (hipStream_t)stream;
    TRY(sam_decode(c, w, B, emb_f32, mask_logits, mask_scores, s));
    hipError_t e = hipSuccess;
    if (tokens_out) e = hipMemcpyAsync(tokens_out, c->sd_tok.as<float>(), (size_t)B * 4 * 256 * 4, hipMemcpyDeviceToDevice, s);
    if (e == hipSuccess && low_res)
        e = hipMemcpyAsync(low_res, c->sd_low.as<float>(), (size_t)B * 2 * 16 * w->S * w->S * 4, hipMemcpyDeviceToDevice, s);
    return e == hipSuccess ? 0 : hip_fail(c, e, "srh_op_sam_decoder");
}

extern "C" int srh_op_sample(srh_ctx* c, const float* emb_f32, int n_tiles, int h, int w, int C, const void* points, int points_dtype,
                             const int32_t* point_tile, int B, int N, float patch, float* out_f32, void* out_f16, void* stream) {
    if (!c || !emb_f32 || !points || (!out_f32 && !out_f16)) return fail(c, SRH_ERR_BAD_ARG, "srh_op_sample: null argument");
    if (points_dtype != SRH_I64 && points_dtype != SRH_F32) return fail(c, SRH_ERR_BAD_ARG, "srh_op_sample: points dtype must be i64 or f32");
    if (B < 0 || N < 0 || h <= 0 || w <= 0 || C <= 0 || C % 4 || n_tiles <= 0 || !(patch > 0.f))
        return fail(c, SRH_ERR_BAD_ARG, "srh_op_sample: bad sizes (C must be a multiple of 4)");
    if (!point_tile && B > n_tiles) return fail(c, SRH_ERR_BAD_ARG, "srh_op_sample: without point_tile, batch b samples tile b: B must be <= n_tiles");
    hipSetDevice(c->device);
    hipStream_t s = (hipStream_t)stream;
    const SampleParams sp = sample_params(emb_f32, n_tiles, h, w, C, points, points_dtype, point_tile, B, N, patch, out_f32, (f16*)out_f16);
    TRYK(c, "bilinear_sample", 0, 0, s, launch_sample(sp, s));
    return 0;
}

extern "C" int srh_op_pair_gather(srh_ctx* c, const void* pf_f16, const void* points, int points_dtype, const void* pairs, int pairs_dtype,
                                  int B, int N, int Ns, int K, int zero_offset, int64_t index_base, void* out_f16, int ld, void* stream) {
    if (!c || !pf_f16 || !points || !pairs || !out_f16) return fail(c, SRH_ERR_BAD_ARG, "srh_op_pair_gather: null argument");
    if (points_dtype != SRH_I64 && points_dtype != SRH_F32) return fail(c, SRH_ERR_BAD_ARG, "srh_op_pair_gather: points dtype must be i64 or f32");
    if (pairs_dtype != SRH_I64 && pairs_dtype != SRH_I32) return fail(c, SRH_ERR_BAD_ARG, "srh_op_pair_gather: pairs dtype must be i64 or i32");
    if (B < 0 || N <= 0 || Ns < 0 || K <= 0) return fail(c, SRH_ERR_BAD_ARG, "srh_op_pair_gather: bad sizes");
    hipSetDevice(c->device);
    hipStream_t s = (hipStream_t)stream;
    const PairGatherParams pg = pair_gather_params((const f16*)pf_f16, points, points_dtype, pairs, pairs_dtype, B, N, Ns, K, zero_offset != 0,
                                                   (long)index_base, (f16*)out_f16, ld);
    TRYK(c, "pair_gather", 0, 0, s, launch_pair_gather(pg, s));
    return 0;
}

// The fused TopoNet trunk alone (topo_fused.hip: pair_proj, the encoder layers, output_proj, sigmoid) on caller-supplied pair rows.
// The kernel reads rows as 16-byte vectors up to column 320 and, at K = 16, the valid bytes four at a time: hence the alignment rules.
extern "C" int srh_op_topo_trunk(srh_ctx* c, const srh_weights* w, const void* pair_f16, int ld, const uint8_t* valid, int nseq, int K,
                                 float* logits, float* scores, void* stream) {
    if (!c || !w || !pair_f16 || !valid) return fail(c, SRH_ERR_BAD_ARG, "srh_op_topo_trunk: null argument");
    if (ld < 320 || ld % 8 != 0) return fail(c, SRH_ERR_BAD_ARG, "srh_op_topo_trunk: ld must be a multiple of 8 and at least 320");
    if (((uintptr_t)pair_f16 & 15) || ((uintptr_t)valid & 3))
        return fail(c, SRH_ERR_BAD_ARG, "srh_op_topo_trunk: pair rows must be 16-byte aligned and valid 4-byte aligned");
    if (K < 1 || K > 64) return fail(c, SRH_ERR_UNSUPPORTED, "srh_op_topo_trunk: K (MAX_NEIGHBOR_QUERIES) must be 1 to 64");
    if (nseq < 0 || (int64_t)nseq * K > 0x7fffffffLL) return fail(c, SRH_ERR_BAD_ARG, "srh_op_topo_trunk: bad sequence count");
    if (!w->tp_stream || !w->tp_params) return fail(c, SRH_ERR_UNSUPPORTED, "srh_op_topo_trunk: the weights have no packed trunk");
    if (nseq == 0 || (!logits && !scores)) return 0;
    hipSetDevice(c->device);
    hipStream_t s = (hipStream_t)stream;
    const TopoFusedParams tf = topo_fused_params(w, (const f16*)pair_f16, ld, valid, nseq, K, logits, scores);
    TRYK(c, "topo_fused", 0, 0, s, launch_topo_fused(tf, s));
    return 0;
}

static int op_attention_impl(srh_ctx* c, const char* who, const void* qkv, const void* rel_h, const void* rel_w, const void* bias_qkv,
                             int B, int S, int heads, int hd, int win, void* out, void* stream) {
    if (!c || !qkv || !rel_h || !rel_w || !bias_qkv || !out) return fail(c, SRH_ERR_BAD_ARG, std::string(who) + ": null argument");
    if (hd != 64 && hd != 80) return fail(c, SRH_ERR_BAD_ARG, std::string(who) + ": head dim must be 64 or 80");
    hipSetDevice(c->device);
    hipStream_t s = (hipStream_t)stream;
    const AttnParams ap = attn_params((const f16*)qkv, (const f16*)rel_h, (const f16*)rel_w, (const f16*)bias_qkv, (f16*)out, B, S, heads, hd, win);
    TRYK(c, "attention", attn_flops(B, S, heads, hd, win), 0, s, launch_attention(ap, s));
    return 0;
}

extern "C" int srh_op_attention(srh_ctx* c, const void* qkv, const void* rel_h, const void* rel_w, const void* bias_qkv,
                                int B, int S, int heads, int win, void* out, void* stream) {
    return op_attention_impl(c, "srh_op_attention", qkv, rel_h, rel_w, bias_qkv, B, S, heads, 64, win, out, stream);
}

// head dim as an argument: 64 (ViT-B/L, attention.hip) or 80 (ViT-H, attention_hdx.hip)
extern "C" int srh_op_attention_hd(srh_ctx* c, const void* qkv, const void* rel_h, const void* rel_w, const void* bias_qkv,
                                   int B, int S, int heads, int hd, int win, void* out, void* stream) {
    return op_attention_impl(c, "srh_op_attention_hd", qkv, rel_h, rel_w, bias_qkv, B, S, heads, hd, win, out, stream);
}

// test-only: the weighted add of pass 1 on scores the caller supplies (f32 [n,P,P,2] on the device), all n tiles in one launch
extern "C" int srh_op_scene_fuse_window(srh_ctx* c, const float* scores, int n, int P, const int32_t* tile_xy, const float* profile,
                                        float* canvas_kp, float* canvas_road, int H, int W, void* stream) {
    if (!c || !scores || !tile_xy || !profile || !canvas_kp || !canvas_road)
        return fail(c, SRH_ERR_BAD_ARG, "srh_op_scene_fuse_window: null argument");
    if (n < 0 || !tile_size_ok(P) || H < P || W < P || !scene_dims_ok(H, W)) return fail(c, SRH_ERR_BAD_ARG, "srh_op_scene_fuse_window: bad sizes");
    if (n == 0) return 0;
    hipSetDevice(c->device);
    hipStream_t s = (hipStream_t)stream;
    TRYK(c, "scene_add_window", 0, (double)n * P * P * 8 * 3, s,
         launch_scene_add_window(scores, n, P, tile_xy, profile, canvas_kp, canvas_road, H, W, s));
    return 0;
}

// test-only: the A matrix of pass 1's crop for n tiles of size P in one orientation (0: the launch of every scene without TTA)
extern "C" int srh_op_patch_im2col(srh_ctx* c, const uint8_t* scene, int H, int W, const int32_t* tile_xy, int n, int P, int orient,
                                   void* out_f16, void* stream) {
    if (!c || !scene || !tile_xy || !out_f16) return fail(c, SRH_ERR_BAD_ARG, "srh_op_patch_im2col: null argument");
    if (n < 0 || n > 65535 || !tile_size_ok(P) || H < P || W < P || !scene_dims_ok(H, W) || orient < 0 || orient > 7)
        return fail(c, SRH_ERR_BAD_ARG, "srh_op_patch_im2col: bad sizes or orientation");
    if (n == 0) return 0;
    hipSetDevice(c->device);
    hipStream_t s = (hipStream_t)stream;
    PatchParams pp;
    pp.src = scene; pp.src_is_u8 = 1; pp.scene_W = W; pp.tile_xy = tile_xy; pp.B = n; pp.P = P; pp.out = (f16*)out_f16;
    const double bytes = (double)n * P * P * 3 * 3;
    if (orient) TRYK(c, "patch_im2col_oriented", 0, bytes, s, launch_patch_im2col_oriented(pp, H, orient, s));
    else TRYK(c, "patch_im2col", 0, bytes, s, launch_patch_im2col(pp, s));
    return 0;
}

// test-only: scores f32 [n,P,P,2] of oriented tiles -> the scene frame (orient 0: a plain copy; pass 1 launches nothing for id)
extern "C" int srh_op_scores_unorient(srh_ctx* c, const float* scores_in, int n, int P, int orient, float* scores_out, void* stream) {
    if (!c || !scores_in || !scores_out || scores_in == scores_out) return fail(c, SRH_ERR_BAD_ARG, "srh_op_scores_unorient: null or aliased argument");
    if (n < 0 || n > 65535 || !tile_size_ok(P) || orient < 0 || orient > 7) return fail(c, SRH_ERR_BAD_ARG, "srh_op_scores_unorient: bad sizes or orientation");
    if (n == 0) return 0;
    hipSetDevice(c->device);
    hipStream_t s = (hipStream_t)stream;
    if (orient == 0) {
        const hipError_t e = hipMemcpyAsync(scores_out, scores_in, (size_t)n * P * P * 8, hipMemcpyDeviceToDevice, s);
        return e == hipSuccess ? 0 : hip_fail(c, e, "srh_op_scores_unorient");
    }
    TRYK(c, "scores_unorient", 0, (double)n * P * P * 8 * 2, s, launch_scores_unorient(scores_in, n, P, orient, scores_out, s));
    return 0;
}

