// C ABI, scene level: pass 1 of infer_one_img over a resident scene (tile batches through encode_batch, api_model.hip) and the mask
// normalisation, with their nodata / FUSE_WINDOW / TTA variants.
#include "ctx.hpp"

// ---- scene level ------------------------------------------------------------------------------------------
static int scene_pass1_impl(srh_ctx* c, const char* who, const srh_weights* w, const uint8_t* scene, int H, int W,
                            const int32_t* tile_xy, int n_tiles, int B, float* canvas_kp, float* canvas_road,
                            float* embeddings_all, void* stream, bool has_window = false, const float* profile = nullptr,
                            const uint8_t* orients = nullptr, int k = 1) {
    if (!c || !w || !scene || !tile_xy || !canvas_kp || !canvas_road || !embeddings_all || (has_window && !profile))
        return fail(c, SRH_ERR_BAD_ARG, std::string(who) + ": null argument");
    if (n_tiles < 0 || B <= 0 || H < w->cfg.patch_size || W < w->cfg.patch_size || !scene_dims_ok(H, W))
        return fail(c, SRH_ERR_BAD_ARG, std::string(who) + ": bad sizes");
    TRY(nonfinite_check(c, who));
    hipSetDevice(c->device);
    hipStream_t s = (hipStream_t)stream;
    const int P = w->cfg.patch_size;
    if (c->scores_ws.ensure((size_t)B * P * P * 2 * 4)) return fail(c, SRH_ERR_HIP, "scores workspace allocation failed");
    const size_t emb_per_tile = (size_t)w->S * w->S * 256;
    if (k > 1 && n_tiles > 0) {       // TTA: an oriented batch's scores before the un-orient, and its embeddings, which nobody reads
        const size_t nb_max = (size_t)std::min(B, n_tiles);
        if (c->tta_scores_ws.ensure(nb_max * P * P * 2 * 4)) return fail(c, SRH_ERR_HIP, "TTA scores workspace allocation failed");
        if (c->emb_ws.ensure(nb_max * emb_per_tile * 4)) return fail(c, SRH_ERR_HIP, "TTA embeddings workspace allocation failed");
    }
    for (int j = 0; j < k; ++j) {     // summation order (orientation, tile); k == 1: the loop of every earlier ABI
        const int orient = orients ? orients[j] : 0;
        for (int off = 0; off < n_tiles; off += B) {
            const int nb = std::min(B, n_tiles - off);
            PatchParams pp;
            pp.src = scene; pp.src_is_u8 = 1; pp.scene_W = W; pp.tile_xy = tile_xy + 2 * off;
            const float* scores = c->scores_ws.as<float>();
            if (orient) {             // oriented crop -> the same encoder and decoder -> scores back to the scene frame (scene_tta.hip)
                TRY(encode_batch(c, w, pp, nb, nullptr, c->tta_scores_ws.as<float>(), c->emb_ws.as<float>(), s, orient, H));
                TRYK(c, "scores_unorient", 0, (double)nb * P * P * 8 * 2, s,
                     launch_scores_unorient(c->tta_scores_ws.as<float>(), nb, P, orient, c->scores_ws.as<float>(), s));
            } else {
                TRY(encode_batch(c, w, pp, nb, nullptr, c->scores_ws.as<float>(), embeddings_all + emb_per_tile * off, s));
            }
            if (has_window)      // FUSE_WINDOW (scene_window.hip): only this launch differs, the encoder and decoder are the same calls
                TRYK(c, "scene_add_window", 0, (double)nb * P * P * 8 * 3, s,
                     launch_scene_add_window(scores, nb, P, tile_xy + 2 * off, profile, canvas_kp, canvas_road, H, W, s));
            else
                TRYK(c, "scene_add", 0, (double)nb * P * P * 8 * 3, s,
                     launch_scene_add(scores, nb, P, tile_xy + 2 * off, canvas_kp, canvas_road, H, W, s));
        }
    }
    return 0;
}

extern "C" int srh_scene_pass1_hw(srh_ctx* c, const srh_weights* w, const uint8_t* scene, int H, int W, const int32_t* tile_xy,
                                  int n_tiles, int B, float* canvas_kp, float* canvas_road, float* embeddings_all,
                                  void* stream) {
    return scene_pass1_impl(c, "srh_scene_pass1_hw", w, scene, H, W, tile_xy, n_tiles, B, canvas_kp, canvas_road, embeddings_all, stream);
}

extern "C" int srh_scene_pass1(srh_ctx* c, const srh_weights* w, const uint8_t* scene, int S, const int32_t* tile_xy,
                               int n_tiles, int B, float* canvas_kp, float* canvas_road, float* embeddings_all,
                               void* stream) {
    return scene_pass1_impl(c, "srh_scene_pass1", w, scene, S, S, tile_xy, n_tiles, B, canvas_kp, canvas_road, embeddings_all, stream);
}

// valid (has_valid): the masks are also 0 on nodata — only the LAST launch differs; without it the two launches of every earlier ABI
static int scene_normalise_impl(srh_ctx* c, const char* who, const float* canvas_kp, const float* canvas_road, int H, int W,
                                const int32_t* tile_xy, int n_tiles, int P, uint8_t* kp_u8, uint8_t* road_u8, void* stream,
                                bool has_valid = false, const uint8_t* valid = nullptr) {
    if (!c || !canvas_kp || !canvas_road || !tile_xy || !kp_u8 || !road_u8 || (has_valid && !valid))
        return fail(c, SRH_ERR_BAD_ARG, std::string(who) + ": null argument");
    if (!scene_dims_ok(H, W) || n_tiles < 0 || P <= 0) return fail(c, SRH_ERR_BAD_ARG, std::string(who) + ": bad sizes");
    hipSetDevice(c->device);
    hipStream_t s = (hipStream_t)stream;
    const size_t npx = (size_t)H * W;
    if (c->counter.ensure(npx * 4)) return fail(c, SRH_ERR_HIP, "counter allocation failed");
    TRYK(c, "scene_count", 0, (double)npx * 4, s, launch_scene_count(c->counter.as<float>(), H, W, tile_xy, n_tiles, P, s));
    SceneNormParams np;
    np.canvas_kp = canvas_kp; np.canvas_road = canvas_road; np.counter = c->counter.as<float>();
    np.kp_u8 = kp_u8; np.road_u8 = road_u8; np.n = (int)npx;
    if (has_valid) TRYK(c, "scene_norm_valid", 0, (double)npx * 15, s, launch_scene_normalise_valid(np, valid, s));
    else TRYK(c, "scene_normalise", 0, (double)npx * 14, s, launch_scene_normalise(np, s));
    return 0;
}

extern "C" int srh_scene_normalise_hw(srh_ctx* c, const float* canvas_kp, const float* canvas_road, int H, int W,
                                      const int32_t* tile_xy, int n_tiles, int P, uint8_t* kp_u8, uint8_t* road_u8,
                                      void* stream) {
    return scene_normalise_impl(c, "srh_scene_normalise_hw", canvas_kp, canvas_road, H, W, tile_xy, n_tiles, P, kp_u8, road_u8, stream);
}

extern "C" int srh_scene_normalise(srh_ctx* c, const float* canvas_kp, const float* canvas_road, int S,
                                   const int32_t* tile_xy, int n_tiles, int P, uint8_t* kp_u8, uint8_t* road_u8,
                                   void* stream) {
    return scene_normalise_impl(c, "srh_scene_normalise", canvas_kp, canvas_road, S, S, tile_xy, n_tiles, P, kp_u8, road_u8, stream);
}

// ---- scene level, validity mask (kernels in scene_valid.hip) -------------------------------------------------------------------
extern "C" int srh_scene_tile_valid(srh_ctx* c, const uint8_t* valid, int H, int W, const int32_t* tile_xy, int n_tiles, int P,
                                    int32_t* counts, void* stream) {
    if (!c || !valid || !tile_xy || !counts) return fail(c, SRH_ERR_BAD_ARG, "srh_scene_tile_valid: null argument");
    if (n_tiles < 0 || P < 32 || (P & 15) || H < P || W < P || !scene_dims_ok(H, W))
        return fail(c, SRH_ERR_BAD_ARG, "srh_scene_tile_valid: bad sizes");
    if (n_tiles == 0) return 0;
    hipSetDevice(c->device);
    hipStream_t s = (hipStream_t)stream;
    TRYK(c, "tile_valid_count", 0, (double)n_tiles * P * P, s, launch_tile_valid_count(valid, H, W, tile_xy, n_tiles, P, counts, s));
    return 0;
}

extern "C" int srh_scene_fill_invalid(srh_ctx* c, uint8_t* scene, const uint8_t* valid, int H, int W, int fill_r, int fill_g,
                                      int fill_b, void* stream) {
    if (!c || !scene || !valid) return fail(c, SRH_ERR_BAD_ARG, "srh_scene_fill_invalid: null argument");
    if (!scene_dims_ok(H, W) || ((fill_r | fill_g | fill_b) & ~255)) return fail(c, SRH_ERR_BAD_ARG, "srh_scene_fill_invalid: bad sizes or fill colour");
    hipSetDevice(c->device);
    hipStream_t s = (hipStream_t)stream;
    TRYK(c, "scene_fill_invalid", 0, (double)H * W, s, launch_scene_fill_invalid(scene, valid, H, W, fill_r, fill_g, fill_b, s));
    return 0;
}

extern "C" int srh_scene_normalise_valid_hw(srh_ctx* c, const float* canvas_kp, const float* canvas_road, int H, int W,
                                            const int32_t* tile_xy, int n_tiles, int P, const uint8_t* valid, uint8_t* kp_u8,
                                            uint8_t* road_u8, void* stream) {
    return scene_normalise_impl(c, "srh_scene_normalise_valid_hw", canvas_kp, canvas_road, H, W, tile_xy, n_tiles, P, kp_u8, road_u8, stream,
                                true, valid);
}

// ---- scene level, window-weighted fusion (kernels in scene_window.hip, behaviour in DESIGN.md §6e) -----------------------------
extern "C" int srh_scene_pass1_window_hw(srh_ctx* c, const srh_weights* w, const uint8_t* scene, int H, int W, const int32_t* tile_xy,
                                         int n_tiles, int B, const float* profile, float* canvas_kp, float* canvas_road,
                                         float* embeddings_all, void* stream) {
    return scene_pass1_impl(c, "srh_scene_pass1_window_hw", w, scene, H, W, tile_xy, n_tiles, B, canvas_kp, canvas_road, embeddings_all, stream,
                            true, profile);
}

extern "C" int srh_scene_normalise_window_hw(srh_ctx* c, const float* canvas_kp, const float* canvas_road, int H, int W,
                                             const int32_t* tile_xy, int n_tiles, int P, const float* profile, const uint8_t* valid,
                                             uint8_t* kp_u8, uint8_t* road_u8, void* stream) {
    if (!c || !canvas_kp || !canvas_road || !tile_xy || !profile || !kp_u8 || !road_u8)
        return fail(c, SRH_ERR_BAD_ARG, "srh_scene_normalise_window_hw: null argument");
    if (!scene_dims_ok(H, W) || n_tiles < 0 || !tile_size_ok(P)) return fail(c, SRH_ERR_BAD_ARG, "srh_scene_normalise_window_hw: bad sizes");
    hipSetDevice(c->device);
    hipStream_t s = (hipStream_t)stream;
    const double npx = (double)H * W;
    // one kernel: the weight sum stays in a register (no counter canvas), so the context's counter workspace is not used
    TRYK(c, "scene_norm_window", 0, npx * (valid ? 11 : 10), s,
         launch_scene_normalise_window(canvas_kp, canvas_road, H, W, tile_xy, n_tiles, P, profile, valid, kp_u8, road_u8, s));
    return 0;
}

// ---- scene level, test-time augmentation over tile orientations (kernels in scene_tta.hip, behaviour in DESIGN.md §6f) ----------------
extern "C" int srh_scene_pass1_tta_hw(srh_ctx* c, const srh_weights* w, const uint8_t* scene, int H, int W, const int32_t* tile_xy,
                                      int n_tiles, int B, const uint8_t* orients, int k, const float* profile, float* canvas_kp,
                                      float* canvas_road, float* embeddings_all, void* stream) {
    if (!orients) return fail(c, SRH_ERR_BAD_ARG, "srh_scene_pass1_tta_hw: null argument");
    if (k < 1 || k > 8) return fail(c, SRH_ERR_BAD_ARG, "srh_scene_pass1_tta_hw: 1 to 8 orientations");
    unsigned seen = 0;
    for (int j = 0; j < k; ++j) {
        if (orients[j] > 7) return fail(c, SRH_ERR_BAD_ARG, "srh_scene_pass1_tta_hw: an orientation code is 0 to 7");
        if (seen & (1u << orients[j])) return fail(c, SRH_ERR_BAD_ARG, "srh_scene_pass1_tta_hw: an orientation is listed twice");
        seen |= 1u << orients[j];
    }
    if (orients[0] != 0) return fail(c, SRH_ERR_BAD_ARG, "srh_scene_pass1_tta_hw: the first orientation must be id (0): its embeddings feed pass 2");
    return scene_pass1_impl(c, "srh_scene_pass1_tta_hw", w, scene, H, W, tile_xy, n_tiles, B, canvas_kp, canvas_road, embeddings_all, stream,
                            profile != nullptr, profile, orients, k);
}


// ---- scene level, border padding (kernel in scene_pad.hip, behaviour in DESIGN.md §6g) ------------------------------------------------
static_assert(SRH_PAD_REFLECT == PAD_REFLECT && SRH_PAD_EDGE == PAD_EDGE && SRH_PAD_CONSTANT == PAD_CONSTANT, "pad modes of the header and the kernel");

extern "C" int srh_scene_pad(srh_ctx* c, const uint8_t* src, int H, int W, int C, int top, int bottom, int left, int right, int mode,
                             const int32_t* fill_rgb, uint8_t* dst, void* stream) {
    if (!c || !src || !dst || (mode == SRH_PAD_CONSTANT && !fill_rgb)) return fail(c, SRH_ERR_BAD_ARG, "srh_scene_pad: null argument");
    if ((C != 1 && C != 3) || mode < SRH_PAD_REFLECT || mode > SRH_PAD_CONSTANT) return fail(c, SRH_ERR_BAD_ARG, "srh_scene_pad: bad channel count or mode");
    const long long Hv = (long long)H + top + bottom, Wv = (long long)W + left + right;
    if (top < 0 || bottom < 0 || left < 0 || right < 0 || !scene_dims_ok(H, W) || Hv > 2147483647LL || Wv > 2147483647LL ||
        !scene_dims_ok((int)Hv, (int)Wv))
        return fail(c, SRH_ERR_BAD_ARG, "srh_scene_pad: bad sizes");
    if (fill_rgb && ((fill_rgb[0] | fill_rgb[1] | fill_rgb[2]) & ~255)) return fail(c, SRH_ERR_BAD_ARG, "srh_scene_pad: bad fill colour");
    hipSetDevice(c->device);
    hipStream_t s = (hipStream_t)stream;
    ScenePadParams p;
    p.src = src; p.dst = dst; p.H = H; p.W = W; p.Hv = (int)Hv; p.Wv = (int)Wv; p.top = top; p.left = left; p.C = C; p.mode = mode;
    if (fill_rgb) p.fill = (uint32_t)fill_rgb[0] | ((uint32_t)fill_rgb[1] << 8) | ((uint32_t)fill_rgb[2] << 16);
    TRYK(c, "scene_pad", 0, ((double)H * W + (double)Hv * Wv) * C, s, launch_scene_pad(p, s));
    return 0;
}

// ---- scene level, groups of small scenes (kernels in scene_group.hip, behaviour in DESIGN.md §6h) ---------------------------------------
extern "C" int srh_scene_group_pack(srh_ctx* c, const uint8_t* src, int64_t src_bytes, const int64_t* table_host, const int64_t* table_dev,
                                    int n, int C, int Ha, int Wa, int mode, const int32_t* fill_rgb, uint8_t* dst, void* stream) {
    if (!c || !src || !table_host || !table_dev || !dst || (mode == SRH_PAD_CONSTANT && !fill_rgb))
        return fail(c, SRH_ERR_BAD_ARG, "srh_scene_group_pack: null argument");
    if ((C != 1 && C != 3) || mode < SRH_PAD_REFLECT || mode > SRH_PAD_CONSTANT)
        return fail(c, SRH_ERR_BAD_ARG, "srh_scene_group_pack: bad channel count or mode");
    if (fill_rgb && ((fill_rgb[0] | fill_rgb[1] | fill_rgb[2]) & ~255)) return fail(c, SRH_ERR_BAD_ARG, "srh_scene_group_pack: bad fill colour");
    if (n < 1 || !scene_dims_ok(Ha, Wa) || !group_table_ok(table_host, n, C, Ha, Wa, src_bytes, false))
        return fail(c, SRH_ERR_BAD_ARG, "srh_scene_group_pack: bad sizes or an inconsistent table");
    hipSetDevice(c->device);
    hipStream_t s = (hipStream_t)stream;
    SceneGroupParams p;
    p.src = src; p.dst = dst; p.table = table_dev; p.n = n; p.Ha = Ha; p.Wa = Wa; p.C = C; p.mode = mode;
    if (fill_rgb) p.fill = (uint32_t)fill_rgb[0] | ((uint32_t)fill_rgb[1] << 8) | ((uint32_t)fill_rgb[2] << 16);
    TRYK(c, "scene_group_pack", 0, ((double)src_bytes + (double)Ha * Wa * C), s, launch_scene_group_pack(p, s));
    return 0;
}

extern "C" int srh_scene_group_crop(srh_ctx* c, const uint8_t* kp, const uint8_t* road, int Ha, int Wa, const int64_t* table_host,
                                    const int64_t* table_dev, int n, uint8_t* out_kp, uint8_t* out_road, int64_t out_bytes, void* stream) {
    if (!c || !kp || !road || !table_host || !table_dev || !out_kp || !out_road) return fail(c, SRH_ERR_BAD_ARG, "srh_scene_group_crop: null argument");
    if (n < 1 || !scene_dims_ok(Ha, Wa) || !group_table_ok(table_host, n, 1, Ha, Wa, out_bytes, true))
        return fail(c, SRH_ERR_BAD_ARG, "srh_scene_group_crop: bad sizes or an inconsistent table");
    hipSetDevice(c->device);
    hipStream_t s = (hipStream_t)stream;
    SceneGroupParams a, b;
    a.src = kp; a.dst = out_kp; a.table = table_dev; a.n = n; a.Ha = Ha; a.Wa = Wa; a.C = 1; a.mode = PAD_EDGE;
    b = a; b.src = road; b.dst = out_road;
    TRYK(c, "scene_group_crop", 0, 4.0 * (double)out_bytes, s, launch_scene_group_crop(a, b, s));
    return 0;
}

// ---- scene level, 16-bit and multi-band scenes (kernels in scene_bands.hip, behaviour in DESIGN.md §6i) -----------------------------------
static int scene_bands_params(srh_ctx* c, const char* who, const void* src, int src_dtype, int64_t n_pixels, int C, const int32_t* select,
                              SceneBandsParams& p) {
    if (!c || !src || !select) return fail(c, SRH_ERR_BAD_ARG, std::string(who) + ": null argument");
    if (src_dtype != SRH_U8 && src_dtype != SRH_U16) return fail(c, SRH_ERR_BAD_ARG, std::string(who) + ": the source is SRH_U8 or SRH_U16");
    if (C < 1 || C > BANDS_MAX_C || n_pixels < 1 || n_pixels > BANDS_MAX_PIXELS)
        return fail(c, SRH_ERR_BAD_ARG, std::string(who) + ": 1 to 16 bands and 1 to 2^31 - 1 pixels");
    for (int b = 0; b < 3; ++b)
        if (select[b] < 0 || select[b] >= C) return fail(c, SRH_ERR_BAD_ARG, std::string(who) + ": a selected band is 0 to C - 1");
    if (src_dtype == SRH_U16 && (reinterpret_cast<uintptr_t>(src) & 1)) return fail(c, SRH_ERR_BAD_ARG, std::string(who) + ": a u16 source is 2-byte aligned");
    p.src = src; p.n = (long)n_pixels; p.C = C; p.wide = src_dtype == SRH_U16;
    for (int b = 0; b < 3; ++b) p.sel[b] = select[b];
    return 0;
}

extern "C" int srh_scene_bands_hist(srh_ctx* c, const void* src, int src_dtype, int64_t n_pixels, int C, const int32_t* select,
                                    const uint8_t* valid, uint32_t* hist, void* stream) {
    SceneBandsParams p;
    TRY(scene_bands_params(c, "srh_scene_bands_hist", src, src_dtype, n_pixels, C, select, p));
    if (!hist || (reinterpret_cast<uintptr_t>(hist) & 3)) return fail(c, SRH_ERR_BAD_ARG, "srh_scene_bands_hist: null or misaligned hist");
    hipSetDevice(c->device);
    hipStream_t s = (hipStream_t)stream;
    p.valid = valid; p.hist = hist;
    TRYK(c, "scene_bands_hist", 0, (double)n_pixels * (3 * (p.wide ? 2 : 1) + (valid ? 1 : 0)), s, launch_scene_bands_hist(p, s));
    return 0;
}

extern "C" int srh_scene_bands_apply(srh_ctx* c, const void* src, int src_dtype, int64_t n_pixels, int C, const int32_t* select,
                                     const uint8_t* lut, uint8_t* dst, void* stream) {
    SceneBandsParams p;
    TRY(scene_bands_params(c, "srh_scene_bands_apply", src, src_dtype, n_pixels, C, select, p));
    if (!lut || !dst) return fail(c, SRH_ERR_BAD_ARG, "srh_scene_bands_apply: null argument");
    hipSetDevice(c->device);
    hipStream_t s = (hipStream_t)stream;
    p.lut = lut; p.dst = dst;
    TRYK(c, "scene_bands_apply", 0, (double)n_pixels * (3 * (p.wide ? 2 : 1) + 3), s, launch_scene_bands_apply(p, s));
    return 0;
}

// ---- scene level, another ground resolution (kernel in scene_scale.hip, behaviour in DESIGN.md §6j) ---------------------------------------
extern "C" int srh_scene_resample(srh_ctx* c, const uint8_t* src, int H, int W, int C, uint8_t* dst, int Ho, int Wo, const int32_t* start_y,
                                  const uint8_t* weights_y, int Ty, int Dy, const int32_t* start_x, const uint8_t* weights_x, int Tx, int Dx,
                                  int mode, const uint8_t* zero_where, int block_h, int block_w, int win_h, int win_w, void* stream) {
    if (!c || !src || !dst || !start_y || !weights_y || !start_x || !weights_x) return fail(c, SRH_ERR_BAD_ARG, "srh_scene_resample: null argument");
    if ((C != 1 && C != 3) || (mode != SCALE_SUM && mode != SCALE_VALID)) return fail(c, SRH_ERR_BAD_ARG, "srh_scene_resample: bad channel count or mode");
    if (H < 1 || W < 1 || Ho < 1 || Wo < 1 || !scene_dims_ok(H, W) || !scene_dims_ok(Ho, Wo)) return fail(c, SRH_ERR_BAD_ARG, "srh_scene_resample: bad sizes");
    if (Ty < 1 || Tx < 1 || Ty > SCALE_MAX_T || Tx > SCALE_MAX_T || Dy < 1 || Dx < 1 || Dy > SCALE_MAX_D || Dx > SCALE_MAX_D)
        return fail(c, SRH_ERR_BAD_ARG, "srh_scene_resample: 1 to 32 taps per axis and weight sums 1 to 32");
    SceneScaleParams p;
    p.src = src; p.dst = dst; p.zero_where = zero_where; p.sy = start_y; p.wy = weights_y; p.sx = start_x; p.wx = weights_x;
    p.H = H; p.W = W; p.Ho = Ho; p.Wo = Wo; p.C = C; p.Ty = Ty; p.Tx = Tx; p.Dy = Dy; p.Dx = Dx; p.mode = mode;
    p.bh = block_h; p.bw = block_w; p.win_h = win_h; p.win_w = win_w; p.magic = scale_magic(Dy * Dx);
    if (!scale_params_ok(p)) return fail(c, SRH_ERR_BAD_ARG, "srh_scene_resample: bad block or window (1..256 outputs per axis, at most 64 KiB of LDS)");
    hipSetDevice(c->device);
    hipStream_t s = (hipStream_t)stream;
    TRYK(c, "scene_resample", 0, ((double)H * W + (double)Ho * Wo) * C, s, launch_scene_resample(p, s));
    return 0;
}

// ---- scene level, connected-component filter of the masks (kernels in mask_clean.hip, behaviour in DESIGN.md §6k) ----------------------------
extern "C" int srh_mask_clean(srh_ctx* c, uint8_t* buf, int64_t buf_bytes, const int64_t* table_host, const int64_t* table_dev, int n,
                              int connectivity, int32_t* parent, int32_t* area, int32_t* peak, int64_t ws_pixels, void* stream) {
    if (!c || !buf || !table_host || !table_dev || !parent || !area || !peak) return fail(c, SRH_ERR_BAD_ARG, "srh_mask_clean: null argument");
    if (connectivity != 4 && connectivity != 8) return fail(c, SRH_ERR_BAD_ARG, "srh_mask_clean: the connectivity is 4 or 8");
    if (((reinterpret_cast<uintptr_t>(parent) | reinterpret_cast<uintptr_t>(area) | reinterpret_cast<uintptr_t>(peak)) & 3))
        return fail(c, SRH_ERR_BAD_ARG, "srh_mask_clean: a misaligned workspace");
    if (!mask_clean_table_ok(table_host, n, buf_bytes, ws_pixels))
        return fail(c, SRH_ERR_BAD_ARG, "srh_mask_clean: an inconsistent table (blocks inside the buffer and disjoint, running BASE and SEG0, thresholds 0 to "
                                        "256, min_area >= 1, at most 2^31 - 1 pixels, all of them in the workspaces)");
    hipSetDevice(c->device);
    hipStream_t s = (hipStream_t)stream;
    MaskCleanParams p;
    p.buf = buf; p.table = table_dev; p.n = n; p.conn = connectivity; p.parent = parent; p.area = area; p.peak = peak;
    p.n_segs = mask_clean_segs(table_host, n);
    const double px = (double)(table_host[(long)(n - 1) * MC_COLS + MC_BASE] + table_host[(long)(n - 1) * MC_COLS + MC_H] * table_host[(long)(n - 1) * MC_COLS + MC_W]);
    TRYK(c, "mask_clean_init", 0, px * 13, s, launch_mask_clean(p, 0, s));
    TRYK(c, "mask_clean_merge", 0, px * 6, s, launch_mask_clean(p, 1, s));
    TRYK(c, "mask_clean_flatten", 0, px * 9, s, launch_mask_clean(p, 2, s));
    TRYK(c, "mask_clean_stats", 0, px * 5, s, launch_mask_clean(p, 3, s));
    TRYK(c, "mask_clean_apply", 0, px * 6, s, launch_mask_clean(p, 4, s));
    return 0;
}

// ---- scene level, the validity mask from a nodata value (kernels in scene_nodata.hip, behaviour in DESIGN.md §6l) ---------------------------
static_assert(SRH_NODATA_ALL == ND_ALL && SRH_NODATA_ANY == ND_ANY, "match modes of the header and the kernel");

static bool ranges_overlap(const void* a, double a_bytes, const void* b, double b_bytes) {
    const double a0 = (double)reinterpret_cast<uintptr_t>(a), b0 = (double)reinterpret_cast<uintptr_t>(b);
    return a0 < b0 + b_bytes && b0 < a0 + a_bytes;
}

extern "C" int srh_scene_nodata_match(srh_ctx* c, const void* src, int src_dtype, int64_t n_pixels, int C, const int32_t* lo, const int32_t* hi,
                                      int match, const uint8_t* and_with, int invert, uint8_t* out, void* stream) {
    if (!c || !src || !lo || !hi || !out) return fail(c, SRH_ERR_BAD_ARG, "srh_scene_nodata_match: null argument");
    if (src_dtype != SRH_U8 && src_dtype != SRH_U16) return fail(c, SRH_ERR_BAD_ARG, "srh_scene_nodata_match: the source is SRH_U8 or SRH_U16");
    if (C < 1 || C > ND_MAX_C || n_pixels < 1 || n_pixels > ND_MAX_PIXELS)
        return fail(c, SRH_ERR_BAD_ARG, "srh_scene_nodata_match: 1 to 16 bands and 1 to 2^31 - 1 pixels");
    if ((match != SRH_NODATA_ALL && match != SRH_NODATA_ANY) || (invert != 0 && invert != 1))
        return fail(c, SRH_ERR_BAD_ARG, "srh_scene_nodata_match: match is SRH_NODATA_ALL / SRH_NODATA_ANY and invert 0 / 1");
    if (src_dtype == SRH_U16 && (reinterpret_cast<uintptr_t>(src) & 1)) return fail(c, SRH_ERR_BAD_ARG, "srh_scene_nodata_match: a u16 source is 2-byte aligned");
    SceneNodataParams p;
    for (int b = 0; b < C; ++b) {
        if (lo[b] < 0 || lo[b] > 65535 || hi[b] < 0 || hi[b] > 65535) return fail(c, SRH_ERR_BAD_ARG, "srh_scene_nodata_match: a bound is 0 to 65535");
        p.lohi[b] = (uint32_t)lo[b] | ((uint32_t)hi[b] << 16);
    }
    const double src_bytes = (double)n_pixels * C * (src_dtype == SRH_U16 ? 2 : 1);
    if (ranges_overlap(out, (double)n_pixels, src, src_bytes) || (and_with && ranges_overlap(out, (double)n_pixels, and_with, (double)n_pixels)))
        return fail(c, SRH_ERR_BAD_ARG, "srh_scene_nodata_match: out overlaps src or and_with");
    p.src = src; p.and_with = and_with; p.out = out; p.n = (long)n_pixels; p.C = C; p.wide = src_dtype == SRH_U16; p.any = match; p.invert = invert;
    hipSetDevice(c->device);
    hipStream_t s = (hipStream_t)stream;
    TRYK(c, "scene_nodata_match", 0, src_bytes + (double)n_pixels * (and_with ? 2 : 1), s, launch_scene_nodata_match(p, s));
    return 0;
}

extern "C" int srh_scene_nodata_grow(srh_ctx* c, const uint8_t* src, uint8_t* dst, int64_t bytes, const int64_t* table_host,
                                     const int64_t* table_dev, int n, int r, const uint8_t* and_with, int invert, void* stream) {
    if (!c || !src || !dst || !table_host || !table_dev) return fail(c, SRH_ERR_BAD_ARG, "srh_scene_nodata_grow: null argument");
    if (r < 1 || r > NG_MAX_R || (invert != 0 && invert != 1)) return fail(c, SRH_ERR_BAD_ARG, "srh_scene_nodata_grow: r is 1 to 16 and invert 0 / 1");
    if (!grow_table_ok(table_host, n, bytes))
        return fail(c, SRH_ERR_BAD_ARG, "srh_scene_nodata_grow: an inconsistent table (1 to 4096 blocks of at least 1 x 1 pixels, inside the buffers and "
                                        "disjoint, at most 2^31 - 1 pixels)");
    if (ranges_overlap(src, (double)bytes, dst, (double)bytes) || (and_with && ranges_overlap(and_with, (double)bytes, dst, (double)bytes)))
        return fail(c, SRH_ERR_BAD_ARG, "srh_scene_nodata_grow: dst overlaps src or and_with");
    hipSetDevice(c->device);
    hipStream_t s = (hipStream_t)stream;
    SceneGrowParams p;
    p.src = src; p.dst = dst; p.and_with = and_with; p.table = table_dev; p.n = n; p.r = r; p.invert = invert;
    double px = 0;
    for (int k = 0; k < n; ++k) px += (double)(table_host[(long)k * NG_COLS + NG_H] * table_host[(long)k * NG_COLS + NG_W]);
    TRYK(c, "scene_nodata_grow", 0, px * (and_with ? 3 : 2), s, launch_scene_nodata_grow(p, grow_max_blocks(table_host, n), s));
    return 0;
}

// ---- scene level, the validity mask from the polygons of an area of interest (kernel in scene_aoi.hip, behaviour in DESIGN.md §6m) ------------
static_assert(SRH_AOI_MAX_POLYGONS == AOI_MAX_POLYGONS && SRH_AOI_MAX_EDGES == AOI_MAX_EDGES, "limits of the header and the kernel");

extern "C" int srh_scene_aoi_fill(srh_ctx* c, const int32_t* edges_host, const int32_t* edges_dev, const int32_t* polys_host, const int32_t* polys_dev,
                                  int n_include, int n_exclude, int H, int W, const uint8_t* and_with, int invert, uint8_t* out, void* stream) {
    if (!c || !edges_host || !edges_dev || !polys_host || !polys_dev || !out) return fail(c, SRH_ERR_BAD_ARG, "srh_scene_aoi_fill: null argument");
    if (H < 1 || W < 1 || (double)H * W > (double)AOI_MAX_PIXELS) return fail(c, SRH_ERR_BAD_ARG, "srh_scene_aoi_fill: H and W are at least 1 and H W at most 2^31 - 1");
    if (invert != 0 && invert != 1) return fail(c, SRH_ERR_BAD_ARG, "srh_scene_aoi_fill: invert is 0 / 1");
    if (reinterpret_cast<uintptr_t>(edges_dev) & 15) return fail(c, SRH_ERR_BAD_ARG, "srh_scene_aoi_fill: the device edge table is 16-byte aligned");
    if (!aoi_table_ok(edges_host, polys_host, n_include, n_exclude))
        return fail(c, SRH_ERR_BAD_ARG, "srh_scene_aoi_fill: an inconsistent table (at most 64 polygons and 16384 edges, offsets a running sum from 0, "
                                        "every edge y0 < y1, coordinates within +-2^28)");
    const double px = (double)H * W;
    if (and_with && ranges_overlap(out, px, and_with, px)) return fail(c, SRH_ERR_BAD_ARG, "srh_scene_aoi_fill: out overlaps and_with");
    SceneAoiParams p;
    p.edges = edges_dev; p.polys = polys_dev; p.and_with = and_with; p.out = out; p.n_include = n_include; p.n_exclude = n_exclude; p.H = H; p.W = W;
    p.invert = invert;
    hipSetDevice(c->device);
    hipStream_t s = (hipStream_t)stream;
    TRYK(c, "scene_aoi_fill", 0, px * (and_with ? 2 : 1) + 16.0 * polys_host[n_include + n_exclude], s, launch_scene_aoi_fill(p, s));
    return 0;
}

// ---- scene level, float32 scenes (kernels in scene_float.hip, behaviour in DESIGN.md §6n) ----------------------------------------------------
static int scene_float_params(srh_ctx* c, const char* who, const void* src, int64_t n_pixels, int C, const int32_t* select, SceneFloatParams& p) {
    if (!c || !src || !select) return fail(c, SRH_ERR_BAD_ARG, std::string(who) + ": null argument");
    if (C < 1 || C > FLOAT_MAX_C || n_pixels < 1 || n_pixels > FLOAT_MAX_PIXELS)
        return fail(c, SRH_ERR_BAD_ARG, std::string(who) + ": 1 to 16 bands and 1 to 2^31 - 1 pixels");
    for (int b = 0; b < 3; ++b)
        if (select[b] < 0 || select[b] >= C) return fail(c, SRH_ERR_BAD_ARG, std::string(who) + ": a selected band is 0 to C - 1");
    if (reinterpret_cast<uintptr_t>(src) & 3) return fail(c, SRH_ERR_BAD_ARG, std::string(who) + ": the f32 source is 4-byte aligned");
    p.src = static_cast<const uint32_t*>(src); p.n = (long)n_pixels; p.C = C;
    for (int b = 0; b < 3; ++b) p.sel[b] = select[b];
    return 0;
}

extern "C" int srh_scene_float_valid(srh_ctx* c, const void* src, int64_t n_pixels, int C, const int32_t* select, const uint32_t* nodata_keys,
                                     int n_nodata, int log, const uint8_t* valid_in, uint8_t* valid_out, void* stream) {
    SceneFloatParams p;
    TRY(scene_float_params(c, "srh_scene_float_valid", src, n_pixels, C, select, p));
    if (!valid_out || n_nodata < 0 || n_nodata > FLOAT_MAX_NODATA || (n_nodata > 0 && !nodata_keys) || (log != 0 && log != 1))
        return fail(c, SRH_ERR_BAD_ARG, "srh_scene_float_valid: null argument, more than 4 nodata keys or log outside 0 / 1");
    const double src_bytes = (double)n_pixels * C * 4;
    if (ranges_overlap(valid_out, (double)n_pixels, src, src_bytes) || (valid_in && ranges_overlap(valid_out, (double)n_pixels, valid_in, (double)n_pixels)))
        return fail(c, SRH_ERR_BAD_ARG, "srh_scene_float_valid: valid_out overlaps src or valid_in");
    p.valid_in = valid_in; p.valid_out = valid_out; p.n_nodata = n_nodata; p.log = log;
    for (int j = 0; j < n_nodata; ++j) p.nodata[j] = nodata_keys[j];
    hipSetDevice(c->device);
    hipStream_t s = (hipStream_t)stream;
    TRYK(c, "scene_float_valid", 0, (double)n_pixels * (12 + (valid_in ? 2 : 1)), s, launch_scene_float_valid(p, s));
    return 0;
}

extern "C" int srh_scene_float_hist(srh_ctx* c, const void* src, int64_t n_pixels, int C, const int32_t* select, const uint8_t* valid,
                                    const uint32_t* targets, int n_targets, uint32_t* hist, void* stream) {
    SceneFloatParams p;
    TRY(scene_float_params(c, "srh_scene_float_hist", src, n_pixels, C, select, p));
    if (!valid || !hist || (reinterpret_cast<uintptr_t>(hist) & 3)) return fail(c, SRH_ERR_BAD_ARG, "srh_scene_float_hist: null valid, or null or misaligned hist");
    if (n_targets < 0 || n_targets > FLOAT_MAX_TARGETS || (n_targets > 0) != (targets != nullptr))
        return fail(c, SRH_ERR_BAD_ARG, "srh_scene_float_hist: 1 to 6 targets, or none and a null list for pass 1");
    for (int t = 0; t < n_targets; ++t) {
        if (targets[2 * t] >= (uint32_t)C || targets[2 * t + 1] > 0xffffu)
            return fail(c, SRH_ERR_BAD_ARG, "srh_scene_float_hist: a target is (band 0 to C - 1, prefix 0 to 65535)");
        p.tband[t] = (int)targets[2 * t]; p.tprefix[t] = targets[2 * t + 1];
    }
    const double src_bytes = (double)n_pixels * C * 4, hist_bytes = (double)(n_targets ? n_targets : 3) * 65536 * 4;
    if (ranges_overlap(hist, hist_bytes, src, src_bytes) || ranges_overlap(hist, hist_bytes, valid, (double)n_pixels))
        return fail(c, SRH_ERR_BAD_ARG, "srh_scene_float_hist: hist overlaps src or valid");
    p.valid = valid; p.hist = hist; p.n_targets = n_targets;
    hipSetDevice(c->device);
    hipStream_t s = (hipStream_t)stream;
    TRYK(c, "scene_float_hist", 0, (double)n_pixels * (n_targets ? 4 * n_targets + 1 : 13), s, launch_scene_float_hist(p, s));
    return 0;
}

extern "C" int srh_scene_float_apply(srh_ctx* c, const void* src, int64_t n_pixels, int C, const int32_t* select, const uint8_t* valid,
                                     const uint32_t* thresholds, uint8_t* dst, void* stream) {
    SceneFloatParams p;
    TRY(scene_float_params(c, "srh_scene_float_apply", src, n_pixels, C, select, p));
    if (!valid || !thresholds || !dst || (reinterpret_cast<uintptr_t>(thresholds) & 3))
        return fail(c, SRH_ERR_BAD_ARG, "srh_scene_float_apply: null argument or a misaligned threshold table");
    const double src_bytes = (double)n_pixels * C * 4, dst_bytes = 3.0 * (double)n_pixels;
    if (ranges_overlap(dst, dst_bytes, src, src_bytes) || ranges_overlap(dst, dst_bytes, valid, (double)n_pixels) || ranges_overlap(dst, dst_bytes, thresholds, 3072.0))
        return fail(c, SRH_ERR_BAD_ARG, "srh_scene_float_apply: dst overlaps src, valid or the thresholds");
    p.valid = valid; p.thr = thresholds; p.dst = dst;
    hipSetDevice(c->device);
    hipStream_t s = (hipStream_t)stream;
    TRYK(c, "scene_float_apply", 0, (double)n_pixels * (12 + 1 + 3), s, launch_scene_float_apply(p, s));
    return 0;
}

// ---- the road graph as a raster (kernels in graph_raster.hip, behaviour in DESIGN.md §6o) ----------------------------------------------------
static_assert(SRH_GRAPH_MAX_SPAN == GR_MAX_SPAN && SRH_GRAPH_MARK_NONE == GR_MARK_NONE && SRH_GRAPH_MARK_SQUARE == GR_MARK_SQUARE &&
              SRH_GRAPH_MARK_DISC == GR_MARK_DISC, "limits and marks of the header and the kernel");

extern "C" int srh_graph_raster(srh_ctx* c, const int32_t* nodes_host, const int32_t* nodes_dev, int N, const int32_t* edges_host,
                                const int32_t* edges_dev, int E, int H, int W, int t, int mark, int r, int edge_value, int node_value, uint8_t* out,
                                void* stream) {
    if (!c || !out || N < 0 || E < 0 || (N > 0 && (!nodes_host || !nodes_dev)) || (E > 0 && (!edges_host || !edges_dev)))
        return fail(c, SRH_ERR_BAD_ARG, "srh_graph_raster: null argument or a negative count");
    if (H < 1 || W < 1 || (double)H * W > (double)GR_MAX_PIXELS) return fail(c, SRH_ERR_BAD_ARG, "srh_graph_raster: H and W are at least 1 and H W at most 2^31 - 1");
    if (t < 1 || t > GR_MAX_WIDTH || mark < GR_MARK_NONE || mark > GR_MARK_DISC || r < 0 || r > GR_MAX_RADIUS)
        return fail(c, SRH_ERR_BAD_ARG, "srh_graph_raster: the width is 1 to 255, the mark SRH_GRAPH_MARK_NONE / SQUARE / DISC and its radius 0 to 127");
    if (edge_value < 1 || edge_value > 255 || node_value < 1 || node_value > 255) return fail(c, SRH_ERR_BAD_ARG, "srh_graph_raster: a class value is 1 to 255");
    if ((reinterpret_cast<uintptr_t>(nodes_dev) | reinterpret_cast<uintptr_t>(edges_dev)) & 3) return fail(c, SRH_ERR_BAD_ARG, "srh_graph_raster: the device tables are 4-byte aligned");
    if (!gr_tables_ok(nodes_host, N, edges_host, E))
        return fail(c, SRH_ERR_BAD_ARG, "srh_graph_raster: an inconsistent table (coordinates within +-2^28, edge indices in [0, N), an edge spans at most "
                                        "16383 px per axis)");
    const double px = (double)H * W;
    if ((N > 0 && ranges_overlap(out, px, nodes_dev, 8.0 * N)) || (E > 0 && ranges_overlap(out, px, edges_dev, 8.0 * E)))
        return fail(c, SRH_ERR_BAD_ARG, "srh_graph_raster: out overlaps a table");
    GraphRasterParams p;
    p.nodes = nodes_dev; p.edges = edges_dev; p.out = out; p.N = N; p.E = E; p.H = H; p.W = W; p.t = t; p.mark = mark; p.r = r;
    p.edge_value = edge_value; p.node_value = node_value;
    hipSetDevice(c->device);
    hipStream_t s = (hipStream_t)stream;
    TRYK(c, "graph_clear", 0, px, s, launch_graph_clear(p, s));
    if (E > 0) TRYK(c, "graph_edges", 0, 24.0 * E, s, launch_graph_edges(p, s));
    if (N > 0 && mark != GR_MARK_NONE) TRYK(c, "graph_nodes", 0, (8.0 + (2.0 * r + 1) * (2.0 * r + 1)) * N, s, launch_graph_nodes(p, s));
    return 0;
}

static bool graph_colour(const int32_t* rgb, uint32_t& out) {
    if (!rgb || ((rgb[0] | rgb[1] | rgb[2]) & ~255)) return false;
    out = (uint32_t)rgb[0] | ((uint32_t)rgb[1] << 8) | ((uint32_t)rgb[2] << 16);
    return true;
}

extern "C" int srh_graph_composite(srh_ctx* c, const uint8_t* cls, const uint8_t* img, int H, int W, const int32_t* background_rgb,
                                   const int32_t* edge_rgb, const int32_t* node_rgb, uint8_t* out, void* stream) {
    if (!c || !cls || !out) return fail(c, SRH_ERR_BAD_ARG, "srh_graph_composite: null argument");
    if (H < 1 || W < 1 || (double)H * W > (double)GR_MAX_PIXELS) return fail(c, SRH_ERR_BAD_ARG, "srh_graph_composite: H and W are at least 1 and H W at most 2^31 - 1");
    GraphCompositeParams p;
    if (!graph_colour(background_rgb, p.colour[0]) || !graph_colour(edge_rgb, p.colour[1]) || !graph_colour(node_rgb, p.colour[2]))
        return fail(c, SRH_ERR_BAD_ARG, "srh_graph_composite: a colour is three host ints 0 to 255");
    const double px = (double)H * W;
    if (ranges_overlap(out, 3 * px, cls, px) || (img && ranges_overlap(out, 3 * px, img, 3 * px)))
        return fail(c, SRH_ERR_BAD_ARG, "srh_graph_composite: out overlaps the class map or the image");
    p.cls = cls; p.img = img; p.out = out; p.n = (long)H * W;
    hipSetDevice(c->device);
    hipStream_t s = (hipStream_t)stream;
    TRYK(c, "graph_composite", 0, px * (img ? 7 : 4), s, launch_graph_composite(p, s));
    return 0;
}

extern "C" int srh_graph_compare(srh_ctx* c, const uint8_t* pred_thin, const uint8_t* pred_wide, const uint8_t* gt_thin, const uint8_t* gt_wide,
                                 const uint8_t* valid, const uint8_t* img, int H, int W, uint64_t* counts, uint8_t* diff, void* stream) {
    if (!c || !pred_thin || !pred_wide || !gt_thin || !gt_wide || !counts) return fail(c, SRH_ERR_BAD_ARG, "srh_graph_compare: null argument");
    if (H < 1 || W < 1 || (double)H * W > (double)GR_MAX_PIXELS) return fail(c, SRH_ERR_BAD_ARG, "srh_graph_compare: H and W are at least 1 and H W at most 2^31 - 1");
    if (reinterpret_cast<uintptr_t>(counts) & 7) return fail(c, SRH_ERR_BAD_ARG, "srh_graph_compare: counts is 8-byte aligned");
    const double px = (double)H * W;
    const void* ins[6] = {pred_thin, pred_wide, gt_thin, gt_wide, valid, img};
    for (int k = 0; k < 6; ++k) {
        if (!ins[k]) continue;
        const double bytes = k == 5 ? 3 * px : px;
        if (ranges_overlap(counts, 32.0, ins[k], bytes) || (diff && ranges_overlap(diff, 3 * px, ins[k], bytes)))
            return fail(c, SRH_ERR_BAD_ARG, "srh_graph_compare: counts or diff overlaps an input");
    }
    if (diff && ranges_overlap(diff, 3 * px, counts, 32.0)) return fail(c, SRH_ERR_BAD_ARG, "srh_graph_compare: diff overlaps counts");
    GraphCompareParams p;
    p.pred_thin = pred_thin; p.pred_wide = pred_wide; p.gt_thin = gt_thin; p.gt_wide = gt_wide; p.valid = valid; p.img = img; p.diff = diff;
    p.counts = reinterpret_cast<unsigned long long*>(counts); p.n = (long)H * W;
    hipSetDevice(c->device);
    hipStream_t s = (hipStream_t)stream;
    TRYK(c, "graph_counts_zero", 0, 32.0, s, launch_graph_counts_zero(p, s));
    TRYK(c, "graph_compare", 0, px * (4 + (valid ? 1 : 0) + (diff ? (img ? 6 : 3) : 0)), s, launch_graph_compare(p, s));
    return 0;
}

// ---- the road-mask evidence under every edge (kernel in edge_support.hip, behaviour in DESIGN.md §6p) ------------------------------------------
extern "C" int srh_graph_edge_stats(srh_ctx* c, const int32_t* nodes_host, const int32_t* nodes_dev, int N, const int32_t* edges_host,
                                    const int32_t* edges_dev, int E, int H, int W, int t, const uint8_t* mask, const uint8_t* valid, int on_level,
                                    int32_t* out, void* stream) {
    if (!c || N < 0 || E < 0 || (N > 0 && (!nodes_host || !nodes_dev)) || (E > 0 && (!edges_host || !edges_dev || !mask || !out)))
        return fail(c, SRH_ERR_BAD_ARG, "srh_graph_edge_stats: null argument or a negative count");
    if (H < 1 || W < 1 || (double)H * W > (double)GR_MAX_PIXELS) return fail(c, SRH_ERR_BAD_ARG, "srh_graph_edge_stats: H and W are at least 1 and H W at most 2^31 - 1");
    if (t < 1 || t > GR_MAX_WIDTH) return fail(c, SRH_ERR_BAD_ARG, "srh_graph_edge_stats: the width is 1 to 255");
    if (on_level < 0 || on_level > 255) return fail(c, SRH_ERR_BAD_ARG, "srh_graph_edge_stats: on_level is 0 to 255");
    if ((reinterpret_cast<uintptr_t>(nodes_dev) | reinterpret_cast<uintptr_t>(edges_dev)) & 3) return fail(c, SRH_ERR_BAD_ARG, "srh_graph_edge_stats: the device tables are 4-byte aligned");
    if (reinterpret_cast<uintptr_t>(out) & 15) return fail(c, SRH_ERR_BAD_ARG, "srh_graph_edge_stats: out is 16-byte aligned");
    if (!gr_tables_ok(nodes_host, N, edges_host, E))
        return fail(c, SRH_ERR_BAD_ARG, "srh_graph_edge_stats: an inconsistent table (coordinates within +-2^28, edge indices in [0, N), an edge spans at most "
                                        "16383 px per axis)");
    if (E == 0) return 0;                        // nothing to write, nothing launched
    const double px = (double)H * W, ob = 16.0 * E;
    if (ranges_overlap(out, ob, nodes_dev, 8.0 * N) || ranges_overlap(out, ob, edges_dev, 8.0 * E) || ranges_overlap(out, ob, mask, px) ||
        (valid && ranges_overlap(out, ob, valid, px)))
        return fail(c, SRH_ERR_BAD_ARG, "srh_graph_edge_stats: out overlaps an input");
    EdgeStatsParams p;
    p.g.nodes = nodes_dev; p.g.edges = edges_dev; p.g.N = N; p.g.E = E; p.g.H = H; p.g.W = W; p.g.t = t;
    p.mask = mask; p.valid = valid; p.on_level = on_level; p.out = out;
    hipSetDevice(c->device);
    hipStream_t s = (hipStream_t)stream;
    TRYK(c, "graph_edge_stats", 0, 40.0 * E, s, launch_graph_edge_stats(p, s));
    return 0;
}

// ---- the road width under every edge (kernels in road_width.hip, behaviour in DESIGN.md §6q) ---------------------------------------------------
extern "C" int srh_road_dist(srh_ctx* c, const uint8_t* mask, int H, int W, int on_level, int R, uint16_t* d2_out, void* stream) {
    if (!c || !mask || !d2_out) return fail(c, SRH_ERR_BAD_ARG, "srh_road_dist: null argument");
    if (H < 1 || W < 1 || (double)H * W > (double)GR_MAX_PIXELS) return fail(c, SRH_ERR_BAD_ARG, "srh_road_dist: H and W are at least 1 and H W at most 2^31 - 1");
    if (on_level < 0 || on_level > 255) return fail(c, SRH_ERR_BAD_ARG, "srh_road_dist: on_level is 0 to 255");
    if (R < 1 || R > RW_MAX_R) return fail(c, SRH_ERR_BAD_ARG, "srh_road_dist: the radius is 1 to 254");
    if (reinterpret_cast<uintptr_t>(d2_out) & 7) return fail(c, SRH_ERR_BAD_ARG, "srh_road_dist: d2_out is 8-byte aligned");
    const double px = (double)H * W;
    if (ranges_overlap(d2_out, 2 * px, mask, px)) return fail(c, SRH_ERR_BAD_ARG, "srh_road_dist: d2_out overlaps the mask");
    hipSetDevice(c->device);
    hipStream_t s = (hipStream_t)stream;
    std::lock_guard<std::mutex> lock(c->road_mu);
    if (c->road_g.ensure((size_t)H * W)) return fail(c, SRH_ERR_HIP, "road distance workspace allocation failed");
    if (ranges_overlap(d2_out, 2 * px, c->road_g.p, px)) return fail(c, SRH_ERR_BAD_ARG, "srh_road_dist: d2_out overlaps the workspace");
    RoadDistParams p;
    p.mask = mask; p.g = c->road_g.as<uint8_t>(); p.d2 = d2_out; p.H = H; p.W = W; p.on_level = on_level; p.R = R;
    const double rows = (double)(RW_COL_ROWS + 2 * R) / RW_COL_ROWS;       // the rows a chunk reads for each row it writes
    TRYK(c, "road_dist_cols", 0, px * (rows + 1), s, launch_road_dist(p, 0, s));
    TRYK(c, "road_dist_rows", 0, px * 3, s, launch_road_dist(p, 1, s));
    return 0;
}

extern "C" int srh_graph_edge_widths(srh_ctx* c, const int32_t* nodes_host, const int32_t* nodes_dev, int N, const int32_t* edges_host,
                                     const int32_t* edges_dev, int E, int H, int W, const uint16_t* d2, int R, int32_t* out, void* stream) {
    if (!c || N < 0 || E < 0 || (N > 0 && (!nodes_host || !nodes_dev)) || (E > 0 && (!edges_host || !edges_dev || !d2 || !out)))
        return fail(c, SRH_ERR_BAD_ARG, "srh_graph_edge_widths: null argument or a negative count");
    if (H < 1 || W < 1 || (double)H * W > (double)GR_MAX_PIXELS) return fail(c, SRH_ERR_BAD_ARG, "srh_graph_edge_widths: H and W are at least 1 and H W at most 2^31 - 1");
    if (R < 1 || R > RW_MAX_R) return fail(c, SRH_ERR_BAD_ARG, "srh_graph_edge_widths: the radius is 1 to 254");
    if ((reinterpret_cast<uintptr_t>(nodes_dev) | reinterpret_cast<uintptr_t>(edges_dev)) & 3) return fail(c, SRH_ERR_BAD_ARG, "srh_graph_edge_widths: the device tables are 4-byte aligned");
    if (reinterpret_cast<uintptr_t>(d2) & 1) return fail(c, SRH_ERR_BAD_ARG, "srh_graph_edge_widths: d2 is 2-byte aligned");
    if (reinterpret_cast<uintptr_t>(out) & 15) return fail(c, SRH_ERR_BAD_ARG, "srh_graph_edge_widths: out is 16-byte aligned");
    if (!gr_tables_ok(nodes_host, N, edges_host, E))
        return fail(c, SRH_ERR_BAD_ARG, "srh_graph_edge_widths: an inconsistent table (coordinates within +-2^28, edge indices in [0, N), an edge spans at most "
                                        "16383 px per axis)");
    if (E == 0) return 0;                        // nothing to write, nothing launched
    const double px = (double)H * W, ob = 32.0 * E;
    if (ranges_overlap(out, ob, nodes_dev, 8.0 * N) || ranges_overlap(out, ob, edges_dev, 8.0 * E) || ranges_overlap(out, ob, d2, 2 * px))
        return fail(c, SRH_ERR_BAD_ARG, "srh_graph_edge_widths: out overlaps an input");
    EdgeWidthParams p;
    p.g.nodes = nodes_dev; p.g.edges = edges_dev; p.g.N = N; p.g.E = E; p.g.H = H; p.g.W = W; p.g.t = 1;
    p.d2 = d2; p.R = R; p.out = out;
    hipSetDevice(c->device);
    hipStream_t s = (hipStream_t)stream;
    TRYK(c, "graph_edge_widths", 0, 56.0 * E, s, launch_graph_edge_widths(p, s));
    return 0;
}

// ---- spur and small-component pruning of the graph (kernels in graph_clean.hip, behaviour in DESIGN.md §6s) -----------------------------------
static_assert(SRH_GRAPH_CLEAN_MAX_ROUNDS == GC_MAX_ROUNDS && SRH_GRAPH_CLEAN_MAX_ITEMS == GC_MAX_ITEMS, "limits of the header and the kernel");

extern "C" int srh_graph_clean(srh_ctx* c, const int32_t* nodes_host, const int32_t* nodes_dev, int N, const int32_t* edges_host,
                               const int32_t* edges_dev, int E, int64_t spur_q, int64_t comp_q, int rounds, uint8_t* state_out, int32_t* out,
                               void* stream) {
    if (!c || N < 0 || E < 0 || (N > 0 && (!nodes_host || !nodes_dev)) || (E > 0 && (!edges_host || !edges_dev || !state_out || !out)))
        return fail(c, SRH_ERR_BAD_ARG, "srh_graph_clean: null argument or a negative count");
    if (N > GC_MAX_ITEMS || E > GC_MAX_ITEMS) return fail(c, SRH_ERR_BAD_ARG, "srh_graph_clean: at most 2^26 nodes and 2^26 edges");
    if (rounds < 1 || rounds > GC_MAX_ROUNDS) return fail(c, SRH_ERR_BAD_ARG, "srh_graph_clean: rounds is 1 to 8");
    if (spur_q < 0 || comp_q < 0) return fail(c, SRH_ERR_BAD_ARG, "srh_graph_clean: a threshold is >= 0 (0: not stated)");
    if ((reinterpret_cast<uintptr_t>(nodes_dev) | reinterpret_cast<uintptr_t>(edges_dev)) & 3) return fail(c, SRH_ERR_BAD_ARG, "srh_graph_clean: the device tables are 4-byte aligned");
    if (reinterpret_cast<uintptr_t>(out) & 15) return fail(c, SRH_ERR_BAD_ARG, "srh_graph_clean: out is 16-byte aligned");
    if (!gr_tables_ok(nodes_host, N, edges_host, E))
        return fail(c, SRH_ERR_BAD_ARG, "srh_graph_clean: an inconsistent table (coordinates within +-2^28, edge indices in [0, N), an edge spans at most "
                                        "16383 px per axis)");
    if (E == 0) return 0;                        // nothing to write, nothing launched
    const double sb = (double)E, ob = 16.0 * E;
    if (ranges_overlap(out, ob, nodes_dev, 8.0 * N) || ranges_overlap(out, ob, edges_dev, 8.0 * E) || ranges_overlap(state_out, sb, nodes_dev, 8.0 * N) ||
        ranges_overlap(state_out, sb, edges_dev, 8.0 * E))
        return fail(c, SRH_ERR_BAD_ARG, "srh_graph_clean: an output overlaps an input");
    if (ranges_overlap(out, ob, state_out, sb)) return fail(c, SRH_ERR_BAD_ARG, "srh_graph_clean: state_out and out overlap");
    hipSetDevice(c->device);
    hipStream_t s = (hipStream_t)stream;
    std::lock_guard<std::mutex> lock(c->clean_mu);
    const size_t ws = gc_workspace_bytes(N, E);
    if (c->clean_ws.ensure(ws, 0.25)) return fail(c, SRH_ERR_HIP, "graph clean workspace allocation failed");
    if (ranges_overlap(out, ob, c->clean_ws.p, (double)c->clean_ws.cap) || ranges_overlap(state_out, sb, c->clean_ws.p, (double)c->clean_ws.cap))
        return fail(c, SRH_ERR_BAD_ARG, "srh_graph_clean: an output overlaps the workspace");
    if (!c->clean_done && hipEventCreateWithFlags(&c->clean_done, hipEventDisableTiming) != hipSuccess) {
        c->clean_done = nullptr;
        return fail(c, SRH_ERR_HIP, "graph clean event creation failed");
    }
    // the call before this one, on whatever stream, has left the workspace before this one's first launch touches it (a no-op on a fresh event)
    if (hipStreamWaitEvent(s, c->clean_done, 0) != hipSuccess) return fail(c, SRH_ERR_HIP, "srh_graph_clean: waiting for the workspace failed");
    GraphCleanParams p;
    p.nodes = nodes_dev; p.edges = edges_dev; p.N = N; p.E = E; p.spur_q = spur_q; p.comp_q = comp_q; p.state = state_out; p.out = out;
    gc_workspace_carve(c->clean_ws.p, N, E, p);
    const double n = (double)N, e = (double)E;
    int rc = 0;
    for (int r = 1; r <= rounds + 1 && !rc; ++r) {
        p.round = r <= rounds ? r : 0;
        p.first = r == 1;
        rc = [&]() -> int {
            TRYK(c, "graph_clean_init", 0, 24 * n + 16 * e, s, launch_graph_clean(p, 0, s));
            TRYK(c, "graph_clean_edges", 0, 9 * e + 32 * e, s, launch_graph_clean(p, 1, s));
            TRYK(c, "graph_clean_chains", 0, 12 * n, s, launch_graph_clean(p, 2, s));
            TRYK(c, "graph_clean_sums", 0, 9 * e + 56 * e, s, launch_graph_clean(p, 3, s));
            TRYK(c, "graph_clean_decide", 0, 9 * e + 36 * e, s, launch_graph_clean(p, 4, s));
            return 0;
        }();
    }
    const hipError_t rec = hipEventRecord(c->clean_done, s);        // also after a failed launch: what was queued still uses the workspace
    if (rc) return rc;
    if (rec != hipSuccess) return hip_fail(c, rec, "srh_graph_clean: recording the workspace event");
    return 0;
}

// ---- a GeoTIFF's decompressed segments -> the scene raster (kernel in scene_tiff.hip, behaviour in DESIGN.md §6r) ---------------------------------
extern "C" int srh_tiff_assemble(srh_ctx* c, const uint8_t* flat, int64_t flat_bytes, const int64_t* table_host, const int64_t* table_dev, int n_seg,
                                 void* out, int H, int W, int C, int dtype, int predictor, int big_endian, void* stream) {
    if (!c || !flat || !table_host || !table_dev || !out) return fail(c, SRH_ERR_BAD_ARG, "srh_tiff_assemble: null argument");
    if (H < 1 || W < 1 || (double)H * W > (double)TIF_MAX_PIXELS) return fail(c, SRH_ERR_BAD_ARG, "srh_tiff_assemble: H and W are at least 1 and H W at most 2^31 - 1");
    if (C < 1 || C > TIF_MAX_BANDS) return fail(c, SRH_ERR_BAD_ARG, "srh_tiff_assemble: 1 to 16 bands");
    if (dtype != SRH_U8 && dtype != SRH_U16 && dtype != SRH_F32) return fail(c, SRH_ERR_BAD_ARG, "srh_tiff_assemble: the samples are SRH_U8, SRH_U16 or SRH_F32");
    const int B = dtype == SRH_U8 ? 1 : dtype == SRH_U16 ? 2 : 4;
    if (predictor < 1 || predictor > 3 || (predictor == 2 && B == 4) || (predictor == 3 && B != 4))
        return fail(c, SRH_ERR_BAD_ARG, "srh_tiff_assemble: predictor 1, 2 with integer samples or 3 with float samples");
    if (big_endian != 0 && big_endian != 1) return fail(c, SRH_ERR_BAD_ARG, "srh_tiff_assemble: big_endian is 0 or 1");
    if (n_seg < 1 || flat_bytes < 1) return fail(c, SRH_ERR_BAD_ARG, "srh_tiff_assemble: at least one segment");
    if (reinterpret_cast<uintptr_t>(flat) & (TIF_ALIGN - 1)) return fail(c, SRH_ERR_BAD_ARG, "srh_tiff_assemble: flat is 16-byte aligned");
    if (reinterpret_cast<uintptr_t>(out) & (uintptr_t)(B - 1)) return fail(c, SRH_ERR_BAD_ARG, "srh_tiff_assemble: out is aligned to its samples");
    if (reinterpret_cast<uintptr_t>(table_dev) & 7) return fail(c, SRH_ERR_BAD_ARG, "srh_tiff_assemble: the device table is 8-byte aligned");
    long max_rows = 0;
    if (!tif_table_ok(table_host, n_seg, flat_bytes, H, W, C, B, &max_rows))
        return fail(c, SRH_ERR_BAD_ARG, "srh_tiff_assemble: an inconsistent table (a segment leaves the flat array or the raster, is misaligned, or its bytes are "
                                        "not rows x columns x samples)");
    const double ob = (double)H * W * C * B;
    if (ranges_overlap(out, ob, flat, (double)flat_bytes) || ranges_overlap(out, ob, table_dev, 56.0 * n_seg))
        return fail(c, SRH_ERR_BAD_ARG, "srh_tiff_assemble: out overlaps an input");
    TiffParams p;
    p.flat = flat; p.table = table_dev; p.n_seg = n_seg; p.max_rows = (int)max_rows; p.out = static_cast<uint8_t*>(out);
    p.H = H; p.W = W; p.C = C; p.B = B; p.predictor = predictor; p.big_endian = big_endian;
    hipSetDevice(c->device);
    hipStream_t s = (hipStream_t)stream;
    TRYK(c, "tiff_assemble", 0, (double)flat_bytes + ob, s, launch_tiff_assemble(p, s));
    return 0;
}
