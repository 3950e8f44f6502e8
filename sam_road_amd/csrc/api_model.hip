// C ABI, the model's launch sequences: SAMRoad.infer_masks_and_img_features (srh_encode_decode; encode_batch is also pass 1's batch,
// api_scene.hip) and infer_toponet.  Host-side C++ only; all arithmetic is in the kernels.
#include "ctx.hpp"

// ---- encoder + decoder -------------------------------------------------------------------------------
double attn_flops(int B, int S, int heads, int hd, int win) {
    if (win == S) return 4.0 * B * heads * (double)S * S * S * S * hd;
    const int nw = (S + win - 1) / win;
    double q = 0;
    for (int wy = 0; wy < nw; ++wy)
        for (int wx = 0; wx < nw; ++wx)
            q += (double)std::min(win, S - wy * win) * std::min(win, S - wx * win);
    return 4.0 * B * heads * q * win * win * hd;
}

static int ensure_encoder_ws(srh_ctx* c, const srh_weights* w, int B) {
    const size_t T = (size_t)B * w->S * w->S, D = w->D;
    int rc = 0;
    rc |= c->a0.ensure(T * 768 * 2);
    rc |= c->x.ensure(T * D * 4);
    rc |= c->xn16.ensure(T * D * 2);
    rc |= c->delta16.ensure(T * D * 2);
    rc |= c->delta16b.ensure(T * D * 2);
    rc |= c->qkv16.ensure(T * 3 * D * 2);
    rc |= c->attn16.ensure(T * D * 2);
    rc |= c->hid16.ensure(T * 4 * D * 2);
    rc |= c->n1.ensure(T * 256 * 4);
    rc |= c->n1_16.ensure(T * 256 * 2);
    rc |= c->n2.ensure(T * 256 * 4);
    rc |= c->emb16.ensure(T * 256 * 2);
    return rc ? fail(c, SRH_ERR_HIP, "workspace allocation failed") : 0;
}

// ---- SAM MaskDecoder branch (model.py:426-443 / :471-488; kernels in sam_decoder.hip, semantics in oracle/sam_decoder.py) ----
int sam_decode(srh_ctx* c, const srh_weights* w, int B, const float* emb, float* logits, float* scores, hipStream_t s) {
    const int S = w->S, HW = S * S, R = B * 4, P = w->cfg.patch_size;
    const size_t T = (size_t)B * HW;
    const SdW& d = w->sd;
    int rc = 0;
    rc |= c->sd_keys.ensure(T * 256 * 4);  rc |= c->sd_keys16.ensure(T * 256 * 2);
    rc |= c->sd_k16.ensure(T * 128 * 2);   rc |= c->sd_v16.ensure(T * 128 * 2);  rc |= c->sd_a16.ensure(T * 128 * 2);
    rc |= c->sd_u0.ensure(T * 256 * 4);    rc |= c->sd_u0_16.ensure(T * 256 * 2); rc |= c->sd_u1_16.ensure(T * 4 * 128 * 2);
    rc |= c->sd_low.ensure((size_t)B * 2 * 16 * HW * 4);
    rc |= c->sd_tok.ensure((size_t)R * (256 * 8 + 2048 + 128 * 4) * 4 + (size_t)B * 3 * (256 * 2 + 32) * 4);
    if (rc) return fail(c, SRH_ERR_HIP, "SAM decoder workspace allocation failed");
    float* keys = c->sd_keys.as<float>();
    f16* keys16 = c->sd_keys16.as<f16>();
    // token-side scratch (f32): q (queries), t0..t6 temporaries [R,256], h [R,2048], small [R,128] x 4, hyper
    float* tb = c->sd_tok.as<float>();
    float* q = tb;              float* t0 = tb + (size_t)R * 256; float* t1 = t0 + (size_t)R * 256; float* t2 = t1 + (size_t)R * 256;
    float* t3 = t2 + (size_t)R * 256; float* qn = t3 + (size_t)R * 256;   /* qn, qn+R*256: two more [R,256] */
    float* hid = tb + (size_t)R * 256 * 8;
    float* s0 = hid + (size_t)R * 2048; float* s1 = s0 + (size_t)R * 128; float* s2 = s1 + (size_t)R * 128; float* s3 = s2 + (size_t)R * 128;
    float* hy0 = s3 + (size_t)R * 128; float* hy1 = hy0 + (size_t)B * 3 * 256; float* hyper = hy1 + (size_t)B * 3 * 256;

    auto lin = [&](const float* x, int ldx, const float* xadd, int add_rows, const float* W, const float* b, int rows, int N, int K,
                   int act, float* y, int ldy) -> int {
        SdLinearParams lp;
        lp.x = x; lp.ldx = ldx; lp.xadd = xadd; lp.add_rows = add_rows; lp.W = W; lp.b = b; lp.rows = rows; lp.N = N; lp.K = K;
        lp.act = act; lp.y = y; lp.ldy = ldy;
        return launch_sd_tok_linear(lp, s);
    };
    auto img_gemm = [&](const char* cls, const f16* A, int K, const f16* W, int N, const float* bias, const float* pos,
                        const float* resid, int act, float* o32, f16* o16, size_t rows) -> int {
        GemmParams g = gemm_nt(A, W, (int)rows, N, K);
        g.bias = bias; g.pos = pos; g.pos_rows = HW; g.resid = resid; g.ldr = N; g.act = act;
        g.out_f32 = o32; g.ldc = N; g.out_f16 = o16; g.ldc16 = N;
        return gemm(c, cls, g, s);
    };
    // token -> image attention + residual + LayerNorm on the tokens: q <- LN(q + attn((q + pe_tok) Wq, (keys + pe) Wk, keys Wv) Wo)
    auto t2i = [&](const SdT2IW& a, const float* ng, const float* nb) -> int {
        TRY(img_gemm("sd_gemm", keys16, 256, a.k_w, 128, a.k_b, a.k_pos, nullptr, 0, nullptr, c->sd_k16.as<f16>(), T));
        TRY(img_gemm("sd_gemm", keys16, 256, a.v_w, 128, a.v_b, nullptr, nullptr, 0, nullptr, c->sd_v16.as<f16>(), T));
        TRYK(c, "sd_token", 0, 0, s, lin(q, 256, d.tokens, 4, a.q_w, a.q_b, R, 128, 256, 0, s0, 128));
        TRYK(c, "sd_attn", 0, 0, s, launch_sd_t2i_attn(s0, c->sd_k16.as<f16>(), c->sd_v16.as<f16>(), s1, B, HW, s));
        TRYK(c, "sd_token", 0, 0, s, lin(s1, 128, nullptr, 1, a.o_w, a.o_b, R, 256, 128, 0, t0, 256));
        TRYK(c, "sd_token", 0, 0, s, launch_sd_tok_ln(q, t0, ng, nb, q, R, s));
        return 0;
    };

    TRYK(c, "sd_prep", 0, (double)T * 256 * 10, s, launch_sd_add_channel(emb, d.no_mask, keys, keys16, T, s));
    // queries = the 4 output tokens, identical for every tile
    for (int b = 0; b < B; ++b)
        if (hipMemcpyAsync(q + (size_t)b * 1024, d.tokens, 4 * 256 * 4, hipMemcpyDeviceToDevice, s) != hipSuccess)
            return fail(c, SRH_ERR_HIP, "token broadcast failed");
    for (int l = 0; l < 2; ++l) {
        const SdLayerW& L = d.layer[l];
        // (1) self attention of the tokens; layer 0 skips the positional term and REPLACES the queries (skip_first_layer_pe)
        const float* pe_tok = l == 0 ? nullptr : d.tokens;
        TRYK(c, "sd_token", 0, 0, s, lin(q, 256, pe_tok, 4, L.self.q_w, L.self.q_b, R, 256, 256, 0, t0, 256));
        TRYK(c, "sd_token", 0, 0, s, lin(q, 256, pe_tok, 4, L.self.k_w, L.self.k_b, R, 256, 256, 0, t1, 256));
        TRYK(c, "sd_token", 0, 0, s, lin(q, 256, nullptr, 1, L.self.v_w, L.self.v_b, R, 256, 256, 0, t2, 256));
        TRYK(c, "sd_attn", 0, 0, s, launch_sd_tok_selfattn(t0, t1, t2, t3, B, s));
        TRYK(c, "sd_token", 0, 0, s, lin(t3, 256, nullptr, 1, L.self.o_w, L.self.o_b, R, 256, 256, 0, t0, 256));
        TRYK(c, "sd_token", 0, 0, s, launch_sd_tok_ln(t0, l == 0 ? nullptr : q, L.n1_g, L.n1_b, q, R, s));
        // (2) tokens attend to the image
        TRY(t2i(L.t2i, L.n2_g, L.n2_b));
        // (3) token MLP
        TRYK(c, "sd_token", 0, 0, s, lin(q, 256, nullptr, 1, L.l1_w, L.l1_b, R, 2048, 256, 2, hid, 2048));
        TRYK(c, "sd_token", 0, 0, s, lin(hid, 2048, nullptr, 1, L.l2_w, L.l2_b, R, 256, 2048, 0, t0, 256));
        TRYK(c, "sd_token", 0, 0, s, launch_sd_tok_ln(q, t0, L.n3_g, L.n3_b, q, R, s));
        // (4) image attends to the tokens: keys <- LN(keys + attn((keys + pe) Wq, (q + pe_tok) Wk, q Wv) Wo)
        TRY(img_gemm("sd_gemm", keys16, 256, L.i2t.q_w, 128, L.i2t.q_b, L.i2t.q_pos, nullptr, 0, nullptr, c->sd_k16.as<f16>(), T));
        TRYK(c, "sd_token", 0, 0, s, lin(q, 256, d.tokens, 4, L.i2t.k_w, L.i2t.k_b, R, 128, 256, 0, s2, 128));
        TRYK(c, "sd_token", 0, 0, s, lin(q, 256, nullptr, 1, L.i2t.v_w, L.i2t.v_b, R, 128, 256, 0, s3, 128));
        TRYK(c, "sd_attn", 0, 0, s, launch_sd_i2t_attn(c->sd_k16.as<f16>(), s2, s3, c->sd_a16.as<f16>(), B, HW, s));
        TRY(img_gemm("sd_gemm", c->sd_a16.as<f16>(), 128, L.i2t.o_w, 256, L.i2t.o_b, nullptr, keys, 0, c->sd_u0.as<float>(), nullptr, T));
        NormParams ln;
        ln.x = c->sd_u0.as<float>(); ln.M = (int)T; ln.D = 256; ln.eps = 1e-5f; ln.gamma = L.n4_g; ln.beta = L.n4_b;
        ln.out_f32 = keys; ln.out_f16 = keys16;
        TRYK(c, "layernorm", 0, (double)T * 256 * 10, s, launch_layernorm(ln, s));
    }
    TRY(t2i(d.fin, d.nf_g, d.nf_b));
    // output_upscaling: ConvT(256 -> 64) -> LayerNorm2d(64) -> GELU -> ConvT(64 -> 32) -> GELU, rows in quad-tree order
    TRY(img_gemm("sd_gemm", keys16, 256, d.up0_w, 256, d.up0_b, nullptr, nullptr, 0, c->sd_u0.as<float>(), nullptr, T));
    TRYK(c, "sd_prep", 0, (double)T * 256 * 6, s, launch_sd_ln64_gelu(c->sd_u0.as<float>(), d.up_ln_g, d.up_ln_b, c->sd_u0_16.as<f16>(), T * 4, s));
    TRY(img_gemm("sd_gemm", c->sd_u0_16.as<f16>(), 64, d.up1_w, 128, d.up1_b, nullptr, nullptr, 1, nullptr, c->sd_u1_16.as<f16>(), T * 4));
    // hyper-network MLPs on the three mask tokens (tokens 1..3 of every tile): [B,3,256] -> [B,3,32]
    for (int i = 0; i < 3; ++i) {
        TRYK(c, "sd_token", 0, 0, s, lin(q + (size_t)(1 + i) * 256, 4 * 256, nullptr, 1, d.hy_w[i][0], d.hy_b[i][0], B, 256, 256, 2, hy0 + (size_t)i * 256, 3 * 256));
        TRYK(c, "sd_token", 0, 0, s, lin(hy0 + (size_t)i * 256, 3 * 256, nullptr, 1, d.hy_w[i][1], d.hy_b[i][1], B, 256, 256, 2, hy1 + (size_t)i * 256, 3 * 256));
        TRYK(c, "sd_token", 0, 0, s, lin(hy1 + (size_t)i * 256, 3 * 256, nullptr, 1, d.hy_w[i][2], d.hy_b[i][2], B, 32, 256, 0, hyper + (size_t)i * 32, 3 * 32));
    }
    TRYK(c, "sd_prep", 0, (double)T * 16 * 72, s, launch_sd_mask(c->sd_u1_16.as<f16>(), hyper, c->sd_low.as<float>(), B, S, s));
    TRYK(c, "sd_prep", 0, (double)B * P * P * 16, s, launch_sd_upsample(c->sd_low.as<float>(), logits, scores, B, 4 * S, P, s));
    (void)qn; (void)t3;
    return 0;
}

// One lane of encode_batch's encoder: tiles [b0, b0 + B) of the batch as a chain of its own on stream s, from the patch im2col to the cast
// in front of the neck.  A lane is a view of the context's workspaces — every pointer starts at the lane's first token row, nothing is
// allocated per lane — with its own pending-branch state.  encode_batch runs ONE lane (the whole batch on the caller's stream: the launch
// sequence as it always was) or TWO half-batch lanes issued alternately, kernel by kernel (tiles never interact in the encoder).
struct EncLane {
    srh_ctx* c; const srh_weights* w; hipStream_t s;
    int idx, lanes;                                       // this lane / how many are in flight (the split-K workspace is shared out by it)
    int b0, B, T;                                         // first tile, tiles, token rows
    f16 *a0, *xn16, *delta16, *delta16b, *qkv16, *attn16, *hid16;
    float* x;
    bool pend_a = false, pend_b = false;                  // delta16 (patch embed / proj) / delta16b (fc2) hold a branch output not yet added to x
    bool x_is_pos = false;                                // x has not been written yet: its value is pos_embed (block 0's first pass)
    int pend_slices = 0; const float* pend_bias = nullptr; // split-K partials of the last branch GEMM wait in the lane's part of c->split_ws
    bool defer_x = false;                                 // both branch GEMMs of the blocks take z192 (same shapes in every block)

    EncLane(srh_ctx* c_, const srh_weights* w_, hipStream_t s_, int idx_, int lanes_, int b0_, int B_)
        : c(c_), w(w_), s(s_), idx(idx_), lanes(lanes_), b0(b0_), B(B_), T(B_ * w_->S * w_->S) {
        const size_t r0 = (size_t)b0 * w->S * w->S, D = w->D;       // blocked-16 hid16: 32-row blocks, so a row offset is the same bytes
        a0 = c->a0.as<f16>() + r0 * 768;       x = c->x.as<float>() + r0 * D;            xn16 = c->xn16.as<f16>() + r0 * D;
        delta16 = c->delta16.as<f16>() + r0 * D; delta16b = c->delta16b.as<f16>() + r0 * D; qkv16 = c->qkv16.as<f16>() + r0 * 3 * D;
        attn16 = c->attn16.as<f16>() + r0 * D;  hid16 = c->hid16.as<f16>() + r0 * 4 * D;
        GemmParams gq = gemm_nt(attn16, w->blocks.empty() ? nullptr : w->blocks[0].proj_w, T, (int)D, (int)D);
        gq.ldc16 = (int)D; gq.out_f16 = delta16; gq.bias = w->blocks.empty() ? nullptr : w->blocks[0].proj_b;
        GemmParams g2 = gq;
        g2.K = 4 * (int)D; g2.lda = 4 * (int)D; g2.ldw = 4 * (int)D;
        defer_x = !w->blocks.empty() && z192_preferred(gq) && z192_preferred(g2);
    }
    int im2col(PatchParams pp, int orient, int scene_H);
    int patch_embed();
    int branch_gemm(const char* cls, const f16* A, int lda, const f16* W, int K, const float* bias, bool second, int a_blocked = 0);
    int fold_pending(NormParams& ln, int& reads);
    int block_ln(const float* gamma, const float* beta, bool write_x, int nf_tag);
    int qkv(const BlockW& b);
    int attention(const BlockW& b);
    int hid_blocked = 0;                                  // fc1 -> fc2: the hidden activation is in the blocked-16 layout
    int fc1(const BlockW& b);
    int fc2(const BlockW& b);
    int neck_cast();
    int n_stages() const;
    int stage(int k, const PatchParams& pp, int orient, int scene_H);
};

int EncLane::im2col(PatchParams pp, int orient, int scene_H) {
    pp.B = B; pp.P = w->cfg.patch_size; pp.out = a0;
    if (pp.scene_W > 0) pp.tile_xy += 2 * b0;            // tiles cropped out of a resident scene
    else pp.src = (const char*)pp.src + (size_t)b0 * pp.P * pp.P * 3 * (pp.src_is_u8 ? 1 : 4);
    if (orient)          // TTA (scene_tta.hip): the crop is read through the orientation; everything after it is the same calls
        TRYK(c, "patch_im2col_oriented", 0, (double)T * 768 * 3, s, launch_patch_im2col_oriented(pp, scene_H, orient, s));
    else
    TRYK(c, "patch_im2col", 0, (double)T * 768 * (pp.src_is_u8 ? 3 : 6), s, launch_patch_im2col(pp, s));
    return 0;
}

int EncLane::patch_embed() {
    const int S = w->S, D = w->D;
    // Residual stream: x stays fp32.  Where the persistent z192 GEMM applies (gemm_z192.hip: fp16 output only), proj / fc2
    // write their branch output (bias included) as fp16 into delta16 and the NEXT LayerNorm pass folds "x += delta" into
    // its read of x — the same HBM bytes as the GEMM-epilogue residual add, but moved out of the GEMM's exposed epilogue
    // into a streaming kernel.  Otherwise the GEMM epilogue adds the residual itself.
    // When BOTH branch GEMMs of a block go through z192, the attention branch (delta16) is not written back to x by the second
    // LayerNorm — it only normalises x + delta16 — and the next block's first LayerNorm folds both branches, (x + delta16) +
    // delta16b, and writes x once per block: 275 instead of 300 MB of LayerNorm traffic per block at B = 16, same sums in the
    // same order bit for bit.
    // Small-M models (ViT-H / ViT-L at 256 px): fc2 runs with split-K, and instead of a reduce pass its f32 partials stay in the
    // workspace for the next LayerNorm pass (or the neck's cast) to fold — x += (slice 0 + slice 1 + ...) + bias, the reduce kernel's
    // order, same bits — one launch and one round trip of x less per block.
    // Patch embedding: where z192 applies (ViT-B widths, enough tiles) it is just another fp16 branch output — conv + bias into delta16 —
    // and block 0's first LayerNorm pass computes the initial residual x = pos_embed[token] + delta16 (a row-modulo read of the
    // [S*S, D] table, NormParams::x_period) and writes x: the proj-shaped GEMM takes 22 instead of 51 us on the f32 + pos epilogue.
    GemmParams g = gemm_nt(a0, w->patch_w, T, D, 768);
    g.bias = w->patch_b;
    GemmParams gz = g;
    gz.out_f16 = delta16; gz.ldc16 = D;
    if (!w->blocks.empty() && z192_preferred(gz)) {
        TRY(gemm(c, "gemm_patch_embed", gz, s, idx, lanes));
        pend_a = true; x_is_pos = true;
    } else {
        g.pos = w->pos; g.pos_rows = S * S; g.out_f32 = x; g.ldc = D;
        TRY(gemm(c, "gemm_patch_embed", g, s, idx, lanes));
    }
    return 0;
}

int EncLane::branch_gemm(const char* cls, const f16* A, int lda, const f16* W, int K, const float* bias, bool second, int a_blocked) {
    const int D = w->D;
    {
        GemmParams gq = gemm_nt(A, W, T, D, K);
        gq.lda = lda; gq.bias = bias; gq.a_blocked16 = a_blocked;
        gq.out_f16 = second ? delta16b : delta16; gq.ldc16 = D;
        if (z192_preferred(gq)) { (second ? pend_b : pend_a) = true; return gemm(c, cls, gq, s, idx, lanes); }
        // Small-M models (ViT-L / ViT-H at 256 px), the attention branch: proj runs unsplit on 128 x 128 ring tiles with ~9 us of fixed cost
        // on a ~9 us loop, and its f32 read-modify-write of x sat in that exposed epilogue.  Its output goes out as fp16 instead (half the
        // store instructions) and the LayerNorm pass that follows anyway folds it into x — the same bytes, moved into the streaming kernel
        // (what the z192 path does for ViT-B).
        if (!second && !pend_a && !pend_slices && (D == 1024 || D == 1280) && gemm_splitk_factor(gq) <= 1) { pend_a = true; return gemm(c, cls, gq, s, idx, lanes); }
        GemmParams gp = gq;
        gp.out_f16 = nullptr; gp.resid = x; gp.ldr = D; gp.out_f32 = x; gp.ldc = D;
        if (const int sk = gemm_splitk_factor(gp); sk > 1 && bias && (D == 1024 || D == 1280) && !pend_slices && !pend_a && !pend_b) {
            gp.defer_reduce = 1;
            pend_slices = sk; pend_bias = bias;
        }
        return gemm(c, cls, gp, s, idx, lanes);
    }
}

int EncLane::fold_pending(NormParams& ln, int& reads) {   // what the pass has to add to x before normalising / casting
    const int D = w->D;
    if (pend_slices && (pend_a || pend_b))            // never both: the fp16 branch would be dropped (branch_gemm defers only when neither is pending)
        return fail(c, SRH_ERR_HIP, "internal: split-K partials and an fp16 branch output pending at the same LayerNorm pass");
    if (pend_slices) {                                // the lane's part of the workspace, as gemm() (ctx.hpp) shared it out
        ln.slices = c->split_ws.as<float>() + (size_t)pend_slices * T * D * idx;
        ln.nslices = pend_slices; ln.slice_stride = (size_t)T * D; ln.slice_bias = pend_bias;
        reads = 2 * pend_slices;                      // in units of 2 bytes per element, as the fp16 branches
    } else if (pend_a && pend_b) { ln.delta16 = delta16; ln.delta16b = delta16b; reads = 2; }
    else if (pend_a) { ln.delta16 = delta16; reads = 1; }
    else if (pend_b) { ln.delta16 = delta16b; reads = 1; }
    return 0;
}

// a LayerNorm pass over x (+ pending branches).  write_x: fold the pending branches into x for good.
int EncLane::block_ln(const float* gamma, const float* beta, bool write_x, int nf_tag) {
    const int S = w->S, D = w->D;
    NormParams ln;
    ln.x = x; ln.M = T; ln.D = D; ln.eps = 1e-6f; ln.out_f16 = xn16;
    ln.gamma = gamma; ln.beta = beta; ln.nf = c->nf_dev; ln.nf_tag = std::min(nf_tag, NF_NECK - 1);
    if (x_is_pos) { ln.x = w->pos; ln.x_period = S * S; }
    int reads = 0;
    TRY(fold_pending(ln, reads));
    const bool wr = (write_x || pend_slices || x_is_pos) && reads > 0;   // partials cannot wait: the next split-K GEMM overwrites the workspace
    ln.x_out = wr ? x : nullptr;
    TRYK(c, "layernorm", 0, (double)T * D * (4 + 2 + 2 * reads + (wr ? 4 : 0)), s, launch_layernorm(ln, s));
    if (wr) { pend_a = pend_b = false; pend_slices = 0; x_is_pos = false; }
    return 0;
}

int EncLane::qkv(const BlockW& b) {
    const int D = w->D;
    GemmParams g = gemm_nt(xn16, b.qkv_w, T, 3 * D, D);
    g.bias = b.qkv_b; g.out_f16 = qkv16; g.ldc16 = 3 * D;
    return gemm(c, "gemm_qkv", g, s, idx, lanes);
}

int EncLane::attention(const BlockW& b) {
    const int S = w->S, heads = w->heads, hd = w->hd;
    const AttnParams ap = attn_params(qkv16, b.rel_h, b.rel_w, b.qkv_b16, attn16, B, S, heads, hd, b.win);
    TRYK(c, b.win == S ? "attn_global" : "attn_window", attn_flops(B, S, heads, hd, b.win), 0, s, launch_attention(ap, s));
    return 0;
}

int EncLane::fc1(const BlockW& b) {
    const int D = w->D;
    GemmParams g1 = gemm_nt(xn16, b.fc1_w, T, 4 * D, D);
    g1.bias = b.fc1_b; g1.act = 1; g1.out_f16 = hid16; g1.ldc16 = 4 * D;
    // the hidden activation lives only between these two launches: when both take gemm_z192 it is kept in the blocked-16 layout
    // (fc1 stores 1 KiB contiguous per instruction, no LDS transposition; fc2's LDS-DMA reads it through per-lane addresses)
    {
        GemmParams t1 = g1, t2 = gemm_nt(hid16, b.fc2_w, T, D, 4 * D);
        t1.out_blocked16 = 1; t2.bias = b.fc2_b;
        t2.out_f16 = delta16b; t2.ldc16 = D; t2.a_blocked16 = 1;
        hid_blocked = z192_preferred(t1) && z192_preferred(t2);
    }
    g1.out_blocked16 = hid_blocked;
    return gemm(c, "gemm_fc1", g1, s, idx, lanes);
}

int EncLane::fc2(const BlockW& b) {
    const int D = w->D;
    return branch_gemm("gemm_fc2", hid16, 4 * D, b.fc2_w, 4 * D, b.fc2_b, true, hid_blocked);
}

int EncLane::neck_cast() {           // x (+ the last block's branch outputs, if still pending) as fp16 for the neck's 1x1 conv
    const int D = w->D;
    NormParams cast;
    cast.x = x; cast.M = T; cast.D = D; cast.out_f16 = xn16;
    int reads = 0;
    TRY(fold_pending(cast, reads));
    TRYK(c, "layernorm", 0, (double)T * D * (6 + 2 * reads), s, launch_layernorm(cast, s));
    return 0;
}

// Auto's shape rule: two lanes only where a HALF batch still runs the patch embed and every block GEMM on gemm_z192 with enough tiles to
// occupy the chip (ViT-B with B/2 * S * S >= 8192) — then no lane touches split-K partials, and every kernel of a lane is the kernel the
// whole batch would run, on half the rows.
static bool lanes_pay(srh_ctx* c, const srh_weights* w, int B) {
    if (B < 2 || B % 2 || w->blocks.empty()) return false;
    const int D = w->D, T = B / 2 * w->S * w->S;
    const BlockW& b = w->blocks[0];
    f16* o = c->delta16.as<f16>();                        // any non-null output: only the shapes are looked at
    auto z = [&](const f16* W, const float* bias, int N, int K, int act) {
        GemmParams g = gemm_nt(o, W, T, N, K);
        g.bias = bias; g.act = act; g.out_f16 = o; g.ldc16 = N;
        return z192_preferred(g);
    };
    return z(w->patch_w, w->patch_b, D, 768, 0) && z(b.qkv_w, b.qkv_b, 3 * D, D, 0) && z(b.proj_w, b.proj_b, D, D, 0) &&
           z(b.fc1_w, b.fc1_b, 4 * D, D, 1) && z(b.fc2_w, b.fc2_b, D, 4 * D, 0);
}

// Lane 1's stream and the two events that tie it to the caller's stream; made at the first two-lane call of the context.
static int ensure_lane_stream(srh_ctx* c) {
    if (!c->lane_stream && hipStreamCreateWithFlags(&c->lane_stream, hipStreamNonBlocking) != hipSuccess) { c->lane_stream = nullptr; return fail(c, SRH_ERR_HIP, "lane stream creation failed"); }
    if (!c->lane_fork && hipEventCreateWithFlags(&c->lane_fork, hipEventDisableTiming) != hipSuccess) { c->lane_fork = nullptr; return fail(c, SRH_ERR_HIP, "lane event creation failed"); }
    if (!c->lane_join && hipEventCreateWithFlags(&c->lane_join, hipEventDisableTiming) != hipSuccess) { c->lane_join = nullptr; return fail(c, SRH_ERR_HIP, "lane event creation failed"); }
    return 0;
}

// A lane's chain as numbered stages, one launch each: 0 patch im2col, 1 patch embed, then per block norm1, qkv, attention, proj, norm2,
// fc1, fc2, and last the cast in front of the neck.
int EncLane::n_stages() const { return 2 + 7 * (int)w->blocks.size() + 1; }
int EncLane::stage(int k, const PatchParams& pp, int orient, int scene_H) {
    if (k == 0) return im2col(pp, orient, scene_H);
    if (k == 1) return patch_embed();
    const int blk = (k - 2) / 7, D = w->D;
    if (blk >= (int)w->blocks.size()) return neck_cast();
    const BlockW& b = w->blocks[blk];
    switch ((k - 2) % 7) {
        case 0: return block_ln(b.ln1_g, b.ln1_b, true, 2 * blk);
        case 1: return qkv(b);
        case 2: return attention(b);
        case 3: return branch_gemm("gemm_proj", attn16, D, b.proj_w, D, b.proj_b, false);
        case 4: return block_ln(b.ln2_g, b.ln2_b, !defer_x, 2 * blk + 1);
        case 5: return fc1(b);
        default: return fc2(b);
    }
}

// How far lane 0 runs ahead: lane 1 is forked behind lane 0's first SRH_LANE_LAG stages and is issued that many launches behind.  3 = behind
// block 0's norm1, one stage out of step: whenever a lane is in a LayerNorm pass (HBM-bound, no LDS) the other one is in a GEMM (one
// wave per SIMD, the LDS), and the two share the CUs.  Measured same-box against one lane at ViT-B 512 px B = 16: lag 0 (lockstep) +0.9 %,
// 3 +2.1 %, 4 (behind qkv) +1.3 %, 5 +0.8 %, 6 / 7 +0.4 % tiles/s (profiles/lanes_ab_same_box.txt).
#ifndef SRH_LANE_LAG
#define SRH_LANE_LAG 3
#endif

int encode_batch(srh_ctx* c, const srh_weights* w, PatchParams pp, int B, float* logits, float* scores, float* emb, hipStream_t s, int orient,
                 int scene_H) {
    const int S = w->S, D = w->D;
    const int T = B * S * S;
    TRY(ensure_encoder_ws(c, w, B));
    // Lanes: srh_ctx_set_lanes' mode; profiling is always one lane, so that the event pairs around a launch time that launch alone
    int nl = 1;
    if (!c->profiling && B % 2 == 0 && (c->lanes_mode == 2 || (c->lanes_mode == 0 && lanes_pay(c, w, B)))) nl = 2;
    c->last_lanes = nl;
    if (nl == 1) {
        EncLane one(c, w, s, 0, 1, 0, B);
        for (int k = 0, n = one.n_stages(); k < n; ++k) TRY(one.stage(k, pp, orient, scene_H));
    } else {
        // Two lanes, their launches issued alternately so that both queues stay fed.  Fork: lane 1 starts behind what is queued on the
        // caller's stream (lane 0's first stages included).  Join: the caller's stream goes on behind lane 1 — on every return path
        // after the fork, so that the caller sees one stream: outputs ordered on it, the input free to be overwritten on it after the call.
        TRY(ensure_lane_stream(c));
        EncLane lane[2] = {EncLane(c, w, s, 0, 2, 0, B / 2), EncLane(c, w, c->lane_stream, 1, 2, B / 2, B / 2)};
        const int n = lane[0].n_stages(), lag = std::min(SRH_LANE_LAG, n);
        for (int k = 0; k < lag; ++k) TRY(lane[0].stage(k, pp, orient, scene_H));
        if (hipEventRecord(c->lane_fork, s) != hipSuccess || hipStreamWaitEvent(c->lane_stream, c->lane_fork, 0) != hipSuccess)
            return fail(c, SRH_ERR_HIP, "lane fork failed");
        int rc = 0;
        for (int k = 0; k < n && !rc; ++k) {
            rc = lane[1].stage(k, pp, orient, scene_H);
            if (!rc && k + lag < n) rc = lane[0].stage(k + lag, pp, orient, scene_H);
        }
        if (hipEventRecord(c->lane_join, c->lane_stream) != hipSuccess || hipStreamWaitEvent(s, c->lane_join, 0) != hipSuccess) {
            hipStreamSynchronize(c->lane_stream);         // the join could not be queued: wait for lane 1 here instead
            if (!rc) return fail(c, SRH_ERR_HIP, "lane join failed");
        }
        if (rc) return rc;
    }
    // neck: 1x1 conv -> LN2d -> 3x3 conv -> LN2d  (channels-last: LN2d is a row LN), on the whole batch
    {
        GemmParams g = gemm_nt(c->xn16.as<f16>(), w->neck0_w, T, 256, D);
        g.out_f32 = c->n1.as<float>(); g.ldc = 256;
        TRY(gemm(c, "gemm_neck", g, s));
        NormParams ln;
        ln.x = c->n1.as<float>(); ln.M = T; ln.D = 256; ln.eps = 1e-6f; ln.gamma = w->neck1_g; ln.beta = w->neck1_b;
        ln.out_f16 = c->n1_16.as<f16>(); ln.nf = c->nf_dev; ln.nf_tag = NF_NECK;
        TRYK(c, "layernorm", 0, (double)T * 256 * 6, s, launch_layernorm(ln, s));
        GemmParams g3 = gemm_nt(c->n1_16.as<f16>(), w->neck2_w, T, 256, 2304);
        g3.lda = 256; g3.conv_S = S; g3.conv_C = 256; g3.out_f32 = c->n2.as<float>(); g3.ldc = 256;
        TRY(gemm(c, "gemm_neck", g3, s));
        ln.x = c->n2.as<float>(); ln.gamma = w->neck3_g; ln.beta = w->neck3_b;
        ln.out_f16 = c->emb16.as<f16>(); ln.out_f32 = emb; ln.nf_tag = NF_NECK + 1;
        TRYK(c, "layernorm", 0, (double)T * 256 * 10, s, launch_layernorm(ln, s));
    }
    if (!logits && !scores) return 0;
    if (w->cfg.use_sam_decoder) return sam_decode(c, w, B, emb, logits, scores, s);
    // map_decoder: all four ConvT layers + LayerNorm2d + GELUs + sigmoid + scatter in ONE kernel (decoder.hip), 8 MB in, the masks out
    {
        const DecodeFusedParams dp = decode_params(c, w, c->emb16.as<f16>(), B, logits, scores);
        const double fl = 2.0 * T * (256.0 * 512 + 4 * 128.0 * 256 + 16 * 64.0 * 128 + 64 * 32.0 * 8);
        TRYK(c, "map_decoder", fl, (double)T * 512 + (double)T * 256 * ((logits ? 8 : 0) + (scores ? 8 : 0)), s, launch_decode_fused(dp, s));
    }
    return 0;
}

extern "C" int srh_encode_decode(srh_ctx* c, const srh_weights* w, const void* rgb, int rgb_dtype, int B,
                                 float* mask_logits, float* mask_scores, float* embeddings, void* stream) {
    if (!c || !w || !rgb || !embeddings || B <= 0) return fail(c, SRH_ERR_BAD_ARG, "srh_encode_decode: bad argument");
    if (rgb_dtype != SRH_F32 && rgb_dtype != SRH_U8) return fail(c, SRH_ERR_BAD_ARG, "rgb dtype must be f32 or u8");
    TRY(nonfinite_check(c, "srh_encode_decode"));          // lazily: what an EARLIER call's LayerNorm passes flagged (no sync here)
    hipSetDevice(c->device);
    PatchParams pp;
    pp.src = rgb; pp.src_is_u8 = rgb_dtype == SRH_U8;
    return encode_batch(c, w, pp, B, mask_logits, mask_scores, embeddings, (hipStream_t)stream);
}

// ---- TopoNet --------------------------------------------------------------------------------------------
static int toponet_impl(srh_ctx* c, const srh_weights* w, const float* embeddings, const void* points,
                        int points_dtype, const void* pairs, int pairs_dtype, const uint8_t* valid, int B, int N,
                        int Ns, int K, float* logits, float* scores, const int* point_tile, int n_tiles, long pair_base, void* stream) {
    if (!c || !w || !embeddings || !points || !pairs || !valid) return fail(c, SRH_ERR_BAD_ARG, "srh_toponet: null argument");
    if (B <= 0 || N < 0 || Ns < 0) return fail(c, SRH_ERR_BAD_ARG, "srh_toponet: bad sizes");
    if (K < 1 || K > 64) return fail(c, SRH_ERR_UNSUPPORTED, "n_pairs (MAX_NEIGHBOR_QUERIES) must be 1 to 64");
    if (points_dtype != SRH_I64 && points_dtype != SRH_F32) return fail(c, SRH_ERR_BAD_ARG, "points dtype must be i64 or f32");
    if (pairs_dtype != SRH_I64 && pairs_dtype != SRH_I32) return fail(c, SRH_ERR_BAD_ARG, "pairs dtype must be i64 or i32");
    if (N == 0 || Ns == 0) return 0;
    hipSetDevice(c->device);
    hipStream_t s = (hipStream_t)stream;
    const size_t NP = (size_t)B * N, R = (size_t)B * Ns * K;
    int rc = 0;
    rc |= c->t_feat16.ensure(NP * 256 * 2, 0.25);
    rc |= c->t_pf16.ensure(NP * 128 * 2, 0.25);
    rc |= c->t_pair16.ensure(R * 320 * 2, 0.25);
    if (rc) return fail(c, SRH_ERR_HIP, "toponet workspace allocation failed");

    const SampleParams sp = sample_params(embeddings, n_tiles, w->S, w->S, 256, points, points_dtype, point_tile, B, N, (float)w->cfg.patch_size,
                                          nullptr, c->t_feat16.as<f16>());
    TRYK(c, "bilinear_sample", 0, (double)NP * 256 * 18, s, launch_sample(sp, s));
    GemmParams g = gemm_nt(c->t_feat16.as<f16>(), w->tp_feat_w, (int)NP, 128, 256);
    g.bias = w->tp_feat_b; g.act = 2; g.out_f16 = c->t_pf16.as<f16>(); g.ldc16 = 128;
    TRY(gemm(c, "gemm_toponet", g, s));
    PairGatherParams pg = pair_gather_params(c->t_pf16.as<f16>(), points, points_dtype, pairs, pairs_dtype, B, N, Ns, K,
                                             w->cfg.toponet_version == 1, pair_base, c->t_pair16.as<f16>(), 320);
    if (point_tile) { pg.point_tile = point_tile; pg.bad = c->nf_dev + NF_PAIRS; }      // ragged rows: pairs stay inside their tile
    TRYK(c, "pair_gather", 0, (double)R * (512 + 640), s, launch_pair_gather(pg, s));
    {
        // pair_proj + encoder layers + output_proj in one register-resident kernel (topo_fused.hip)
        const TopoFusedParams tf = topo_fused_params(w, c->t_pair16.as<f16>(), 320, valid, B * Ns, K, logits, scores);
        const double fl = (double)R * (2.0 * 320 * 128 + tf.nlayers * (2.0 * 128 * 768 + 4.0 * K * 128) + 256);
        TRYK(c, "topo_fused", fl, 0, s, launch_topo_fused(tf, s));
        return 0;
    }
}

extern "C" int srh_toponet(srh_ctx* c, const srh_weights* w, const float* embeddings, const void* points,
                           int points_dtype, const void* pairs, int pairs_dtype, const uint8_t* valid, int B, int N,
                           int Ns, int K, float* logits, float* scores, void* stream) {
    return toponet_impl(c, w, embeddings, points, points_dtype, pairs, pairs_dtype, valid, B, N, Ns, K, logits, scores, nullptr, 0, 0, stream);
}

// The query rows of MANY tiles in one call, without padding every tile to the longest one of its batch: rows are the concatenated
// per-tile point lists (srh_pass2_pack_ragged), every point names the tile whose embeddings it samples, pairs index the flat list.
// The sampler, feature_proj, pair gather and the fused trunk treat every row on its own, so the scores are those of srh_toponet.
extern "C" int srh_toponet_ragged(srh_ctx* c, const srh_weights* w, const float* embeddings, int n_tiles, const float* points,
                                  const int32_t* point_tile, const int32_t* pairs, const uint8_t* valid, int64_t R, int K,
                                  const int64_t* tile_offsets, float* scores, void* stream) {
    if (!point_tile || !scores) return fail(c, SRH_ERR_BAD_ARG, "srh_toponet_ragged: null argument");
    if (n_tiles <= 0) return fail(c, SRH_ERR_BAD_ARG, "srh_toponet_ragged: n_tiles must be the number of tiles in `embeddings`");
    if (R < 0) return fail(c, SRH_ERR_BAD_ARG, "srh_toponet_ragged: bad row count");
    if (K < 1 || K > 64) return fail(c, SRH_ERR_UNSUPPORTED, "srh_toponet_ragged: n_pairs (MAX_NEIGHBOR_QUERIES) must be 1 to 64");
    // Workspace bound (the reference's pass 2 is bounded by INFER_BATCH_SIZE, inferencer.py:179-207): with the tiles' row offsets the
    // scene is scored in chunks of whole tiles of at most RAGGED_CHUNK_PAIRS pairs (16 384 rows at K = 16) — rows are independent and a
    // pair only names rows of its own tile, so the chunks' scores are those of the one launch, bit for bit — and the pair workspace
    // stays below ~210 MB whatever K and however large the scene (it grew with the scene before: 0.6 GB for a 48 k-row CityScale scene,
    // ~10 GB for an 8192^2 one).  Without offsets the caller's rows go through ONE launch and must fit 4x that bound.
    constexpr int64_t RAGGED_CHUNK_PAIRS = 16384 * 16;
    const int64_t chunk_rows = RAGGED_CHUNK_PAIRS / K;
    if (!tile_offsets) {
        if (R * K > 4 * RAGGED_CHUNK_PAIRS)
            return fail(c, SRH_ERR_BAD_ARG, "srh_toponet_ragged: more than 1048576 pairs (rows x n_pairs) need tile_offsets (chunked at tile boundaries)");
        return toponet_impl(c, w, embeddings, points, SRH_F32, pairs, SRH_I32, valid, 1, (int)R, (int)R, K, nullptr, scores, point_tile, n_tiles, 0, stream);
    }
    if (tile_offsets[0] != 0 || tile_offsets[n_tiles] != R) return fail(c, SRH_ERR_BAD_ARG, "srh_toponet_ragged: tile_offsets must run from 0 to R");
    for (int t = 0; t < n_tiles; ++t)
        if (tile_offsets[t + 1] < tile_offsets[t]) return fail(c, SRH_ERR_BAD_ARG, "srh_toponet_ragged: tile_offsets must ascend");
    for (int ta = 0; ta < n_tiles;) {
        int tb = ta + 1;                                                          // at least one tile (a tile above the bound is its own chunk)
        while (tb < n_tiles && tile_offsets[tb + 1] - tile_offsets[ta] <= chunk_rows) ++tb;
        const int64_t r0 = tile_offsets[ta], n = tile_offsets[tb] - r0;
        if (n > 0x7fffffffLL / (2 * K)) return fail(c, SRH_ERR_BAD_ARG, "srh_toponet_ragged: a single tile has too many rows");
        if (n > 0)
            TRY(toponet_impl(c, w, embeddings, points + 2 * r0, SRH_F32, pairs + 2 * (int64_t)K * r0, SRH_I32, valid + (int64_t)K * r0, 1, (int)n, (int)n,
                             K, nullptr, scores + (int64_t)K * r0, point_tile + r0, n_tiles, (long)r0, stream));
        ta = tb;
    }
    return 0;
}
