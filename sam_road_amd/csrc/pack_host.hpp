// Weight packing: state_dict entries -> the image of the device arena + the pointer table's fix-ups.  Pure host arithmetic, no HIP
// header: api_weights.hip uploads the result, tests/pack_layout_check.cpp checks it on a CPU.
//   Packer pk; pk.layout_only = ...; pk.d2h = ...; pack_model(pk, w, tensors, n);
//   -> pk.host (arena image), pk.fix (pointer slot of *w, arena offset), pk.missing (first missing or mis-shaped name)
// layout_only: no tensor is read; the SAME sequence of allocations as a real pass, so the layout depends on w->cfg alone (srh_weights_import).
#pragma once
#include <cmath>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "pack_layout.hpp"
#include "weights.hpp"

namespace srh {
namespace {      // internal linkage: the including unit exports none of it

// One 16 (out) x 32 (in) MFMA A fragment of the f32 matrix W (row length ldw), rows row0 .. row0 + 15, k block kb: lane l = (row i = l & 15,
// k group g = l >> 4) holds 8 halves W[row0 + i][k(kb, g, j)].  A matrix whose input is read from memory has the natural order
// k = 32 kb + 8 g + j; one whose input is a C-layout tile pair of the previous MFMA the permuted k = 32 kb + 16 (j >> 2) + 4 g + (j & 3).
// k >= kmax, or W == nullptr, gives zeros.
inline void write_frag(f16* o, const float* W, int ldw, int row0, int kb, bool perm, int kmax) {
    for (int l = 0; l < 64; ++l)
        for (int j = 0; j < 8; ++j) {
            const int i = l & 15, g = l >> 4;
            const int k = perm ? 32 * kb + 16 * (j >> 2) + 4 * g + (j & 3) : 32 * kb + 8 * g + j;
            o[l * 8 + j] = (W && k < kmax) ? (f16)W[(size_t)(row0 + i) * ldw + k] : (f16)0.f;
        }
}

// A ConvTranspose2d(k2, s2) layer is a per-pixel GEMM to 4 x cout columns, n = (ky * 2 + kx) * cout + co: element (n, ci) of the GEMM
// weight is element convt_src of the layer's weight [cin][cout][ky][kx]
inline size_t convt_src(size_t n, size_t ci, size_t cout) { return (ci * cout + n % cout) * 4 + n / cout; }

struct Packer {
    bool layout_only = false;
    bool (*d2h)(void* dst, const void* src, size_t bytes) = nullptr;   // device -> host copy for on_device tensors (none: they fail)
    std::vector<char> host;                       // staging image of the device arena
    std::vector<std::pair<void**, size_t>> fix;   // pointer slots to patch with arena + offset
    std::string missing;
    std::vector<std::pair<std::string, size_t>>* asked = nullptr;   // if set: every (name, element count) the pass asks for, in order
    std::map<std::string, const srh_named_tensor*> by_name;
    std::vector<float> tmp;

    size_t alloc(size_t bytes) {
        const size_t off = (host.size() + 255) & ~size_t(255);
        host.resize(off + bytes);
        return off;
    }
    // fetch tensor as host f32 (copying from device if needed); checks element count
    const float* get(const std::string& name, size_t expect) {
        if (asked) asked->push_back({name, expect});
        if (layout_only) return nullptr;
        auto it = by_name.find(name);
        if (it == by_name.end()) { if (missing.empty()) missing = name; return nullptr; }
        const srh_named_tensor* t = it->second;
        size_t n = 1;
        for (int i = 0; i < t->ndim; ++i) n *= (size_t)t->shape[i];
        if (n != expect) { if (missing.empty()) missing = name + " (shape mismatch)"; return nullptr; }
        if (!t->on_device) return reinterpret_cast<const float*>(t->data);
        tmp.resize(n);
        if (!d2h || !d2h(tmp.data(), t->data, n * 4)) {
            if (missing.empty()) missing = name + " (D2H copy failed)";
            return nullptr;
        }
        return tmp.data();
    }
    template <class T> void slot(T** dst, size_t off) { fix.push_back({reinterpret_cast<void**>(dst), off}); }
    template <class T> T* at(size_t off) { return reinterpret_cast<T*>(host.data() + off); }

    void put_f32(float** dst, const std::string& name, size_t n) {
        const float* src = get(name, n);
        const size_t off = alloc(n * 4);
        if (src) memcpy(host.data() + off, src, n * 4);
        slot(dst, off);
    }
    // fp16 copy with an index map: out[i] = src[map(i)]
    template <class Map>
    void put_f16(f16** dst, const std::string& name, size_t n_src, size_t n_out, Map map) {
        const float* src = get(name, n_src);
        const size_t off = alloc(n_out * 2);
        if (src)
            for (size_t i = 0; i < n_out; ++i) at<f16>(off)[i] = (f16)src[map(i)];
        slot(dst, off);
    }
    void put_f16_same(f16** dst, const std::string& name, size_t n) {
        put_f16(dst, name, n, n, [](size_t i) { return i; });
    }
    // n f32 parameters into a block allocated at poff, from float index idx
    void put_prm(size_t poff, size_t idx, const std::string& name, size_t n) {
        const float* src = get(name, n);
        if (src) memcpy(host.data() + poff + idx * 4, src, n * 4);
    }
};

// Weights of the fused TopoNet trunk (topo_fused.hip): every matrix cut into write_frag fragments in the exact order the kernel
// consumes them.  pair_proj reads its input from memory (natural k, 258 of 320 columns); every later matrix reads activations that
// are C-layout tile pairs of the previous MFMA (permuted k).
inline void pack_topo_fused(Packer& pk, srh_weights* w, int nl) {
    const std::string T = "topo_net.";
    const size_t soff = pk.alloc((size_t)tf_nfrag(nl) * FRAG_BYTES), poff = pk.alloc((size_t)tf_nprm(nl) * 4);
    size_t f = 0;      // next fragment
    auto frag = [&](const float* W, int ldw, int row0, int kb, bool perm) { write_frag(pk.at<f16>(soff) + f++ * 512, W, ldw, row0, kb, perm, ldw); };
    {
        const float* W = pk.get(T + "pair_proj.weight", 128 * 258);
        for (int kb = 0; kb < 10; ++kb)
            for (int rt = 0; rt < 8; ++rt) frag(W, 258, 16 * rt, kb, false);
    }
    pk.put_prm(poff, TF_P_PAIR_B, T + "pair_proj.bias", 128);
    for (int l = 0; l < nl; ++l) {
        const std::string L = T + "transformer_encoder.layers." + std::to_string(l) + ".";
        const size_t pb = tf_pb(l);
        {
            const float* W = pk.get(L + "self_attn.in_proj_weight", 384 * 128);
            for (int c = 0; c < 8; ++c)
                for (int kb = 0; kb < 4; ++kb) frag(W, 128, 256 + 16 * c, kb, true);                    // V
            for (int h = 0; h < 4; ++h)
                for (int i = 0; i < 4; ++i)                                                             // Q 2h, Q 2h+1, K 2h, K 2h+1
                    for (int kb = 0; kb < 4; ++kb) frag(W, 128, (i >> 1) * 128 + 16 * (2 * h + (i & 1)), kb, true);
        }
        for (const char* m : {"self_attn.out_proj.weight", "linear1.weight", "linear2.weight"}) {
            const float* W = pk.get(L + m, 128 * 128);
            for (int rt = 0; rt < 8; ++rt)
                for (int kb = 0; kb < 4; ++kb) frag(W, 128, 16 * rt, kb, true);
        }
        pk.put_prm(poff, pb + TF_P_QKV_B, L + "self_attn.in_proj_bias", 384);
        pk.put_prm(poff, pb + TF_P_OUT_B, L + "self_attn.out_proj.bias", 128);
        pk.put_prm(poff, pb + TF_P_LN1_G, L + "norm1.weight", 128);
        pk.put_prm(poff, pb + TF_P_LN1_B, L + "norm1.bias", 128);
        pk.put_prm(poff, pb + TF_P_FC1_B, L + "linear1.bias", 128);
        pk.put_prm(poff, pb + TF_P_FC2_B, L + "linear2.bias", 128);
        pk.put_prm(poff, pb + TF_P_LN2_G, L + "norm2.weight", 128);
        pk.put_prm(poff, pb + TF_P_LN2_B, L + "norm2.bias", 128);
    }
    pk.put_prm(poff, tf_pb(nl), T + "output_proj.weight", 128);
    pk.put_prm(poff, tf_pb(nl) + 128, T + "output_proj.bias", 1);
    pk.slot(&w->tp_stream, soff);
    pk.slot(&w->tp_params, poff);
}

// Weights of the fused map_decoder (decoder.hip decode_fused_kernel; reference model.py:286-295): the ConvT layers as GEMM weights
// (convt_src), cut into write_frag fragments.  Layer 0 reads its input from memory (natural k order); layers 3 and 5 read C-layout tile
// pairs of the previous MFMA (permuted k order).  Fragment order and parameter offsets: pack_layout.hpp.
inline void pack_decoder_fused(Packer& pk, srh_weights* w) {
    const size_t foff = pk.alloc((size_t)(DF_FRAGS0 + DF_FRAGS3 + DF_FRAGS5) * FRAG_BYTES), poff = pk.alloc((size_t)DF_NPRM * 4);
    size_t f = 0;
    std::vector<float> wg;                                 // the layer's GEMM weight [4 * cout][cin]
    auto load = [&](const std::string& name, int cin, int cout) -> const float* {
        const float* src = pk.get(name, (size_t)cin * cout * 4);
        if (!src) return nullptr;
        wg.resize((size_t)4 * cout * cin);
        for (size_t n = 0; n < (size_t)4 * cout; ++n)
            for (int ci = 0; ci < cin; ++ci) wg[n * cin + ci] = src[convt_src(n, ci, cout)];
        return wg.data();
    };
    auto frag = [&](const float* W, int ldw, int row0, int kb, bool perm) { write_frag(pk.at<f16>(foff) + f++ * 512, W, ldw, row0, kb, perm, ldw); };
    {
        const float* W = load("map_decoder.0.weight", 256, 128);
        for (int s1 = 0; s1 < 4; ++s1)
            for (int kb = 0; kb < 8; ++kb)
                for (int rt = 0; rt < 8; ++rt) frag(W, 256, s1 * 128 + 16 * rt, kb, false);
    }
    {
        const float* W = load("map_decoder.3.weight", 128, 64);
        for (int s2 = 0; s2 < 4; ++s2)
            for (int kb = 0; kb < 4; ++kb)
                for (int rt = 0; rt < 4; ++rt) frag(W, 128, s2 * 64 + 16 * rt, kb, true);
    }
    {
        const float* W = load("map_decoder.5.weight", 64, 32);
        for (int kb = 0; kb < 2; ++kb)
            for (int rt = 0; rt < 8; ++rt) frag(W, 64, 16 * rt, kb, true);
    }
    pk.put_prm(poff, DF_P_B0, "map_decoder.0.bias", 128);
    pk.put_prm(poff, DF_P_LN_G, "map_decoder.1.weight", 128);
    pk.put_prm(poff, DF_P_LN_B, "map_decoder.1.bias", 128);
    pk.put_prm(poff, DF_P_B3, "map_decoder.3.bias", 64);
    pk.put_prm(poff, DF_P_B5, "map_decoder.5.bias", 32);
    if (const float* src = pk.get("map_decoder.7.weight", 32 * 2 * 4))
        for (int nn = 0; nn < 8; ++nn)
            for (int ci = 0; ci < 32; ++ci) pk.at<float>(poff)[DF_P_W7 + nn * 32 + ci] = src[convt_src(nn, ci, 2)];
    pk.put_prm(poff, DF_P_B7, "map_decoder.7.bias", 2);
    pk.slot(&w->dec_frags, foff);
    pk.slot(&w->dec_prm, poff);
}

// SAM MaskDecoder branch: prompt_encoder.* / mask_decoder.* (fork key names; oracle/sam_decoder.py).  The random-Fourier
// positional encoding of the S x S grid (get_dense_pe) is constant: pe and every pe . W^T the decoder needs are computed here.
inline void pack_sam_decoder(Packer& pk, srh_weights* w) {
    const int S = w->S, HW = S * S;
    SdW& d = w->sd;
    const std::string PE = "prompt_encoder.", MD = "mask_decoder.", TR = "mask_decoder.transformer.";
    pk.put_f32(&d.no_mask, PE + "no_mask_embed.weight", 256);
    // parameters the no-prompt path never reads must still be present in a checkpoint of this branch
    for (const char* k : {"point_embeddings.0.weight", "point_embeddings.1.weight", "point_embeddings.2.weight",
                          "point_embeddings.3.weight", "not_a_point_embed.weight"}) (void)pk.get(PE + k, 256);
    {
        const float* it = pk.get(MD + "iou_token.weight", 256);
        std::vector<float> tok(4 * 256, 0.f);
        if (it) memcpy(tok.data(), it, 256 * 4);
        const float* mt = pk.get(MD + "mask_tokens.weight", 3 * 256);
        if (mt) memcpy(tok.data() + 256, mt, 3 * 256 * 4);
        const size_t off = pk.alloc(4 * 256 * 4);
        memcpy(pk.host.data() + off, tok.data(), 4 * 256 * 4);
        pk.slot(&d.tokens, off);
    }
    // pe[y*S + x][c]: coords ((x + .5)/S, (y + .5)/S) -> 2c - 1 -> @ G[2,128] -> 2 pi -> sin | cos
    std::vector<float> pe((size_t)HW * 256, 0.f);
    {
        const float* G = pk.get(PE + "pe_layer.positional_encoding_gaussian_matrix", 2 * 128);
        if (G)
            for (int y = 0; y < S; ++y)
                for (int x = 0; x < S; ++x) {
                    const float cx = 2.f * (((float)x + 0.5f) / (float)S) - 1.f, cy = 2.f * (((float)y + 0.5f) / (float)S) - 1.f;
                    for (int j = 0; j < 128; ++j) {
                        const float a = 2.f * 3.14159265358979323846f * (cx * G[j] + cy * G[128 + j]);
                        pe[((size_t)y * S + x) * 256 + j] = sinf(a);
                        pe[((size_t)y * S + x) * 256 + 128 + j] = cosf(a);
                    }
                }
    }
    // pe [HW,256] . W[128,256]^T -> [HW,128] f32.  W comes straight from get(): nothing is fetched before it has been consumed
    auto put_pos = [&](float** dst, const std::string& name) {
        const float* W = pk.get(name, 128 * 256);
        const size_t off = pk.alloc((size_t)HW * 128 * 4);
        if (W) {
            float* o = pk.at<float>(off);
            for (int t = 0; t < HW; ++t)
                for (int n = 0; n < 128; ++n) {
                    double a = 0.0;
                    for (int k = 0; k < 256; ++k) a += (double)pe[(size_t)t * 256 + k] * W[(size_t)n * 256 + k];
                    o[(size_t)t * 128 + n] = (float)a;
                }
        }
        pk.slot(dst, off);
    };
    auto put_t2i = [&](SdT2IW& a, const std::string& base) {
        pk.put_f32(&a.q_w, base + "q_proj.weight", 128 * 256); pk.put_f32(&a.q_b, base + "q_proj.bias", 128);
        pk.put_f16_same(&a.k_w, base + "k_proj.weight", 128 * 256); pk.put_f32(&a.k_b, base + "k_proj.bias", 128);
        pk.put_f16_same(&a.v_w, base + "v_proj.weight", 128 * 256); pk.put_f32(&a.v_b, base + "v_proj.bias", 128);
        pk.put_f32(&a.o_w, base + "out_proj.weight", 256 * 128); pk.put_f32(&a.o_b, base + "out_proj.bias", 256);
        put_pos(&a.k_pos, base + "k_proj.weight");
    };
    auto put_i2t = [&](SdI2TW& a, const std::string& base) {
        pk.put_f16_same(&a.q_w, base + "q_proj.weight", 128 * 256); pk.put_f32(&a.q_b, base + "q_proj.bias", 128);
        pk.put_f32(&a.k_w, base + "k_proj.weight", 128 * 256); pk.put_f32(&a.k_b, base + "k_proj.bias", 128);
        pk.put_f32(&a.v_w, base + "v_proj.weight", 128 * 256); pk.put_f32(&a.v_b, base + "v_proj.bias", 128);
        pk.put_f16_same(&a.o_w, base + "out_proj.weight", 256 * 128); pk.put_f32(&a.o_b, base + "out_proj.bias", 256);
        put_pos(&a.q_pos, base + "q_proj.weight");
    };
    for (int l = 0; l < 2; ++l) {
        SdLayerW& L = d.layer[l];
        const std::string B_ = TR + "layers." + std::to_string(l) + ".";
        pk.put_f32(&L.self.q_w, B_ + "self_attn.q_proj.weight", 256 * 256); pk.put_f32(&L.self.q_b, B_ + "self_attn.q_proj.bias", 256);
        pk.put_f32(&L.self.k_w, B_ + "self_attn.k_proj.weight", 256 * 256); pk.put_f32(&L.self.k_b, B_ + "self_attn.k_proj.bias", 256);
        pk.put_f32(&L.self.v_w, B_ + "self_attn.v_proj.weight", 256 * 256); pk.put_f32(&L.self.v_b, B_ + "self_attn.v_proj.bias", 256);
        pk.put_f32(&L.self.o_w, B_ + "self_attn.out_proj.weight", 256 * 256); pk.put_f32(&L.self.o_b, B_ + "self_attn.out_proj.bias", 256);
        put_t2i(L.t2i, B_ + "cross_attn_token_to_image.");
        put_i2t(L.i2t, B_ + "cross_attn_image_to_token.");
        pk.put_f32(&L.n1_g, B_ + "norm1.weight", 256); pk.put_f32(&L.n1_b, B_ + "norm1.bias", 256);
        pk.put_f32(&L.n2_g, B_ + "norm2.weight", 256); pk.put_f32(&L.n2_b, B_ + "norm2.bias", 256);
        pk.put_f32(&L.n3_g, B_ + "norm3.weight", 256); pk.put_f32(&L.n3_b, B_ + "norm3.bias", 256);
        pk.put_f32(&L.n4_g, B_ + "norm4.weight", 256); pk.put_f32(&L.n4_b, B_ + "norm4.bias", 256);
        pk.put_f32(&L.l1_w, B_ + "mlp.lin1.weight", 2048 * 256); pk.put_f32(&L.l1_b, B_ + "mlp.lin1.bias", 2048);
        pk.put_f32(&L.l2_w, B_ + "mlp.lin2.weight", 256 * 2048); pk.put_f32(&L.l2_b, B_ + "mlp.lin2.bias", 256);
    }
    put_t2i(d.fin, TR + "final_attn_token_to_image.");
    pk.put_f32(&d.nf_g, TR + "norm_final_attn.weight", 256); pk.put_f32(&d.nf_b, TR + "norm_final_attn.bias", 256);
    // output_upscaling: ConvTranspose2d weight -> GEMM weight (convt_src), bias replicated x4
    auto convt = [&](f16** dst, float** bdst, const std::string& idx, size_t cin, size_t cout) {
        pk.put_f16(dst, MD + "output_upscaling." + idx + ".weight", cin * cout * 4, 4 * cout * cin,
                   [cin, cout](size_t i) { return convt_src(i / cin, i % cin, cout); });
        const float* bsrc = pk.get(MD + "output_upscaling." + idx + ".bias", cout);
        const size_t off = pk.alloc(4 * cout * 4);
        if (bsrc)
            for (size_t r = 0; r < 4; ++r) memcpy(pk.host.data() + off + r * cout * 4, bsrc, cout * 4);
        pk.slot(bdst, off);
    };
    convt(&d.up0_w, &d.up0_b, "0", 256, 64);
    pk.put_f32(&d.up_ln_g, MD + "output_upscaling.1.weight", 64); pk.put_f32(&d.up_ln_b, MD + "output_upscaling.1.bias", 64);
    convt(&d.up1_w, &d.up1_b, "3", 64, 32);
    for (int i = 0; i < 3; ++i)
        for (int l = 0; l < 3; ++l) {
            const std::string H = MD + "output_hypernetworks_mlps." + std::to_string(i) + ".layers." + std::to_string(l) + ".";
            const int out = l == 2 ? 32 : 256;
            pk.put_f32(&d.hy_w[i][l], H + "weight", (size_t)out * 256); pk.put_f32(&d.hy_b[i][l], H + "bias", out);
        }
    // iou_prediction_head: its output is discarded by the reference (model.py:430 `low_res_logits, iou_predictions`); only presence is checked
    for (int l = 0; l < 3; ++l) {
        const std::string H = MD + "iou_prediction_head.layers." + std::to_string(l) + ".";
        (void)pk.get(H + "weight", (size_t)(l == 2 ? 3 : 256) * 256); (void)pk.get(H + "bias", l == 2 ? 3 : 256);
    }
}

// The whole model.  The caller has validated w->cfg and set w->S / D / heads / hd from it.
inline void pack_model(Packer& pk, srh_weights* w, const srh_named_tensor* tensors, int n) {
    const srh_model_cfg* cfg = &w->cfg;
    const int D = w->D, S = w->S, hd = w->hd;
    for (int i = 0; i < n; ++i) pk.by_name[tensors[i].name] = &tensors[i];
    const std::string E = "image_encoder.";

    pk.put_f16(&w->patch_w, E + "patch_embed.proj.weight", (size_t)D * 768, (size_t)D * 768, [](size_t i) {
        const size_t nidx = i / 768, k = i % 768;
        const size_t ky = k / 48, kx = (k % 48) / 3, ch = k % 3;
        return nidx * 768 + ch * 256 + ky * 16 + kx;
    });
    pk.put_f32(&w->patch_b, E + "patch_embed.proj.bias", D);
    pk.put_f32(&w->pos, E + "pos_embed", (size_t)S * S * D);

    w->blocks.resize(cfg->depth);
    for (int i = 0; i < cfg->depth; ++i) {
        BlockW& b = w->blocks[i];
        bool global = false;
        for (int g = 0; g < cfg->n_global; ++g) global |= cfg->global_attn_indexes[g] == i;
        b.win = global ? S : cfg->window_size;
        const std::string B_ = E + "blocks." + std::to_string(i) + ".";
        pk.put_f32(&b.ln1_g, B_ + "norm1.weight", D);
        pk.put_f32(&b.ln1_b, B_ + "norm1.bias", D);
        pk.put_f32(&b.ln2_g, B_ + "norm2.weight", D);
        pk.put_f32(&b.ln2_b, B_ + "norm2.bias", D);
        pk.put_f16_same(&b.qkv_w, B_ + "attn.qkv.weight", (size_t)3 * D * D);
        pk.put_f32(&b.qkv_b, B_ + "attn.qkv.bias", (size_t)3 * D);
        pk.put_f16_same(&b.qkv_b16, B_ + "attn.qkv.bias", (size_t)3 * D);
        pk.put_f16_same(&b.rel_h, B_ + "attn.rel_pos_h", (size_t)(2 * b.win - 1) * hd);
        pk.put_f16_same(&b.rel_w, B_ + "attn.rel_pos_w", (size_t)(2 * b.win - 1) * hd);
        pk.put_f16_same(&b.proj_w, B_ + "attn.proj.weight", (size_t)D * D);
        pk.put_f32(&b.proj_b, B_ + "attn.proj.bias", D);
        pk.put_f16_same(&b.fc1_w, B_ + "mlp.lin1.weight", (size_t)4 * D * D);
        pk.put_f32(&b.fc1_b, B_ + "mlp.lin1.bias", (size_t)4 * D);
        pk.put_f16_same(&b.fc2_w, B_ + "mlp.lin2.weight", (size_t)4 * D * D);
        pk.put_f32(&b.fc2_b, B_ + "mlp.lin2.bias", D);
    }
    pk.put_f16_same(&w->neck0_w, E + "neck.0.weight", (size_t)256 * D);
    pk.put_f32(&w->neck1_g, E + "neck.1.weight", 256);
    pk.put_f32(&w->neck1_b, E + "neck.1.bias", 256);
    pk.put_f16(&w->neck2_w, E + "neck.2.weight", (size_t)256 * 256 * 9, (size_t)256 * 2304, [](size_t i) {
        const size_t nidx = i / 2304, k = i % 2304, tap = k / 256, ch = k % 256;
        return (nidx * 256 + ch) * 9 + tap;
    });
    pk.put_f32(&w->neck3_g, E + "neck.3.weight", 256);
    pk.put_f32(&w->neck3_b, E + "neck.3.bias", 256);

    if (cfg->use_sam_decoder) pack_sam_decoder(pk, w);
    else pack_decoder_fused(pk, w);

    // TopoNet
    const std::string T = "topo_net.";
    pk.put_f16_same(&w->tp_feat_w, T + "feature_proj.weight", 128 * 256);
    pk.put_f32(&w->tp_feat_b, T + "feature_proj.bias", 128);
    w->tp_layers = cfg->toponet_version != 2 ? 3 : 0;
    pack_topo_fused(pk, w, w->tp_layers);
}

}  // namespace
}  // namespace srh
