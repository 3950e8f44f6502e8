// The packed model weights: a table of pointers into one device arena (internal; ctx.hpp includes it).  No HIP header: the host-only
// packer (pack_host.hpp) fills the table's slots with arena offsets, api_weights.hip turns them into device pointers.
#pragma once
#include <cstddef>
#include <vector>

#include "../../include/samroad_hip.h"

namespace srh { typedef _Float16 f16; }      // as common.hpp
using srh::f16;

struct BlockW {
    int win = 0;
    float *ln1_g, *ln1_b, *ln2_g, *ln2_b, *qkv_b, *proj_b, *fc1_b, *fc2_b;
    f16 *qkv_w, *qkv_b16, *rel_h, *rel_w, *proj_w, *fc1_w, *fc2_w;
};
// SAM MaskDecoder branch (USE_SAM_DECODER; sam_decoder.hip).  Attention a: image-side projection weights fp16 + the
// positional term pe . W^T precomputed at pack time; token-side weights f32.
struct SdAttnW { float *q_w, *q_b, *k_w, *k_b, *v_w, *v_b, *o_w, *o_b; };                        // token-side self attention (f32)
struct SdT2IW { float *q_w, *q_b, *o_w, *o_b; f16 *k_w, *v_w; float *k_b, *v_b, *k_pos; };     // token -> image
struct SdI2TW { f16 *q_w, *o_w; float *q_b, *o_b, *q_pos, *k_w, *k_b, *v_w, *v_b; };           // image -> token
struct SdLayerW {
    SdAttnW self; SdT2IW t2i; SdI2TW i2t;
    float *n1_g, *n1_b, *n2_g, *n2_b, *n3_g, *n3_b, *n4_g, *n4_b, *l1_w, *l1_b, *l2_w, *l2_b;
};
struct SdW {
    float *no_mask, *tokens;                 // [256], [4,256] = iou_token | mask_tokens
    SdLayerW layer[2];
    SdT2IW fin; float *nf_g, *nf_b;
    f16 *up0_w, *up1_w; float *up0_b, *up_ln_g, *up_ln_b, *up1_b;
    float *hy_w[3][3], *hy_b[3][3];
};
struct srh_weights {
    srh_model_cfg cfg;
    SdW sd;
    int S = 0, D = 0, heads = 0, hd = 0;
    void* arena = nullptr; size_t arena_bytes = 0;
    f16* patch_w; float* patch_b; float* pos;
    std::vector<BlockW> blocks;
    f16 *neck0_w, *neck2_w; float *neck1_g, *neck1_b, *neck3_g, *neck3_b;
    char* dec_frags = nullptr; float* dec_prm = nullptr;          // fused map_decoder (decoder.hip): packed MFMA fragments + f32 parameters
    f16* tp_feat_w; float* tp_feat_b;
    char* tp_stream = nullptr; float* tp_params = nullptr;       // fused trunk (topo_fused.hip)
    int tp_layers = 0;                                            // encoder layers of the trunk (0: TOPONET_VERSION no_transformer)
};
