// Layout of the packed weights that a fused kernel and the host packer (pack_host.hpp) must agree on: fragment counts and f32 parameter
// offsets of the fused map_decoder (decoder.hip) and of the fused TopoNet trunk (topo_fused.hip).  Plain constexpr values: no HIP header,
// usable from host and device code.
#pragma once

namespace srh {

constexpr int FRAG_BYTES = 1024;              // one 16 (out) x 32 (in) fp16 MFMA A fragment

// ---- fused map_decoder: frags L0 [sub1 4][kb 8][rt 8] | L3 [sub2 4][kb 4][rt 4] | L5 [kb 2][rt 8], then the f32 parameters
constexpr int DF_FRAGS0 = 4 * 8 * 8, DF_FRAGS3 = 4 * 4 * 4, DF_FRAGS5 = 2 * 8;
// b0[128] | ln gamma[128] | ln beta[128] | b3[64] | b5[32] | w7[8][32] (n = (ky*2+kx)*2 + class) | b7[2]: 738 floats, padded to
// 3 KiB (the kernel stages them by three 1-KiB LDS-DMA pieces)
constexpr int DF_P_B0 = 0, DF_P_LN_G = 128, DF_P_LN_B = 256, DF_P_B3 = 384, DF_P_B5 = 448, DF_P_W7 = 480, DF_P_B7 = 736, DF_NPRM = 768;

// ---- fused TopoNet trunk: pair_proj [kb 10][rt 8], then per encoder layer V | Q K per head | out_proj | linear1 | linear2 (the
// kernel consumes them in chunks of TF_CHUNK_FRAGS); parameters pair_proj bias[128] | per layer TF_P_LAYER | output_proj w[128] b[1] (+ 3 pad)
constexpr int TF_CHUNK_FRAGS = 16;
constexpr int TF_FRAGS_PAIR = 10 * 8;
constexpr int TF_F_V = 0, TF_F_QK = 32, TF_F_OUT = 96, TF_F_FC1 = 128, TF_F_FC2 = 160, TF_FRAGS_LAYER = 192;   // per layer, from its first fragment
constexpr int TF_P_PAIR_B = 0, TF_P_LAYER0 = 128, TF_P_LAYER = 1280, TF_P_TAIL = 132;
constexpr int TF_P_QKV_B = 0, TF_P_OUT_B = 384, TF_P_LN1_G = 512, TF_P_LN1_B = 640, TF_P_FC1_B = 768, TF_P_FC2_B = 896, TF_P_LN2_G = 1024,
              TF_P_LN2_B = 1152;                                                                             // per layer, from tf_pb(l)
constexpr int tf_nfrag(int nl) { return TF_FRAGS_PAIR + TF_FRAGS_LAYER * nl; }    // = the first fragment of layer nl
constexpr int tf_pb(int l) { return TF_P_LAYER0 + TF_P_LAYER * l; }                // first parameter of layer l; tf_pb(nl): output_proj
constexpr int tf_nprm(int nl) { return tf_pb(nl) + TF_P_TAIL; }

}  // namespace srh
