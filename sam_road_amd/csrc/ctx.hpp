// What the api_*.hip units share (internal): the context and its workspaces, the packed weights, error reporting, the profiled launch
// wrappers and the parameter blocks that the model path and the test-only srh_op_* entries both build.  Host-side C++ only.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/samroad_hip.h"
#include "kernels.hpp"
#include "weights.hpp"

using namespace srh;

#define SRH_INTERNAL __attribute__((visibility("hidden")))      // shared among the api_*.hip units, not exported

// A context workspace.  It registers itself with its context when it is constructed: srh_ctx_destroy and srh_ctx_device_bytes walk
// that list, so a new workspace is named once, as a member of srh_ctx.
struct DevBuf {
    void* p = nullptr;
    size_t cap = 0;
    explicit DevBuf(std::vector<DevBuf*>& all) { all.push_back(this); }
    DevBuf(const DevBuf&) = delete;
    // grow-only; `slack` (a fraction of the request) is added when a buffer's size follows the data (the TopoNet
    // workspaces scale with the number of graph points of a batch): hipFree + hipMalloc synchronise the device, so
    // growing by a few rows per batch would cost milliseconds per call
    int ensure(size_t bytes, double slack = 0.0) {
        if (bytes <= cap) return 0;
        if (p) hipFree(p);
        p = nullptr; cap = 0;
        const size_t want = bytes + (size_t)(bytes * slack);
        if (hipMalloc(&p, want) != hipSuccess) return SRH_ERR_HIP;
        cap = want;
        return 0;
    }
    void release() { if (p) hipFree(p); p = nullptr; cap = 0; }
    template <class T> T* as() const { return reinterpret_cast<T*>(p); }
};

struct ProfEntry { int cls; hipEvent_t e0, e1; double flops, bytes; };

struct SRH_INTERNAL srh_ctx {
    int device = 0;
    std::string err;
    std::vector<DevBuf*> bufs;   // every DevBuf below (declared before them: it is constructed first)
    // encoder / decoder workspace
    DevBuf a0{bufs}, x{bufs}, xn16{bufs}, delta16{bufs}, delta16b{bufs}, qkv16{bufs}, attn16{bufs}, hid16{bufs}, n1{bufs}, n1_16{bufs}, n2{bufs},
        emb16{bufs};
    DevBuf scores_ws{bufs}, emb_ws{bufs}, counter{bufs}, split_ws{bufs};
    DevBuf tta_scores_ws{bufs};  // TTA: the scores of an oriented batch before they are brought back to the scene frame (emb_ws: its embeddings)
    ZTileTables ztab;            // gemm_z192's tile-order tables (one bounded slab, freed with the context)
    // non-finite sentinel: NF_SLOTS flags in host-mapped pinned memory (nf_host; nf_dev = the same bytes as the device sees them).
    // The LayerNorm passes set flag `tag` when a row's variance is not finite (NormParams::nf) — an fp16 overflow upstream.  Nothing is
    // copied or synchronised in the hot loop: a set flag crosses PCIe once, the host reads its own memory at the next call.
    unsigned* nf_host = nullptr; unsigned* nf_dev = nullptr;
    // SAM MaskDecoder branch workspace
    DevBuf sd_keys{bufs}, sd_keys16{bufs}, sd_k16{bufs}, sd_v16{bufs}, sd_a16{bufs}, sd_u0{bufs}, sd_u0_16{bufs}, sd_u1_16{bufs}, sd_low{bufs},
        sd_tok{bufs};
    // toponet workspace
    DevBuf t_feat16{bufs}, t_pf16{bufs}, t_pair16{bufs};
    // ROAD_WIDTH: the column pass's distances between the two launches of srh_road_dist.  The entry runs on writer threads: the lock is
    // held from the workspace's growth to the second launch, and calls on one stream are ordered by it.
    DevBuf road_g{bufs};
    std::mutex road_mu;
    // GRAPH_CLEAN: the forests and sums of srh_graph_clean, about 24 B per node and 25 B per edge.  The entry runs on writer threads: the lock
    // is held from the workspace's growth to the last launch, and a call on another stream waits on the device (clean_done, recorded behind
    // the last launch of every call) until the call before it has left the workspace.
    DevBuf clean_ws{bufs};
    std::mutex clean_mu;
    hipEvent_t clean_done = nullptr;
    // profiling
    bool profiling = false;
    std::vector<std::string> cls_names;
    std::vector<ProfEntry> prof;
    std::vector<hipEvent_t> ev_pool;
    size_t ev_used = 0;
    // lanes (api_model.hip encode_batch): a batch as two half-batch chains, lane 0 on the caller's stream and lane 1 on this one
    int lanes_mode = 0;          // srh_ctx_set_lanes: 0 auto, 1 one lane, 2 two lanes whenever B is even
    int last_lanes = 1;          // what the last encode_batch ran
    hipStream_t lane_stream = nullptr;                      // created at the first two-lane call, destroyed with the context
    hipEvent_t lane_fork = nullptr, lane_join = nullptr;    // caller's stream -> lane 1 -> caller's stream
};

constexpr int NF_SLOTS = 128, NF_NECK = 64, NF_DECODER = 66;   // tags: 2 * block + (0 norm1 | 1 norm2), neck LN2d 64 / 65, map_decoder LN2d 66
constexpr int NF_PAIRS = 67;                                    // ABI 9: srh_toponet_ragged's pair gather saw a pair outside its row's tile

static int fail(srh_ctx* c, int code, const std::string& msg) {
    if (c) c->err = msg;
    return code;
}
static int hip_fail(srh_ctx* c, hipError_t e, const char* where) {
    return fail(c, SRH_ERR_HIP, std::string(where) + ": " + hipGetErrorString(e));
}

// api_ctx.hip: the profiler's bookkeeping, and the sentinel flags as the host sees them now (0, or SRH_ERR_* + message, flags cleared)
SRH_INTERNAL int cls_id(srh_ctx* c, const char* name);
SRH_INTERNAL hipEvent_t next_event(srh_ctx* c);
SRH_INTERNAL int nonfinite_check(srh_ctx* c, const char* who);

template <class F>
static int run(srh_ctx* c, const char* cls, double flops, double bytes, hipStream_t s, F&& f) {
    if (!c->profiling) return f();
    ProfEntry pe;
    pe.cls = cls_id(c, cls);
    pe.flops = flops; pe.bytes = bytes;
    pe.e0 = next_event(c);
    pe.e1 = next_event(c);
    hipEventRecord(pe.e0, s);
    const int rc = f();
    hipEventRecord(pe.e1, s);
    c->prof.push_back(pe);
    return rc;
}

// lane / lanes: the caller is chain `lane` of `lanes` equal ones in flight at once (encode_batch); each has its own part of the split-K workspace
static int gemm(srh_ctx* c, const char* cls, const GemmParams& p_in, hipStream_t s, int lane = 0, int lanes = 1) {
    GemmParams p = p_in;
    p.ztab = &c->ztab;
    const int sk = gemm_splitk_factor(p);
    if (sk > 1) {       // small-M layers (ViT-L / ViT-H at 256 px): deterministic split-K through a ctx-owned f32 workspace
        const size_t part = (size_t)sk * p.M * p.N;
        if (c->split_ws.ensure(part * 4 * lanes)) return fail(c, SRH_ERR_HIP, "split-K workspace allocation failed");
        p.splitk = sk; p.split_ws = c->split_ws.as<float>() + part * lane;
    }
    const double fl = 2.0 * p.M * (double)p.N * p.K;
    const int rc = run(c, cls, fl, 0.0, s, [&] { return launch_gemm(p, s); });
    if (rc) return fail(c, rc == -2 ? SRH_ERR_UNSUPPORTED : SRH_ERR_HIP, std::string("gemm ") + cls + " launch failed");
    return 0;
}

#define TRY(expr) do { const int rc_ = (expr); if (rc_) return rc_; } while (0)
#define TRYK(c, cls, fl, by, s, call) do { const int rc_ = run(c, cls, fl, by, s, [&] { return (call); }); \
    if (rc_) return fail(c, rc_ == -2 ? SRH_ERR_UNSUPPORTED : SRH_ERR_HIP, std::string(cls) + ": kernel launch failed"); } while (0)

// A scene's pixel count must fit an int: the scene kernels index canvas pixels with one (byte offsets are 64-bit).
static bool scene_dims_ok(int H, int W) { return H > 0 && W > 0 && (long long)H * W <= 2147483647LL; }
static bool tile_size_ok(int P) { return P >= 128 && P <= 1024 && P % 16 == 0; }

// api_model.hip: one batch of tiles through encoder + neck + decoder (orient / scene_H: TTA's oriented crop, scene_tta.hip)
SRH_INTERNAL double attn_flops(int B, int S, int heads, int hd, int win);
SRH_INTERNAL int encode_batch(srh_ctx* c, const srh_weights* w, PatchParams pp, int B, float* logits, float* scores, float* emb, hipStream_t s,
                              int orient = 0, int scene_H = 0);
// api_model.hip: the SAM MaskDecoder branch of encode_batch on a neck output emb f32 [B*S*S, 256] (srh_op_sam_decoder runs the same call).
// It leaves the queries after norm_final_attn [B,4,256] at the start of c->sd_tok and sd_mask's output [B,2,4S,4S] in c->sd_low.
SRH_INTERNAL int sam_decode(srh_ctx* c, const srh_weights* w, int B, const float* emb, float* logits, float* scores, hipStream_t s);

// ---- parameter blocks: the model path and the srh_op_* entry of the same kernel build them here, so an op test runs the model's pattern
// plain [M,K] . [N,K]^T: both operands dense; outputs, epilogue and a conv's lda / ldw are set by the caller
static GemmParams gemm_nt(const f16* A, const f16* W, int M, int N, int K) {
    GemmParams g;
    g.A = A; g.lda = K; g.W = W; g.ldw = K; g.M = M; g.N = N; g.K = K;
    return g;
}
// qkv [tokens, 3 D] -> out [tokens, D], D = heads * hd; rel-pos bias derived inside the attention kernel from the two tables
static AttnParams attn_params(const f16* qkv, const f16* rel_h, const f16* rel_w, const f16* bias_qkv, f16* out, int B, int S, int heads, int hd,
                              int win) {
    const int D = heads * hd;
    AttnParams ap;
    ap.table_h = rel_h; ap.table_w = rel_w;
    ap.qkv = qkv; ap.ld = 3 * D; ap.bias_qkv = bias_qkv;
    ap.out = out; ap.ldo = D; ap.B = B; ap.S = S; ap.heads = heads; ap.hd = hd; ap.win = win;
    ap.scale = 1.0f / sqrtf((float)hd);
    return ap;
}
static DecodeFusedParams decode_params(const srh_ctx* c, const srh_weights* w, const f16* emb16, int B, float* logits, float* scores) {
    DecodeFusedParams dp;
    dp.emb16 = emb16; dp.frags = w->dec_frags; dp.prm = w->dec_prm; dp.B = B; dp.S = w->S;
    dp.logits = logits; dp.scores = scores; dp.nf = c->nf_dev; dp.nf_tag = NF_DECODER;
    return dp;
}
static SampleParams sample_params(const float* emb, int n_tiles, int h, int w, int C, const void* points, int points_dtype, const int* point_tile,
                                  int B, int N, float patch, float* out_f32, f16* out_f16) {
    SampleParams sp;
    sp.emb = emb; sp.points = points; sp.points_i64 = points_dtype == SRH_I64; sp.B = B; sp.N = N;
    sp.h = h; sp.w = w; sp.C = C; sp.patch = patch; sp.out_f32 = out_f32; sp.out_f16 = out_f16;
    sp.point_tile = point_tile; sp.n_tiles = n_tiles;
    return sp;
}
// ragged rows (point_tile / bad) are set by the caller
static PairGatherParams pair_gather_params(const f16* pf, const void* points, int points_dtype, const void* pairs, int pairs_dtype, int B, int N,
                                           int Ns, int K, bool zero_offset, long index_base, f16* out, int ld) {
    PairGatherParams pg;
    pg.pf = pf; pg.points = points; pg.points_i64 = points_dtype == SRH_I64;
    pg.pairs = pairs; pg.pairs_i64 = pairs_dtype == SRH_I64; pg.B = B; pg.N = N; pg.Ns = Ns; pg.Kp = K;
    pg.zero_offset = zero_offset; pg.out = out; pg.ld = ld; pg.index_base = index_base;
    return pg;
}
// the fused trunk on the packed stream / parameter block / layer count of `w`
static TopoFusedParams topo_fused_params(const srh_weights* w, const f16* pair, int ld, const uint8_t* valid, int nseq, int K, float* logits,
                                         float* scores) {
    TopoFusedParams tf;
    tf.pair = pair; tf.ld_pair = ld; tf.valid = valid; tf.stream = w->tp_stream; tf.params = w->tp_params;
    tf.nlayers = w->tp_layers; tf.nseq = nseq; tf.K = K; tf.logits = logits; tf.scores = scores;
    return tf;
}
