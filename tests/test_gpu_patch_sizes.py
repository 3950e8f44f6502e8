"""PATCH_SIZE = 16 S for every 8 <= S <= 64 (128 .. 1024 px), not only 256 / 512 / 1024: the runtime-S global attention kernel
(attention.hip attn_global_kernel<WP, OCC, true>), the fused map_decoder's partial last job (decoder.hip), windowed attention with a
partly padded single window, and the whole model — shallow and full depth, the USE_SAM_DECODER branch and the scene pipeline — at
sizes the 256 / 512 / 1024 kernels never see, against the oracle / the op-level references.  Run on an MI355X: pytest -m gpu."""
import ctypes as C
import warnings

import numpy as np
import pytest
import torch

import heads_ref
import scene_kit
import tolerances as T
from oracle.samroad import AttrDict, SAMRoadOracle
from oracle.synth import synth_queries, synth_scene, synth_state_dict, synth_state_dict_keyed, synth_tiles
from test_gpu_heads import _decoder_net
from test_gpu_model import build_pair, rel_l2
from test_gpu_ops import ref_sam_attention

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from sam_road_amd import _lib
    assert torch.cuda.is_available(), "gpu-marked test needs a GPU"
    return _lib.Context.get(0)


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


# ---- attention op -------------------------------------------------------------------------------------------------------------------
def _ref_attention(qkv, rel_h, rel_w, bias, B, S, heads, win, hd):
    """ref_sam_attention, also for S < win (one window, partly padding): the tile padded to win x win with pad tokens (= the qkv bias,
    real keys) is one S = win window; the output cropped back to S x S."""
    if S >= win:
        return ref_sam_attention(qkv, rel_h, rel_w, bias, B, S, heads, win, hd)
    C3 = qkv.shape[1]
    full = bias.view(1, 1, 1, C3).expand(B, win, win, C3).clone()
    full[:, :S, :S] = qkv.view(B, S, S, C3)
    out = ref_sam_attention(full.reshape(B * win * win, C3), rel_h, rel_w, bias, B, win, heads, win, hd)
    return out.view(B, win, win, -1)[:, :S, :S].reshape(B * S * S, -1)


def _attention_case(ctx, B, S, heads, win, hd, seed):
    """test_gpu_ops.test_sam_attention's peaked inputs (q, k ~ N(0, 1.5), rel-pos tables 0.3, pad-key bias 0.5)."""
    D = heads * hd
    g = torch.Generator().manual_seed(seed)
    qkv = (torch.randn(B * S * S, 3 * D, generator=g) * 1.5).half()
    bias = (torch.randn(3 * D, generator=g) * 0.5).half()
    rel_h = (torch.randn(2 * win - 1, hd, generator=g) * 0.3).half()
    rel_w = (torch.randn(2 * win - 1, hd, generator=g) * 0.3).half()
    ref = _ref_attention(qkv, rel_h, rel_w, bias, B, S, heads, win, hd)
    out = torch.full((B * S * S, D), float("nan"), device="cuda", dtype=torch.half)
    dq, dh, dw, db = qkv.cuda(), rel_h.cuda(), rel_w.cuda(), bias.cuda()
    if hd == 64:
        ctx.check(ctx.lib.srh_op_attention(ctx.handle, _p(dq), _p(dh), _p(dw), _p(db), B, S, heads, win, _p(out), None), "srh_op_attention")
    else:
        ctx.check(ctx.lib.srh_op_attention_hd(ctx.handle, _p(dq), _p(dh), _p(dw), _p(db), B, S, heads, hd, win, _p(out), None),
                  "srh_op_attention_hd")
    torch.cuda.synchronize()
    got = out.cpu().float()
    assert torch.isfinite(got).all(), "unwritten or non-finite outputs"
    err = (got - ref).abs()
    tag = "patch_sizes_op_attention[S=%d,win=%d,hd=%d]" % (S, win, hd)
    T.check(tag + " max-abs", err.max().item(), T.ATTN_OP_MAX)
    T.check(tag + " mean-abs", err.mean().item(), T.ATTN_OP_MEAN)


# Global windows of every width class of the runtime-S kernel: WP 16 (S = 8, 12: two window rows per key tile, odd pad rows), WP 32
# (20, 24, 25: one row per tile, pad columns; 25 is odd, S * S = 625 is no multiple of the 128-query block), WP 64 (40, 48, 63: two
# tiles per row, the second one mostly pad columns).  heads = 4 at B = 2 takes the XCD-aware workgroup order, heads = 3 the plain one.
@pytest.mark.parametrize("S,heads", [(8, 3), (12, 4), (20, 3), (24, 4), (25, 3), (40, 4), (48, 3), (63, 3)])
def test_global_attention_any_s(ctx, S, heads):
    _attention_case(ctx, 2, S, heads, S, 64, seed=7000 + S)


# Windows of 14 at sizes the 256 / 512 / 1024 tiles never produce: S = 8 (one window, 64 real queries and 132 pad keys), 24 and 25
# (2 x 2 windows, edge windows of 10 / 11 rows), 40 (3 x 3, edge windows of 12 rows); hd 80 is attention_hdx.hip's windowed kernel.
@pytest.mark.parametrize("S", [8, 24, 25, 40])
@pytest.mark.parametrize("hd", [64, 80])
def test_window_attention_any_s(ctx, S, hd):
    _attention_case(ctx, 2, S, 3, 14, hd, seed=8000 + S + hd)


# ---- fused map_decoder ----------------------------------------------------------------------------------------------------------------
# T = B S S tokens in jobs of 16: (10, 1) and (25, 1) end on a partial job (100 = 6 x 16 + 4, 625 = 39 x 16 + 1)
@pytest.mark.parametrize("S,B", [(8, 2), (10, 1), (24, 3), (25, 1), (48, 1)])
def test_map_decoder_op_any_s(ctx, S, B):
    net = _decoder_net(S, seed=300 + S + B)
    _, wh = net._weights(torch.device("cuda", 0))
    P = 16 * S
    g = torch.Generator().manual_seed(S * 1000 + B + 1)
    emb = torch.randn(B * S * S, 256, generator=g).half()
    # the neck output lives in a larger buffer: rows past B S S are Inf — a pad lane of the last job must not read them
    buf = torch.full((B * S * S + 16, 256), float("inf"), dtype=torch.half)
    buf[:B * S * S] = emb
    demb = buf.cuda()

    def run(want_logits, want_scores):
        lg = torch.full((B, P, P, 2), float("nan"), device="cuda") if want_logits else None
        sc = torch.full((B, P, P, 2), float("nan"), device="cuda") if want_scores else None
        ctx.check(ctx.lib.srh_op_map_decoder(ctx.handle, wh, _p(demb), B, _p(lg), _p(sc), None), "srh_op_map_decoder")
        torch.cuda.synchronize()
        return (lg.cpu() if lg is not None else None), (sc.cpu() if sc is not None else None)

    lg, sc = run(True, True)
    assert torch.isfinite(lg).all() and torch.isfinite(sc).all(), "unwritten or non-finite outputs"
    lg_only, _ = run(True, False)
    _, sc_only = run(False, True)
    assert torch.equal(lg_only, lg) and torch.equal(sc_only, sc), "one output alone must give the bits of the both-outputs run"
    ref_l, ref_s = heads_ref.map_decoder_ref(emb.float().view(B, S, S, 256), net.state_dict())
    el = (lg.double() - ref_l).abs().max().item()
    es = (sc.double() - ref_s).abs().max().item()
    T.check(f"patch_sizes_map_decoder_op_S{S}_B{B}_logit", el, T.DEC_OP_LOGIT)
    T.check(f"patch_sizes_map_decoder_op_S{S}_B{B}_score", es, T.DEC_OP_SCORE)
    ctx.check(ctx.lib.srh_ctx_check(ctx.handle, None, 1), "srh_ctx_check")      # no Inf / NaN sentinel: the pad lanes stayed out


# ---- whole model --------------------------------------------------------------------------------------------------------------------
def _cfg(version, patch, **kw):
    return dict(SAM_VERSION=version, PATCH_SIZE=patch, TOPONET_VERSION="normal", SAM_CKPT_PATH="") | kw


# two blocks, one windowed and one global: ViT-B over every width class and a partial decoder job (400 px: S = 25, B = 1), ViT-L (16
# heads), ViT-H (hd 80: attention_hdx.hip windows, the generic kernel for the 24 x 24 global window)
@pytest.mark.parametrize("version,patch,B", [("vit_b", 128, 2), ("vit_b", 384, 2), ("vit_b", 400, 1), ("vit_b", 640, 1),
                                             ("vit_b", 768, 1), ("vit_l", 384, 1), ("vit_h", 384, 1)])
def test_shallow_encoder_parity_any_size(version, patch, B):
    cfg = _cfg(version, patch, ENCODER_DEPTH=2, ENCODER_GLOBAL_ATTN_INDEXES=[1])
    oracle, net = build_pair(cfg)
    rgb = synth_tiles(B, patch, seed=4)
    s_ref, e_ref = oracle.infer_masks_and_img_features(rgb)
    s, e = net.infer_masks_and_img_features(rgb.cuda())
    assert tuple(e.shape) == tuple(e_ref.shape) == (B, 256, patch // 16, patch // 16)
    assert tuple(s.shape) == tuple(s_ref.shape)
    e, s = e.cpu(), s.cpu()
    assert torch.isfinite(e).all() and torch.isfinite(s).all()
    tag = f"patch_sizes_shallow_{version}_{patch}_B{B}"
    T.check(tag + "_emb_rel_l2", rel_l2(e, e_ref), T.EMB_REL_L2_SHALLOW)
    T.check(tag + "_mask_score", (s - s_ref).abs().max().item(), T.MASK_SCORE)


CFG384 = _cfg("vit_b", 384)


@pytest.mark.parametrize("B", [4, 16])      # 2304 tokens; 9216 tokens (the z192 GEMM bodies)
def test_full_depth_vitb_384(B):
    oracle, net = build_pair(CFG384, seed=384 + B)
    rgb = synth_tiles(B, 384, seed=B)
    s_ref, e_ref = oracle.infer_masks_and_img_features(rgb)
    s, e = net.infer_masks_and_img_features(rgb.cuda())
    e, s = e.cpu(), s.cpu()
    assert torch.isfinite(e).all() and torch.isfinite(s).all()
    tag = f"patch_sizes_full_vitb384_B{B}"
    T.check(tag + "_emb_rel_l2", rel_l2(e, e_ref), T.EMB_REL_L2)
    T.check(tag + "_emb_max_abs", (e - e_ref).abs().max().item(), T.EMB_MAX_ABS)
    T.check(tag + "_mask_score", (s - s_ref).abs().max().item(), T.MASK_SCORE)


def test_full_forward_vitb_384_with_toponet():
    oracle, net = build_pair(CFG384, seed=3840)
    B = 2
    rgb = synth_tiles(B, 384, seed=11)
    points, pairs, valid = synth_queries(B, 96, 384, seed=13)
    ml_r, ms_r, tl_r, ts_r = oracle(rgb, points, pairs, valid)
    ml, ms, tl, ts = [t.cpu() for t in net(rgb.cuda(), points.cuda(), pairs.cuda(), valid.cuda())]
    v = valid.bool()
    assert v.any() and torch.isfinite(ts[..., 0][v]).all()
    T.check("patch_sizes_forward_vitb384_mask_score", (ms - ms_r).abs().max().item(), T.MASK_SCORE)
    T.check("patch_sizes_forward_vitb384_topo_score", (ts[..., 0][v] - ts_r[..., 0][v]).abs().max().item(), T.TOPO_SCORE)
    agree = ((ts[..., 0][v] > 0.5) == (ts_r[..., 0][v] > 0.5)).float().mean().item()
    T.check("patch_sizes_forward_vitb384_topo_decisions", agree, T.TOPO_DECISIONS, at_least=True)


def test_sam_decoder_384_vs_oracle():
    """USE_SAM_DECODER at 384 px: 24 x 24 image tokens, 96^2 low-res masks bilinearly upsampled to 384^2, all 12 encoder blocks."""
    from sam_road_amd import Config, SAMRoad
    cfg = _cfg("vit_b", 384, USE_SAM_DECODER=True)
    warnings.simplefilter("ignore")
    oracle = SAMRoadOracle(AttrDict(cfg)).eval()
    sd = synth_state_dict_keyed(oracle, 41)
    oracle.load_state_dict(sd, strict=True)
    net = SAMRoad(Config(cfg))
    net.load_state_dict(sd, strict=True)
    net.eval().to("cuda")
    rgb = synth_tiles(2, 384, seed=14)
    ms_r, e_r = oracle.infer_masks_and_img_features(rgb)
    ms, e = net.infer_masks_and_img_features(rgb.cuda())
    ms = ms.cpu()
    assert ms.shape == ms_r.shape and torch.isfinite(ms).all()
    T.check("patch_sizes_samdec_384_mask_score", (ms - ms_r).abs().max().item(), T.SAMDEC_SCORE)


# ---- scene ----------------------------------------------------------------------------------------------------------------------------
SCENE_CFG = _cfg("vit_b", 384, ENCODER_DEPTH=2, ENCODER_GLOBAL_ATTN_INDEXES=[1], INFER_BATCH_SIZE=4, SAMPLE_MARGIN=32,
                 INFER_PATCHES_PER_EDGE=3, ITSC_THRESHOLD=0.5, ROAD_THRESHOLD=0.5, TOPO_THRESHOLD=0.5, ITSC_NMS_RADIUS=8,
                 ROAD_NMS_RADIUS=16, NEIGHBOR_RADIUS=64, MAX_NEIGHBOR_QUERIES=16)
SCENE = 640


def test_scene_384_tiles():
    """infer_one_img with 384-px tiles (3 x 3 tiles over a 640-px scene, a ragged last batch of 1): the u8 masks of pass 1 against
    oracle.scene, then the graph stage-wise on identical inputs, as tests/test_gpu_scene.py does at 256 px."""
    from sam_road_amd import Config
    from sam_road_amd.inferencer import infer_one_img
    oracle, net = scene_kit.build_pair(SCENE_CFG, seed=78)
    img = synth_scene(SCENE, seed=9)
    ref = scene_kit.oracle_scene(oracle, img, SCENE_CFG["INFER_PATCHES_PER_EDGE"], cfg=SCENE_CFG)
    assert len(ref[0]) == 9
    cfg = dict(SCENE_CFG, **scene_kit.thresholds(ref[2], ref[3]))
    got = infer_one_img(net, img, Config(cfg))
    for mask, mask_r in zip(got[2:], ref[2:]):
        d = np.abs(mask.astype(int) - mask_r.astype(int))
        T.check("patch_sizes_scene384_u8_within1", (d <= 1).mean(), T.U8_WITHIN1, at_least=True)
    scene_kit.check_scene_parity(None, got, ref, cfg, oracle)


# ---- the range ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("patch", [112, 1040, 200])
def test_out_of_range_patch_size_is_refused_at_pack_time(patch):
    """Below 128, above 1024 or not a multiple of 16: the weights do not pack, and the message names the supported range."""
    from sam_road_amd import Config, SAMRoad
    from sam_road_amd._lib import SrhError
    warnings.simplefilter("ignore")
    net = SAMRoad(Config(_cfg("vit_b", patch, ENCODER_DEPTH=1, ENCODER_GLOBAL_ATTN_INDEXES=[])))
    net.load_state_dict(synth_state_dict(net, 5), strict=True)
    net.eval().to("cuda")
    with pytest.raises(SrhError, match="128 to 1024"):
        net._weights(torch.device("cuda", 0))
