"""Op-level parity of the SAM MaskDecoder branch (USE_SAM_DECODER: csrc/sam_decoder.hip's nine kernels, the image-side GEMMs and
LayerNorm, in the launch sequence of sam_decode(), csrc/api_model.hip) through the test-only export srh_op_sam_decoder, against
tests/samdec_ref.py samdec_ref in float64.

The model is samdec_ref.samdec_fill's: fp16-representable image-side matrices, biases / betas ~ N(0, 1), gammas in +-[1, 2], peaked,
in-between and flat heads in every attention, mask logits up to +-20 with a quarter of the scores undecided.  tests/test_samdec_ref.py
shows on the CPU that these inputs meet those conditions on every shape below and that a wrong scale, a swapped head, a dropped
positional term, a wrong mask token, sub-pixel order, hyper-network or upsample rule moves these outputs by >= 10x the bounds used here.
With the synth_state_dict weights of the three whole-model tests none of that holds: there the most peaked token->image head puts
0.042 on its best key at S = 16 and 0.015 at S = 32 (11 x and 16 x the uniform weight), the most peaked image->token head 0.27 on its best
of 4 keys, and max|logit| is 1.7 (test_synthetic_weights_are_never_peaked records it).

Shapes: the smallest at which each path exists — S = 8 (HW = 64: three waves of sd_t2i_attn_kernel own no key, a workgroup of
sd_i2t_attn_kernel is half empty), S = 9 and 25 (odd grids, ragged GEMM M, HW no multiple of 64), S = 16 (the 256-px geometry; B = 5 for
the stride-addressed token rows), S = 32, and S = 64 (66,688 bytes of dynamic LDS: the opt-in above 64 KiB).  Run on an MI355X:
pytest -m gpu."""
import ctypes as C
import warnings

import pytest
import torch

import samdec_ref as R
import tolerances as T

pytestmark = pytest.mark.gpu

SEED = 2                      # tests/test_samdec_ref.py proves the conditions and the discrimination for this model
CANARY = 64
SRH_ERR_BAD_ARG, SRH_ERR_UNSUPPORTED = -1, -2      # include/samroad_hip.h
NAMES = ("logits", "scores", "tokens", "low")


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


_NETS = {}


def _net(S, sam_decoder=True):
    """The HIP model of one patch size with samdec_fill's SAM decoder (one encoder block: the op tests never run it)."""
    if (S, sam_decoder) not in _NETS:
        from oracle.synth import synth_state_dict
        from sam_road_amd import Config, SAMRoad
        assert torch.cuda.is_available(), "gpu-marked test needs a GPU"
        warnings.simplefilter("ignore")
        net = SAMRoad(Config(dict(SAM_VERSION="vit_b", PATCH_SIZE=16 * S, TOPONET_VERSION="normal", SAM_CKPT_PATH="", ENCODER_DEPTH=1,
                                  ENCODER_GLOBAL_ATTN_INDEXES=[], USE_SAM_DECODER=sam_decoder)))
        sd = synth_state_dict(net, SEED)
        sd.update(R.samdec_fill(sd, SEED))
        net.load_state_dict(sd, strict=True)
        _NETS[S, sam_decoder] = net.eval().to("cuda")
    return _NETS[S, sam_decoder]


def _handles(S):
    net = _net(S)
    ctx, wh = net._weights(torch.device("cuda", 0))
    return ctx, wh, {k: v.detach().cpu() for k, v in net.state_dict().items()}


def _sizes(S, B):
    P = 16 * S
    return dict(logits=B * P * P * 2, scores=B * P * P * 2, tokens=B * 4 * 256, low=B * 2 * 16 * S * S)


def _run(ctx, wh, emb, S, B, want=NAMES, expect=0):
    """One srh_op_sam_decoder call on host embeddings -> dict name -> host tensor, each its size + CANARY long and NaN where nothing was
    stored (None for an output that was not asked for)."""
    d_emb = emb.cuda()                                          # held until the synchronize below
    bufs = {k: (torch.full((n + CANARY,), float("nan"), device="cuda") if k in want else None) for k, n in _sizes(S, B).items()}
    rc = ctx.lib.srh_op_sam_decoder(ctx.handle, wh, _p(d_emb), B, *(_p(bufs[k]) for k in NAMES), None)
    torch.cuda.synchronize()
    assert rc == expect, (rc, ctx.lib.srh_last_error(ctx.handle))
    return {k: (v.cpu() if v is not None else None) for k, v in bufs.items()}


def _same_bits(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


_RUNS = {}


def _case(S, B):
    """(emb, the device's four outputs, the float64 reference's) of a shape, computed once and shared by the tests."""
    if (S, B) not in _RUNS:
        ctx, wh, sd = _handles(S)
        emb = R.samdec_inputs(B, S, R.case_seed(S, B))
        _RUNS[S, B] = emb, _run(ctx, wh, emb, S, B), dict(zip(NAMES, R.samdec_ref(emb, sd, S)))
    return _RUNS[S, B]


@pytest.mark.parametrize("S,B", R.SHAPES)
def test_sam_decoder_op(S, B):
    emb, got, ref = _case(S, B)
    bounds = dict(logits=T.SAMDEC_OP_LOGIT, scores=T.SAMDEC_OP_SCORE, tokens=T.SAMDEC_OP_TOKENS, low=T.SAMDEC_OP_LOWRES)
    err = {}
    for k, n in _sizes(S, B).items():
        assert torch.isfinite(got[k][:n]).all(), f"S={S} B={B}: unwritten or non-finite {k}"
        assert torch.isnan(got[k][n:]).all(), f"S={S} B={B}: a store past the end of {k}"
        err[k] = (got[k][:n].double() - ref[k].reshape(-1)).abs().max().item()      # every element
    print(f"[samdec_op S={S} B={B}] " + " ".join(f"{k} max-abs {v:.3e}" for k, v in err.items()) +
          f"  (max|logit| {ref['logits'].abs().max().item():.1f})")
    for k, tag in zip(NAMES, ("logit", "score", "tokens", "lowres")):
        T.check(f"samdec_op_s{S}_b{B}_{tag}", err[k], bounds[k])


@pytest.mark.parametrize("S,B", R.SHAPES)
def test_upsample_is_exact_on_the_device_low_res(S, B):
    """sd_upsample_kernel alone: the returned logits against a float64 bilinear x4 of the RETURNED low_res, the returned scores against the
    float64 sigmoid of the returned logits — f32 arithmetic on given inputs, every pixel, all borders and corners of every tile."""
    _, got, _ = _case(S, B)
    P, n = 16 * S, _sizes(S, B)
    low = got["low"][:n["low"]].double().reshape(B, 2, 4 * S, 4 * S)
    logits = got["logits"][:n["logits"]].double().reshape(B, P, P, 2)
    scores = got["scores"][:n["scores"]].double().reshape(B, P, P, 2)
    d = (logits - R.upsample4_ref(low).permute(0, 2, 3, 1)).abs()
    edge = torch.zeros(P, dtype=torch.bool)
    edge[:2] = edge[-2:] = True                                 # the rows / columns whose taps are clamped
    border = (edge.view(P, 1) | edge.view(1, P)).view(1, P, P, 1).expand_as(d)
    scale = low.abs().max().item()
    print(f"[samdec_upsample S={S} B={B}] logits / max|low_res| ({scale:.1f}): all {d.max().item() / scale:.3e}, clamped border "
          f"{d[border].max().item() / scale:.3e}; scores {(scores - torch.sigmoid(logits)).abs().max().item():.3e}")
    T.check(f"samdec_upsample_s{S}_b{B}", d.max().item() / scale, T.SAMDEC_UPSAMPLE_F32)
    T.check(f"samdec_sigmoid_s{S}_b{B}", (scores - torch.sigmoid(logits)).abs().max().item(), T.SAMDEC_SIGMOID_F32)


def test_outputs_are_optional():
    S, B = 9, 2
    ctx, wh, _ = _handles(S)
    emb, full, _ = _case(S, B)
    for want in (("logits",), ("scores",), ("logits", "scores"), ("tokens",), ("low",)):
        got = _run(ctx, wh, emb, S, B, want=want)
        for k in NAMES:
            if k in want:
                assert _same_bits(got[k], full[k]), f"{k} alone ({want}) differs from the full call"
            else:
                assert got[k] is None
    again = _run(ctx, wh, emb, S, B)
    assert all(_same_bits(again[k], full[k]) for k in NAMES), "a second identical call gives other bits"


def test_tiles_do_not_see_each_other():
    """Every kernel of the branch computes a row from its own tile, in an order that does not depend on the tile's position in the batch."""
    S, B = 9, 4
    ctx, wh, _ = _handles(S)
    emb = R.samdec_inputs(B, S, R.case_seed(S, B)).reshape(B, S * S * 256)
    base = _run(ctx, wh, emb.reshape(-1, 256), S, B)
    n = _sizes(S, B)
    perm = torch.tensor([2, 0, 3, 1])
    moved = _run(ctx, wh, emb[perm].reshape(-1, 256).contiguous(), S, B)
    for k in NAMES:
        a, b = base[k][:n[k]].reshape(B, -1), moved[k][:n[k]].reshape(B, -1)
        assert _same_bits(b, a[perm].contiguous()), f"{k}: a tile's result depends on its position in the batch"
    other = emb.clone()
    other[1] = R.samdec_inputs(1, S, 7).reshape(-1)
    swapped = _run(ctx, wh, other.reshape(-1, 256), S, B)
    keep = torch.tensor([0, 2, 3])
    for k in NAMES:
        a, b = base[k][:n[k]].reshape(B, -1), swapped[k][:n[k]].reshape(B, -1)
        assert _same_bits(b[keep].contiguous(), a[keep].contiguous()), f"{k}: a tile's result depends on another tile's embeddings"
        assert not _same_bits(b[1].contiguous(), a[1].contiguous())


def test_op_is_what_the_model_runs():
    """srh_encode_decode with these weights, then srh_op_sam_decoder on the embeddings it returned: the same logits and scores bit for bit,
    so the op-level results speak for the product path."""
    from oracle.synth import synth_tiles
    S, B = 16, 2
    net = _net(S)
    ctx, wh, _ = _handles(S)
    logits, scores, emb = net._encode(synth_tiles(B, 16 * S, seed=5).cuda(), True, True)
    torch.cuda.synchronize()
    emb = emb.permute(0, 2, 3, 1)
    assert emb.is_contiguous() and torch.isfinite(emb).all()
    got = _run(ctx, wh, emb.reshape(-1, 256).cpu(), S, B)
    n = _sizes(S, B)
    assert _same_bits(got["logits"][:n["logits"]], logits.cpu().reshape(-1)), "the op's logits are not the model's"
    assert _same_bits(got["scores"][:n["scores"]], scores.cpu().reshape(-1)), "the op's scores are not the model's"


def test_refusals():
    S, B = 8, 2
    ctx, wh, _ = _handles(S)
    _, wh_naive = _net(S, sam_decoder=False)._weights(torch.device("cuda", 0))
    d_emb = R.samdec_inputs(B, S, 1).cuda()
    bufs = [torch.full((n + CANARY,), float("nan"), device="cuda") for n in _sizes(S, B).values()]
    call = ctx.lib.srh_op_sam_decoder
    cases = [("weights without use_sam_decoder", SRH_ERR_UNSUPPORTED, (ctx.handle, wh_naive, _p(d_emb), B)),
             ("null embeddings", SRH_ERR_BAD_ARG, (ctx.handle, wh, None, B)),
             ("null weights", SRH_ERR_BAD_ARG, (ctx.handle, None, _p(d_emb), B)),
             ("null context", SRH_ERR_BAD_ARG, (None, wh, _p(d_emb), B)),
             ("B = 0", SRH_ERR_BAD_ARG, (ctx.handle, wh, _p(d_emb), 0)),
             ("B = -1", SRH_ERR_BAD_ARG, (ctx.handle, wh, _p(d_emb), -1))]
    for name, want, args in cases:
        rc = call(*args, *(_p(b) for b in bufs), None)
        torch.cuda.synchronize()
        assert rc == want, (name, rc)
        assert all(torch.isnan(b).all() for b in bufs), f"{name}: something was launched"
    assert call(ctx.handle, wh, _p(d_emb), B, None, None, None, None, None) == 0          # no output: a no-op
    # and the same buffers through a good call
    assert call(ctx.handle, wh, _p(d_emb), B, *(_p(b) for b in bufs), None) == 0
    torch.cuda.synchronize()
    for b, n in zip(bufs, _sizes(S, B).values()):
        assert torch.isfinite(b[:n]).all() and torch.isnan(b[n:]).all()
