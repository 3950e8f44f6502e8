"""Op-level parity of the fused TopoNet trunk (csrc/topo_fused.hip topo_fused_kernel: pair_proj, three post-LN encoder layers, output_proj
and the sigmoid in one kernel) through the test-only export srh_op_topo_trunk, against tests/heads_ref.py topo_trunk_ref in float64.

The model is heads_ref.topo_fill's: fp16-representable matrices, biases / betas ~ N(0, 1), gammas in +-[1, 2], peaked and flat softmax
rows — tests/test_heads_ref.py shows on the CPU that a rotated bias, a swapped head, a wrong scale or a wrong mask moves these
outputs by >= 10x the bounds used here.  Every token mapping of the kernel (K <= 15 packed, K = 16, wave groups of 2 .. 4) at each
boundary of its dispatch, sequence counts around one workgroup pass and just above the grid's 256 passes (the persistent loop's
second walk), and the properties its header claims: slot / tile-mate independence, zero weights on the pad columns, no store past
the last row.  One chain test runs srh_toponet on the same model against heads_ref.toponet_ref.  Run on an MI355X: pytest -m gpu."""
import ctypes as C
import warnings

import pytest
import torch

import heads_ref
import tolerances as T

pytestmark = pytest.mark.gpu

SEED = 2                      # tests/test_heads_ref.py proves the discrimination for this model
KS = [1, 2, 3, 5, 8, 15, 16, 17, 32, 33, 48, 49, 64]
VERSIONS = ["normal", "no_transformer"]
CANARY = 64
TF_NW, TF_GRID = 8, 256       # csrc/topo_fused.hip: waves per workgroup, workgroups of the persistent grid
SRH_ERR_BAD_ARG, SRH_ERR_UNSUPPORTED = -1, -2      # include/samroad_hip.h


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


_NETS = {}


def _topo_net(seed, version):
    """The HIP model with heads_ref.topo_fill's TopoNet (the oracle-side twin is tests/test_heads_ref.py _topo_net)."""
    if (seed, version) not in _NETS:
        from oracle.synth import synth_state_dict
        from sam_road_amd import Config, SAMRoad
        warnings.simplefilter("ignore")
        net = SAMRoad(Config(dict(SAM_VERSION="vit_b", PATCH_SIZE=256, TOPONET_VERSION=version, SAM_CKPT_PATH="", ENCODER_DEPTH=1,
                                  ENCODER_GLOBAL_ATTN_INDEXES=[])))
        sd = synth_state_dict(net, seed)
        sd.update(heads_ref.topo_fill(sd, seed))
        net.load_state_dict(sd, strict=True)
        _NETS[seed, version] = net.eval().to("cuda")
    return _NETS[seed, version]


def _handles(version):
    assert torch.cuda.is_available(), "gpu-marked test needs a GPU"
    net = _topo_net(SEED, version)
    ctx, wh = net._weights(torch.device("cuda", 0))
    sd = {k: v.detach().cpu() for k, v in net.state_dict().items() if k.startswith("topo_net.")}
    return ctx, wh, sd


def _units_per_pass(K, version):
    """(units per workgroup pass, pair rows per unit) as tf_launch counts them."""
    if K == 16:
        return TF_NW, 16                                       # one sequence per wave
    if version == "no_transformer":
        return TF_NW * 16, 1                                   # no attention: a tile is 16 consecutive pair rows
    if K < 16:
        slot = 1 << (K - 1).bit_length()                       # K rounded up to a power of two
        return TF_NW * (16 // slot), K
    return TF_NW // ((K + 15) // 16), K                        # G waves per sequence, the spare waves of G = 3 idle


def _seq_counts(K, version):
    """1, one unit less and one more than a workgroup pass, and just above the 256 passes of the grid (a second walk of the loop)."""
    per, rows_per_unit = _units_per_pass(K, version)
    if rows_per_unit == 1:                                     # units are pair rows: the sequence counts whose rows straddle the marks
        marks = [max(1, (per - 1) // K), per // K + 1, TF_GRID * per // K + 1]
    else:
        marks = [max(1, per - 1), per + 1, TF_GRID * per + 1]
    return sorted({1, *marks})


def _run(ctx, wh, rows, valid, nseq, K, ld, want_logits=True, want_scores=True, expect=0):
    """One srh_op_topo_trunk call on host tensors -> (logits, scores) on the host, each nseq*K + CANARY long and NaN where nothing was
    stored."""
    n = nseq * K
    d_rows, d_valid = rows.cuda(), valid.cuda()                # held until the synchronize below
    lg = torch.full((n + CANARY,), float("nan"), device="cuda") if want_logits else None
    sc = torch.full((n + CANARY,), float("nan"), device="cuda") if want_scores else None
    rc = ctx.lib.srh_op_topo_trunk(ctx.handle, wh, _p(d_rows), ld, _p(d_valid), nseq, K, _p(lg), _p(sc), None)
    torch.cuda.synchronize()
    assert rc == expect, (rc, ctx.lib.srh_last_error(ctx.handle))
    return (lg.cpu() if lg is not None else None), (sc.cpu() if sc is not None else None)


def _same_bits(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


@pytest.mark.parametrize("version", VERSIONS)
@pytest.mark.parametrize("K", KS)
def test_topo_trunk_op(K, version):
    ctx, wh, sd = _handles(version)
    worst_l = worst_s = 0.0
    for nseq in _seq_counts(K, version):
        n = nseq * K
        rows, valid = heads_ref.topo_trunk_inputs(nseq, K, seed=1000 * K + nseq)
        lg, sc = _run(ctx, wh, rows, valid, nseq, K, 320)
        tag = f"K={K} {version} nseq={nseq}"
        assert torch.isfinite(lg[:n]).all() and torch.isfinite(sc[:n]).all(), f"{tag}: unwritten or non-finite outputs"
        assert torch.isnan(lg[n:]).all() and torch.isnan(sc[n:]).all(), f"{tag}: a store past row nseq*K"

        ref_l, ref_s = heads_ref.topo_trunk_ref(rows, valid, sd, K)
        d = heads_ref.topo_defined(valid).reshape(-1)
        el = (lg[:n].double() - ref_l)[d].abs().max().item()
        es = (sc[:n].double() - ref_s)[d].abs().max().item()
        print(f"[topo_trunk {tag}] rows {n}: logits max-abs {el:.3e}, scores {es:.3e}")
        worst_l, worst_s = max(worst_l, el), max(worst_s, es)

        lg_only, none = _run(ctx, wh, rows, valid, nseq, K, 320, want_scores=False)
        assert none is None and _same_bits(lg_only, lg), f"{tag}: logits alone differ from the both-outputs call"
        none, sc_only = _run(ctx, wh, rows, valid, nseq, K, 320, want_logits=False)
        assert none is None and _same_bits(sc_only, sc), f"{tag}: scores alone differ from the both-outputs call"
        lg2, sc2 = _run(ctx, wh, rows, valid, nseq, K, 320)
        assert _same_bits(lg2, lg) and _same_bits(sc2, sc), f"{tag}: a second identical call gives other bits"

        # every sequence in another slot, tile, wave group and workgroup: the same bits
        lg_r, sc_r = _run(ctx, wh, rows.view(nseq, K, 320).flip(0).reshape(n, 320).contiguous(), valid.flip(0).contiguous(), nseq, K, 320)
        assert _same_bits(lg_r[:n].view(nseq, K).flip(0), lg[:n].view(nseq, K)), f"{tag}: logits depend on the sequence's position"
        assert _same_bits(sc_r[:n].view(nseq, K).flip(0), sc[:n].view(nseq, K)), f"{tag}: scores depend on the sequence's position"

        # the packed pair_proj fragments are zero on columns 258 .. 319: finite garbage there changes nothing
        g = torch.Generator().manual_seed(nseq)
        junk = rows.clone()
        junk[:, 258:] = (torch.randn(n, 62, generator=g) * 100).half()
        lg_j, sc_j = _run(ctx, wh, junk, valid, nseq, K, 320)
        assert _same_bits(lg_j, lg) and _same_bits(sc_j, sc), f"{tag}: columns 258 .. 319 reach the outputs"

        # a wider row stride; nothing beyond column 319 is read
        wide = torch.full((n, 328), float("nan"), dtype=torch.float16)
        wide[:, :320] = rows
        lg_w, sc_w = _run(ctx, wh, wide, valid, nseq, K, 328)
        assert _same_bits(lg_w, lg) and _same_bits(sc_w, sc), f"{tag}: ld = 328 differs from ld = 320"
    bound_l, bound_s = heads_ref.topo_op_bounds(T, version)
    T.check(f"topo_trunk_op_k{K}_{version}_logit", worst_l, bound_l)
    T.check(f"topo_trunk_op_k{K}_{version}_score", worst_s, bound_s)


def test_topo_trunk_refusals_launch_nothing():
    ctx, wh, _ = _handles("normal")
    K, nseq = 5, 3
    rows, valid = heads_ref.topo_trunk_inputs(nseq, K, seed=1)
    d_rows, d_valid = rows.cuda(), torch.zeros(nseq * K + 4, dtype=torch.uint8, device="cuda")
    d_valid[:nseq * K] = valid.reshape(-1).cuda()
    lg = torch.full((64 * nseq + CANARY,), float("nan"), device="cuda")
    sc = torch.full((64 * nseq + CANARY,), float("nan"), device="cuda")
    call = ctx.lib.srh_op_topo_trunk
    cases = [("ld below 320", SRH_ERR_BAD_ARG, (_p(d_rows), 312, _p(d_valid), nseq, K)),
             ("ld no multiple of 8", SRH_ERR_BAD_ARG, (_p(d_rows), 324, _p(d_valid), nseq, K)),
             ("null pair rows", SRH_ERR_BAD_ARG, (None, 320, _p(d_valid), nseq, K)),
             ("null valid", SRH_ERR_BAD_ARG, (_p(d_rows), 320, None, nseq, K)),
             ("valid not 4-byte aligned", SRH_ERR_BAD_ARG, (_p(d_rows), 320, C.c_void_p(d_valid.data_ptr() + 1), nseq, K)),
             ("K = 0", SRH_ERR_UNSUPPORTED, (_p(d_rows), 320, _p(d_valid), nseq, 0)),
             ("K = 65", SRH_ERR_UNSUPPORTED, (_p(d_rows), 320, _p(d_valid), nseq, 65)),
             ("nseq = 0", 0, (_p(d_rows), 320, _p(d_valid), 0, K))]
    for name, want, args in cases:
        rc = call(ctx.handle, wh, *args, _p(lg), _p(sc), None)
        torch.cuda.synchronize()
        assert rc == want, (name, rc)
        assert torch.isnan(lg).all() and torch.isnan(sc).all(), f"{name}: something was launched"
    assert call(None, wh, _p(d_rows), 320, _p(d_valid), nseq, K, _p(lg), _p(sc), None) == SRH_ERR_BAD_ARG
    assert call(ctx.handle, None, _p(d_rows), 320, _p(d_valid), nseq, K, _p(lg), _p(sc), None) == SRH_ERR_BAD_ARG
    torch.cuda.synchronize()
    assert torch.isnan(lg).all() and torch.isnan(sc).all()
    # and the same buffers through a good call
    assert call(ctx.handle, wh, _p(d_rows), 320, _p(d_valid), nseq, K, _p(lg), _p(sc), None) == 0
    torch.cuda.synchronize()
    assert torch.isfinite(lg[:nseq * K]).all() and torch.isnan(lg[nseq * K:]).all()


@pytest.mark.parametrize("i64", [False, True])
@pytest.mark.parametrize("K", [5, 16, 33])
def test_toponet_chain(K, i64):
    """srh_toponet (sampler, feature_proj, gather, trunk) on the O(1)-parameter model: feature_proj's bias and ReLU too."""
    net = _topo_net(SEED, "normal")
    patch = 256
    emb, points, pairs, valid = heads_ref.toponet_chain_inputs(K, i64, patch)
    outside = ((points < 0) | (points > patch)).any(-1)
    assert outside.any() and not outside.all()
    lg, sc = net._topo(emb.permute(0, 3, 1, 2).cuda(), points.cuda(), pairs.cuda(), valid.cuda(), True)
    torch.cuda.synchronize()
    lg, sc = lg.cpu().reshape(-1), sc.cpu().reshape(-1)
    ref_l, ref_s = heads_ref.toponet_ref(emb, points, pairs, valid, net.state_dict(), patch)
    d = heads_ref.topo_defined(valid).reshape(-1)
    assert torch.isfinite(lg[d]).all() and torch.isfinite(sc[d]).all()
    tag = f"topo_chain_k{K}_{'i64' if i64 else 'f32'}"
    T.check(tag + "_logit", (lg.double() - ref_l)[d].abs().max().item(), T.TOPO_CHAIN_LOGIT)
    T.check(tag + "_score", (sc.double() - ref_s)[d].abs().max().item(), T.TOPO_CHAIN_SCORE)
