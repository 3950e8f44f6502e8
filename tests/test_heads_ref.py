"""CPU pins of the float64 references in tests/heads_ref.py to oracle/samroad.py's modules (map_decoder, BilinearSampler,
TopoNet's pair gather in fp32; TopoNet's trunk in float64) on seeded inputs: a wrong reference fails here, on any host, instead of on
the GPU box where tests/test_gpu_heads.py and tests/test_gpu_topo_trunk.py compare the HIP kernels with it.  For the trunk also the
proof that its test model and inputs discriminate: the shape of the layer-0 attention, and every single mistake of a list moving the
reference's outputs by >= 10x the bounds of the GPU tests."""
import warnings

import pytest
import torch

import heads_ref
import tolerances as T
from oracle.samroad import AttrDict, SAMRoadOracle

PIN = 1e-5
PIN64 = 1e-10      # float64 against float64: rounding only (outputs of O(1..10), sums of a few hundred terms)


def _oracle(**kw):
    warnings.simplefilter("ignore")
    cfg = dict(SAM_VERSION="vit_b", PATCH_SIZE=256, TOPONET_VERSION="normal", SAM_CKPT_PATH="", ENCODER_DEPTH=1,
               ENCODER_GLOBAL_ATTN_INDEXES=[]) | kw
    torch.manual_seed(0)
    return SAMRoadOracle(AttrDict(cfg)).eval()


def _fill_decoder(model, g):
    """Decoder parameters away from the defaults: LayerNorm2d gamma / beta far from 1 / 0, layer-7 bias not -3."""
    with torch.no_grad():
        for (idx, cin, cout), std in zip(heads_ref._MD_LAYERS, heads_ref.DECODER_STDS):
            conv = model.map_decoder[idx]
            conv.weight.copy_(torch.randn(cin, cout, 2, 2, generator=g) * std)
            conv.bias.copy_(torch.randn(cout, generator=g))
        ln = model.map_decoder[1]
        ln.weight.copy_((1.0 + torch.rand(128, generator=g)) * torch.sign(torch.randn(128, generator=g)))
        ln.bias.copy_(3 * torch.rand(128, generator=g) - 1.5)
        model.map_decoder[7].bias.copy_(torch.tensor([0.7, -1.3]))


def test_map_decoder_ref_matches_oracle():
    model = _oracle()
    g = torch.Generator().manual_seed(3)
    _fill_decoder(model, g)
    emb = torch.randn(2, 256, 16, 16, generator=g)
    with torch.no_grad():
        want = model.map_decoder(emb)                              # fp32 NCHW logits
    logits, scores = heads_ref.map_decoder_ref(emb.permute(0, 2, 3, 1), model.state_dict(), tiles_per_step=1)
    want = want.permute(0, 2, 3, 1).double()
    assert want.abs().max() > 8, "the pin should reach large logits"
    scale = max(1.0, want.abs().max().item())
    assert (logits - want).abs().max().item() < PIN * scale
    assert (scores - torch.sigmoid(want)).abs().max().item() < PIN


def test_sample_ref_matches_oracle():
    model = _oracle(PATCH_SIZE=512)
    g = torch.Generator().manual_seed(4)
    emb = torch.randn(3, 384, 32, 32, generator=g)
    edge = torch.tensor([0.0, 0.5, 7.5, 8.0, 8.25, 503.75, 504.0, 511.0, 511.5, 512.0, -1.0, -8.0, -9.0, -100.0, 513.0, 520.0, 521.0, 612.0])
    pts = torch.cartesian_prod(edge, edge)
    pts = torch.cat([pts, torch.rand(200, 2, generator=g) * 560 - 24]).unsqueeze(0).expand(3, -1, -1).contiguous()
    with torch.no_grad():
        want = model.bilinear_sampler(emb, pts).reshape(-1, 384).double()
    got = heads_ref.sample_ref(emb.permute(0, 2, 3, 1), pts, 512)
    assert want.abs().max() > 1 and (want == 0).any(), "the pin should cover outside points"
    assert (got - want).abs().max().item() < PIN
    # point_tile: the same rows through explicit (clamped) tile indices
    tiles = torch.tensor([-5, 0, 1, 2, 7]).repeat_interleave(pts.shape[1])[:3 * pts.shape[1]]
    got_t = heads_ref.sample_ref(emb.permute(0, 2, 3, 1), pts, 512, point_tile=tiles)
    want_t = torch.cat([want[tiles.clamp(0, 2)[i * pts.shape[1]] * pts.shape[1]:][:pts.shape[1]] for i in range(3)])
    assert torch.equal(got_t, heads_ref.sample_ref(emb.permute(0, 2, 3, 1), pts, 512, point_tile=tiles.clamp(0, 2)))
    assert (got_t - want_t).abs().max().item() < PIN


def test_pair_gather_ref_matches_oracle():
    for version in ("normal", "no_offset"):
        model = _oracle(TOPONET_VERSION=version)
        g = torch.Generator().manual_seed(5)
        B, N, Ns, K = 2, 23, 7, 16
        feats = torch.randn(B, N, 256, generator=g)
        points = (torch.rand(B, N, 2, generator=g) * 300 - 20)
        pairs = torch.randint(0, N, (B, Ns, K, 2), generator=g)
        valid = torch.rand(B, Ns, K, generator=g) < 0.7
        seen = {}
        def grab(mod, inp, out):            # the pair rows TopoNet feeds pair_proj (model.py:104-116)
            seen["x"] = inp[0].detach()
        hook = model.topo_net.pair_proj.register_forward_hook(grab)
        with torch.no_grad():
            model.topo_net(points, feats, pairs, valid)
            pf = torch.relu(model.topo_net.feature_proj(feats))
        hook.remove()
        want = seen["x"].reshape(-1, 258).double()
        got = heads_ref.pair_gather_ref(pf, points, pairs, 264, zero_offset=version == "no_offset")
        assert ((got[:, :258] - want).abs() / want.abs().clamp(min=1)).max().item() < PIN   # the offsets are fp32 differences of O(100)
        assert not got[:, 258:].any()
        # negative indices wrap as Python's; a base shifts every index
        neg = torch.where(pairs % 2 == 0, pairs - N, pairs)
        assert torch.equal(heads_ref.pair_gather_ref(pf, points, neg, 264), heads_ref.pair_gather_ref(pf, points, pairs, 264))
        assert torch.equal(heads_ref.pair_gather_ref(pf, points, pairs + 1000, 320, index_base=1000)[:, :264],
                           heads_ref.pair_gather_ref(pf, points, pairs, 264))


# ---- the TopoNet trunk: topo_trunk_ref against the oracle, and proof that the trunk tests' model and inputs discriminate ----------------
SEED = 2
_TL = heads_ref._TL


def _topo_net(seed, version):
    """The oracle with the O(1)-parameter TopoNet of the trunk tests (heads_ref.topo_fill): fp16-representable matrices, biases and
    betas ~ N(0, 1), gammas in +-[1, 2], q / k rows scaled head by head.  tests/test_gpu_topo_trunk.py loads the same entries
    into the HIP model."""
    model = _oracle(TOPONET_VERSION=version)
    model.load_state_dict(heads_ref.topo_fill(model.state_dict(), seed), strict=False)
    return model


_NETS = {}


def _topo_sd(version):
    if version not in _NETS:
        _NETS[version] = {k: v.clone() for k, v in _topo_net(SEED, version).state_dict().items() if k.startswith("topo_net.")}
    return _NETS[version]


@pytest.mark.parametrize("version", ["normal", "no_transformer"])
@pytest.mark.parametrize("K", [1, 5, 16, 33, 64])
def test_topo_trunk_ref_matches_oracle(K, version):
    """oracle.samroad.TopoNet in float64, fed the pair rows in place of its own gather, on the defined slots (nn.TransformerEncoder's
    treatment of the others depends on the torch version)."""
    nseq = 21
    tn = _topo_net(SEED, version).topo_net.double()
    rows, valid = heads_ref.topo_trunk_inputs(nseq, K, seed=K)
    hook = tn.pair_proj.register_forward_pre_hook(lambda mod, inp: (rows[:, :258].double().view(1, nseq * K, 258),))
    with torch.no_grad():
        want_l, want_s = tn(torch.zeros(1, 2, 2, dtype=torch.float64), torch.zeros(1, 2, 256, dtype=torch.float64),
                            torch.zeros(1, nseq, K, 2, dtype=torch.int64), valid.view(1, nseq, K))
    hook.remove()
    logits, scores = heads_ref.topo_trunk_ref(rows, valid, _topo_sd(version), K)
    d = heads_ref.topo_defined(valid).reshape(-1)
    assert d.sum() > nseq * K // 3 and (~d).any() == (K > 1)
    assert (logits - want_l.reshape(-1))[d].abs().max().item() < PIN64 * max(1.0, want_l.abs().max().item())
    assert (scores - want_s.reshape(-1))[d].abs().max().item() < PIN64


PEAKED_SHARE = 0.25       # of the layer-0 softmax rows with >= 8 valid keys: largest weight > 0.9 ...
FLAT_SHARE = 0.25         # ... and largest weight < 0.5
MASKED_TOP_SHARE = 0.25   # of the rows of sequences with masked keys: the largest raw logit belongs to a masked key


@pytest.mark.parametrize("K", [16, 33, 64])
def test_topo_inputs_reach_peaked_and_flat_attention(K):
    nseq = 28
    rows, valid = heads_ref.topo_trunk_inputs(nseq, K, seed=K)
    probe = {}
    heads_ref.topo_trunk_ref(rows, valid, _topo_sd("normal"), K, probe=probe)
    mask, p, s = probe["mask"], probe["p"], probe["s"]
    assert torch.allclose(p.sum(-1), torch.ones(()).double()) and not p[~mask[:, None, None, :].expand_as(p)].any()
    many = (mask.sum(-1) >= 8)[:, None, None].expand(nseq, 4, K)
    top = p.amax(-1)[many]
    assert top.numel() >= 4 * K * 8
    peaked, flat = (top > 0.9).double().mean().item(), (top < 0.5).double().mean().item()
    print(f"[topo inputs K={K}] rows {top.numel()}  peaked {peaked:.2f}  flat {flat:.2f}")
    assert peaked >= PEAKED_SHARE and flat >= FLAT_SHARE
    # a max taken before the mask would pick a masked key's logit in these rows
    partial = ~mask.all(-1)
    top_is_masked = ~torch.gather(mask[:, None, None, :].expand_as(s), 3, s.argmax(-1, keepdim=True))[..., 0]
    share = top_is_masked[partial].double().mean().item()
    print(f"[topo inputs K={K}] masked key holds the row's largest raw logit: {share:.2f}")
    assert share >= MASKED_TOP_SHARE


def _rolled(sd, key, shift, lo=0, hi=None):
    out = dict(sd)
    t = sd[key].clone().reshape(-1)
    hi = t.numel() if hi is None else hi
    t[lo:hi] = torch.roll(t[lo:hi], shift)
    out[key] = t.reshape(sd[key].shape)
    return out


def _mutations(sd, K):
    """(name, state dict, mutate) of every single mistake the trunk tests must see."""
    D = heads_ref.TOPO_D
    n_layers = sum(1 for k in sd if k.endswith("norm1.weight"))
    muts = []
    for shift in (4, 16):
        muts.append((f"pair_proj.bias rot{shift}", _rolled(sd, "topo_net.pair_proj.bias", shift), None))
        muts.append((f"output_proj.weight rot{shift}", _rolled(sd, "topo_net.output_proj.weight", shift), None))
        for L in range(n_layers):
            pre = f"{_TL}{L}."
            # the k part of in_proj_bias is exempt: it adds q . bk, the same for every key of a softmax row, which cancels
            # (test_topo_k_bias_is_invisible asserts that on the reference)
            muts.append((f"L{L} q bias rot{shift}", _rolled(sd, pre + "self_attn.in_proj_bias", shift, 0, D), None))
            muts.append((f"L{L} v bias rot{shift}", _rolled(sd, pre + "self_attn.in_proj_bias", shift, 2 * D, 3 * D), None))
            for name in ("self_attn.out_proj.bias", "linear1.bias", "linear2.bias", "norm1.weight", "norm1.bias", "norm2.weight", "norm2.bias"):
                muts.append((f"L{L} {name} rot{shift}", _rolled(sd, pre + name, shift), None))
    dropped = dict(sd)
    dropped["topo_net.output_proj.bias"] = torch.zeros(1)
    muts.append(("output_proj.bias dropped", dropped, None))
    if n_layers:
        muts.append(("V heads 0 and 1 swapped", sd, dict(swap_v_heads=(0, 1))))
        muts.append(("scale 128^-0.5", sd, dict(scale=128 ** -0.5)))
        if K > 1:
            muts.append(("key mask ignored", sd, dict(ignore_mask=True)))
            muts.append(("key mask shifted by one key", sd, dict(mask_shift=1)))
            muts.append(("all-invalid flip omitted", sd, dict(no_flip=True)))
        if K <= 8:
            muts.append(("packed neighbour's keys visible", sd, dict(leak=True)))
    return muts


@pytest.mark.parametrize("version", ["normal", "no_transformer"])
@pytest.mark.parametrize("K", [5, 16, 33])
def test_topo_mutations_move_the_outputs(K, version):
    """Each mistake, made in the reference alone, moves the defined outputs of the trunk tests' inputs by at least 10x the bound the
    GPU tests hold the kernel to: a kernel that made it would fail them.  One K per token mapping of the kernel (packed slots, one
    wave, wave groups); not K = 1, where the softmax is the constant 1 and q, the scale and the mask cannot show."""
    nseq = 28
    sd = _topo_sd(version)
    rows, valid = heads_ref.topo_trunk_inputs(nseq, K, seed=K)
    d = heads_ref.topo_defined(valid).reshape(-1)
    base_l, base_s = heads_ref.topo_trunk_ref(rows, valid, sd, K)
    bound_l, bound_s = heads_ref.topo_op_bounds(T, version)
    weak = []
    for name, msd, mutate in _mutations(sd, K):
        lg, sc = heads_ref.topo_trunk_ref(rows, valid, msd, K, mutate=mutate)
        assert torch.isfinite(lg).all()
        dl, ds = (lg - base_l)[d].abs().max().item(), (sc - base_s)[d].abs().max().item()
        print(f"[topo mutation K={K} {version}] {name}: logits move {dl:.3f} ({dl / bound_l:.0f}x), scores {ds:.4f} ({ds / bound_s:.0f}x)")
        if dl < 10 * bound_l or ds < 10 * bound_s:
            weak.append((name, dl, ds))
    assert not weak, weak


@pytest.mark.parametrize("K", [5, 16, 33])
def test_topo_k_bias_is_invisible(K):
    """The k part of in_proj_bias adds q . bk to every logit of a softmax row, which cancels: no test can see it, so the mutation list
    leaves it out."""
    sd = _topo_sd("normal")
    rows, valid = heads_ref.topo_trunk_inputs(14, K, seed=K)
    base_l, _ = heads_ref.topo_trunk_ref(rows, valid, sd, K)
    D = heads_ref.TOPO_D
    for L in range(3):
        lg, _ = heads_ref.topo_trunk_ref(rows, valid, _rolled(sd, f"{_TL}{L}.self_attn.in_proj_bias", 4, D, 2 * D), K)
        assert (lg - base_l).abs().max().item() < 1e-9


def test_toponet_ref_matches_oracle():
    """The chain (sampler, feature_proj, gather, trunk) against the oracle's TopoNet in fp32, up to the chain's own fp16 roundings."""
    model = _topo_net(SEED, "normal")
    g = torch.Generator().manual_seed(8)
    B, N, Ns, K = 2, 30, 9, 5
    emb = torch.randn(B, 256, 16, 16, generator=g)
    points = torch.rand(B, N, 2, generator=g) * 296 - 20
    pairs = torch.randint(0, N, (B, Ns, K, 2), generator=g)
    valid = torch.rand(B, Ns, K, generator=g) < 0.6
    with torch.no_grad():
        want_l, _ = model.topo_net(points, model.bilinear_sampler(emb, points), pairs, valid)
    logits, _ = heads_ref.toponet_ref(emb.permute(0, 2, 3, 1), points, pairs, valid, model.state_dict(), 256)
    d = heads_ref.topo_defined(valid).reshape(-1)
    # fp16 roundings of three buffers (relative 2^-11 each) through three layers: a few 1e-3 of logits of O(3)
    assert (logits - want_l.reshape(-1).double())[d].abs().max().item() < 3e-2


@pytest.mark.parametrize("i64", [False, True])
@pytest.mark.parametrize("K", [5, 16, 33])
def test_toponet_chain_sees_feature_proj_bias(K, i64):
    """The chain test's inputs (tests/test_gpu_topo_trunk.py): feature_proj's bias rotated by 4 moves the outputs by >= 10x its bounds."""
    sd = _topo_net(SEED, "normal").state_dict()
    emb, points, pairs, valid = heads_ref.toponet_chain_inputs(K, i64)
    d = heads_ref.topo_defined(valid).reshape(-1)
    base_l, base_s = heads_ref.toponet_ref(emb, points, pairs, valid, sd, 256)
    lg, sc = heads_ref.toponet_ref(emb, points, pairs, valid, _rolled(sd, "topo_net.feature_proj.bias", 4), 256)
    assert (lg - base_l)[d].abs().max().item() >= 10 * T.TOPO_CHAIN_LOGIT
    assert (sc - base_s)[d].abs().max().item() >= 10 * T.TOPO_CHAIN_SCORE
