"""CPU pins of the float64 references in tests/heads_ref.py to oracle/samroad.py's fp32 modules (map_decoder, BilinearSampler,
TopoNet's pair gather) on seeded inputs: a wrong reference fails here, on any host, instead of on the GPU box where
tests/test_gpu_heads.py compares the HIP kernels with it."""
import warnings

import torch

import heads_ref
from oracle.samroad import AttrDict, SAMRoadOracle

PIN = 1e-5


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
