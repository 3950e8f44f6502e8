"""Op-level parity of the heads after the encoder (through the C ABI's test-only exports) against the float64 references of
tests/heads_ref.py: the fused map_decoder (decoder.hip decode_fused_kernel), the bilinear sampler and the pair gather
(topo.hip), and srh_toponet_ragged's chunking at tile boundaries.  Run on an MI355X: pytest -m gpu."""
import ctypes as C
import warnings

import numpy as np
import pytest
import torch

import heads_ref
import tolerances as T

pytestmark = pytest.mark.gpu

SRH_F32, SRH_I32, SRH_I64 = 0, 3, 4


@pytest.fixture(scope="module")
def ctx():
    from sam_road_amd import _lib
    assert torch.cuda.is_available(), "gpu-marked test needs a GPU"
    return _lib.Context.get(0)


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _net(patch, seed, **kw):
    from oracle.synth import synth_state_dict
    from sam_road_amd import Config, SAMRoad
    warnings.simplefilter("ignore")
    net = SAMRoad(Config(dict(SAM_VERSION="vit_b", PATCH_SIZE=patch, TOPONET_VERSION="normal", SAM_CKPT_PATH="", ENCODER_DEPTH=1,
                              ENCODER_GLOBAL_ATTN_INDEXES=[]) | kw))
    net.load_state_dict(synth_state_dict(net, seed), strict=True)
    return net.eval()


# ---- map_decoder ------------------------------------------------------------------------------------------------------------------
def _decoder_net(S, seed):
    """A model whose map_decoder reaches the tails: pre-activations of about +-8 at every GELU (gelu_fast's whole range), logits of
    about +-15 (a saturated sigmoid), LayerNorm2d gamma in +-[1, 2] and beta in [-1.5, 1.5], layer-7 bias (0.7, -1.3) — every value
    fp16-representable, so the kernel's fp16 weight copies are exact."""
    net = _net(16 * S, seed)
    g = torch.Generator().manual_seed(seed)
    md = net.map_decoder
    with torch.no_grad():
        for (idx, cin, cout), std in zip(heads_ref._MD_LAYERS, heads_ref.DECODER_STDS):
            md[idx].weight.copy_((torch.randn(cin, cout, 2, 2, generator=g) * std).half().float())
            md[idx].bias.copy_(torch.randn(cout, generator=g).half().float())
        md[1].weight.copy_(((1.0 + torch.rand(128, generator=g)) * torch.sign(torch.randn(128, generator=g))).half().float())
        md[1].bias.copy_((3 * torch.rand(128, generator=g) - 1.5).half().float())
        md[7].bias.copy_(torch.tensor([0.7, -1.3]))
    return net.to("cuda")


def _subpixel_summary(err):
    """err [B, P, P, 2] -> the worst error per class and per quadrant of every level of the decoder's quad tree: output pixel
    (y, x) of token (py, px) is y = 16 py + 8 s1y + 4 s2y + 2 s3y + ky (the same for x), so bit 3 - l of y and x names the
    quadrant at level l (l = 0: sub1 of layer 0 ... l = 3: the last layer's 2 x 2 pixels)."""
    P = err.shape[1]
    yy = torch.arange(P).view(P, 1)
    xx = torch.arange(P).view(1, P)
    out = {f"class{c}": err[..., c].max().item() for c in range(2)}
    e = err.amax(dim=(0, 3))
    for lvl, name in enumerate(("sub1", "sub2", "sub3", "pixel")):
        bit = 3 - lvl
        q = ((yy >> bit) & 1) * 2 + ((xx >> bit) & 1)
        out[name] = [round(e[q == k].max().item(), 6) for k in range(4)]
    return out


@pytest.mark.parametrize("S,B", [(16, 1),      # 16 jobs: one per wave, fewer jobs than waves
                                 (32, 20),     # 1280 jobs per sub-pixel on 64 x 16 waves after the workgroup cap: uneven
                                 (32, 64),     # 4 jobs per wave
                                 (64, 3)])     # 1024-px tiles
def test_map_decoder_op(ctx, S, B):
    net = _decoder_net(S, seed=100 + S + B)
    _, wh = net._weights(torch.device("cuda", 0))
    P = 16 * S
    g = torch.Generator().manual_seed(S * 1000 + B)
    emb = torch.randn(B * S * S, 256, generator=g).half()
    demb = emb.cuda()

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
    assert ref_l.abs().max() > 10 and (ref_l.abs() < 1).any(), "the weights should reach a saturated sigmoid and its steep part"
    el = (lg.double() - ref_l).abs()
    es = (sc.double() - ref_s).abs()
    where = {"logits": _subpixel_summary(el), "scores": _subpixel_summary(es)}
    print(f"[map_decoder S={S} B={B}] {where}")
    T.check(f"map_decoder_op_S{S}_B{B}_logit", el.max().item(), T.DEC_OP_LOGIT)
    T.check(f"map_decoder_op_S{S}_B{B}_score", es.max().item(), T.DEC_OP_SCORE)
    ctx.check(ctx.lib.srh_ctx_check(ctx.handle, None, 1), "srh_ctx_check")      # the LayerNorm2d saw no Inf / NaN


# ---- bilinear sampler -----------------------------------------------------------------------------------------------------------------
def _sample_points(patch, i64, n_rand, g):
    """Every pair of the edge coordinates (the tile's border 0 / patch, the first and last texel centres at patch / (2 w) from it,
    1 px and 100 px outside, the taps' half-weight points) and random points around the tile, fractional for f32."""
    c = 16                                                     # image pixels per embedding texel (patch = 16 w)
    if i64:
        edge = [0, 1, c // 2 - 1, c // 2, c // 2 + 1, patch - c // 2, patch - 1, patch, -1, -c // 2, -c // 2 - 1, -100,
                patch + 1, patch + c // 2, patch + c // 2 + 1, patch + 100]
        rnd = torch.randint(-24, patch + 24, (n_rand, 2), generator=g)
        dt = torch.int64
    else:
        edge = [0.0, 0.5, c / 2 - 0.5, c / 2, c / 2 + 0.25, patch - c / 2 - 0.5, patch - c / 2, patch - 1, patch - 0.5, patch,
                -1.0, -c / 2, -c / 2 - 1, -100.0, patch + 1, patch + c / 2, patch + c / 2 + 1, patch + 100]
        rnd = torch.rand(n_rand, 2, generator=g) * (patch + 48) - 24
        dt = torch.float32
    e = torch.tensor(edge, dtype=dt)
    return torch.cat([torch.cartesian_prod(e, e), rnd.to(dt)])


def _f16_ulp(x):
    a = x.abs().clamp(min=2.0 ** -14)
    return torch.exp2(torch.floor(torch.log2(a)) - 10)


@pytest.mark.parametrize("C_", [128, 256, 384])
@pytest.mark.parametrize("i64", [False, True])
@pytest.mark.parametrize("S,tiles", [(32, False), (16, True)])
def test_sample_op(ctx, C_, i64, S, tiles):
    patch = 16 * S
    n_tiles = 3
    g = torch.Generator().manual_seed(C_ + S + (7 if i64 else 0) + (11 if tiles else 0))
    emb = torch.randn(n_tiles, S, S, C_, generator=g) * 3.0
    pts1 = _sample_points(patch, i64, 300, g)
    N = pts1.shape[0]
    if tiles:
        # ragged rows: every point names its tile; indices outside [0, n_tiles) clamp (-3 -> 0, 9 -> 2)
        B = 4
        pt = torch.tensor([2, -3, 1, 9], dtype=torch.int32).repeat_interleave(N)
    else:
        B, pt = n_tiles, None
    pts = pts1.unsqueeze(0).expand(B, N, 2).contiguous()
    ref = heads_ref.sample_ref(emb, pts, patch, point_tile=pt)
    o32 = torch.full((B * N, C_), float("nan"), device="cuda")
    o16 = torch.full((B * N, C_), float("nan"), device="cuda", dtype=torch.half)
    d_emb, d_pts, d_pt = emb.cuda(), pts.cuda(), (pt.cuda() if pt is not None else None)     # held: the library reads them later
    ctx.check(ctx.lib.srh_op_sample(ctx.handle, _p(d_emb), n_tiles, S, S, C_, _p(d_pts), SRH_I64 if i64 else SRH_F32, _p(d_pt),
                                    B, N, float(patch), _p(o32), _p(o16), None), "srh_op_sample")
    torch.cuda.synchronize()
    o32, o16 = o32.cpu(), o16.cpu()
    assert (ref == 0).all(dim=1).any() and (ref.abs() > 1).any(), "the points should cover outside (zero) and inside taps"
    assert torch.isfinite(o32).all() and torch.isfinite(o16).all(), "unwritten outputs"
    zero_rows = (ref == 0).all(dim=1)
    assert (o32[zero_rows] == 0).all(), "a point with every tap outside the map must sample exactly 0"
    T.check(f"sample_op_S{S}_C{C_}_{'i64' if i64 else 'f32'}{'_tiles' if tiles else ''}",
            (o32.double() - ref).abs().max().item() / emb.abs().max().item(), T.SAMPLE_OP_F32)
    # the fp16 copy is the f32 result rounded once
    assert ((o16.float() - o32).abs() <= _f16_ulp(o32)).all(), "fp16 output is not the f32 output rounded to fp16"


# ---- pair gather --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pairs_i64", [False, True])
@pytest.mark.parametrize("points_i64", [False, True])
@pytest.mark.parametrize("zero_offset", [False, True])
@pytest.mark.parametrize("ld", [264, 320])
@pytest.mark.parametrize("index_base", [0, 1000])
def test_pair_gather_op(ctx, pairs_i64, points_i64, zero_offset, ld, index_base):
    B, N, Ns, K = 3, 37, 11, 16
    g = torch.Generator().manual_seed(ld + index_base + 2 * pairs_i64 + points_i64)
    pf = torch.randn(B, N, 128, generator=g).half()
    if points_i64:
        points = torch.randint(-300, 300, (B, N, 2), generator=g)
    else:
        points = torch.randint(-1200, 1200, (B, N, 2), generator=g).float() / 4     # the f32 differences are exact
    if index_base:
        pairs = torch.randint(0, N, (B, Ns, K, 2), generator=g) + index_base         # a chunk of a longer row list: no wrap
    else:
        pairs = torch.randint(-N, N, (B, Ns, K, 2), generator=g)                     # negative: Python's wrap
        assert (pairs < 0).any()
    pairs = pairs.to(torch.int64 if pairs_i64 else torch.int32)
    rows = B * Ns * K
    ref = heads_ref.pair_gather_ref(pf, points, pairs, ld, zero_offset=zero_offset, index_base=index_base).half()
    out = torch.full((rows + 1, ld), float("nan"), device="cuda", dtype=torch.half)  # + one guard row
    d_pf, d_points, d_pairs = pf.cuda(), points.cuda(), pairs.cuda()                     # held: the library reads them later
    ctx.check(ctx.lib.srh_op_pair_gather(ctx.handle, _p(d_pf), _p(d_points), SRH_I64 if points_i64 else SRH_F32,
                                         _p(d_pairs), SRH_I64 if pairs_i64 else SRH_I32, B, N, Ns, K, int(zero_offset),
                                         index_base, _p(out), ld, None), "srh_op_pair_gather")
    torch.cuda.synchronize()
    out = out.cpu()
    assert torch.isnan(out[rows]).all(), "the gather wrote past its last row"
    got = out[:rows]
    bad = (got.view(torch.int16) != ref.view(torch.int16))
    assert not bad.any(), f"{int(bad.sum())} halves differ; first at (row, col) {bad.nonzero()[0].tolist()}"


# ---- srh_toponet_ragged: chunks of whole tiles --------------------------------------------------------------------------------------
RAGGED_CHUNK_ROWS = 16384       # include/samroad_hip.h srh_toponet_ragged


def _ragged_scene(seed):
    g = torch.Generator().manual_seed(seed)
    n_tiles, K = 40, 16
    counts = torch.randint(300, 700, (n_tiles,), generator=g)
    off = np.concatenate([[0], np.cumsum(counts.numpy())]).astype(np.int64)
    R = int(off[-1])
    assert R > RAGGED_CHUNK_ROWS + 1000
    tile = torch.repeat_interleave(torch.arange(n_tiles, dtype=torch.int32), counts)
    points = torch.rand(R, 2, generator=g) * 276 - 10
    lo = torch.from_numpy(off[:-1])[tile.long()]
    tgt = lo[:, None] + (torch.rand(R, K, generator=g) * counts[tile.long()][:, None]).long()
    pairs = torch.stack([torch.arange(R)[:, None].expand(R, K), tgt], -1).to(torch.int32).contiguous()
    valid = (torch.rand(R, K, generator=g) < 0.7).to(torch.uint8)
    valid[5] = 0                                               # an all-invalid row (flipped to all-valid, model.py:129-130)
    emb = torch.randn(n_tiles, 256, 16, 16, generator=g)
    return emb, points, tile, pairs, valid, off


def _chunk_starts(off):
    """The first tile of every chunk after the first, as srh_toponet_ragged cuts them."""
    starts, ta, n = [], 0, len(off) - 1
    while ta < n:
        tb = ta + 1
        while tb < n and off[tb + 1] - off[ta] <= RAGGED_CHUNK_ROWS:
            tb += 1
        if tb < n:
            starts.append(tb)
        ta = tb
    return starts


@pytest.fixture(scope="module")
def ragged():
    net = _net(256, 77).to("cuda")
    emb, points, tile, pairs, valid, off = _ragged_scene(9)
    assert _chunk_starts(off), "the scene must need more than one chunk"
    return net, [t.cuda() for t in (emb, points, tile, pairs, valid)], off


def test_ragged_chunks_same_bits(ragged):
    net, (emb, points, tile, pairs, valid), off = ragged
    one = net.infer_toponet_ragged(emb, points, tile, pairs, valid).cpu().numpy()
    chunked = net.infer_toponet_ragged(emb, points, tile, pairs, valid, tile_offsets=off).cpu().numpy()
    net.check_finite()                                         # no pair was flagged
    assert np.isfinite(one[valid.cpu().numpy().astype(bool)]).all()
    np.testing.assert_array_equal(chunked, one)                # every entry, invalid slots included: rows are independent


@pytest.mark.parametrize("where", ["previous_chunk", "next_chunk", "negative"])
def test_ragged_pair_outside_its_tile_fails_loudly(ragged, where):
    """A pair naming a row of another tile across a chunk boundary used to be rebased into the chunk, wrapped (negative) or
    clamped, and silently gathered an unrelated row: chunked and unchunked scores differed.  It is an error now (ABI 9), with and
    without tile_offsets, and the error is reported once."""
    from sam_road_amd import _lib
    net, (emb, points, tile, pairs, valid), off = ragged
    tb = _chunk_starts(off)[0]
    bad = pairs.clone()
    if where == "previous_chunk":
        bad[int(off[tb]), 3, 1] = int(off[tb]) - 1             # first row of a chunk -> last row of the previous tile (and chunk)
    elif where == "next_chunk":
        bad[int(off[tb]) - 1, 5, 1] = int(off[tb])             # last row of a chunk -> first row of the next one
    else:
        bad[int(off[tb]) + 2, 7, 1] = -1                       # no Python wrap in the flat row list
    for kw in (dict(tile_offsets=off), {}):
        with pytest.raises(_lib.SrhError, match="outside its own tile"):
            net.infer_toponet_ragged(emb, points, tile, bad, valid, **kw)
            net.check_finite()
        net.check_finite()                                     # reported once, then clear
