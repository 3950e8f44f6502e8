"""TopoNet at every MAX_NEIGHBOR_QUERIES (K) from 1 to 64 (ABI 10) against the CPU oracle: the fused trunk's three mappings (K <= 15
packed into power-of-two slots of a 16-token tile, K = 16, K >= 17 over a group of waves; csrc/topo_fused.hip), the ragged pass-2
entry point and the scene pipeline.  Run on an MI355X: pytest -m gpu."""
import warnings

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle.samroad import AttrDict, SAMRoadOracle
from oracle.synth import synth_queries, synth_scene, synth_state_dict, synth_tiles

import tolerances as T

KS = [1, 2, 3, 5, 8, 12, 15, 17, 24, 31, 32, 48, 64]
CFG = dict(SAM_VERSION="vit_b", PATCH_SIZE=512, TOPONET_VERSION="normal", SAM_CKPT_PATH="", ENCODER_DEPTH=1, ENCODER_GLOBAL_ATTN_INDEXES=[])
# appending invalid slots to a sequence could change only the f32 reduction order of its softmax; measured 0.0 (bit-identical) for
# all five (K, K') pairs on an MI355X: the added keys contribute exact zeros in aligned blocks of the sum trees (csrc/topo_fused.hip)
PAD_INVARIANCE = 1e-6


def _pair(version, seed=1234):
    from sam_road_amd import Config, SAMRoad
    warnings.simplefilter("ignore")
    cfg = dict(CFG, TOPONET_VERSION=version)
    oracle = SAMRoadOracle(AttrDict(cfg)).eval()
    sd = synth_state_dict(oracle, seed)
    oracle.load_state_dict(sd, strict=True)
    net = SAMRoad(Config(cfg))
    net.load_state_dict(sd, strict=True)
    return oracle, net.eval().to("cuda")


_PAIRS = {}


def pair(version):
    if version not in _PAIRS:
        _PAIRS[version] = _pair(version)
    return _PAIRS[version]


def _emb(B, seed):
    return torch.randn(B, 256, 32, 32, generator=torch.Generator().manual_seed(seed))


def _oracle_scores(oracle, emb, points, pairs, valid):
    with torch.no_grad():
        feats = oracle.bilinear_sampler(emb, points)
        return oracle.topo_net(points, feats, pairs, valid)


def _defined(valid):
    """Slots whose score is part of the contract: the valid ones, and every slot of a sequence without any (model.py:129-130)."""
    v = valid.bool().clone()
    v[~v.any(-1)] = True
    return v


def _check(tag, ts, ts_r, valid):
    v = _defined(valid)
    assert torch.isfinite(ts[..., 0][v]).all()
    T.check(tag + "_score", (ts[..., 0][v] - ts_r[..., 0][v]).abs().max().item(), T.TOPO_SCORE)
    agree = ((ts[..., 0][v] > 0.5) == (ts_r[..., 0][v] > 0.5)).float().mean().item()
    T.check(tag + "_decisions", agree, T.TOPO_DECISIONS, at_least=True)


@pytest.mark.parametrize("version", ["normal", "no_offset", "no_transformer"])
@pytest.mark.parametrize("K", KS)
def test_infer_toponet_vs_oracle(K, version):
    """synth_queries (the reference's KDTree kNN(K+1) queries) through infer_toponet at every regime boundary, i64 and i32 pairs."""
    oracle, net = pair(version)
    B = 3
    points, pairs, valid = synth_queries(B, 600, 512, k=K, seed=100 + K)
    emb = _emb(B, K)
    _, ts_r = _oracle_scores(oracle, emb, points, pairs, valid)
    ts = net.infer_toponet(emb.cuda(), points.cuda(), pairs.cuda(), valid.cuda()).cpu()
    assert tuple(ts.shape) == tuple(pairs.shape[:3]) + (1,)
    _check(f"topo_k{K}_{version}", ts, ts_r, valid)
    ts32 = net.infer_toponet(emb.cuda(), points.cuda(), pairs.to(torch.int32).cuda(), valid.cuda()).cpu()
    v = _defined(valid)
    assert torch.equal(ts32[..., 0][v], ts[..., 0][v])


@pytest.mark.parametrize("K", [1, 3, 8, 24, 64])
def test_forward_logits_vs_oracle(K):
    """SAMRoad.forward (encoder + map decoder + TopoNet with logits) with pairs [B,N,K,2]."""
    oracle, net = pair("normal")
    rgb = synth_tiles(1, 512, seed=2)
    points, pairs, valid = synth_queries(1, 300, 512, k=K, seed=7)
    _, _, tl_r, ts_r = oracle(rgb, points, pairs, valid)
    _, _, tl, ts = (t.cpu() for t in net(rgb.cuda(), points.cuda(), pairs.cuda(), valid.cuda()))
    v = _defined(valid)
    T.check(f"forward_k{K}_topo_logit", (tl[..., 0][v] - tl_r[..., 0][v]).abs().max().item(), T.TOPO_LOGIT)
    _check(f"forward_k{K}", ts, ts_r, valid)


def _random_queries(B, Ns, K, seed, n_points=50):
    g = torch.Generator().manual_seed(seed)
    points = torch.randint(-8, 520, (B, n_points, 2), generator=g)
    src = torch.randint(0, n_points, (B, Ns, 1), generator=g).expand(B, Ns, K)
    pairs = torch.stack([src, torch.randint(0, n_points, (B, Ns, K), generator=g)], -1)
    valid = torch.rand(B, Ns, K, generator=g) < 0.5
    return points, pairs, valid


@pytest.mark.parametrize("B,Ns", [(3, 37), (2, 29), (1, 1)])
@pytest.mark.parametrize("K", [2, 5, 7, 13, 16, 20, 33, 50, 64])
def test_adversarial_valid_patterns(K, B, Ns):
    """All-invalid sequences (the flip), exactly one valid slot (first / last / middle), valid slots that are no prefix, K not a
    multiple of 4 (byte-addressed valid), and sequence counts that leave partial packs and partial wave groups."""
    oracle, net = pair("normal")
    points, pairs, valid = synth_queries(B, Ns, 512, k=K, seed=K * 100 + Ns)
    assert tuple(valid.shape) == (B, Ns, K)
    flat = valid.view(-1, K)
    for i, row in enumerate(range(0, flat.shape[0], 3)):
        kind = i % 4
        flat[row] = False
        if kind == 1:
            flat[row, K - 1] = True
        elif kind == 2:
            flat[row, K // 2] = True
        elif kind == 3:
            flat[row, 0] = True
    if flat.shape[0] > 1:
        flat[1, ::2] = True                                    # not a prefix
        flat[1, 1::2] = False
    emb = _emb(B, 5)
    _, ts_r = _oracle_scores(oracle, emb, points, pairs, valid)
    ts = net.infer_toponet(emb.cuda(), points.cuda(), pairs.cuda(), valid.cuda()).cpu()
    v = _defined(valid)
    assert torch.isfinite(ts[..., 0][v]).all()
    T.check(f"topo_adversarial_k{K}_{B}x{Ns}_score", (ts[..., 0][v] - ts_r[..., 0][v]).abs().max().item(), T.TOPO_SCORE)


@pytest.mark.parametrize("version", ["normal", "no_transformer"])
@pytest.mark.parametrize("K", [1, 2, 3, 5, 8, 12, 16, 20, 33, 64])
def test_sequences_are_isolated(K, version):
    """Permuting the sequences changes their packed-tile mates, slots, wave groups and workgroups, and must leave every sequence's
    scores bit-identical: a leaky block-diagonal mask or a wrong exchange slot would show."""
    _, net = pair(version)
    points, pairs, valid = _random_queries(1, 203, K, seed=K)
    valid.view(-1, K)[::7] = False
    emb = _emb(1, 9).cuda()
    perm = torch.randperm(203, generator=torch.Generator().manual_seed(K))
    a = net.infer_toponet(emb, points.cuda(), pairs.cuda(), valid.cuda()).cpu()
    b = net.infer_toponet(emb, points.cuda(), pairs[:, perm].cuda(), valid[:, perm].cuda()).cpu()
    v = _defined(valid)
    assert torch.equal(a[:, perm][..., 0][v[:, perm]], b[..., 0][v[:, perm]])


@pytest.mark.parametrize("K,K2", [(5, 16), (5, 32), (5, 64), (20, 32), (20, 64)])
def test_invalid_slot_padding_invariance(K, K2):
    """Appending invalid slots to every sequence leaves the scores of its valid slots unchanged (exactly, up to the f32 order)."""
    _, net = pair("normal")
    points, pairs, valid = synth_queries(2, 200, 512, k=K, seed=3)
    emb = _emb(2, 11).cuda()
    B, Ns = pairs.shape[:2]
    pad_pairs = torch.cat([pairs, pairs[:, :, :1].expand(B, Ns, K2 - K, 2)], 2)
    pad_valid = torch.cat([valid, torch.zeros(B, Ns, K2 - K, dtype=valid.dtype)], 2)
    keep = valid.bool().any(-1, keepdim=True) & valid.bool()   # an all-invalid sequence attends to its pad slots too once padded
    a = net.infer_toponet(emb, points.cuda(), pairs.cuda(), valid.cuda()).cpu()[..., 0]
    b = net.infer_toponet(emb, points.cuda(), pad_pairs.cuda(), pad_valid.cuda()).cpu()[..., :K, 0]
    assert keep.sum() > 1000
    T.check(f"topo_pad_invariance_k{K}_to_{K2}", (a[keep] - b[keep]).abs().max().item(), PAD_INVARIANCE)


# ---- srh_toponet_ragged ---------------------------------------------------------------------------------------------------------
def _ragged_scene(K, seed, n_tiles, lo, hi):
    g = torch.Generator().manual_seed(seed)
    counts = torch.randint(lo, hi, (n_tiles,), generator=g)
    off = np.concatenate([[0], np.cumsum(counts.numpy())]).astype(np.int64)
    R = int(off[-1])
    tile = torch.repeat_interleave(torch.arange(n_tiles, dtype=torch.int32), counts)
    points = (torch.rand(R, 2, generator=g) * 532 - 10).round()
    first = torch.from_numpy(off[:-1])[tile.long()]
    local = (torch.rand(R, K, generator=g) * counts[tile.long()][:, None]).long()
    pairs = torch.stack([torch.arange(R)[:, None].expand(R, K), first[:, None] + local], -1).to(torch.int32).contiguous()
    valid = (torch.rand(R, K, generator=g) < 0.6).to(torch.uint8)
    valid[5] = 0
    emb = torch.randn(n_tiles, 256, 32, 32, generator=g)
    return emb, points, tile, pairs, valid, off, counts


@pytest.mark.parametrize("K", [8, 24, 64])
def test_ragged_equals_padded(K):
    """infer_toponet_ragged over the flat rows of 7 tiles == infer_toponet over the same tiles padded to the longest, row by row."""
    _, net = pair("normal")
    emb, points, tile, pairs, valid, off, counts = _ragged_scene(K, K, 7, 20, 90)
    flat = net.infer_toponet_ragged(emb.cuda(), points.cuda(), tile.cuda(), pairs.cuda(), valid.cuda()).cpu()
    net.check_finite()
    N = int(counts.max())
    B = len(counts)
    pp = torch.zeros(B, N, 2)
    pq = torch.zeros(B, N, K, 2, dtype=torch.int64)
    pv = torch.zeros(B, N, K, dtype=torch.uint8)
    for t in range(B):
        a, b = int(off[t]), int(off[t + 1])
        pp[t, :b - a] = points[a:b]
        pq[t, :b - a] = pairs[a:b].long() - a
        pv[t, :b - a] = valid[a:b]
    padded = net.infer_toponet(emb.cuda(), pp.cuda(), pq.cuda(), pv.cuda()).cpu()[..., 0]
    for t in range(B):
        a, b = int(off[t]), int(off[t + 1])
        v = _defined(valid[a:b])
        assert torch.equal(flat[a:b][v], padded[t, :b - a][v])


@pytest.mark.parametrize("K", [8, 24, 64])
def test_ragged_chunks_same_bits_at_k(K):
    """Chunked by tile_offsets (bounded by pairs: 16 384 x 16 per chunk) == one launch, bit for bit; at K = 64 the scene crosses
    several chunk boundaries.  A pair outside its tile still sets the ABI-9 error."""
    from sam_road_amd import _lib
    _, net = pair("normal")
    emb, points, tile, pairs, valid, off, _ = _ragged_scene(K, 3, 40, 250, 350)
    R = int(off[-1])
    chunk_rows = 16384 * 16 // K
    starts, ta = [], 0
    while ta < 40:
        tb = ta + 1
        while tb < 40 and off[tb + 1] - off[ta] <= chunk_rows:
            tb += 1
        starts.append(tb)
        ta = tb
    if K == 64:
        assert len(starts) >= 3, starts
    args = [t.cuda() for t in (emb, points, tile, pairs, valid)]
    one = net.infer_toponet_ragged(*args).cpu().numpy()
    chunked = net.infer_toponet_ragged(*args, tile_offsets=off).cpu().numpy()
    net.check_finite()
    np.testing.assert_array_equal(chunked, one)
    assert np.isfinite(one[valid.numpy().astype(bool)]).all() and R * K <= 65536 * 16
    bad = pairs.clone()
    bad[int(off[starts[0] if len(starts) > 1 else 20]), 3 % K, 1] = int(off[starts[0] if len(starts) > 1 else 20]) - 1   # previous tile
    with pytest.raises(_lib.SrhError, match="outside its own tile"):
        net.infer_toponet_ragged(args[0], args[1], args[2], bad.cuda(), args[4], tile_offsets=off)
        net.check_finite()
    net.check_finite()


SRH_ERR_UNSUPPORTED = -2          # include/samroad_hip.h


@pytest.mark.parametrize("K", [0, 65])
def test_unsupported_k_from_c_abi(K):
    import ctypes as C
    from sam_road_amd import _lib
    _, net = pair("normal")
    K_ok = 4
    emb = _emb(1, 1).cuda()
    points, pairs, valid = _random_queries(1, 3, K_ok, seed=1)
    net.infer_toponet(emb, points.cuda(), pairs.cuda(), valid.cuda())       # the context and weights exist
    ctx, wh = net._weights(emb.device)
    e = emb.permute(0, 2, 3, 1).contiguous()
    pts, prs, vld = points.cuda().contiguous(), pairs.cuda().contiguous(), valid.to(torch.uint8).cuda().contiguous()
    out = torch.empty(64 * 3 + 1, device="cuda")
    rc = ctx.lib.srh_toponet(ctx.handle, wh, e.data_ptr(), pts.data_ptr(), _lib.SRH_I64, prs.data_ptr(), _lib.SRH_I64, vld.data_ptr(),
                             1, 50, 3, K, None, out.data_ptr(), None)
    assert rc == SRH_ERR_UNSUPPORTED
    pt = torch.zeros(3, dtype=torch.int32, device="cuda")
    pf = torch.zeros(3, 2, device="cuda")
    rc = ctx.lib.srh_toponet_ragged(ctx.handle, wh, e.data_ptr(), 1, pf.data_ptr(), pt.data_ptr(), prs.to(torch.int32).data_ptr(),
                                    vld.data_ptr(), 3, K, None, out.data_ptr(), None)
    assert rc == SRH_ERR_UNSUPPORTED
    torch.cuda.synchronize()


# ---- the scene pipeline ------------------------------------------------------------------------------------------------------------
from scene_kit import CFG as SCENE_CFG
from scene_kit import check_scene_parity, oracle_scene, thresholds
from scene_kit import pair as scene_pair  # noqa: F401  (a fixture)


@pytest.mark.parametrize("K", [8, 32])
def test_infer_one_img_end_to_end_at_k(scene_pair, K):
    """infer_one_img at MAX_NEIGHBOR_QUERIES = K on the 448-px synthetic scene, stage-wise against oracle.scene (as
    test_gpu_scene.py::test_infer_one_img_end_to_end does at K = 16)."""
    from sam_road_amd import Config
    from sam_road_amd.inferencer import infer_one_img
    oracle, net = scene_pair
    img = synth_scene(448, seed=6)
    cfg = dict(SCENE_CFG, MAX_NEIGHBOR_QUERIES=K)
    ref = oracle_scene(oracle, img, cfg["INFER_PATCHES_PER_EDGE"], cfg=cfg)
    cfg.update(thresholds(ref[2], ref[3]))
    check_scene_parity(None, infer_one_img(net, img, Config(cfg)), ref, cfg, oracle)


def test_infer_imgs_pipeline_equals_serial_at_k32(scene_pair):
    from sam_road_amd import Config
    from sam_road_amd.inferencer import infer_imgs, infer_one_img
    _, net = scene_pair
    imgs = [synth_scene(size, seed=s) for size, s in ((448, 6), (384, 7), (448, 8))]
    _, _, kp0, road0 = infer_one_img(net, imgs[0], Config(dict(SCENE_CFG, MAX_NEIGHBOR_QUERIES=32)))
    cfg = Config(dict(SCENE_CFG, MAX_NEIGHBOR_QUERIES=32, **thresholds(kp0, road0)))
    want = [infer_one_img(net, im, cfg) for im in imgs]
    assert max(w[1].shape[0] for w in want) > 20
    got = list(infer_imgs(net, iter(imgs), cfg, tile_sharded=False))
    assert len(got) == len(want)
    for w, g in zip(want, got):
        for a, b in zip(w, g):
            np.testing.assert_array_equal(np.asarray(a), np.asarray(b))
