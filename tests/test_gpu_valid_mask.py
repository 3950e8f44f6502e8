"""Scenes with a per-pixel validity mask (nodata) on the HIP path.  Run on an MI355X: pytest -m gpu.

The reference has no nodata handling, so the behaviour is pinned by COMPOSITION of what is already pinned: the masked run must equal,
bit for bit, the existing scene_pass1 / scene_normalise / extract_graph_points / edge_votes / votes_to_edges applied by hand to the
filled scene and the kept tiles that numpy selects (no tolerance).  The parity tests against the CPU oracle build the oracle's result
from oracle.scene's pieces on the same filled scene and kept tiles and reuse the bounds of test_rect_scene_parity_with_oracle.

Masks: (a) all true, (b) a diagonal band of about half the scene, (c) a rectangle of nodata strictly inside the scene, (d) all
false, (e) a single valid pixel, (f) only the left part valid, so that whole tile columns drop out.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from scene_kit import (CFG, FILL, PARITY_SCENES, SCENES, check_scene_parity, kernel_rows, make_mask, np_counts, np_kept, oracle_scene, pair,  # noqa: F401
                       rect_grid, rect_scene)
from scene_kit import net_for as _net_for
from scene_kit import same_bits as _same
from scene_kit import thresholds as _thresholds
from scene_kit import xy_of as _xy

MASKS = ("all", "band", "hole", "none", "pixel", "left")


# ---- 1. the count kernel -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P", [128, 144, 256, 400, 512])
@pytest.mark.parametrize("H,W", [(640, 640), (523, 701), (512, 1031)])
def test_tile_valid_count_equals_numpy(H, W, P):
    """Exact integer counts for every tile of every mask: square, odd-W and P = 128 ... 512 tilings, tile origins not divisible by 16,
    masks whose valid bytes are 1, 255 and arbitrary non-zero values, a bool tensor, tiles touching all four scene borders."""
    net = _net_for(P)
    rng = np.random.default_rng(H * 7 + W + P)
    infos = rect_grid(H, W, 0, P, [3, 4]) + [(0, (x, y), (x + P, y + P)) for x, y in
                                             ((1, 0), (W - P, H - P), (W - P - 1, min(3, H - P)), (7, H - P),
                                              (min(15, W - P), min(15, H - P)), (min(16, W - P), min(17, H - P)))]
    assert all(0 <= x0 and 0 <= y0 and x1 <= W and y1 <= H for _, (x0, y0), (x1, y1) in infos)
    xy = _xy(infos)
    assert any(int(x) % 16 for x in xy[:, 0].tolist())
    masks = {k: make_mask(k, H, W) for k in MASKS}
    masks["noise"] = rng.random((H, W)) < 0.37
    for kind, m in masks.items():
        want = np_counts(m, infos)
        for scale in ("bool", 1, 255, "any"):
            if scale == "bool":
                t = torch.from_numpy(m)
            elif scale == "any":
                t = torch.from_numpy((m * rng.integers(1, 256, size=m.shape)).astype(np.uint8))
            else:
                t = torch.from_numpy(m.astype(np.uint8) * np.uint8(scale))
            got = net.scene_tile_valid(t.cuda(), xy)
            assert got.dtype == torch.int32 and got.shape == (len(infos),)
            np.testing.assert_array_equal(got.cpu().numpy().astype(np.int64), want, err_msg=f"{kind} {scale} {H}x{W} P={P}")
    # a view into a larger allocation: the mask's base address is not 16-byte aligned
    big = torch.zeros(H * W + 64, dtype=torch.uint8, device="cuda")
    for off in (1, 5, 16):
        v = big[off:off + H * W].view(H, W)
        v.copy_(torch.from_numpy(masks["noise"].astype(np.uint8)))
        np.testing.assert_array_equal(net.scene_tile_valid(v, xy).cpu().numpy(), np_counts(masks["noise"], infos))
    assert net.scene_tile_valid(torch.from_numpy(masks["noise"]).cuda(), xy[:0]).shape == (0,)


# ---- 2. the fill kernel --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", [(384, 640), (401, 523), (259, 257)])
def test_scene_fill_invalid_equals_numpy(pair, H, W):
    _, net = pair
    img = rect_scene(H, W, 3)
    rng = np.random.default_rng(W)
    masks = {k: make_mask(k, H, W) for k in MASKS}
    masks["noise"] = rng.random((H, W)) < 0.5
    for kind, m in masks.items():
        for fill in (FILL, (0, 255, 7)):
            want = np.where(m[..., None], img, np.array(fill, np.uint8))
            scene = torch.from_numpy(img.copy()).cuda()
            out = net.scene_fill_invalid(scene, torch.from_numpy(m).cuda(), fill)
            assert out.data_ptr() == scene.data_ptr()                          # in place
            np.testing.assert_array_equal(out.cpu().numpy(), want, err_msg=f"{kind} {fill}")
    # base addresses off the 4-byte grid: the one-pixel-per-thread form
    big_s = torch.zeros(H * W * 3 + 16, dtype=torch.uint8, device="cuda")
    big_v = torch.zeros(H * W + 16, dtype=torch.uint8, device="cuda")
    s, v = big_s[1:1 + H * W * 3].view(H, W, 3), big_v[3:3 + H * W].view(H, W)
    s.copy_(torch.from_numpy(img))
    v.copy_(torch.from_numpy(masks["noise"].astype(np.uint8) * 200))
    net.scene_fill_invalid(s, v, FILL)
    np.testing.assert_array_equal(s.cpu().numpy(), np.where(masks["noise"][..., None], img, np.array(FILL, np.uint8)))
    assert int(big_s[0]) == 0 and int(big_s[1 + H * W * 3:].max()) == 0        # nothing beside the scene was written


# ---- 3.-5. masked run == composition of the existing pieces ---------------------------------------------------------------------
def _composition(net, img, valid, per_edge, cfg_extra=None, frac=0.0):
    """The masked result built by hand from the parts that exist without this feature: (emb, kp_c, road_c, kp_u8, road_u8, infos, xy)."""
    P, bs = CFG["PATCH_SIZE"], CFG["INFER_BATCH_SIZE"]
    H, W = valid.shape
    infos = rect_grid(H, W, CFG["SAMPLE_MARGIN"], P, per_edge)
    kept = np_kept(valid, infos, P, frac)
    infos = [infos[i] for i in kept]
    filled = np.where(valid[..., None], img, np.array(FILL, np.uint8))
    xy = _xy(infos)
    kp_c, road_c, emb = net.scene_pass1(torch.from_numpy(np.ascontiguousarray(filled)).cuda(), xy, bs)
    kp_u8, road_u8 = net.scene_normalise(kp_c, road_c, xy)
    kp_m, road_m = kp_u8.cpu().numpy().copy(), road_u8.cpu().numpy().copy()
    kp_m[~valid] = 0
    road_m[~valid] = 0
    return emb, kp_c, road_c, kp_m, road_m, infos, xy


@pytest.mark.parametrize("kind", ["band", "hole", "left", "pixel"])
@pytest.mark.parametrize("scene", list(SCENES))
def test_masked_run_equals_composition_bit_for_bit(pair, scene, kind):
    from sam_road_amd import Config
    from sam_road_amd.graph_points import extract_graph_points
    from sam_road_amd.inferencer import edge_votes, infer_one_img, scene_tiles, votes_to_edges
    _, net = pair
    H, W, per_edge, seed = SCENES[scene]
    img, valid = rect_scene(H, W, seed), make_mask(kind, H, W)
    frac = 0.25 if kind == "left" else 0.0
    emb, kp_c, road_c, kp_m, road_m, infos, xy = _composition(net, img, valid, per_edge, frac=frac)
    n_all = len(rect_grid(H, W, CFG["SAMPLE_MARGIN"], CFG["PATCH_SIZE"], per_edge))
    print(f"{scene} {kind}: {len(infos)} of {n_all} tiles kept")
    # the band and the hole leave valid pixels in every tile of these small scenes; the pixel and the left part drop tiles
    assert 0 < len(infos) <= n_all and (len(infos) < n_all or kind in ("band", "hole"))
    if kind == "pixel":
        assert len(infos) == sum(x0 <= 21 < x1 and y0 <= H // 2 + 3 < y1 for _, (x0, y0), (x1, y1) in rect_grid(H, W, 16, 256, per_edge))
    if kind == "left":                                   # whole tile columns drop out
        assert max(p[1][0] for p in infos) < max(p[1][0] for p in rect_grid(H, W, 16, 256, per_edge))
    thr = _thresholds(kp_m, road_m) if kind != "pixel" else {}
    cfg = Config(dict(CFG, INFER_PATCHES_PER_EDGE=per_edge, MIN_VALID_FRACTION=frac, **thr))
    assert scene_tiles(img.shape, cfg, valid=valid, net=net) == infos
    # the stages of infer_one_img, seen one by one through the same shim methods it calls
    valid_d = torch.from_numpy(valid).cuda()
    filled_d = net.scene_fill_invalid(torch.from_numpy(img.copy()).cuda(), valid_d, FILL)
    kp2, road2, emb2 = net.scene_pass1(filled_d, xy, CFG["INFER_BATCH_SIZE"])
    _same(emb2.cpu().numpy(), emb.cpu().numpy())
    _same(kp2.cpu().numpy(), kp_c.cpu().numpy())
    _same(road2.cpu().numpy(), road_c.cpu().numpy())
    kpu, roadu = net.scene_normalise(kp2, road2, xy, valid=valid_d)
    _same(kpu.cpu().numpy(), kp_m)
    _same(roadu.cpu().numpy(), road_m)
    # the whole call
    img_before = img.copy()
    nodes, edges, kp_o, road_o = infer_one_img(net, img, cfg, valid=valid)
    np.testing.assert_array_equal(img, img_before)       # the caller's array is never written
    _same(kp_o, kp_m)
    _same(road_o, road_m)
    assert not kp_o[~valid].any() and not road_o[~valid].any()
    pts = extract_graph_points(kp_m, road_m, cfg)
    _same(nodes, pts[:, ::-1])
    if pts.shape[0]:
        assert valid[nodes[:, 0], nodes[:, 1]].all()     # no node on nodata
        votes = edge_votes(net, emb, pts, infos, 0, len(infos), cfg, torch.device("cuda"))
        _same(edges, votes_to_edges(*votes, pts.shape[0], cfg.TOPO_THRESHOLD))
    if kind != "pixel":
        assert pts.shape[0] > 20 and edges.shape[0] > 20
    # what lies under nodata does not matter
    noise = img.copy()
    noise[~valid] = np.random.default_rng(1).integers(0, 256, size=(int((~valid).sum()), 3), dtype=np.uint8)
    for a, b in zip(infer_one_img(net, noise, cfg, valid=valid.astype(np.uint8) * 255), (nodes, edges, kp_o, road_o)):
        _same(a, b)


@pytest.mark.parametrize("scene", list(SCENES))
def test_all_true_mask_equals_no_mask(pair, scene):
    from sam_road_amd import Config
    from sam_road_amd.inferencer import infer_one_img
    _, net = pair
    H, W, per_edge, seed = SCENES[scene]
    img = rect_scene(H, W, seed)
    _, _, kp0, road0 = infer_one_img(net, img, Config(dict(CFG, INFER_PATCHES_PER_EDGE=per_edge)))
    cfg = dict(CFG, INFER_PATCHES_PER_EDGE=per_edge, **_thresholds(kp0, road0))
    want = infer_one_img(net, img, Config(cfg))
    assert want[0].shape[0] > 20 and want[1].shape[0] > 20
    for frac in (0.0, 1.0):
        for m in (np.ones((H, W), bool), np.full((H, W), 255, np.uint8)):
            got = infer_one_img(net, img, Config(dict(cfg, MIN_VALID_FRACTION=frac)), valid=m)
            for a, b in zip(got, want):
                _same(a, b)


def test_all_false_mask_launches_no_encoder(pair):
    from sam_road_amd import Config, _lib
    from sam_road_amd.inferencer import infer_imgs, infer_one_img, scene_tiles
    _, net = pair
    H, W, per_edge, seed = SCENES["401x523"]
    img = rect_scene(H, W, seed)
    cfg = Config(dict(CFG, INFER_PATCHES_PER_EDGE=per_edge))
    infer_one_img(net, img, cfg)                         # weights packed, workspaces allocated
    ctx = _lib.Context.get(torch.cuda.current_device())
    with kernel_rows(ctx) as rows:
        out = infer_one_img(net, img, cfg, valid=np.zeros((H, W), bool))
        # the single valid pixel lies in one or more tiles; with MIN_VALID_FRACTION above 1 / P^2 none is kept
        out2 = infer_one_img(net, img, Config(dict(cfg, MIN_VALID_FRACTION=0.5)), valid=make_mask("pixel", H, W))
        names = sorted(rows())
    print("kernel classes of the two calls:", names)
    assert names == ["tile_valid_count"], names
    for o in (out, out2, list(infer_imgs(net, [img], cfg, valids=[np.zeros((H, W), np.uint8)]))[0]):
        nodes, edges, kp, road = o
        assert nodes.shape == (0, 2) and edges.shape == (0, 2)
        assert kp.shape == road.shape == (H, W) and kp.dtype == road.dtype == np.uint8 and not kp.any() and not road.any()
    assert scene_tiles((H, W), cfg, valid=np.zeros((H, W), bool), net=net) == []
    assert len(scene_tiles((H, W), cfg, valid=make_mask("pixel", H, W), net=net)) >= 1


def test_profile_rows_of_a_masked_call(pair):
    """A masked call launches the three new kernel classes and not the unmasked normalise; an unmasked call launches none of them."""
    from sam_road_amd import Config, _lib
    from sam_road_amd.inferencer import infer_one_img
    _, net = pair
    H, W, per_edge, seed = SCENES["384x640"]
    img = rect_scene(H, W, seed)
    cfg = Config(dict(CFG, INFER_PATCHES_PER_EDGE=per_edge))
    infer_one_img(net, img, cfg)
    ctx = _lib.Context.get(torch.cuda.current_device())
    with kernel_rows(ctx) as rows:
        infer_one_img(net, img, cfg)
        plain = rows()
        infer_one_img(net, img, cfg, valid=make_mask("band", H, W))
        masked = rows()
    new = {"tile_valid_count", "scene_fill_invalid", "scene_norm_valid"}
    assert not (plain & new) and "scene_normalise" in plain
    assert new <= masked and "scene_normalise" not in masked
    assert masked - new <= plain and len(masked - new) > 5             # the encoder and decoder classes of an unmasked call


# ---- 6. the pipelined loop ------------------------------------------------------------------------------------------------------
def test_infer_imgs_mixed_masked_and_unmasked_equal_serial(pair):
    """Masked and unmasked scenes of different shapes through the software-pipelined loop — a masked 640 x 384 scene right after an
    unmasked 384 x 640 one (same bytes in the reused page-locked staging buffers, another row pitch), an all-false scene in the
    middle — equal infer_one_img scene by scene, array for array, on two consecutive runs."""
    from sam_road_amd import Config
    from sam_road_amd.inferencer import infer_imgs, infer_one_img
    _, net = pair
    shapes = [(384, 640), (640, 384), (401, 523), (448, 448), (640, 384), (384, 640), (401, 523)]
    kinds = [None, "band", "hole", "none", None, "left", "band"]
    imgs = [rect_scene(h, w, 50 + i) for i, (h, w) in enumerate(shapes)]
    valids = [None if k is None else make_mask(k, h, w) for k, (h, w) in zip(kinds, shapes)]
    valids[2] = valids[2].astype(np.uint8) * 255
    _, _, kp0, road0 = infer_one_img(net, imgs[0], Config(dict(CFG)))
    cfg = Config(dict(CFG, **_thresholds(kp0, road0)))
    want = [infer_one_img(net, im, cfg, valid=v) for im, v in zip(imgs, valids)]
    print("points / edges per scene:", [(w[0].shape[0], w[1].shape[0]) for w in want])
    assert all(w[0].shape[0] > 20 and w[1].shape[0] > 20 for w, k in zip(want, kinds) if k != "none")
    assert want[3][0].shape[0] == 0
    for v, w in zip(valids, want):
        if v is not None:
            assert not w[2][v == 0].any() and not w[3][v == 0].any()
    for _ in range(2):
        got = list(infer_imgs(net, iter(imgs), cfg, valids=iter(valids)))
        assert len(got) == len(want)
        for w, g in zip(want, got):
            for a, b in zip(w, g):
                _same(a, b)
    # no masks at all: the loop as it was
    for w, g in zip([infer_one_img(net, im, cfg) for im in imgs[:3]], infer_imgs(net, iter(imgs[:3]), cfg)):
        for a, b in zip(w, g):
            _same(a, b)


# ---- 7. the C entries reject what their siblings reject ---------------------------------------------------------------------------
def test_abi_rejects_bad_arguments(pair):
    from sam_road_amd import Config, _lib
    from sam_road_amd.inferencer import infer_one_img
    _, net = pair
    dev = torch.device("cuda")
    ctx, _ = net._weights(dev)
    buf = torch.zeros(1024, dtype=torch.float32, device=dev)
    xy = torch.zeros((1, 2), dtype=torch.int32, device=dev)
    p, s, lib = buf.data_ptr(), net._stream(dev), ctx.lib
    for H, W in ((255, 640), (640, 255), (46341, 46341), (0, 640), (640, -1)):
        assert lib.srh_scene_tile_valid(ctx.handle, p, H, W, xy.data_ptr(), 1, 256, p, s) == -1, (H, W)
    for P in (0, -16, 250, 8):
        assert lib.srh_scene_tile_valid(ctx.handle, p, 640, 640, xy.data_ptr(), 1, P, p, s) == -1, P
    assert lib.srh_scene_tile_valid(ctx.handle, p, 640, 640, xy.data_ptr(), -1, 256, p, s) == -1
    for args in ((None, 640, 640, xy.data_ptr(), 1, 256, p), (p, 640, 640, None, 1, 256, p), (p, 640, 640, xy.data_ptr(), 1, 256, None)):
        assert lib.srh_scene_tile_valid(ctx.handle, *args, s) == -1
    for H, W in ((46341, 46341), (0, 640), (640, -1)):
        assert lib.srh_scene_fill_invalid(ctx.handle, p, p, H, W, 1, 2, 3, s) == -1, (H, W)
        assert lib.srh_scene_normalise_valid_hw(ctx.handle, p, p, H, W, xy.data_ptr(), 1, 256, p, p, p, s) == -1, (H, W)
    for fill in ((256, 0, 0), (0, -1, 0), (0, 0, 1000)):
        assert lib.srh_scene_fill_invalid(ctx.handle, p, p, 8, 8, *fill, s) == -1, fill
    assert lib.srh_scene_fill_invalid(ctx.handle, None, p, 8, 8, 1, 2, 3, s) == -1
    assert lib.srh_scene_fill_invalid(ctx.handle, p, None, 8, 8, 1, 2, 3, s) == -1
    assert lib.srh_scene_normalise_valid_hw(ctx.handle, p, p, 8, 8, xy.data_ptr(), 1, 256, None, p, p, s) == -1
    assert lib.srh_scene_normalise_valid_hw(ctx.handle, p, p, 8, 8, xy.data_ptr(), -1, 256, p, p, p, s) == -1
    with pytest.raises(_lib.SrhError):
        ctx.check(lib.srh_scene_tile_valid(ctx.handle, p, 255, 640, xy.data_ptr(), 1, 256, p, s), "srh_scene_tile_valid")
    # a tile outside the scene is not read: it counts -1, and the Python layer refuses it
    v = torch.ones((300, 300), dtype=torch.uint8, device=dev)
    out = net.scene_tile_valid(v, torch.tensor([[0, 0], [45, 0], [0, 45], [-1, 0], [44, 44]], dtype=torch.int32))
    assert out.cpu().tolist() == [65536, -1, -1, -1, 65536]
    # the Python surface refuses before the device is touched
    img = rect_scene(384, 640, 41)
    cfg = dict(CFG, INFER_PATCHES_PER_EDGE=[3, 5])
    ok = np.ones((384, 640), bool)
    for valid, extra in ((ok[:, :639], {}), (ok[None], {}), (ok.astype(np.float32), {}), (ok.astype(np.int32), {}),
                         (ok, dict(MIN_VALID_FRACTION=-0.1)), (ok, dict(MIN_VALID_FRACTION=1.5)), (ok, dict(MIN_VALID_FRACTION="half")),
                         (ok, dict(NODATA_FILL=[1, 2])), (ok, dict(NODATA_FILL=[1, 2, 256])), (ok, dict(NODATA_FILL=[1.0, 2, 3])),
                         (ok, dict(NODATA_FILL=7))):
        with pytest.raises(ValueError):
            infer_one_img(net, img, Config(dict(cfg, **extra)), valid=valid)


# ---- against the oracle -----------------------------------------------------------------------------------------------------------
# Scenes and seeds were chosen WITH THE ORACLE ALONE on the CPU (points from the oracle's own masks), so that the oracle yields well
# over 200 edges inside the valid area — the symmetric-difference cap max(2, 2 %) is then a condition, not a measurement:
#   (valid share, tiles kept, points, voted edges, oracle edges, share within TOPO_SCORE of the threshold)
#   384x640 band: 0.496, 15, 252, 4678, 571, 0.47 %        384x640 hole: 0.921, 15, 432, 7936, 753, 0.43 %
#   523x701 band: 0.496, 20, 260, 3933, 409, 0.48 %        523x701 hole: 0.947, 20, 525, 8652, 731, 0.35 %
#   401x523 hole: 0.907, 16, 254, 4015, 529, 0.55 %        (401x523 band: 119 points, 212 edges — too close to 200, not used)
PARITY_CASES = [("384x640", "band"), ("384x640", "hole"), ("523x701", "band"), ("523x701", "hole"), ("401x523", "hole")]


@pytest.mark.parametrize("scene,kind", PARITY_CASES)
def test_masked_scene_parity_with_oracle(pair, scene, kind):
    """The checks and bounds of test_rect_scene_parity_with_oracle (tests/tolerances.py) on a masked scene."""
    from sam_road_amd import Config
    from sam_road_amd.inferencer import infer_one_img
    oracle, net = pair
    H, W, per_edge, seed = PARITY_SCENES[scene]
    img, valid = rect_scene(H, W, seed), make_mask(kind, H, W)
    ref = oracle_scene(oracle, img, per_edge, valid=valid)
    cfg = dict(CFG, INFER_PATCHES_PER_EDGE=per_edge, **_thresholds(ref[2], ref[3]))
    got = infer_one_img(net, img, Config(cfg), valid=valid)
    # the scene must give the oracle at least 200 edges for the 2 % cap to be a condition
    check_scene_parity(f"valid_{kind}_{scene}", got, ref, cfg, oracle, valid=valid, min_oracle_edges=200)
