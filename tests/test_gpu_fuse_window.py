"""FUSE_WINDOW (window-weighted fusion of overlapping tiles) on the HIP path.  Run on an MI355X: pytest -m gpu.

The reference fuses with a uniform mean, so there is nothing of it to compare a window against.  What is checked instead:
  * the arithmetic of the three weighted canvas steps against the rule restated in float64 numpy in this file (op level: seeded
    scores, no model), with bounds derived from the f32 format and not from what the kernels give;
  * identities with the unweighted kernels (an all-ones profile gives their bytes; a constant 0.5 gives a quarter of the canvases
    and the same masks) and independence of how the tile list is cut into calls;
  * the scene-level calls as a COMPOSITION of the pieces, bit for bit, and against the CPU oracle's per-tile scores fused by the same
    float64 rule, with the bounds of test_rect_scene_parity_with_oracle.
No statement about the quality of the roads is made or could be made here: there are no trained weights and no dataset.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from scene_kit import (CFG, FILL, PARITY_SCENES, SCENES, check_scene_parity, fuse_f64, kernel_rows, make_mask, np_kept, oracle_scene, pair,  # noqa: F401
                       rect_grid, rect_scene)
from scene_kit import dev as _dev
from scene_kit import net_for as _net_for
from scene_kit import same_bits as _same
from scene_kit import thresholds as _thresholds
from scene_kit import xy_of as _xy


def profile_f64(kind, P, seed=0):
    """The 1-D profiles in float64 (the formulas of DESIGN.md §6e, restated)."""
    i = np.arange(P, dtype=np.float64)
    if kind == "hann":
        return np.sin(np.pi * (i + 0.5) / P) ** 2
    if kind == "triangle":
        return np.minimum(i + 0.5, P - i - 0.5) * 2.0 / P
    if kind == "random":
        return np.random.default_rng(1000 + P + seed).uniform(0.01, 1.0, size=P)
    if kind == "ones":
        return np.ones(P)
    raise KeyError(kind)


def scene_shapes(P):
    """Square, rectangular, and a scene whose row pitch W is odd."""
    return {"square": (2 * P + P // 2, 2 * P + P // 2), "rect": (2 * P, 3 * P + 40), "oddW": (2 * P + 17, 2 * P + P // 4 + 1)}


def tile_list(kind, H, W, P, seed):
    rng = np.random.default_rng(seed)
    grid = np.array([p[1] for p in rect_grid(H, W, 0, P, [3, 4])], dtype=np.int32)
    if kind == "grid":
        return grid
    if kind == "holes":                                                        # a grid with tiles removed
        return grid[[i for i in range(len(grid)) if i % 3 != 1]]
    if kind == "arbitrary":                                                    # any order, the four corners, one tile twice
        xy = np.stack([rng.integers(0, W - P + 1, size=9), rng.integers(0, H - P + 1, size=9)], 1).astype(np.int32)
        xy = np.concatenate([xy, [[0, 0], [W - P, H - P], [W - P, 0], [0, H - P]], xy[3:4], xy[3:4]]).astype(np.int32)
        return xy[rng.permutation(len(xy))]
    raise KeyError(kind)


# ---- 1. the weighted add against float64 ------------------------------------------------------------------------------------------
# Bound (derived, not measured): every term is positive, so the f32 sum of n products lies within (n + 1) 2^-24 relative of the exact
# value (one rounding of the weight product, one per fused multiply-add; the prior canvas value is one more positive term).  The
# scenes keep n <= 64, asserted below: (64 + 2) 2^-24 = 3.9e-6, and the test asserts 1e-5.
ADD_REL = 1e-5
MAX_COVER = 64


@pytest.mark.parametrize("lists", ["grid", "holes", "arbitrary"])
@pytest.mark.parametrize("shape", ["square", "rect", "oddW"])
@pytest.mark.parametrize("P", [128, 208, 512])
def test_weighted_add_against_float64(P, shape, lists):
    net = _net_for(P)
    H, W = scene_shapes(P)[shape]
    assert shape != "oddW" or W % 2 == 1
    xy = tile_list(lists, H, W, P, seed=P + H)
    assert xy[:, 0].min() >= 0 and xy[:, 1].min() >= 0 and xy[:, 0].max() <= W - P and xy[:, 1].max() <= H - P
    rng = np.random.default_rng(P * 31 + W)
    scores = rng.random((len(xy), P, P, 2), dtype=np.float32)                  # uniform in [0, 1)
    prior = rng.random((2, H, W), dtype=np.float32)
    scores_d, xy_d = _dev(scores), _dev(xy)
    for kind in ("hann", "triangle", "random"):
        w1 = profile_f64(kind, P).astype(np.float32)
        kp_r, road_r, _, cnt = fuse_f64((H, W), xy, scores, w1, prior)
        assert 0 < cnt.max() <= MAX_COVER and ((cnt == 0).any() or lists != "arbitrary")      # the arbitrary lists leave pixels uncovered
        kp_d, road_d = _dev(prior[0]), _dev(prior[1])
        net.op_scene_fuse_window(scores_d, xy_d, _dev(w1), kp_d, road_d)
        on = cnt > 0
        for name, got, ref, pri in (("kp", kp_d.cpu().numpy(), kp_r, prior[0]), ("road", road_d.cpu().numpy(), road_r, prior[1])):
            rel = np.abs(got[on].astype(np.float64) - ref[on]) / ref[on]
            print(f"[fuse_window] add P={P} {shape} {lists} {kind} {name}: max covering tiles {cnt.max()}, max rel err {rel.max():.3e} (bound {ADD_REL:.0e})")
            assert rel.max() <= ADD_REL
            np.testing.assert_array_equal(got[~on].view(np.uint32), pri[~on].view(np.uint32))      # uncovered: the prior value, exactly


# ---- 2. independence of how the tile list is cut into calls --------------------------------------------------------------------------
@pytest.mark.parametrize("P,shape", [(208, "oddW"), (128, "rect")])
def test_chunking_gives_identical_bits(P, shape):
    net = _net_for(P)
    H, W = scene_shapes(P)[shape]
    # 27 tiles, and 81 for the second case: more than the 64 tiles a wave looks at in one step of the kernel
    xy = np.concatenate([tile_list(k, H, W, P, seed=sd) for sd in ((3,) if P == 208 else (3, 5, 6)) for k in ("arbitrary", "grid")]).astype(np.int32)
    assert len(xy) == (27 if P == 208 else 81)
    rng = np.random.default_rng(P)
    scores = rng.random((len(xy), P, P, 2), dtype=np.float32)
    w1 = _dev(profile_f64("hann", P).astype(np.float32))
    scores_d, xy_d = _dev(scores), _dev(xy)
    out = []
    for step in (len(xy), 7, 1):
        kp, road = torch.zeros((H, W), device="cuda"), torch.zeros((H, W), device="cuda")
        for off in range(0, len(xy), step):
            net.op_scene_fuse_window(scores_d[off:off + step].contiguous(), xy_d[off:off + step].contiguous(), w1, kp, road)
        out.append((kp.cpu().numpy(), road.cpu().numpy()))
    assert out[0][0].max() > 0
    for kp, road in out[1:]:
        _same(kp, out[0][0])
        _same(road, out[0][1])


# ---- 3. identities with the unweighted kernels ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("scene", list(SCENES))
def test_ones_profile_gives_the_unweighted_bytes_and_half_gives_a_quarter(pair, scene):
    _, net = pair
    H, W, per_edge, seed = SCENES[scene]
    P, bs = CFG["PATCH_SIZE"], CFG["INFER_BATCH_SIZE"]
    img = _dev(rect_scene(H, W, seed))
    xy = _xy(rect_grid(H, W, CFG["SAMPLE_MARGIN"], P, per_edge))
    valid = _dev(make_mask("band", H, W))
    kp0, road0, emb0 = net.scene_pass1(img, xy, bs)
    base = (net.scene_normalise(kp0, road0, xy), net.scene_normalise(kp0, road0, xy, valid=valid))
    ones = torch.ones(P, device="cuda")
    kp1, road1, emb1 = net.scene_pass1(img, xy, bs, window=ones)
    _same(emb1.cpu().numpy(), emb0.cpu().numpy())
    _same(kp1.cpu().numpy(), kp0.cpu().numpy())
    _same(road1.cpu().numpy(), road0.cpu().numpy())
    for want, kw in zip(base, (dict(), dict(valid=valid))):
        got = net.scene_normalise(kp1, road1, xy, window=ones, **kw)
        _same(got[0].cpu().numpy(), want[0].cpu().numpy())
        _same(got[1].cpu().numpy(), want[1].cpu().numpy())
    assert base[0][0].max() > 0 and not base[1][0].cpu().numpy()[~make_mask("band", H, W)].any()
    half = torch.full((P,), 0.5, device="cuda")
    kp2, road2, emb2 = net.scene_pass1(img, xy, bs, window=half)
    _same(emb2.cpu().numpy(), emb0.cpu().numpy())
    _same(kp2.cpu().numpy(), kp0.cpu().numpy() * np.float32(0.25))              # a power of two: exactly one quarter
    _same(road2.cpu().numpy(), road0.cpu().numpy() * np.float32(0.25))
    for want, kw in zip(base, (dict(), dict(valid=valid))):
        got = net.scene_normalise(kp2, road2, xy, window=half, **kw)
        _same(got[0].cpu().numpy(), want[0].cpu().numpy())
        _same(got[1].cpu().numpy(), want[1].cpu().numpy())


# ---- 4. the weighted normalise against float64 -----------------------------------------------------------------------------------------
# By the bound of test 1, the f32 weight sum is within 3.9e-6 relative of the exact one; the division and the multiplication add
# 2^-24 each, so (canvas / Wsum) * 255 is within 255 * 4.1e-6 = 1.1e-3 < 4e-3 of the float64 level.  Where the float64 level is
# farther than that from an integer the u8 must be equal; elsewhere within one level.  The near-integer set is 2 * 4e-3 = 0.8 % of the
# pixels for levels spread evenly; asserted <= 2 % on the float64 numbers themselves.
NORM_LEVEL = 4e-3


@pytest.mark.parametrize("lists", ["grid", "holes", "arbitrary"])
@pytest.mark.parametrize("P,shape", [(128, "rect"), (208, "oddW"), (512, "square")])
def test_weighted_normalise_against_float64(P, shape, lists):
    net = _net_for(P)
    H, W = scene_shapes(P)[shape]
    xy = tile_list(lists, H, W, P, seed=P + H)
    rng = np.random.default_rng(P * 17 + H)
    scores = rng.random((len(xy), P, P, 2), dtype=np.float32)
    valid = make_mask("band", H, W)
    for kind in ("hann", "triangle", "random"):
        w1 = profile_f64(kind, P, seed=1).astype(np.float32)
        kp64, road64, ws, cnt = fuse_f64((H, W), xy, scores, w1)
        assert 0 < cnt.max() <= MAX_COVER
        canv = [c.astype(np.float32) for c in (kp64, road64)]                  # the f32 canvases handed to the kernel
        on = cnt > 0
        for v in (None, valid):
            got = net.scene_normalise(_dev(canv[0]), _dev(canv[1]), _dev(xy), window=_dev(w1), **({} if v is None else dict(valid=_dev(v))))
            live = on if v is None else on & v
            for name, g, c32 in zip(("kp", "road"), got, canv):
                g = g.cpu().numpy()
                assert g.dtype == np.uint8 and g.shape == (H, W)
                assert not g[~live].any()                                      # uncovered, and invalid under a mask
                lv = c32[live].astype(np.float64) / ws[live] * 255.0
                near = np.abs(lv - np.rint(lv)) <= NORM_LEVEL
                share = near.mean()
                d = np.abs(g[live].astype(np.int64) - np.floor(lv).astype(np.int64))
                print(f"[fuse_window] normalise P={P} {shape} {lists} {kind} {name} valid={v is not None}: near-integer share {share:.4f} "
                      f"(<= 0.02), differing there {int((d[near] > 0).sum())}, differing elsewhere {int((d[~near] > 0).sum())}")
                assert share <= 0.02
                assert (d[~near] == 0).all()
                assert d.max() <= 1


# ---- 5. the scene-level calls are a composition of the pieces --------------------------------------------------------------------------
SCENE_CASES = [("384x640", None), ("401x523", None), ("384x640", "left")]     # the masked one drops whole tile columns (frac 0.25)


@pytest.mark.parametrize("window", ["hann", "triangle"])
@pytest.mark.parametrize("scene,kind", SCENE_CASES)
def test_windowed_run_equals_composition_bit_for_bit(pair, scene, kind, window):
    from sam_road_amd import Config
    from sam_road_amd.graph_points import extract_graph_points
    from sam_road_amd.inferencer import edge_votes, fuse_window, infer_one_img, votes_to_edges
    _, net = pair
    H, W, per_edge, seed = SCENES[scene]
    P, bs = CFG["PATCH_SIZE"], CFG["INFER_BATCH_SIZE"]
    img = rect_scene(H, W, seed)
    infos = rect_grid(H, W, CFG["SAMPLE_MARGIN"], P, per_edge)
    valid, frac, filled = None, 0.0, img
    if kind is not None:
        valid, frac = make_mask(kind, H, W), 0.25
        kept = np_kept(valid, infos, P, frac)
        assert 0 < len(kept) < len(infos)
        infos = [infos[i] for i in kept]
        filled = np.ascontiguousarray(np.where(valid[..., None], img, np.array(FILL, np.uint8)))
    base = dict(CFG, INFER_PATCHES_PER_EDGE=per_edge, MIN_VALID_FRACTION=frac, FUSE_WINDOW=window)
    w1 = fuse_window(Config(base))
    np.testing.assert_array_equal(w1, profile_f64(window, P).astype(np.float32))
    w_d, xy, scene_d = _dev(w1), _xy(infos), _dev(filled)
    valid_d = None if valid is None else _dev(valid)
    # the pieces
    kp0, road0, emb0 = net.scene_pass1(scene_d, xy, bs)
    kp_c, road_c, emb = net.scene_pass1(scene_d, xy, bs, window=w_d)
    _same(emb.cpu().numpy(), emb0.cpu().numpy())                               # the embeddings do not depend on the window
    assert not np.array_equal(kp_c.cpu().numpy(), kp0.cpu().numpy())
    # the weighted canvases are the weighted add of this pass's own per-tile scores: the same batches through infer_masks_and_img_features
    # (same batch sizes, hence the same kernels: exact, no BATCH_INDEP_SCORE needed)
    kp_f, road_f = torch.zeros((H, W), device="cuda"), torch.zeros((H, W), device="cuda")
    for off in range(0, len(infos), bs):
        tiles = np.stack([filled[y0:y1, x0:x1] for _, (x0, y0), (x1, y1) in infos[off:off + bs]])
        scores, e = net.infer_masks_and_img_features(_dev(tiles))
        _same(e.cpu().numpy(), emb[off:off + bs].cpu().numpy())
        net.op_scene_fuse_window(scores.contiguous(), xy[off:off + bs].contiguous(), w_d, kp_f, road_f)
    _same(kp_c.cpu().numpy(), kp_f.cpu().numpy())
    _same(road_c.cpu().numpy(), road_f.cpu().numpy())
    kp_u8, road_u8 = net.scene_normalise(kp_c, road_c, xy, window=w_d, **({} if valid is None else dict(valid=valid_d)))
    kp_m, road_m = kp_u8.cpu().numpy(), road_u8.cpu().numpy()
    plain = net.scene_normalise(kp0, road0, xy)
    assert not np.array_equal(kp_m, plain[0].cpu().numpy())                    # the window changes the masks
    # the whole call
    thr = _thresholds(kp_m, road_m)
    cfg = Config(dict(base, **thr))
    nodes, edges, kp_o, road_o = infer_one_img(net, img, cfg, valid=valid)
    _same(kp_o, kp_m)
    _same(road_o, road_m)
    pts = extract_graph_points(kp_m, road_m, cfg)
    _same(nodes, pts[:, ::-1])
    assert pts.shape[0] > 20
    votes = edge_votes(net, emb, pts, infos, 0, len(infos), cfg, torch.device("cuda"))
    want_edges = votes_to_edges(*votes, pts.shape[0], cfg.TOPO_THRESHOLD)
    _same(edges, want_edges)
    assert edges.shape[0] > 20
    if valid is not None:
        assert not kp_o[~valid].any() and not road_o[~valid].any() and valid[nodes[:, 0], nodes[:, 1]].all()
    # a profile given as a sequence is the same thing
    for a, b in zip(infer_one_img(net, img, Config(dict(cfg, FUSE_WINDOW=w1.tolist())), valid=valid), (nodes, edges, kp_o, road_o)):
        _same(a, b)


# ---- 6. the pipelined loop; uniform is the key absent ---------------------------------------------------------------------------------
def test_infer_imgs_with_a_window_equals_serial_and_uniform_equals_absent(pair):
    from sam_road_amd import Config, _lib
    from sam_road_amd.inferencer import infer_imgs, infer_one_img
    _, net = pair
    shapes = [(384, 640), (640, 384), (401, 523), (448, 448), (384, 640), (401, 523)]
    kinds = [None, "band", "hole", "none", "left", None]
    imgs = [rect_scene(h, w, 50 + i) for i, (h, w) in enumerate(shapes)]
    valids = [None if k is None else make_mask(k, h, w) for k, (h, w) in zip(kinds, shapes)]
    _, _, kp0, road0 = infer_one_img(net, imgs[0], Config(dict(CFG, FUSE_WINDOW="hann")))
    thr = _thresholds(kp0, road0)
    for window in ("hann", "triangle"):
        cfg = Config(dict(CFG, FUSE_WINDOW=window, **thr))
        want = [infer_one_img(net, im, cfg, valid=v) for im, v in zip(imgs, valids)]
        print(f"{window}: points / edges per scene:", [(w[0].shape[0], w[1].shape[0]) for w in want])
        assert all(w[0].shape[0] > 20 and w[1].shape[0] > 20 for w, k in zip(want, kinds) if k != "none")
        got = list(infer_imgs(net, iter(imgs), cfg, valids=iter(valids)))
        assert len(got) == len(want)
        for w, g in zip(want, got):
            for a, b in zip(w, g):
                _same(a, b)
    # 'uniform' (and None) is the key absent, bit for bit, and launches no window kernel
    absent = Config(dict(CFG, **thr))
    want = [infer_one_img(net, im, absent, valid=v) for im, v in zip(imgs[:3], valids[:3])]
    assert not np.array_equal(want[0][2], infer_one_img(net, imgs[0], Config(dict(CFG, FUSE_WINDOW="hann", **thr)))[2])
    ctx = _lib.Context.get(torch.cuda.current_device())
    with kernel_rows(ctx) as rows:
        for v in ("uniform", None):
            cfg = Config(dict(absent, FUSE_WINDOW=v))
            for w, g in zip(want, [infer_one_img(net, im, cfg, valid=m) for im, m in zip(imgs[:3], valids[:3])]):
                for a, b in zip(w, g):
                    _same(a, b)
            for w, g in zip(want, infer_imgs(net, iter(imgs[:3]), cfg, valids=iter(valids[:3]))):
                for a, b in zip(w, g):
                    _same(a, b)
        uniform = rows()
        infer_one_img(net, imgs[0], Config(dict(absent, FUSE_WINDOW="hann")))
        infer_one_img(net, imgs[1], Config(dict(absent, FUSE_WINDOW="hann")), valid=valids[1])
        windowed = rows()
    new = {"scene_add_window", "scene_norm_window"}
    print("kernel classes, uniform:", sorted(uniform), "| windowed:", sorted(windowed))
    assert not (new & uniform) and {"scene_add", "scene_count", "scene_normalise"} <= uniform
    assert new <= windowed and not ({"scene_add", "scene_count", "scene_normalise", "scene_norm_valid"} & windowed)


# ---- the C entries reject what their unweighted twins reject ----------------------------------------------------------------------------
def test_abi_rejects_bad_arguments(pair):
    _, net = pair
    dev = torch.device("cuda")
    ctx, wh = net._weights(dev)
    buf = torch.zeros(1024, dtype=torch.float32, device=dev)
    xy = torch.zeros((1, 2), dtype=torch.int32, device=dev)
    p, s, lib, q = buf.data_ptr(), net._stream(dev), ctx.lib, xy.data_ptr()
    for H, W in ((46341, 46341), (0, 640), (640, -1)):
        assert lib.srh_scene_normalise_window_hw(ctx.handle, p, p, H, W, q, 1, 256, p, None, p, p, s) == -1, (H, W)
        assert lib.srh_scene_pass1_window_hw(ctx.handle, wh, p, H, W, q, 1, 5, p, p, p, p, s) == -1, (H, W)
        assert lib.srh_op_scene_fuse_window(ctx.handle, p, 1, 256, q, p, p, p, H, W, s) == -1, (H, W)
    for H, W in ((255, 640), (640, 255)):                                      # smaller than a tile
        assert lib.srh_scene_pass1_window_hw(ctx.handle, wh, p, H, W, q, 1, 5, p, p, p, p, s) == -1, (H, W)
        assert lib.srh_op_scene_fuse_window(ctx.handle, p, 1, 256, q, p, p, p, H, W, s) == -1, (H, W)
    for P in (0, -16, 250, 8, 112, 1040):                                      # not a tile size
        assert lib.srh_scene_normalise_window_hw(ctx.handle, p, p, 2048, 2048, q, 1, P, p, None, p, p, s) == -1, P
        assert lib.srh_op_scene_fuse_window(ctx.handle, p, 1, P, q, p, p, p, 2048, 2048, s) == -1, P
    ok_n = (p, p, 640, 640, q, 1, 256, p, None, p, p)
    for i in (0, 1, 4, 7, 9, 10):                                              # every pointer but the nullable mask
        args = list(ok_n)
        args[i] = None
        assert lib.srh_scene_normalise_window_hw(ctx.handle, *args, s) == -1, i
    assert lib.srh_scene_normalise_window_hw(ctx.handle, p, p, 640, 640, q, -1, 256, p, None, p, p, s) == -1
    ok_p = (wh, p, 640, 640, q, 1, 5, p, p, p, p)
    for i in (0, 1, 4, 7, 8, 9, 10):
        args = list(ok_p)
        args[i] = None
        assert lib.srh_scene_pass1_window_hw(ctx.handle, *args, s) == -1, i
    assert lib.srh_scene_pass1_window_hw(ctx.handle, wh, p, 640, 640, q, -1, 5, p, p, p, p, s) == -1
    assert lib.srh_scene_pass1_window_hw(ctx.handle, wh, p, 640, 640, q, 1, 0, p, p, p, p, s) == -1
    ok_o = (p, 1, 256, q, p, p, p, 640, 640)
    for i in (0, 3, 4, 5, 6):
        args = list(ok_o)
        args[i] = None
        assert lib.srh_op_scene_fuse_window(ctx.handle, *args, s) == -1, i
    assert lib.srh_op_scene_fuse_window(ctx.handle, p, -1, 256, q, p, p, p, 640, 640, s) == -1
    # the shim refuses a window of another length, dtype or device before the library is called
    scene = torch.zeros((384, 640, 3), dtype=torch.uint8, device=dev)
    for w in (torch.ones(255, device=dev), torch.ones(256, device=dev, dtype=torch.float64), torch.ones(256)):
        with pytest.raises(ValueError, match="window"):
            net.scene_pass1(scene, xy, 5, window=w)
        with pytest.raises(ValueError, match="window"):
            net.scene_normalise(torch.zeros((384, 640), device=dev), torch.zeros((384, 640), device=dev), xy, window=w)


# ---- 7. against the oracle ------------------------------------------------------------------------------------------------------------
# Scenes, masks and windows were chosen WITH THE ORACLE ALONE on the CPU (points from the oracle's own masks) so that its graph has well
# over 20 points and 50 voted edges:   (tiles, points, voted edges, oracle edges, share within TOPO_SCORE of the threshold)
#   384x640 unmasked hann: 15, 470, 8834, 675, 0.34 %      523x701 hole triangle: 20, 593, 10232, 811, 0.33 %
#   384x640 band hann:     15, 257, 4732, 554, 0.46 %
PARITY_CASES = [("384x640", None, "hann"), ("523x701", "hole", "triangle"), ("384x640", "band", "hann")]


@pytest.mark.parametrize("scene,kind,window", PARITY_CASES)
def test_windowed_scene_parity_with_oracle(pair, scene, kind, window):
    """The assertions and bounds of test_rect_scene_parity_with_oracle (tests/tolerances.py) on a window-fused scene."""
    from sam_road_amd import Config
    from sam_road_amd.inferencer import infer_one_img
    oracle, net = pair
    H, W, per_edge, seed = PARITY_SCENES[scene]
    img = rect_scene(H, W, seed)
    valid = None if kind is None else make_mask(kind, H, W)
    w1 = profile_f64(window, CFG["PATCH_SIZE"]).astype(np.float32)
    ref = oracle_scene(oracle, img, per_edge, valid=valid, window=w1)
    cfg = dict(CFG, INFER_PATCHES_PER_EDGE=per_edge, FUSE_WINDOW=window, **_thresholds(ref[2], ref[3]))
    got = infer_one_img(net, img, Config(cfg), valid=valid)
    check_scene_parity(f"fuse_window_{window}_{kind or 'unmasked'}_{scene}", got, ref, cfg, oracle, valid=valid)
