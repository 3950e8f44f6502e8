"""SCENE_SCALE (scenes at another ground resolution, resampled on the device) on the HIP path.  Run on an MI355X: pytest -m gpu.

The reference has no such step and the rule is exact, so the behaviour is pinned by COMPOSITION of what is already pinned: the kernel must
equal resample.resample_ref byte for byte (which tests/test_scene_scale_host.py pins against rational arithmetic), and a run with the key
must equal, bit for bit, the existing pipeline on the numpy-resampled scene (and mask), its masks brought back by resample_ref and its
nodes mapped by the node rule.  No tolerance anywhere.
"""
import ctypes
import warnings

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from scene_kit import CFG, kernel_rows, make_mask, pair, rect_grid, rect_scene, run_cli  # noqa: F401
from scene_kit import net_for as _net_for
from scene_kit import same_bits as _same
from scene_kit import thresholds as _thresholds
from scene_kit import xy_of as _xy

from sam_road_amd.resample import axis_tables, block_plan, map_nodes, out_size, resample_ref

P, MARGIN, BS = CFG["PATCH_SIZE"], CFG["SAMPLE_MARGIN"], CFG["INFER_BATCH_SIZE"]
SHAPES = [(37, 53), (1, 64), (64, 1), (401, 523), (3, 6000)]
SCALES = [(1, 2), (2, 3), (3, 10), (1, 8), (15, 16), (16, 15), (3, 2), (10, 3), (4, 1)]


# ---- 1. the kernel ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scale", SCALES, ids=[f"{p}_{q}" for p, q in SCALES])
@pytest.mark.parametrize("shape", SHAPES, ids=[f"{h}x{w}" for h, w in SHAPES])
def test_scene_resample_equals_resample_ref(shape, scale):
    net = _net_for(P)
    (H, W), (p, q) = shape, scale
    Ho, Wo = out_size(H, p, q), out_size(W, p, q)
    rng = np.random.default_rng(H * 1000 + W + 7 * p + q)
    img = rng.integers(0, 256, size=(H, W, 3), dtype=np.uint8)
    grey = np.ascontiguousarray(img[..., 1])
    mask = rng.random((H, W)) < 0.9
    zw = rng.random((H, W)) < 0.7

    def check(src, want, **kw):
        t = torch.from_numpy(src).cuda()
        out = net.scene_resample(t, *kw.pop("scale", (p, q)), **{k: (torch.from_numpy(v).cuda() if isinstance(v, np.ndarray) else v) for k, v in kw.items()})
        assert out.dtype == t.dtype and tuple(out.shape) == want.shape and out.is_contiguous() and out.data_ptr() != t.data_ptr()
        np.testing.assert_array_equal(out.cpu().numpy(), want, err_msg=f"{src.dtype} {src.shape} {kw}")
        np.testing.assert_array_equal(t.cpu().numpy(), src)                      # the source is untouched

    want3, want1 = resample_ref(img, p, q), resample_ref(grey, p, q)
    assert want3.shape == (Ho, Wo, 3) and want1.shape == (Ho, Wo)
    check(img, want3)                                                            # C = 3 and C = 1, the separable form and the direct one
    check(grey, want1)
    check(img, want3, direct=True)
    check(grey, want1, direct=True)
    for m in (mask, mask.astype(np.uint8) * 200):                                # the validity rule: bool -> bool, u8 -> u8 of value 1
        check(m, resample_ref(m, p, q, valid_rule=True), valid_rule=True)
    assert resample_ref(mask.astype(np.uint8) * 200, p, q, valid_rule=True).max() <= 1
    # the way back to an explicit size, with and without zero_where (bool and u8)
    check(want1, resample_ref(want1, q, p, out_shape=(H, W)), scale=(q, p), out_shape=(H, W))
    check(want1, resample_ref(want1, q, p, out_shape=(H, W), zero_where=zw), scale=(q, p), out_shape=(H, W), zero_where=zw)
    check(want3, resample_ref(want3, q, p, out_shape=(H, W), zero_where=zw), scale=(q, p), out_shape=(H, W), zero_where=zw.astype(np.uint8) * 9)
    # a source view at byte offsets 1 and 3 of a larger allocation: no row is aligned against the 16-byte pieces it is staged in
    for off in (1, 3):
        for src, want in ((img, want3), (grey, want1)):
            big = torch.full((src.size + 16,), 0xA5, dtype=torch.uint8, device="cuda")
            v = big[off:off + src.size].view(src.shape)
            v.copy_(torch.from_numpy(src))
            before = big.cpu().numpy().copy()
            np.testing.assert_array_equal(net.scene_resample(v, p, q).cpu().numpy(), want)
            np.testing.assert_array_equal(net.scene_resample(v, p, q, direct=True).cpu().numpy(), want)
            np.testing.assert_array_equal(big.cpu().numpy(), before)


def test_scene_resample_rejects_bad_arguments():
    from sam_road_amd import _lib
    net = _net_for(P)
    dev = torch.device("cuda")
    ctx, _ = net._weights(dev)
    lib, s = ctx.lib, net._stream(dev)
    H, W, p, q = 16, 24, 1, 2
    src = torch.zeros((H, W, 3), dtype=torch.uint8, device=dev)
    dst = torch.zeros((8, 12, 3), dtype=torch.uint8, device=dev)
    tab = {}
    for n in (H, W):
        st, w, T, D = axis_tables(n, p, q)
        tab[n] = (torch.from_numpy(st).cuda(), torch.from_numpy(w).cuda(), T, D)
    (sy, wy, T, D), (sx, wx, _, _) = tab[H], tab[W]
    bh, bw, wh, ww = block_plan(T, T, p, q, 3)

    def call(**kw):
        a = dict(src=src.data_ptr(), H=H, W=W, C=3, dst=dst.data_ptr(), Ho=8, Wo=12, sy=sy.data_ptr(), wy=wy.data_ptr(), Ty=T, Dy=D, sx=sx.data_ptr(),
                 wx=wx.data_ptr(), Tx=T, Dx=D, mode=0, zw=None, bh=bh, bw=bw, wh=wh, ww=ww)
        a.update(kw)
        return lib.srh_scene_resample(ctx.handle, *a.values(), s)

    assert call() == 0 and call(wh=0, ww=0) == 0 and call(mode=1, C=1) == 0
    bad = [dict(C=2), dict(C=4), dict(Ty=0), dict(Tx=0), dict(Ty=33), dict(Dy=0), dict(Dx=33), dict(H=-16), dict(W=0), dict(Ho=-8), dict(Wo=0), dict(mode=2),
           dict(mode=-1), dict(src=None), dict(dst=None), dict(sy=None), dict(wy=None), dict(sx=None), dict(wx=None),
           dict(H=46341, W=46341), dict(Ho=46341, Wo=46341), dict(H=2 ** 31 - 1, W=2), dict(Ho=65536, Wo=32768),      # products that overflow an int
           dict(bh=0), dict(bw=257), dict(bh=-1), dict(wh=0), dict(ww=0), dict(wh=-1, ww=-1), dict(wh=200, ww=200), dict(wh=5000, ww=1)]
    for kw in bad:
        assert call(**kw) == -1, kw
    with pytest.raises(_lib.SrhError):
        ctx.check(call(C=2), "srh_scene_resample")
    for t in (torch.zeros((8, 8, 3), dtype=torch.float32, device=dev), torch.zeros((8, 8, 4), dtype=torch.uint8, device=dev),
              torch.zeros((8, 8, 2), dtype=torch.uint8, device=dev), torch.zeros((8, 16, 3), dtype=torch.uint8, device=dev)[:, ::2],
              torch.zeros((8,), dtype=torch.uint8, device=dev)):
        with pytest.raises(ValueError):
            net.scene_resample(t, 1, 2)
    for args, kw in (((3, 3), {}), ((0, 2), {}), ((1, -2), {}), ((1.0, 2), {}), ((1, 2), dict(out_shape=(0, 4))), ((1, 2), dict(out_shape=(65536, 32768))),
                     ((1, 2), dict(zero_where=torch.ones((7, 12), dtype=torch.uint8, device=dev))),
                     ((1, 2), dict(zero_where=torch.ones((8, 12), dtype=torch.float32, device=dev)))):
        with pytest.raises(ValueError):
            net.scene_resample(src, *args, **kw)
    torch.cuda.synchronize()


# ---- 3. / 4. a run with the key == the existing pipeline on the numpy-resampled scene, brought back -----------------------------------------
def _check_against_composition(net, img, per_edge, key, p, q):
    from sam_road_amd import Config
    from sam_road_amd.graph_points import extract_graph_points
    from sam_road_amd.inferencer import edge_votes, infer_one_img, scene_tiles, votes_to_edges
    H, W = img.shape[:2]
    small = resample_ref(img, p, q)
    Hm, Wm = small.shape[:2]
    infos = rect_grid(Hm, Wm, MARGIN, P, per_edge)
    xy = _xy(infos)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        kp_c, road_c, emb = net.scene_pass1(torch.from_numpy(small).cuda(), xy, BS)
        kp_u8, road_u8 = net.scene_normalise(kp_c, road_c, xy)
        kp_m, road_m = kp_u8.cpu().numpy(), road_u8.cpu().numpy()
        plain = Config(dict(CFG, INFER_PATCHES_PER_EDGE=per_edge, **_thresholds(kp_m, road_m)))
        cfg = Config(dict(plain, SCENE_SCALE=key))
        tiles = scene_tiles(img.shape, cfg)
        assert list(tiles) == infos and tiles.scale == (p, q) and tiles.model_shape == (Hm, Wm)
        whole = infer_one_img(net, small, plain)                                 # the existing pipeline on the host-resampled scene
        img_before = img.copy()
        nodes, edges, kp_o, road_o = infer_one_img(net, img, cfg)
    np.testing.assert_array_equal(img, img_before)
    assert kp_o.shape == road_o.shape == (H, W) and kp_o.dtype == road_o.dtype == np.uint8
    _same(whole[2], kp_m)
    _same(whole[3], road_m)
    _same(kp_o, resample_ref(kp_m, q, p, out_shape=(H, W)))
    _same(road_o, resample_ref(road_m, q, p, out_shape=(H, W)))
    pts = extract_graph_points(kp_m, road_m, plain)
    _same(nodes, map_nodes(pts[:, ::-1], (H, W), p, q))
    _same(nodes, map_nodes(whole[0], (H, W), p, q))
    _same(edges, whole[1])
    votes = edge_votes(net, emb, pts, infos, 0, len(infos), plain, torch.device("cuda"))
    _same(edges, votes_to_edges(*votes, pts.shape[0], plain.TOPO_THRESHOLD))
    print(f"{H}x{W} at {p}/{q} -> {Hm}x{Wm}: {len(infos)} tiles, {pts.shape[0]} points, {edges.shape[0]} edges")
    assert pts.shape[0] > 20 and edges.shape[0] > 20
    assert nodes.min() >= 0 and nodes[:, 0].max() < H and nodes[:, 1].max() < W
    assert len({tuple(n) for n in nodes.tolist()}) == nodes.shape[0]             # no duplicate node
    return (nodes, edges, kp_o, road_o), cfg, plain, small


def test_downscale_on_the_odd_pitch_scene(pair):
    """802 x 1046 at 1/2: the model frame is the 401 x 523 odd-pitch geometry of the pad tests."""
    _, net = pair
    got, _, _, small = _check_against_composition(net, rect_scene(802, 1046, 43), 4, [1, 2], 1, 2)
    assert small.shape == (401, 523, 3) and got[0][:, 0].max() >= 401            # scene coordinates


def test_upscale(pair):
    """268 x 349 at 3/2: the model frame is 402 x 524; the scene is larger than the model sees it nowhere."""
    _, net = pair
    _, _, _, small = _check_against_composition(net, rect_scene(268, 349, 43), 4, {"scene_gsd": 1.5, "model_gsd": 1.0}, 3, 2)
    assert small.shape == (402, 524, 3)


# ---- 5. changes nothing ---------------------------------------------------------------------------------------------------------------------
def test_unit_scale_and_absent_key_change_nothing(pair):
    from sam_road_amd import Config, _lib
    from sam_road_amd.inferencer import infer_one_img
    _, net = pair
    img = rect_scene(802, 1046, 43)
    small = resample_ref(img, 1, 2)
    plain = Config(dict(CFG, INFER_PATCHES_PER_EDGE=4))
    ctx = _lib.Context.get(torch.cuda.current_device())
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        with kernel_rows(ctx) as rows:
            bare = infer_one_img(net, small, plain)
            rows_plain = rows()
            unit = infer_one_img(net, small, Config(dict(plain, SCENE_SCALE=[3, 3])))
            rows_unit = rows()
            none = infer_one_img(net, small, Config(dict(plain, SCENE_SCALE=None)))
            rows_none = rows()
            infer_one_img(net, img, Config(dict(plain, SCENE_SCALE=[1, 2])))
            rows_half = rows()
    for a, b, c in zip(bare, unit, none):
        _same(a, b)
        _same(a, c)
    assert "scene_resample" not in rows_plain and rows_unit == rows_plain == rows_none
    assert rows_half == rows_plain | {"scene_resample"}


# ---- 6. everything at once ------------------------------------------------------------------------------------------------------------------
def test_scale_with_mask_window_tta_and_pad(pair):
    """576 x 960 at 2/3 (model frame 384 x 640), the band mask, FUSE_WINDOW hann, TTA [id, rot90], SCENE_PAD {border 8, edge}: equals the
    existing pipeline with those keys on the numpy-resampled scene and the mask resampled by the validity rule, brought back."""
    from sam_road_amd import Config
    from sam_road_amd.inferencer import infer_one_img, scene_tiles
    _, net = pair
    H, W, p, q = 576, 960, 2, 3
    img, valid = rect_scene(H, W, 41), make_mask("band", H, W)
    small, valid_m = resample_ref(img, p, q), resample_ref(valid, p, q, valid_rule=True)
    assert small.shape == (384, 640, 3) and valid_m.shape == (384, 640) and valid_m.dtype == bool and 0 < valid_m.sum() < valid_m.size
    extra = dict(INFER_PATCHES_PER_EDGE=[3, 5], FUSE_WINDOW="hann", TTA=["id", "rot90"], SCENE_PAD={"border": 8, "mode": "edge"})
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        _, _, kp0, road0 = infer_one_img(net, small, Config(dict(CFG, **extra)), valid=valid_m)
        plain = Config(dict(CFG, **extra, **_thresholds(kp0, road0)))
        cfg = Config(dict(plain, SCENE_SCALE=[p, q]))
        whole = infer_one_img(net, small, plain, valid=valid_m)
        nodes, edges, kp, road = infer_one_img(net, img, cfg, valid=valid)
        tiles = scene_tiles(img.shape, cfg, valid=valid, net=net)
        tiles_m = scene_tiles(small.shape, plain, valid=valid_m, net=net)
    _same(kp, resample_ref(whole[2], q, p, out_shape=(H, W), zero_where=valid))
    _same(road, resample_ref(whole[3], q, p, out_shape=(H, W), zero_where=valid))
    _same(nodes, map_nodes(whole[0], (H, W), p, q))
    _same(edges, whole[1])
    print(f"{len(tiles)} tiles kept, {nodes.shape[0]} points, {edges.shape[0]} edges")
    assert nodes.shape[0] > 20 and edges.shape[0] > 20
    assert not kp[~valid].any() and not road[~valid].any() and road[valid].any()
    assert valid[nodes[:, 0], nodes[:, 1]].all()                                 # every node on a valid scene pixel
    assert tiles == tiles_m and 0 < len(tiles) <= 15 and tiles.scale == (p, q) and tiles.model_shape == (384, 640)
    assert tiles.pads == tiles_m.pads == (8, 8, 8, 8) and tiles.orientations == ["id", "rot90"] and tiles_m.scale == (1, 1)


# ---- 7. the loops ---------------------------------------------------------------------------------------------------------------------------
def test_infer_imgs_pipelined_equals_infer_one_img(pair):
    """[802 x 1046, 600 x 640, 802 x 1046] at 1/2 through the software-pipelined loop, twice over — the third scene reuses the first one's
    page-locked staging of both mask downloads — and once with a mask on the middle scene: infer_one_img's tuples, in order."""
    from sam_road_amd import Config
    from sam_road_amd.inferencer import infer_imgs, infer_one_img
    _, net = pair
    imgs = [rect_scene(802, 1046, 43), rect_scene(600, 640, 48), rect_scene(802, 1046, 47)]
    base = Config(dict(CFG, SCENE_SCALE=[1, 2]))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        _, _, kp0, road0 = infer_one_img(net, imgs[0], base)
        cfg = Config(dict(base, **_thresholds(kp0, road0)))
        want = [infer_one_img(net, im, cfg) for im in imgs]
        print("points / edges per scene:", [(w[0].shape[0], w[1].shape[0]) for w in want])
        assert [w[2].shape for w in want] == [(802, 1046), (600, 640), (802, 1046)]
        assert want[0][0].shape[0] > 20 and want[0][1].shape[0] > 20 and all(w[0].shape[0] > 5 for w in want)
        for _ in range(2):
            got = list(infer_imgs(net, iter(imgs), cfg))
            assert len(got) == 3
            for w, g in zip(want, got):
                for a, b in zip(w, g):
                    _same(a, b)
        valids = [None, make_mask("band", 600, 640), None]
        want_v = [infer_one_img(net, im, cfg, valid=v) for im, v in zip(imgs, valids)]
        assert not want_v[1][3][~valids[1]].any() and want_v[1][3].any()
        for w, g in zip(want_v, infer_imgs(net, iter(imgs), cfg, valids=iter(valids))):
            for a, b in zip(w, g):
                _same(a, b)


# ---- 8. the CLI -----------------------------------------------------------------------------------------------------------------------------
def test_cli_writes_scene_sized_masks_and_scene_coordinates(pair, tmp_path, monkeypatch):
    from PIL import Image
    from sam_road_amd import Config
    from sam_road_amd import cli
    from sam_road_amd.formats import convert_to_sat2graph_format
    _, net = pair
    img = rect_scene(600, 640, 48)
    monkeypatch.chdir(tmp_path)
    Image.fromarray(img).save("rgb.png")
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        _, _, kp0, road0 = infer_one_img_at(net, img, dict(CFG, SCENE_SCALE=[1, 2]))
        cfg = dict(CFG, **_thresholds(kp0, road0))
        want = infer_one_img_at(net, img, dict(cfg, SCENE_SCALE=[1, 2]))
        got = run_cli(cli, net, tmp_path, monkeypatch, "scale", cfg, ["rgb.png"], "--device", "cuda", "--scene-scale", "1", "2")["rgb"]
    assert got[0].shape == got[1].shape == (600, 640) and got[3]["SCENE_SCALE"] == [1, 2]
    np.testing.assert_array_equal(got[0], want[2])
    np.testing.assert_array_equal(got[1], want[3])
    assert want[0].shape[0] > 5 and want[0][:, 0].max() >= 300                   # scene coordinates, beyond the 300 x 320 model frame
    assert got[2] == convert_to_sat2graph_format(want[0], want[1])


def infer_one_img_at(net, img, cfg):
    from sam_road_amd import Config
    from sam_road_amd.inferencer import infer_one_img
    return infer_one_img(net, img, Config(cfg))
