"""Scenes with a per-pixel validity mask (nodata), the GPU-free part: the selection rule and the argument errors against numpy, the
C-ABI surface, the tile-sharded loops on gloo / CPU, and the CLI plumbing — all through a numpy stand-in of the three shim methods
(scene_tile_valid, scene_fill_invalid, scene_normalise(valid=)) of the CPU stand-in model of tests/scene_kit.py (feature "valid")."""
import warnings

import numpy as np
import pytest
import torch

from sam_road_amd import Config, _lib
from sam_road_amd.inferencer import infer_imgs, infer_one_img, scene_tiles, select_tiles
from sam_road_amd.tiling import get_patch_info_hw

from scene_kit import HOST_CFG as _CFG
from scene_kit import SceneStandIn, _CountOnly, assert_abi_11, compare_worlds, make_mask, run_cli, run_worlds
from scene_kit import rect_scene as _rect_scene
from scene_kit import same_tuple as _same_tuple


# ---- selection rule ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W,per_edge,P", [(401, 523, 4, 128), (384, 640, [3, 5], 128), (640, 640, 3, 256)])
def test_selection_rule_against_numpy(H, W, per_edge, P):
    cfg = dict(PATCH_SIZE=P, SAMPLE_MARGIN=16, INFER_PATCHES_PER_EDGE=per_edge, MAX_NEIGHBOR_QUERIES=16)
    net = _CountOnly(P)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        infos = get_patch_info_hw(0, H, W, 16, P, per_edge)
        assert scene_tiles((H, W), Config(cfg)) == infos == scene_tiles((H, W, 3), Config(cfg))
        dropped_some = False
        for kind in ("all", "band", "hole", "none", "pixel_mid", "left"):
            m = make_mask(kind, H, W)
            counts = np.array([m[y0:y1, x0:x1].sum() for _, (x0, y0), (x1, y1) in infos])
            for frac in (None, 0, 0.25, 0.5, 1.0, 1):
                f = 0.0 if frac is None else float(frac)
                want = [p for p, c in zip(infos, counts) if c > 0 and c >= f * P * P]
                c = Config(cfg if frac is None else dict(cfg, MIN_VALID_FRACTION=frac))
                for v in (m, m.astype(np.uint8), m.astype(np.uint8) * 255, np.asfortranarray(m)):
                    assert scene_tiles((H, W), c, valid=v, net=net) == want, (kind, frac)
                dropped_some |= 0 < len(want) < len(infos)
                if kind == "all":
                    assert want == infos
                if kind == "none":
                    assert want == []
                if kind == "pixel_mid":
                    assert len(want) == (0 if f > 0 else int((counts > 0).sum())) and (f > 0 or len(want) >= 1)
        assert dropped_some
    np.testing.assert_array_equal(select_tiles([0, 1, 16384, 4096, 4095], 128, 0.25), [2, 3])
    np.testing.assert_array_equal(select_tiles([0, 1, 16384], 128, 0.0), [1, 2])
    np.testing.assert_array_equal(select_tiles([16383, 16384], 128, 1.0), [1])
    with pytest.raises(ValueError):
        select_tiles([5, -1], 128, 0.0)
    with pytest.raises(ValueError, match="net"):
        scene_tiles((H, W), Config(cfg), valid=np.ones((H, W), bool))


def test_arguments_are_refused_before_the_model_is_touched():
    class Untouchable(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.w = torch.nn.Parameter(torch.zeros(1))

        def __getattr__(self, name):
            if name.startswith("scene_") or name.startswith("infer_"):
                raise AssertionError(f"the model was touched: {name}")
            return super().__getattr__(name)

    net = Untouchable()
    H, W = 384, 640
    img = np.zeros((H, W, 3), np.uint8)
    ok = np.ones((H, W), bool)
    cfg = dict(_CFG, SAMPLE_MARGIN=0, INFER_PATCHES_PER_EDGE=[3, 5])
    bad = [(ok[:, :639], {}, "shape"), (ok.T, {}, "shape"), (ok[None], {}, "shape"), (ok.astype(np.float32), {}, "dtype"),
           (ok.astype(np.int32), {}, "dtype"), (ok.astype(np.int8), {}, "dtype"),
           (ok, dict(MIN_VALID_FRACTION=-0.1), "MIN_VALID_FRACTION"), (ok, dict(MIN_VALID_FRACTION=1.5), "MIN_VALID_FRACTION"),
           (ok, dict(MIN_VALID_FRACTION="half"), "MIN_VALID_FRACTION"), (ok, dict(MIN_VALID_FRACTION=True), "MIN_VALID_FRACTION"),
           (ok, dict(MIN_VALID_FRACTION=float("nan")), "MIN_VALID_FRACTION"),
           (ok, dict(NODATA_FILL=[1, 2]), "NODATA_FILL"), (ok, dict(NODATA_FILL=[1, 2, 256]), "NODATA_FILL"),
           (ok, dict(NODATA_FILL=[1, -2, 3]), "NODATA_FILL"), (ok, dict(NODATA_FILL=[1.0, 2, 3]), "NODATA_FILL"),
           (ok, dict(NODATA_FILL=7), "NODATA_FILL"), (ok, dict(NODATA_FILL="124,116,104"), "NODATA_FILL")]
    for valid, extra, what in bad:
        c = Config(dict(cfg, **extra))
        with pytest.raises(ValueError, match=what):
            infer_one_img(net, img, c, device="cpu", valid=valid)
        with pytest.raises(ValueError, match=what):
            list(infer_imgs(net, [img], c, device="cpu", valids=[valid]))
        with pytest.raises(ValueError, match=what):
            list(infer_imgs(net, [img], c, device="cpu", valids=[valid], tile_sharded=True, pipelined=True))
        with pytest.raises(ValueError, match=what):
            scene_tiles(img.shape, c, valid=valid, net=net)


# ---- the pipeline on the stand-in ----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def standin():
    warnings.simplefilter("ignore")
    cfg = dict(_CFG, SAMPLE_MARGIN=0, INFER_PATCHES_PER_EDGE=[3, 5])
    return SceneStandIn(cfg, ("valid",)), cfg


def test_masked_scene_on_the_standin(standin):
    """valid=None calls scene_normalise without a `valid` argument and none of the mask methods; an all-true mask gives the same
    tuple; a masked run runs the kept tiles only, leaves the caller's array alone, predicts nothing on nodata and does not depend on
    what lies under nodata; NODATA_FILL reaches the fill; the three loops agree."""
    net, cfg = standin
    H, W = 384, 640
    img = _rect_scene(H, W, 60)
    net.calls.clear()
    plain = infer_one_img(net, img, Config(cfg), device="cpu")
    assert net.calls == [("pass1", 15)]
    base = SceneStandIn(cfg)                                  # the stand-in without the feature: scene_normalise has no `valid`
    _same_tuple(infer_one_img(base, img, Config(cfg), device="cpu"), plain)
    _same_tuple(infer_one_img(net, img, Config(cfg), device="cpu", valid=np.ones((H, W), bool)), plain)
    band = make_mask("band", H, W)
    infos = get_patch_info_hw(0, H, W, 0, 128, [3, 5])
    n_kept = sum(bool(band[y0:y1, x0:x1].any()) for _, (x0, y0), (x1, y1) in infos)
    assert 0 < n_kept < 15
    before = img.copy()
    net.calls.clear()
    got = infer_one_img(net, img, Config(dict(cfg, NODATA_FILL=[1, 2, 3])), device="cpu", valid=band)
    assert net.calls == [("tile_valid", 15), ("fill", (1, 2, 3)), ("pass1", n_kept)]
    np.testing.assert_array_equal(img, before)
    got = infer_one_img(net, img, Config(cfg), device="cpu", valid=band)
    nodes, edges, kp, road = got
    assert nodes.shape[0] > 30 and edges.shape[0] > 100
    assert band[nodes[:, 0], nodes[:, 1]].all() and not kp[~band].any() and not road[~band].any()
    noise = img.copy()
    noise[~band] = 255 - noise[~band]
    _same_tuple(infer_one_img(net, noise, Config(cfg), device="cpu", valid=band.astype(np.uint8) * 7), got)
    # the loops: mixed list, entries None, an all-false scene in the middle
    imgs = [img, _rect_scene(640, 384, 61), img, _rect_scene(401, 523, 62)]
    valids = [band, None, np.zeros((H, W), bool), make_mask("hole", 401, 523)]
    want = [infer_one_img(net, im, Config(dict(cfg, INFER_PATCHES_PER_EDGE=4 if im.shape[0] == 401 else cfg["INFER_PATCHES_PER_EDGE"] if im.shape[0] == 384 else [5, 3])),
                          device="cpu", valid=v) for im, v in zip(imgs, valids)]
    assert want[2][0].shape == (0, 2) and want[2][1].shape == (0, 2) and not want[2][2].any() and want[2][2].shape == (H, W)
    same_grid = [0, 2]                                        # the scenes one config tiles as 3 x 5
    for kw in (dict(), dict(tile_sharded=True), dict(tile_sharded=True, pipelined=True)):
        out = list(infer_imgs(net, iter([imgs[i] for i in same_grid]), Config(cfg), device="cpu", valids=iter([valids[i] for i in same_grid]), **kw))
        for i, o in zip(same_grid, out):
            _same_tuple(o, want[i])


# ---- C ABI surface ------------------------------------------------------------------------------------------------------------------
def test_abi_symbol_tables_agree_and_number_is_11():
    assert_abi_11((("srh_scene_tile_valid", 9), ("srh_scene_fill_invalid", 9), ("srh_scene_normalise_valid_hw", 12)))
    assert len(_lib.SYMBOLS["srh_scene_normalise_valid_hw"][1]) == len(_lib.SYMBOLS["srh_scene_normalise_hw"][1]) + 1


# ---- tile-sharded loops on gloo -------------------------------------------------------------------------------------------------------
def _spec(shapes, kinds, overrides, mode):
    """The masked stand-in; in the pipelined runs the serial tile-sharded loop of infer_imgs is checked against infer_one_img too."""
    return dict(features=("valid",), shapes=shapes, kinds=kinds, overrides=overrides, mode=mode, checks=("serial_loop",))


@pytest.mark.parametrize("overrides,must_be_identical", [
    (dict(SAMPLE_MARGIN=0, INFER_PATCHES_PER_EDGE=[3, 5]), True),    # 3 x 5 disjoint tiles, 13 kept under the band
    (dict(INFER_PATCHES_PER_EDGE=[4, 6]), False),                    # overlapping tiles
])
def test_serial_tile_sharded_world3_masked(overrides, must_be_identical):
    shapes, kinds = [(384, 640), (384, 640), (384, 640)], ["band", "none", "left"]
    res = run_worlds((1, 3), _spec(shapes, kinds, overrides, "serial"))
    compare_worlds(res[1], res[3], shapes, kinds, must_be_identical)


def test_pipelined_tile_sharded_world2_masked():
    """The pipelined tile-sharded loop on two ranks over masked, unmasked and empty scenes of three shapes: equal to the serial
    tile-sharded loop of the same world exactly (checked inside the ranks), and to the single-process run."""
    shapes = [(384, 640), (640, 384), (401, 523), (384, 640), (448, 448)]
    kinds = ["band", None, "none", "left", "hole"]
    res = run_worlds((1, 2), _spec(shapes, kinds, None, "pipelined"))
    compare_worlds(res[1], res[2], shapes, kinds, False)


# ---- CLI ----------------------------------------------------------------------------------------------------------------------------
def test_cli_valid_masks_and_rgba(tmp_path, monkeypatch, standin):
    from PIL import Image
    import sam_road_amd.inferencer as inf
    from sam_road_amd import cli
    net, cfg = standin
    H, W = 384, 640
    img = _rect_scene(H, W, 60)
    band, left = make_mask("band", H, W), make_mask("left", H, W)
    monkeypatch.chdir(tmp_path)
    Image.fromarray(img).save("rgb.png")
    np.save("scene.npy", img)
    Image.fromarray(np.dstack([img, band.astype(np.uint8) * 255])).save("rgba.png")
    Image.fromarray(left.astype(np.uint8) * 255).save("left.png")
    np.save("band.npy", band)
    np.testing.assert_array_equal(inf.read_rgb_img("rgba.png"), img)             # read_rgb_img still drops alpha
    np.testing.assert_array_equal(inf.read_alpha_valid("rgba.png"), band)
    assert inf.read_alpha_valid("rgb.png") is None
    np.testing.assert_array_equal(inf.read_valid_mask("left.png"), left)
    pal = Image.fromarray(np.where(left, 1, 0).astype(np.uint8), mode="P")       # a palette PNG whose entry 0 is transparent (tRNS)
    pal.putpalette([0, 0, 0, 200, 100, 50] + [0] * 762)
    pal.save("pal.png", transparency=0)
    assert inf.has_alpha("pal.png") and inf.has_alpha("rgba.png") and not inf.has_alpha("rgb.png") and not inf.has_alpha("scene.npy")
    np.testing.assert_array_equal(inf.read_alpha_valid("pal.png"), left)

    def run(name, images, *argv):
        return run_cli(cli, net, tmp_path, monkeypatch, name, cfg, images, *argv)

    want = {k: infer_one_img(net, img, Config(cfg), device="cpu", valid=v) for k, v in (("plain", None), ("band", band), ("left", left))}
    from sam_road_amd.formats import convert_to_sat2graph_format
    graph = lambda r: convert_to_sat2graph_format(r[0], r[1])

    def check(got, key):
        itsc, road, g, _ = got
        np.testing.assert_array_equal(itsc, want[key][2])
        np.testing.assert_array_equal(road, want[key][3])
        assert g == graph(want[key])

    # explicit mask files, parallel to --images; '-' = no mask
    out = run("a", ["rgb.png", "scene.npy", "rgba.png"], "--valid-masks", "left.png", "band.npy", "-")
    check(out["rgb"], "left")
    check(out["scene"], "band")
    check(out["rgba"], "plain")                               # mask files were given: the alpha channel is not consulted
    # no mask files: an RGBA file uses alpha > 0, an RGB file has no mask
    out = run("b", ["rgba.png", "rgb.png"])
    check(out["rgba"], "band")
    check(out["rgb"], "plain")
    assert not out["rgba"][0][~band].any() and not out["rgba"][1][~band].any()
    with pytest.raises(SystemExit):
        inf.main(["--config", "a.yaml", "--checkpoint", "none", "--device", "cpu", "--output_dir", "c", "--images", "rgb.png", "--valid-masks"])
    with pytest.raises(SystemExit):
        inf.main(["--config", "a.yaml", "--checkpoint", "none", "--device", "cpu", "--output_dir", "d", "--valid-masks", "left.png"])
