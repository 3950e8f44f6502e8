"""FUSE_WINDOW (window-weighted fusion of overlapping tiles), the GPU-free part: the profiles against their formulas, the
argument errors, the C-ABI surface, the orchestration of the three loops and of the tile-sharded loops on gloo / CPU, and the CLI —
through scene_pass1(window=) / scene_normalise(window=) of the CPU stand-in of tests/scene_kit.py (features "valid", "window").
Everything multi-rank here runs on gloo / CPU only."""
import os
import re
import shutil
import subprocess
import warnings

import numpy as np
import pytest
import torch

from sam_road_amd import Config, _lib
from sam_road_amd import cli
from sam_road_amd import inferencer as inf
from sam_road_amd.inferencer import infer_imgs, infer_one_img

from scene_kit import HOST_CFG as _CFG
from scene_kit import SceneStandIn, assert_abi_11, compare_worlds, make_mask, run_cli, run_worlds
from scene_kit import rect_scene as _rect_scene
from scene_kit import same_tuple as _same_tuple

SIZES = (128, 208, 512, 1024)


def test_fuse_window_is_public():
    assert callable(inf.fuse_window) and inf.FUSE_WINDOW_NAMES == ("uniform", "hann", "triangle")


# ---- the profiles -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P", SIZES)
def test_profiles_match_their_formulas(P):
    cfg = lambda v: Config(dict(PATCH_SIZE=P, FUSE_WINDOW=v))
    for absent in (Config(dict(PATCH_SIZE=P)), cfg(None), cfg("uniform"), cfg(" Uniform ")):
        assert inf.fuse_window(absent) is None
    i = np.arange(P, dtype=np.float64)
    want = {"hann": np.sin(np.pi * (i + 0.5) / P) ** 2, "triangle": np.minimum(i + 0.5, P - i - 0.5) * 2 / P}
    for name, w64 in want.items():
        w = inf.fuse_window(cfg(name))
        assert isinstance(w, np.ndarray) and w.dtype == np.float32 and w.shape == (P,) and w.flags.c_contiguous
        np.testing.assert_array_equal(w, w64.astype(np.float32))              # float64 on the host, rounded once
        np.testing.assert_array_equal(w, w[::-1])                              # symmetric
        assert (w > 0).all() and w.min() >= 2.0 ** -20 and w.max() <= 1.0      # strictly positive, inside the range
        assert w.argmax() in (P // 2 - 1, P // 2) and (np.diff(w[:P // 2]) > 0).all()
        np.testing.assert_array_equal(inf.fuse_window(cfg(name.upper())), w)
    assert want["hann"].min() > 2.0 ** -20                                     # 2.35e-6 at P = 1024
    # a sequence is taken as given (list, tuple, array; ints too), rounded once to f32
    rng = np.random.default_rng(P)
    seq = rng.uniform(0.01, 1.0, size=P)
    for v in (seq, seq.tolist(), tuple(seq.tolist()), seq.astype(np.float32)):
        np.testing.assert_array_equal(inf.fuse_window(cfg(v)), np.asarray(v).astype(np.float32))
    np.testing.assert_array_equal(inf.fuse_window(cfg([1] * P)), np.ones(P, np.float32))
    edge = np.full(P, 1.0)
    edge[0], edge[-1] = 2.0 ** -20, 2.0 ** 20                                   # both ends of the range are allowed
    np.testing.assert_array_equal(inf.fuse_window(cfg(edge)), edge.astype(np.float32))


def _bad_windows(P):
    ok = np.full(P, 0.5)

    def with_value(v):
        a = ok.copy()
        a[P // 3] = v
        return a
    return [("gauss", "one of"), ("", "one of"), (7, "one of"), (0.5, "one of"), (True, "one of"), ({"name": "hann"}, "one of"),
            (ok[:-1], "exactly"), (np.append(ok, 0.5), "exactly"), ([], "exactly"), (ok.reshape(2, -1), "exactly"), ([0.5], "exactly"),
            (with_value(0.0), "inside"), (with_value(-0.5), "inside"), (with_value(np.nan), "inside"), (with_value(np.inf), "inside"),
            (with_value(-np.inf), "inside"), (with_value(2.0 ** -21), "inside"), (with_value(2.0 ** 21), "inside"),
            (with_value(1e300), "inside"), (["a"] * P, "numbers"), ([None] * P, "numbers"), ([True] * P, "numbers")]


@pytest.mark.parametrize("P", SIZES)
def test_every_bad_window_is_a_value_error(P):
    for v, what in _bad_windows(P):
        with pytest.raises(ValueError, match=what):
            inf.fuse_window(Config(dict(PATCH_SIZE=P, FUSE_WINDOW=v)))
    with pytest.raises(ValueError, match="exactly"):                           # a profile made for another tile size
        inf.fuse_window(Config(dict(PATCH_SIZE=P, FUSE_WINDOW=[0.5] * (P + 16))))


def test_bad_windows_are_refused_before_the_model_is_touched():
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
    cfg = dict(_CFG, SAMPLE_MARGIN=0, INFER_PATCHES_PER_EDGE=[3, 5])
    for v, what in _bad_windows(128):
        c = Config(dict(cfg, FUSE_WINDOW=v))
        with pytest.raises(ValueError, match=what):
            infer_one_img(net, img, c, device="cpu")
        with pytest.raises(ValueError, match=what):
            infer_one_img(net, img, c, device="cpu", valid=np.ones((H, W), bool))
        with pytest.raises(ValueError, match=what):
            list(infer_imgs(net, [img], c, device="cpu"))
        with pytest.raises(ValueError, match=what):
            list(infer_imgs(net, [img], c, device="cpu", tile_sharded=True))
        with pytest.raises(ValueError, match=what):
            list(infer_imgs(net, [img], c, device="cpu", tile_sharded=True, pipelined=True))


# ---- the pipeline on a stand-in ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def standin():
    warnings.simplefilter("ignore")
    cfg = dict(_CFG, INFER_PATCHES_PER_EDGE=[4, 6])                            # overlapping tiles: the window changes the masks
    return SceneStandIn(cfg, ("valid", "window")), cfg


def _fused_f64(net, img, infos, w1, valid=None):
    """The rule restated in float64 on the stand-in's own per-tile scores: (kp, road) as float64 level values (ratio * 255), -1 = uncovered."""
    H, W = img.shape[:2]
    P = net.P
    w2 = np.outer(w1.astype(np.float64), w1.astype(np.float64))
    kp, road, ws = np.zeros((H, W)), np.zeros((H, W)), np.zeros((H, W))
    for _, (x0, y0), _ in infos:
        s, _ = net.oracle.infer_masks_and_img_features(torch.from_numpy(img[y0:y0 + P, x0:x0 + P]).float()[None])
        s = s[0].numpy().astype(np.float64)
        kp[y0:y0 + P, x0:x0 + P] += w2 * s[:, :, 0]
        road[y0:y0 + P, x0:x0 + P] += w2 * s[:, :, 1]
        ws[y0:y0 + P, x0:x0 + P] += w2
    on = ws > 0 if valid is None else (ws > 0) & valid
    out = [np.where(on, c / np.where(ws > 0, ws, 1.0) * 255.0, -1.0) for c in (kp, road)]
    return out[0], out[1]


def test_windowed_scene_on_the_standin(standin):
    net, cfg = standin
    H, W = 384, 640
    img = _rect_scene(H, W, 60)
    n_tiles = 24
    # uniform / None / absent: the calls of today, with the arguments of today (the base stand-in does not know `window`)
    base = SceneStandIn(cfg)
    plain = infer_one_img(base, img, Config(cfg), device="cpu")
    for v in ("uniform", None):
        _same_tuple(infer_one_img(base, img, Config(dict(cfg, FUSE_WINDOW=v)), device="cpu"), plain)
        _same_tuple(list(infer_imgs(base, [img], Config(dict(cfg, FUSE_WINDOW=v)), device="cpu"))[0], plain)
        _same_tuple(list(infer_imgs(base, [img], Config(dict(cfg, FUSE_WINDOW=v)), device="cpu", tile_sharded=True, pipelined=True))[0], plain)
    net.calls.clear()
    _same_tuple(infer_one_img(net, img, Config(dict(cfg, FUSE_WINDOW="uniform")), device="cpu"), plain)
    assert net.calls == [("pass1", n_tiles)]
    infos = inf.scene_tiles((H, W), Config(cfg))
    band = make_mask("band", H, W)
    kept = [p for p in infos if band[p[1][1]:p[2][1], p[1][0]:p[2][0]].any()]
    assert 0 < len(kept) < n_tiles
    rng = np.random.default_rng(5)
    for v in ("hann", "triangle", rng.uniform(0.01, 1.0, size=128).tolist()):
        c = Config(dict(cfg, FUSE_WINDOW=v))
        w1 = inf.fuse_window(c)
        net.calls.clear()
        got = infer_one_img(net, img, c, device="cpu")
        assert net.calls == [("pass1_window", n_tiles), ("normalise_window", n_tiles)]
        nodes, edges, kp, road = got
        assert nodes.shape[0] > 30 and edges.shape[0] > 100
        assert not np.array_equal(kp, plain[2]) and not np.array_equal(road, plain[3])       # the window changes the masks
        for mask, lv in zip((kp, road), _fused_f64(net, img, infos, w1)):
            assert not mask[lv < 0].any()
            d = np.abs(mask[lv >= 0].astype(np.float64) - np.floor(lv[lv >= 0]))
            assert d.max() <= 1 and (d == 0).mean() > 0.98
        # nodata composes: selection and fill first, the window on the kept list
        net.calls.clear()
        gm = infer_one_img(net, img, c, device="cpu", valid=band)
        assert net.calls == [("tile_valid", n_tiles), ("fill", (124, 116, 104)), ("pass1_window", len(kept)), ("normalise_window", len(kept))]
        assert not gm[2][~band].any() and not gm[3][~band].any() and band[gm[0][:, 0], gm[0][:, 1]].all()
        filled = np.where(band[..., None], img, np.array((124, 116, 104), np.uint8))
        for mask, lv in zip(gm[2:], _fused_f64(net, filled, kept, w1, valid=band)):
            assert not mask[lv < 0].any()
            assert np.abs(mask[lv >= 0].astype(np.float64) - np.floor(lv[lv >= 0])).max() <= 1
        # the three loops agree with infer_one_img (world 1)
        if v != "hann":
            continue
        for kw in (dict(), dict(tile_sharded=True), dict(tile_sharded=True, pipelined=True)):
            out = list(infer_imgs(net, iter([img, img]), c, device="cpu", valids=iter([None, band]), **kw))
            _same_tuple(out[0], got)
            _same_tuple(out[1], gm)


# ---- C ABI surface ------------------------------------------------------------------------------------------------------------------
def test_abi_has_the_window_entries_and_stays_11():
    assert_abi_11((("srh_scene_pass1_window_hw", 13), ("srh_scene_normalise_window_hw", 13), ("srh_op_scene_fuse_window", 11)))
    assert len(_lib.SYMBOLS["srh_scene_pass1_window_hw"][1]) == len(_lib.SYMBOLS["srh_scene_pass1_hw"][1]) + 1
    assert len(_lib.SYMBOLS["srh_scene_normalise_window_hw"][1]) == len(_lib.SYMBOLS["srh_scene_normalise_valid_hw"][1]) + 1


def test_window_kernels_compile_for_gfx950_without_a_gpu():
    hipcc = next((c for c in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", shutil.which("hipcc")) if c and os.path.exists(c)), None)
    if hipcc is None:
        pytest.skip("hipcc not found")
    from sam_road_amd import build
    assert "scene_window.hip" in build.SOURCES
    r = subprocess.run([hipcc, *build.FLAGS, "-S", "--cuda-device-only", os.path.join(build.CSRC, "scene_window.hip"), "-o", "-"],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    for kernel in ("scene_add_window_kernel", "scene_norm_window_kernelILb0E", "scene_norm_window_kernelILb1E"):
        m = re.search(r"^(_Z\w*" + re.escape(kernel) + r"\w*):", r.stdout, re.M)
        assert m, kernel
        body = r.stdout[m.start():r.stdout.index(".Lfunc_end", m.start())]
        assert "scratch_" not in body and "global_atomic" not in body          # no spill, no atomics: a fixed summation order


# ---- tile-sharded loops on gloo ---------------------------------------------------------------------------------------------------------
def _spec(shapes, kinds, overrides, mode):
    """The windowed stand-in; every rank checks that each pass 1 was the weighted one and that rank 0 alone normalises."""
    return dict(features=("valid", "window"), shapes=shapes, kinds=kinds, overrides=overrides, mode=mode, checks=("window_calls",))


@pytest.mark.parametrize("overrides,must_be_identical", [
    (dict(SAMPLE_MARGIN=0, INFER_PATCHES_PER_EDGE=[3, 5], FUSE_WINDOW="hann"), True),     # disjoint tiles: one addend per pixel
    (dict(INFER_PATCHES_PER_EDGE=[4, 6], FUSE_WINDOW="triangle"), False),                 # overlapping tiles
])
def test_serial_tile_sharded_world3_with_a_window(overrides, must_be_identical):
    """World 3 against one process, with the identity conditions of tests/test_valid_mask_host.py: a disjoint tiling is identical; with
    overlapping tiles the ranks' f32 partial sums are associated differently, so a u8 may differ by one level."""
    shapes, kinds = [(384, 640), (384, 640), (384, 640)], [None, "band", "left"]
    res = run_worlds((1, 3), _spec(shapes, kinds, overrides, "serial"))
    compare_worlds(res[1], res[3], shapes, kinds, must_be_identical)


def test_pipelined_tile_sharded_world2_with_a_window():
    shapes = [(384, 640), (640, 384), (401, 523), (448, 448)]
    kinds = ["band", None, "none", "hole"]
    res = run_worlds((1, 2), _spec(shapes, kinds, dict(FUSE_WINDOW="hann"), "pipelined"))
    compare_worlds(res[1], res[2], shapes, kinds, False)


# ---- CLI ------------------------------------------------------------------------------------------------------------------------------
def test_cli_takes_the_key_and_the_flag(tmp_path, monkeypatch, standin):
    import yaml
    from PIL import Image
    from sam_road_amd.formats import convert_to_sat2graph_format
    net, cfg = standin
    img = _rect_scene(384, 640, 60)
    monkeypatch.chdir(tmp_path)
    Image.fromarray(img).save("rgb.png")
    plain, hann = cfg, dict(cfg, FUSE_WINDOW="hann")

    def run(name, config, *argv):
        return run_cli(cli, net, tmp_path, monkeypatch, name, config, ["rgb.png"], *argv)["rgb"]

    want = {k: infer_one_img(net, img, Config(dict(cfg, **({} if k == "uniform" else dict(FUSE_WINDOW=k)))), device="cpu")
            for k in ("uniform", "hann", "triangle")}
    assert not np.array_equal(want["hann"][3], want["triangle"][3]) and not np.array_equal(want["hann"][3], want["uniform"][3])

    def check(got, key):
        np.testing.assert_array_equal(got[0], want[key][2])
        np.testing.assert_array_equal(got[1], want[key][3])
        assert got[2] == convert_to_sat2graph_format(want[key][0], want[key][1])

    check(run("a", plain), "uniform")
    check(run("b", hann), "hann")                                        # the key comes from the YAML
    got = run("c", plain, "--fuse-window", "triangle")                  # the flag sets it
    check(got, "triangle")
    assert got[3]["FUSE_WINDOW"] == "triangle"
    check(run("d", hann, "--fuse-window", "uniform"), "uniform")        # and overrides the YAML
    with pytest.raises(SystemExit):
        inf.main(["--config", "a.yaml", "--checkpoint", "none", "--device", "cpu", "--output_dir", "e", "--images", "rgb.png",
                  "--fuse-window", "gauss"])
    with open("bad.yaml", "w") as f:
        yaml.safe_dump(dict(cfg, DATASET="cityscale", FUSE_WINDOW="gauss"), f)
    monkeypatch.setattr(cli, "_build_net", lambda *a: (_ for _ in ()).throw(AssertionError("the model was built")))
    with pytest.raises(ValueError, match="one of"):
        inf.main(["--config", "bad.yaml", "--checkpoint", "none", "--device", "cpu", "--output_dir", "f", "--images", "rgb.png"])
