"""TTA (test-time augmentation over the 8 tile orientations), the GPU-free part: the plan and its errors, the host
orientation helpers against the numpy table, the C-ABI surface, the CLI, scene_tiles, and the orchestration of the three scene loops
through scene_pass1(tta=) of the CPU stand-in of tests/scene_kit.py (features "valid", "window", "tta")."""
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
from sam_road_amd.inferencer import infer_imgs, infer_one_img, orient_tile, tta_plan, unorient_tile

from scene_kit import HOST_CFG as _CFG
from scene_kit import NAMES, SceneStandIn, assert_abi_11, make_mask, run_cli
from scene_kit import ORIENT as TABLE      # the table of DESIGN.md §6f, restated: those expressions ARE the definition
from scene_kit import rect_scene as _rect_scene
from scene_kit import same_tuple as _same_tuple


# ---- the plan ---------------------------------------------------------------------------------------------------------------------
def test_tta_plan_names_codes_and_default():
    assert inf.TTA_NAMES == NAMES
    for absent in (Config({}), Config(dict(TTA=None))):
        assert tta_plan(absent) == (["id"], [0])
    assert tta_plan(Config(dict(TTA=["id"]))) == (["id"], [0])
    assert tta_plan(Config(dict(TTA=list(NAMES)))) == (list(NAMES), list(range(8)))
    assert tta_plan(Config(dict(TTA=("id", "rot90", "flip_v")))) == (["id", "rot90", "flip_v"], [0, 5, 2])
    assert tta_plan(Config(dict(TTA="id,flip_h, Rot90"))) == (["id", "flip_h", "rot90"], [0, 1, 5])      # the CLI's form
    for i, n in enumerate(NAMES[1:], 1):
        assert tta_plan(Config(dict(TTA=["id", n]))) == (["id", n], [0, i])


BAD = [(["flip_h", "id"], "first"), (["rot90"], "first"), (["id", "flip_h", "flip_h"], "twice"), (["id", "id"], "twice"),
       (["id", "rot45"], "one of"), (["id", 5], "one of"), (["id", None], "one of"), ("id,spin", "one of"), ("", "one of"),
       ([], "1 to 8"), (list(NAMES) + ["id"], "1 to 8"), (7, "sequence"), ({"a": 1}, "sequence"), (True, "sequence")]


def test_every_bad_tta_is_a_value_error_before_the_model_is_touched():
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
    for v, what in BAD:
        c = Config(dict(cfg, TTA=v))
        with pytest.raises(ValueError, match=what):
            tta_plan(c)
        with pytest.raises(ValueError, match=what):
            inf.scene_tiles((H, W), c)
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


# ---- the host helpers -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P", [16, 48, 208])
def test_orient_tile_is_the_table_and_unorient_is_its_inverse(P):
    rng = np.random.default_rng(P)
    T = rng.integers(0, 256, size=(P, P, 3), dtype=np.uint8)
    for A in (T, T[:, :, 0]):
        assert not np.array_equal(A, A.swapaxes(0, 1)) and not np.array_equal(A, A[::-1]) and not np.array_equal(A, A[:, ::-1])
    out = {}
    for name in NAMES:
        out[name] = np.ascontiguousarray(orient_tile(T, name))
        np.testing.assert_array_equal(out[name], TABLE[name](T))
        assert out[name].shape == T.shape and out[name].dtype == T.dtype
        np.testing.assert_array_equal(unorient_tile(orient_tile(T, name), name), T)
        np.testing.assert_array_equal(orient_tile(unorient_tile(T, name), name), T)
        S = rng.standard_normal((P, P, 2)).astype(np.float32)                   # a score tile, and a 2-D array
        np.testing.assert_array_equal(unorient_tile(orient_tile(S, name), name), S)
        np.testing.assert_array_equal(orient_tile(T[:, :, 1], name), TABLE[name](T[:, :, 1]))
    for i, a in enumerate(NAMES):                                               # the 8 results are pairwise different
        for b in NAMES[i + 1:]:
            assert not np.array_equal(out[a], out[b]), (a, b)
    # codes 0-4 and 7 are their own inverse, 5 and 6 each other's
    for name in NAMES:
        inv = {"rot90": "rot270", "rot270": "rot90"}.get(name, name)
        np.testing.assert_array_equal(orient_tile(orient_tile(T, name), inv), T)
    with pytest.raises(ValueError, match="one of"):
        orient_tile(T, "rot45")
    with pytest.raises(ValueError, match="square"):
        orient_tile(T[:, :-1], "flip_h")


# ---- scene_tiles ------------------------------------------------------------------------------------------------------------------
def test_scene_tiles_lists_the_orientations():
    H, W = 384, 640
    cfg = dict(_CFG, INFER_PATCHES_PER_EDGE=[3, 5])
    plain = inf.scene_tiles((H, W), Config(cfg))
    assert plain.orientations == ["id"] and isinstance(plain, list) and len(plain) == 15
    plan = inf.scene_tiles((H, W, 3), Config(dict(cfg, TTA=["id", "rot90", "flip_v"])))
    assert plan.orientations == ["id", "rot90", "flip_v"]
    assert plan == plain                                                        # the tiles are the same: every one runs once per orientation


# ---- C ABI surface ----------------------------------------------------------------------------------------------------------------
def test_abi_has_the_tta_entries_and_stays_11():
    assert_abi_11((("srh_scene_pass1_tta_hw", 15), ("srh_op_patch_im2col", 10), ("srh_op_scores_unorient", 7)))
    assert len(_lib.SYMBOLS["srh_scene_pass1_tta_hw"][1]) == len(_lib.SYMBOLS["srh_scene_pass1_window_hw"][1]) + 2


def test_tta_kernels_compile_for_gfx950_without_a_gpu():
    hipcc = next((c for c in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", shutil.which("hipcc")) if c and os.path.exists(c)), None)
    if hipcc is None:
        pytest.skip("hipcc not found")
    from sam_road_amd import build
    assert "scene_tta.hip" in build.SOURCES
    r = subprocess.run([hipcc, *build.FLAGS, "-S", "--cuda-device-only", os.path.join(build.CSRC, "scene_tta.hip"), "-o", "-"],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    for kernel, lds in (("patch_im2col_flip_kernel", False), ("patch_im2col_transpose_kernel", True),
                        ("scores_unorient_flip_kernel", False), ("scores_unorient_transpose_kernel", True)):
        m = re.search(r"^(_Z\w*" + re.escape(kernel) + r"\w*):", r.stdout, re.M)
        assert m, kernel
        body = r.stdout[m.start():r.stdout.index(".Lfunc_end", m.start())]
        assert "scratch_" not in body and "global_atomic" not in body          # no spill; a permutation has no atomics
        assert ("ds_read" in body or "ds_load" in body) == lds, kernel          # the axis-swapping codes go through the LDS, the flips do not


# ---- the pipeline on a stand-in ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def standin():
    warnings.simplefilter("ignore")
    cfg = dict(_CFG, INFER_PATCHES_PER_EDGE=[3, 5])
    return SceneStandIn(cfg, ("valid", "window", "tta")), cfg


def _mean_levels(net, img, infos, names):
    """The float64 mean over (orientation, tile) of the stand-in's own per-tile scores, as mask levels (x 255); -1 = uncovered."""
    H, W = img.shape[:2]
    P = net.P
    acc, cnt = np.zeros((2, H, W)), np.zeros((H, W))
    for name in names:
        for _, (x0, y0), _ in infos:
            crop = np.ascontiguousarray(orient_tile(img[y0:y0 + P, x0:x0 + P], name))
            s, _ = net.oracle.infer_masks_and_img_features(torch.from_numpy(crop).float()[None])
            s = unorient_tile(s[0].detach().numpy().astype(np.float64), name)
            acc[0, y0:y0 + P, x0:x0 + P] += s[:, :, 0]
            acc[1, y0:y0 + P, x0:x0 + P] += s[:, :, 1]
            cnt[y0:y0 + P, x0:x0 + P] += 1
    return [np.where(cnt > 0, a / np.maximum(cnt, 1) * 255.0, -1.0) for a in acc]


def test_tta_scene_on_the_standin(standin):
    net, cfg = standin
    H, W = 384, 640
    img = _rect_scene(H, W, 60)
    n = 15
    infos = list(inf.scene_tiles((H, W), Config(cfg)))
    # key absent / None / ['id']: the calls of today with the arguments of today
    net.calls.clear()
    plain = infer_one_img(net, img, Config(cfg), device="cpu")
    assert net.calls == [("pass1", n), ("normalise", n)]
    for v in (None, ["id"], "id"):
        net.calls.clear()
        _same_tuple(infer_one_img(net, img, Config(dict(cfg, TTA=v)), device="cpu"), plain)
        assert net.calls == [("pass1", n), ("normalise", n)]
    names = ["id", "rot90", "flip_h"]
    c = Config(dict(cfg, TTA=names))
    net.calls.clear()
    got = infer_one_img(net, img, c, device="cpu")
    assert net.calls == [("pass1_tta", n, (0, 5, 1), False), ("normalise", 3 * n)]      # normalise sees the 3-fold list
    nodes, edges, kp, road = got
    assert nodes.shape[0] > 30 and edges.shape[0] > 100
    assert not np.array_equal(kp, plain[2]) and not np.array_equal(road, plain[3])       # TTA changes the masks
    for mask, lv in zip((kp, road), _mean_levels(net, img, infos, names)):
        assert not mask[lv < 0].any()
        d = np.abs(mask[lv >= 0].astype(np.float64) - np.floor(lv[lv >= 0]))
        assert d.max() <= 1 and (d == 0).mean() > 0.98
    # nodata composes (selection and fill once, then every orientation on the kept list), and so does a window
    band = make_mask("band", H, W)
    kept = [p for p in infos if band[p[1][1]:p[2][1], p[1][0]:p[2][0]].any()]
    assert 0 < len(kept) < n
    net.calls.clear()
    gm = infer_one_img(net, img, c, device="cpu", valid=band)
    assert net.calls == [("tile_valid", n), ("fill", (124, 116, 104)), ("pass1_tta", len(kept), (0, 5, 1), False), ("normalise", 3 * len(kept))]
    assert not gm[2][~band].any() and not gm[3][~band].any() and band[gm[0][:, 0], gm[0][:, 1]].all()
    cw = Config(dict(c, FUSE_WINDOW="hann"))
    net.calls.clear()
    gw = infer_one_img(net, img, cw, device="cpu")
    assert net.calls == [("pass1_tta", n, (0, 5, 1), True), ("normalise", 3 * n), ("normalise_window", 3 * n)]
    assert not np.array_equal(gw[3], got[3])
    # the three loops agree with infer_one_img (world 1)
    for kw in (dict(), dict(tile_sharded=True), dict(tile_sharded=True, pipelined=True)):
        out = list(infer_imgs(net, iter([img, img]), c, device="cpu", valids=iter([None, band]), **kw))
        _same_tuple(out[0], got)
        _same_tuple(out[1], gm)
        _same_tuple(list(infer_imgs(net, [img], cw, device="cpu", **kw))[0], gw)


def test_the_four_entry_paths_make_the_same_calls(standin):
    """infer_one_img, infer_imgs, and the serial and the pipelined tile-sharded loop share one pass-1 front end: for every feature
    combination they call the model with the same arguments in the same order and return the same tuple."""
    net, cfg = standin
    H, W = 384, 640
    img = _rect_scene(H, W, 60)
    band = make_mask("band", H, W)
    n = 15
    kept = sum(bool(band[p[1][1]:p[2][1], p[1][0]:p[2][0]].any()) for p in inf.scene_tiles((H, W), Config(cfg)))
    combos = [(dict(), None, [("pass1", n), ("normalise", n)]),
              (dict(FUSE_WINDOW="hann"), band, [("tile_valid", n), ("fill", (124, 116, 104)), ("pass1_window", kept), ("normalise", kept),
                                                ("normalise_window", kept)]),
              (dict(FUSE_WINDOW="hann", TTA=["id", "rot90"]), band,
               [("tile_valid", n), ("fill", (124, 116, 104)), ("pass1_tta", kept, (0, 5), True), ("normalise", 2 * kept), ("normalise_window", 2 * kept)])]
    paths = [lambda c, v: infer_one_img(net, img, c, device="cpu", valid=v)]
    for kw in (dict(), dict(tile_sharded=True), dict(tile_sharded=True, pipelined=True)):
        paths.append(lambda c, v, kw=kw: list(infer_imgs(net, [img], c, device="cpu", valids=[v], **kw))[0])
    results = []
    for extra, valid, want_calls in combos:
        c = Config(dict(cfg, **extra))
        first = None
        for run in paths:
            net.calls.clear()
            got = run(c, valid)
            assert net.calls == want_calls
            if first is None:
                first = got
                assert got[0].shape[0] > 30 and got[1].shape[0] > 100
            else:
                _same_tuple(got, first)
        results.append(first)
    assert not np.array_equal(results[0][3], results[1][3]) and not np.array_equal(results[1][3], results[2][3])


# ---- CLI --------------------------------------------------------------------------------------------------------------------------
def test_cli_takes_the_key_and_the_flag(tmp_path, monkeypatch, standin):
    from PIL import Image
    from sam_road_amd.formats import convert_to_sat2graph_format
    net, cfg = standin
    img = _rect_scene(384, 640, 60)
    monkeypatch.chdir(tmp_path)
    Image.fromarray(img).save("rgb.png")
    plain, two = cfg, dict(cfg, TTA=["id", "flip_v"])

    def run(name, config, *argv):
        return run_cli(cli, net, tmp_path, monkeypatch, name, config, ["rgb.png"], *argv)["rgb"]

    want = {k: infer_one_img(net, img, Config(dict(cfg, **({} if k == "plain" else dict(TTA=k.split(","))))), device="cpu")
            for k in ("plain", "id,flip_v", "id,rot270")}
    assert not np.array_equal(want["id,flip_v"][3], want["plain"][3]) and not np.array_equal(want["id,flip_v"][3], want["id,rot270"][3])

    def check(got, key):
        np.testing.assert_array_equal(got[0], want[key][2])
        np.testing.assert_array_equal(got[1], want[key][3])
        assert got[2] == convert_to_sat2graph_format(want[key][0], want[key][1])

    check(run("a", plain), "plain")
    check(run("b", two), "id,flip_v")                                    # the key comes from the YAML
    got = run("c", plain, "--tta", "id,rot270")                          # the flag sets it
    check(got, "id,rot270")
    assert got[3]["TTA"] == ["id", "rot270"]
    check(run("d", two, "--tta", "id"), "plain")                         # and overrides the YAML
    monkeypatch.setattr(cli, "_build_net", lambda *a: (_ for _ in ()).throw(AssertionError("the model was built")))
    for bad, what in (("flip_h,id", "first"), ("id,spin", "one of"), ("id,id", "twice")):
        with pytest.raises(ValueError, match=what):
            inf.main(["--config", "a.yaml", "--checkpoint", "none", "--device", "cpu", "--output_dir", "e", "--images", "rgb.png", "--tta", bad])
