"""SCENE_NODATA without a GPU: the key and its refusals, the rule against an independent restatement in plain loops, the
kernels' own per-item code under the host sanitizers, the ABI, and the whole loop on the CPU stand-in — a run with the key must equal,
exactly, the same loop called with valid = nodata_ref(raw, key, valid)."""
import os
import re
import shutil
import subprocess
import warnings

import numpy as np
import pytest
import torch

from sam_road_amd import Config
from sam_road_amd import cli
from sam_road_amd import inferencer as inf
from sam_road_amd.inferencer import _empty_result, infer_imgs, infer_one_img, scene_tiles
from sam_road_amd.nodata import SceneNodata, grow_ref, nodata_ref, nodata_table, scene_nodata_check, scene_nodata_key, scene_nodata_override
from sam_road_amd.radiometry import band_luts, stretch_from_hist

import scene_nodata_kit as nk
from scene_kit import E2E_CFG, HOST_CFG, SCENES, SceneStandIn, assert_abi_11, free_port, rect_scene, run_cli, same_tuple

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _key(v):
    return scene_nodata_key(Config(SCENE_NODATA=v))


# ---- the key ------------------------------------------------------------------------------------------------------------------------------------
def test_key_every_accepted_form():
    assert scene_nodata_key(Config()) is None and _key(None) is None and _key({}) is None
    assert _key(0) == SceneNodata(0, 0, False, 1, 8, 0) == _key({"value": 0}) == _key({"value": np.int64(0)})
    assert _key([0, 0, 0]) == SceneNodata((0, 0, 0), 0, False, 1, 8, 0) == _key({"value": (0, 0, 0)})
    assert _key(65535).value == 65535 and _key([65535]).value == (65535,)
    full = _key({"value": [1, 2, 3, 4], "tolerance": 2, "match": "Any ", "min_area": 50, "connectivity": 4, "grow": 16})
    assert full == SceneNodata((1, 2, 3, 4), 2, True, 50, 4, 16)
    assert _key({"value": 7, "match": "all", "grow": 0, "min_area": 1, "connectivity": 8, "tolerance": 0}) == SceneNodata(7, 0, False, 1, 8, 0)
    # per scene: the ranges clamp at both ends of the dtype
    u8, u16 = np.zeros((2, 2, 3), np.uint8), np.zeros((2, 2, 4), np.uint16)
    assert scene_nodata_check(u8, _key({"value": [0, 254, 100], "tolerance": 3})) == ([0, 251, 97], [3, 255, 103])
    assert scene_nodata_check(u16, _key({"value": 65535, "tolerance": 70000})) == ([0] * 4, [65535] * 4)
    assert scene_nodata_check(u16, _key(300)) == ([300] * 4, [300] * 4)


BAD_KEYS = ("0", 1.5, True, {"valeu": 0}, {"value": 0, "area": 3}, {"tolerance": 1}, {"value": True}, {"value": 1.0}, {"value": "0"}, {"value": -1},
            {"value": 65536}, {"value": []}, {"value": [0] * 17}, {"value": [0, True, 0]}, {"value": [0, 0.5, 0]}, [0, -1, 0], {"value": 0, "tolerance": -1},
            {"value": 0, "tolerance": 1.0}, {"value": 0, "tolerance": True}, {"value": 0, "min_area": 0}, {"value": 0, "min_area": 2.0},
            {"value": 0, "min_area": True}, {"value": 0, "grow": -1}, {"value": 0, "grow": 17}, {"value": 0, "grow": 1.0}, {"value": 0, "grow": True},
            {"value": 0, "connectivity": 6}, {"value": 0, "connectivity": True}, {"value": 0, "connectivity": "8"}, {"value": 0, "match": "most"},
            {"value": 0, "match": 1}, {"value": 0, "match": None})


class _Untouchable(torch.nn.Module):
    """A model object nothing may be called on: a refusal must come before the device is touched."""

    def __init__(self):
        super().__init__()
        self.w = torch.nn.Parameter(torch.zeros(1))


def test_every_refusal_is_a_value_error_before_the_model_is_touched():
    net, img = _Untouchable(), rect_scene(300, 300, 1)
    for bad in BAD_KEYS:
        with pytest.raises(ValueError, match="SCENE_NODATA"):
            _key(bad)
        for call in (lambda cfg: infer_one_img(net, img, cfg, device="cpu"), lambda cfg: list(infer_imgs(net, iter([img]), cfg, device="cpu")),
                     lambda cfg: list(infer_imgs(net, iter([img]), cfg, device="cpu", group=2)), lambda cfg: scene_tiles(img.shape, cfg, net=net, img=img)):
            with pytest.raises(ValueError, match="SCENE_NODATA"):
                call(Config(dict(HOST_CFG, SCENE_NODATA=bad)))
    # per scene, where _scene_plan checks the scene: a value outside the dtype's range, a list that is not one per band
    u16 = np.zeros((300, 300, 4), np.uint16)
    bands = dict(select=[0, 1, 2])
    for scene, extra, bad in ((img, {}, 256), (img, {}, [0, 0]), (img, {}, [0, 0, 0, 0]), (img, {}, [0, 300, 0]), (u16, dict(SCENE_BANDS=bands), [0, 0, 0]),
                              (u16, dict(SCENE_BANDS=bands), [0] * 5)):
        cfg = Config(dict(HOST_CFG, SCENE_NODATA=bad, **extra))
        for call in (lambda: infer_one_img(net, scene, cfg, device="cpu"), lambda: list(infer_imgs(net, iter([scene]), cfg, device="cpu")),
                     lambda: list(infer_imgs(net, iter([scene, scene]), cfg, device="cpu", group=2)), lambda: scene_tiles(scene.shape[:2], cfg, net=net, img=scene)):
            with pytest.raises(ValueError, match="SCENE_NODATA"):
                call()
    # the area rule and a group beyond srh_mask_clean's image limit
    with pytest.raises(ValueError, match="SCENE_NODATA"):
        list(infer_imgs(net, iter([img]), Config(dict(HOST_CFG, SCENE_NODATA={"value": 0, "min_area": 2})), device="cpu", group=4097))
    # scene_tiles: with the key the plan depends on the pixels
    with pytest.raises(ValueError, match="depends on the pixels"):
        scene_tiles(img.shape, Config(dict(HOST_CFG, SCENE_NODATA=0)))
    with pytest.raises(ValueError, match="shape"):
        scene_tiles((200, 300), Config(dict(HOST_CFG, SCENE_NODATA=0)), net=net, img=img)
    assert len(scene_tiles(img.shape, Config(HOST_CFG))) == 25                   # without the key it is the call it was


def test_cli_flags_lay_over_the_key():
    base = Config(SCENE_NODATA={"value": [0, 0, 0], "tolerance": 2, "grow": 1})
    assert scene_nodata_override(base) == {"value": [0, 0, 0], "tolerance": 2, "grow": 1}
    assert scene_nodata_override(base, value=[255]) == {"value": 255, "tolerance": 2, "grow": 1}
    assert scene_nodata_override(base, value=[1, 2, 3], grow=4, match="any", min_area=9, tolerance=0) == \
        {"value": [1, 2, 3], "tolerance": 0, "grow": 4, "match": "any", "min_area": 9}
    assert scene_nodata_override(Config(), value=[0]) == {"value": 0} and scene_nodata_override(Config(SCENE_NODATA=7), grow=2) == {"value": 7, "grow": 2}
    with pytest.raises(ValueError, match="SCENE_NODATA"):
        scene_nodata_override(Config(SCENE_NODATA="x"), grow=2)
    with pytest.raises(ValueError, match="value is required"):
        _key(scene_nodata_override(Config(), grow=2))


# ---- the rule against an independent restatement ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,C", [(np.uint8, 3), (np.uint16, 4)])
def test_ref_equals_the_plain_loops(dtype, C):
    levels = 256 if dtype == np.uint8 else 65536
    rng = np.random.default_rng(C)
    n = 0
    for v in (0, levels - 1, 2):
        for t in (0, 2, 5):                               # v - t clamps at 0 and v + t at levels - 1
            for any_band in (False, True):
                for conn in (8, 4):
                    H, W = int(rng.integers(9, 30)), int(rng.integers(9, 30))
                    near = rng.integers(0, 7, size=(H, W, C)) if v < 8 else levels - 1 - rng.integers(0, 7, size=(H, W, C))
                    raw = near.astype(dtype)
                    raw[rng.random((H, W)) < 0.35] = v    # clumps of the value itself, so that the area rule has components of many sizes
                    value = v if (n & 1) else [v] * C
                    if isinstance(value, list) and v == 2:
                        value[0] = 4                      # per-band values
                    valid = (rng.random((H, W)) < 0.8) if (n & 2) else None
                    for min_area, grow in ((1, 0), (4, 0), (1, 2), (6, 1), (3, 16)):
                        key = _key({"value": value, "tolerance": t, "match": "any" if any_band else "all", "min_area": min_area, "connectivity": conn, "grow": grow})
                        got = nodata_ref(raw, key, valid)
                        want = nk.loops_ref(raw, value, t, any_band, min_area, conn, grow, valid)
                        assert got.dtype == np.uint8 and got.flags.c_contiguous and set(np.unique(got)) <= {0, 1}
                        np.testing.assert_array_equal(got, want, err_msg=str((v, t, any_band, conn, min_area, grow)))
                        n += 1
                        if (min_area, grow) == (4, 0) and not any_band and t == 0:
                            bare = nodata_ref(raw, key._replace(min_area=1), valid)
                            assert (got != bare).any() or v == 2       # the area rule clears something on these clumps
    assert n == 3 * 3 * 2 * 2 * 5
    # the grow alone, and the two statements of it
    s = (rng.random((40, 33)) < 0.01).astype(np.uint8) * 9
    for r in (1, 2, 16, 50):
        np.testing.assert_array_equal(grow_ref(s, r), nk.window_max(s, r))
    assert grow_ref(s, 0).tolist() == (s != 0).astype(np.uint8).tolist()


def test_the_kit_scenes_are_what_they_say():
    H, W, _, seed = SCENES["401x523"]
    img, painted = nk.collar_scene(H, W, seed)
    collar = nk.collar_of(H, W)
    fringe = nk.collar_of(H, W, shift=3) & ~collar
    assert (img[collar] == 0).all() and set(np.unique(img[fringe])) == {1, 2, 3} and (img[~painted & ~fringe] >= 8).all()
    from scipy import ndimage
    labels, n = ndimage.label(painted & ~collar, structure=np.ones((3, 3)))
    areas = sorted(np.bincount(labels.ravel())[1:].tolist())
    assert areas == [1] * nk.N_SINGLES + [5, 12, 25, 40]
    width = fringe.sum(1)[:100]
    assert 2 <= width.min() and width.max() <= 8          # 2-3 px measured across the collar's edge (more along a row of a slanted edge)
    raw, painted16 = nk.raw16_scene(H, W, seed)
    assert raw.dtype == np.uint16 and raw.shape == (H, W, 4) and (raw[painted16] == 65535).all() and (raw[~painted16] < 65535).all()
    assert nodata_ref(nk.plain_scene(H, W, seed), _key({"value": 0, "tolerance": 3})).all()


# ---- the kernels' own code, on the CPU ----------------------------------------------------------------------------------------------------------
def test_kernel_addressing_on_the_cpu(tmp_path):
    """tests/scene_nodata_check.cpp runs every item of whole match and grow launches through the kernels' own per-item code
    (csrc/scene_nodata_piece.hpp) as a stand-alone host program built with the address and undefined-behaviour sanitizers, against a
    second plain restatement: the source at every 16-byte misalignment, source / destination / LDS stand-ins heap blocks of their exact
    sizes.  A byte read or written outside them ends it."""
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    cxx = next((c for c in (os.path.join(rocm, "llvm", "bin", "clang++"), os.path.join(rocm, "lib", "llvm", "bin", "clang++")) if os.path.exists(c)), None)
    if cxx is None:
        pytest.skip("no ROCm clang++")
    exe = str(tmp_path / "scene_nodata_check")
    csrc = os.path.join(ROOT, "sam_road_amd", "csrc")
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", csrc,
                        os.path.join(ROOT, "tests", "scene_nodata_check.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    assert "scene nodata OK" in r.stdout


def test_kernels_compile_for_gfx950_without_a_gpu():
    hipcc = next((c for c in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", shutil.which("hipcc")) if c and os.path.exists(c)), None)
    if hipcc is None:
        pytest.skip("hipcc not found")
    from sam_road_amd import build
    assert "scene_nodata.hip" in build.SOURCES
    r = subprocess.run([hipcc, *build.FLAGS, "-S", "--cuda-device-only", os.path.join(build.CSRC, "scene_nodata.hip"), "-o", "-"],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    for name, lds in (("scene_nodata_match_kernelIhE", 0), ("scene_nodata_match_kernelItE", 0), ("scene_nodata_grow_kernel", 15360)):
        m = re.search(r"^(_Z\w*%s\w*):" % name, r.stdout, re.M)
        assert m, f"{name} is not in the code object"
        meta = r.stdout[r.stdout.index(".amdhsa_kernel " + m.group(1)):]
        meta = meta[:meta.index(".end_amdhsa_kernel")]
        assert int(re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", meta).group(1)) == 0          # no scratch
        assert int(re.search(r"\.amdhsa_group_segment_fixed_size (\d+)", meta).group(1)) == lds
        assert int(re.search(r"\.amdhsa_uses_dynamic_stack (\d+)", meta).group(1)) == 0
        body = r.stdout[r.stdout.index(m.group(1) + ":"):r.stdout.index(".amdhsa_kernel " + m.group(1))]
        assert "atomic" not in body
        if lds == 0:
            assert "global_load_dwordx4" in body and "ds_" not in body       # 16-byte loads, no LDS


# ---- C ABI surface --------------------------------------------------------------------------------------------------------------------------------
def test_abi_has_the_two_entries_and_stays_11():
    header, lib = assert_abi_11((("srh_scene_nodata_match", 12), ("srh_scene_nodata_grow", 11)))
    assert "SCENE_NODATA" in header
    # refused without a context, before anything is launched
    assert lib.srh_scene_nodata_match(None, None, 2, 4, 3, None, None, 0, None, 0, None, None) == -1
    assert lib.srh_scene_nodata_grow(None, None, None, 16, None, None, 1, 2, None, 0, None) == -1


# ---- the whole loop on the CPU stand-in -------------------------------------------------------------------------------------------------------------
H, W, PER_EDGE, SEED = SCENES["401x523"]
CFG = dict(HOST_CFG, INFER_PATCHES_PER_EDGE=PER_EDGE)
FULL = dict(value=0, tolerance=3, min_area=50, grow=2)
_NETS = {}


def standin(*features):
    warnings.simplefilter("ignore")
    torch.set_num_threads(4)
    if features not in _NETS:
        _NETS[features] = nk.NodataStandIn(dict(CFG), features)
    _NETS[features].calls.clear()
    return _NETS[features]


def _run(net, img, cfg, **kw):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return infer_one_img(net, img, Config(cfg), device="cpu", **kw)


def _loop(net, imgs, cfg, **kw):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return list(infer_imgs(net, iter(imgs), Config(cfg), device="cpu", **kw))


@pytest.fixture(scope="module")
def collar():
    return nk.collar_scene(H, W, SEED)


def test_infer_one_img_equals_the_composition(collar):
    img, painted = collar
    net = standin("valid")
    plain = _run(net, img, CFG)
    assert not nk.nodata_calls(net)                                              # with the key absent the new methods are never called
    for kw in (FULL, dict(value=0), 0, dict(value=[0, 0, 0], tolerance=3, match="any"), dict(value=0, min_area=13), dict(value=0, grow=1)):
        key = _key(kw)
        valid = nodata_ref(img, key)
        want = _run(net, img, CFG, valid=valid)
        net.calls.clear()
        got = _run(net, img, dict(CFG, SCENE_NODATA=kw))
        same_tuple(got, want)
        assert not got[2][valid == 0].any() and not got[3][valid == 0].any() and got[3].any() and (got[3] != plain[3]).any()
        names = [c[0] for c in net.calls if c[0] in ("nodata_match", "mask_clean", "nodata_grow")]
        if key.min_area == 1 and key.grow == 0:
            assert names == ["nodata_match"] and net.calls[0][-1] is True        # ONE call, and it writes the finished mask (invert)
        else:
            assert names == ["nodata_match"] + ["mask_clean"] * (key.min_area > 1) + (["nodata_grow"] if key.grow else ["nodata_match"])
    # a caller's mask is ANDed in: the last step takes it
    caller = np.ones((H, W), bool)
    caller[250:, 300:] = False
    net.calls.clear()
    got = _run(net, img, dict(CFG, SCENE_NODATA=FULL), valid=caller)
    same_tuple(got, _run(net, img, CFG, valid=nodata_ref(img, _key(FULL), caller)))
    assert [c for c in net.calls if c[0] == "nodata_grow"][0][3] is True and not got[3][250:, 300:].any() and got[3].any()
    # the plan of scene_tiles is the run's
    frac = dict(CFG, MIN_VALID_FRACTION=0.9, SCENE_NODATA=FULL)
    tiles = scene_tiles(img.shape, Config(frac), net=net, img=img)
    assert list(tiles) == list(scene_tiles(img.shape, Config(dict(CFG, MIN_VALID_FRACTION=0.9)), valid=nodata_ref(img, _key(FULL)), net=net))
    assert 0 < len(tiles) < len(scene_tiles(img.shape, Config(CFG)))


def test_the_pipelined_loop_over_the_three_scene_kinds(collar):
    img, _ = collar
    net = standin("valid")
    clean, empty = nk.plain_scene(384, 640, 41), np.zeros((300, 421, 3), np.uint8)
    key = _key(FULL)
    assert nodata_ref(clean, key).all() and not nodata_ref(empty, key).any()
    imgs = [img, clean, empty, img]
    wants = [_run(net, im, CFG, valid=nodata_ref(im, key)) for im in imgs]
    unmasked = _run(net, clean, CFG)
    net.calls.clear()
    res = _loop(net, imgs, dict(CFG, SCENE_NODATA=FULL))
    assert len(res) == 4
    for got, want in zip(res, wants):
        same_tuple(got, want)
    same_tuple(res[1], unmasked)                                                 # no hit pixel: the all-true-mask result
    same_tuple(res[2], _empty_result(300, 421))                                  # all nodata: no pass 1
    assert [c[1] for c in net.calls if c[0] == "pass1"] == [len(scene_tiles(im.shape, Config(CFG))) for im in (img, clean, img)]
    # the serial tile-sharded loop (world 1) and the pipelined tile-sharded one inherit it
    for kw in (dict(tile_sharded=True), dict(tile_sharded=True, pipelined=True)):
        for got, want in zip(_loop(net, imgs, dict(CFG, SCENE_NODATA=FULL), **kw), wants):
            same_tuple(got, want)
    # with the key absent the stand-in's new methods are never called, masked or not
    net.calls.clear()
    _loop(net, imgs[:2], CFG, valids=[nodata_ref(img, key), None])
    _loop(net, imgs[:2], dict(CFG, SCENE_NODATA=None))
    assert not nk.nodata_calls(net) and not [c for c in net.calls if c[0] == "mask_clean"]
    bare = SceneStandIn(dict(CFG))
    assert not hasattr(bare, "scene_nodata_match")
    same_tuple(_loop(bare, [img], CFG)[0], _run(net, img, CFG))


def test_u16_four_bands_with_a_percentile_stretch():
    """The ranges must be those of the derived-valid pixels."""
    net = standin("valid")
    raw, painted = nk.raw16_scene(H, W, SEED)
    bands = dict(select=[2, 1, 0], stretch=dict(percentile=[2, 98]))
    kw = dict(value=65535, tolerance=3, min_area=50, grow=2)
    cfg = dict(CFG, SCENE_BANDS=bands)
    valid = nodata_ref(raw, _key(kw))
    want = _run(net, raw, cfg, valid=valid)
    net.calls.clear()
    net.tables.clear()
    got = _run(net, raw, dict(cfg, SCENE_NODATA=kw))
    same_tuple(got, want)
    order = [c[0] for c in net.calls if c[0] in ("nodata_match", "mask_clean", "nodata_grow", "bands_hist", "bands_apply")]
    assert order == ["nodata_match", "mask_clean", "nodata_grow", "bands_hist", "bands_apply"]        # in front of SCENE_BANDS
    assert [c for c in net.calls if c[0] == "bands_hist"][0][2] is True          # the histogram counts under the derived mask
    hist = np.stack([np.bincount(raw[..., b][valid != 0], minlength=65536) for b in bands["select"]])
    np.testing.assert_array_equal(net.tables[0], band_luts(stretch_from_hist(hist, 2, 98), 1.0, 65536))
    hist_all = np.stack([np.bincount(raw[..., b].ravel(), minlength=65536) for b in bands["select"]])
    assert stretch_from_hist(hist_all, 2, 98) != stretch_from_hist(hist, 2, 98)  # the collar would have moved the ranges
    assert got[3].any()


def test_scene_scale_scene_pad_window_and_tta(collar):
    img, _ = collar
    key = _key(FULL)
    valid = nodata_ref(img, key)
    # SCENE_SCALE [1, 2]: the derived mask is resampled by the validity rule and kept as zero_where for the way back
    net = standin("valid")
    big, _ = nk.collar_scene(2 * H, 2 * W, SEED)
    scaled = dict(CFG, SCENE_SCALE=[1, 2])
    vbig = nodata_ref(big, key)
    got = _run(net, big, dict(scaled, SCENE_NODATA=FULL))
    same_tuple(got, _run(net, big, scaled, valid=vbig))
    assert got[2].shape == (2 * H, 2 * W) and not got[3][vbig == 0].any() and got[3].any()
    # SCENE_PAD 24: the derived mask is padded like a passed one
    net = standin("valid", "pad")
    padded = dict(CFG, SCENE_PAD=24)
    net.calls.clear()
    got = _run(net, img, dict(padded, SCENE_NODATA=FULL))
    same_tuple(got, _run(net, img, padded, valid=valid))
    assert [c[0] for c in net.calls if c[0] in ("nodata_match", "pad", "pass1")][:4] == ["nodata_match", "pad", "pad", "pass1"] and got[3].any()
    # hann with TTA = [id, rot90]
    net = standin("valid", "window", "tta")
    aug = dict(CFG, FUSE_WINDOW="hann", TTA=["id", "rot90"])
    got = _run(net, img, dict(aug, SCENE_NODATA=FULL))
    same_tuple(got, _run(net, img, aug, valid=valid))
    assert got[3].any() and not got[3][valid == 0].any()


def test_group_of_three_with_one_empty_scene():
    net = standin("valid", "pad")
    shapes = [(288, 288), (300, 421), (401, 523)]
    imgs = [nk.collar_scene(h, w, 50 + i)[0] for i, (h, w) in enumerate(shapes)]
    imgs[1] = np.zeros((300, 421, 3), np.uint8)
    key = _key(FULL)
    gcfg = dict(CFG, INFER_PATCHES_PER_EDGE=2, SCENE_PAD=24)
    callers = [None, None, np.ones((401, 523), np.uint8)]
    callers[2][:, 450:] = 0
    for valids in (None, callers):
        vs = valids or [None] * 3
        wants = _loop(net, imgs, gcfg, group=3, valids=[nodata_ref(im, key, v) for im, v in zip(imgs, vs)])
        net.calls.clear()
        res = _loop(net, imgs, dict(gcfg, SCENE_NODATA=FULL), group=3, **({} if valids is None else dict(valids=valids)))
        for got, want, hw in zip(res, wants, shapes):
            assert got[2].shape == hw
            same_tuple(got, want)
        same_tuple(res[1], _empty_result(300, 421))
        assert res[0][3].any() and res[2][3].any()
        # ONE match over the ragged buffer, ONE mask_clean and ONE grow over the three H x W blocks at the offsets of tables[1]
        match, clean, grow = ([c for c in net.calls if c[0] == name] for name in ("nodata_match", "mask_clean", "nodata_grow"))
        assert len(match) == len(clean) == len(grow) == 1 and match[0][1] == (sum(h * w for h, w in shapes), 3)
        offs = np.cumsum([0] + [h * w for h, w in shapes[:-1]]).tolist()
        assert grow[0][1] == [(o, h, w) for o, (h, w) in zip(offs, shapes)] and grow[0][3] is (valids is not None)
        assert [c[2] for c in net.calls if c[0] == "group_pack"] == [3, 1]
    # a group the stream closes early (one scene left): the single-scene path
    res = _loop(net, imgs + [imgs[0]], dict(gcfg, SCENE_NODATA=FULL), group=3)
    same_tuple(res[3], res[0])


# 512 x 512 in four disjoint tiles, one per batch: every canvas pixel has ONE addend and every tile runs alone in both worlds
GLOO_CFG = dict(E2E_CFG, SAMPLE_MARGIN=0, INFER_PATCHES_PER_EDGE=2, INFER_BATCH_SIZE=1, SCENE_NODATA=FULL)


def _rank(world, rank, port, out):
    """One rank of a tile-sharded run on gloo / CPU: puts (rank, infer_one_img's result, its nodata calls)."""
    import torch.distributed as dist
    warnings.simplefilter("ignore")
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        torch.set_num_threads(2)
        net = nk.NodataStandIn(dict(GLOO_CFG), ("valid",))
        res = infer_one_img(net, nk.collar_scene(512, 512, 6)[0], Config(GLOO_CFG), device="cpu")
        out.put((rank, None if res is None else [np.asarray(a) for a in res], [c[0] for c in net.calls if c[0] in ("nodata_match", "mask_clean", "nodata_grow")]))
    except Exception:  # pragma: no cover
        import traceback
        out.put((rank, "ERR " + traceback.format_exc(), None))
    finally:
        dist.destroy_process_group()


def test_tile_sharded_world2_equals_world1_and_every_rank_derives_the_mask():
    import torch.multiprocessing as mp
    warnings.simplefilter("ignore")
    torch.set_num_threads(2)                                                     # as the ranks
    net, img = nk.NodataStandIn(dict(GLOO_CFG), ("valid",)), nk.collar_scene(512, 512, 6)[0]
    one = infer_one_img(net, img, Config(GLOO_CFG), device="cpu")
    unkeyed = {k: v for k, v in GLOO_CFG.items() if k != "SCENE_NODATA"}
    same_tuple(one, infer_one_img(net, img, Config(unkeyed), device="cpu", valid=nodata_ref(img, _key(FULL))))
    assert one[3].any() and (one[3] != infer_one_img(net, img, Config(unkeyed), device="cpu")[3]).any()
    ctx = mp.get_context("spawn")
    port, q = free_port(), ctx.Queue()
    procs = [ctx.Process(target=_rank, args=(2, r, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    got = dict((r, (res, calls)) for r, res, calls in (q.get(timeout=600) for _ in range(2)))
    for p in procs:
        p.join(timeout=60)
    assert not any(isinstance(res, str) for res, _ in got.values()), got
    # every rank holds the raw scene and derives the same integers: the same three steps on both, no collective
    assert got[1][0] is None and got[0][1] == got[1][1] == ["nodata_match", "mask_clean", "nodata_grow"]
    same_tuple(got[0][0], one)


def test_cli_takes_the_flags_beside_valid_masks(tmp_path, monkeypatch, collar):
    from PIL import Image
    from sam_road_amd.formats import convert_to_sat2graph_format
    img, _ = collar
    net = standin("valid")
    monkeypatch.chdir(tmp_path)
    Image.fromarray(img).save("rgb.png")
    caller = np.ones((H, W), np.uint8)
    caller[250:, 300:] = 0
    np.save("caller.npy", caller)

    def run(name, config, *argv):
        return run_cli(cli, net, tmp_path, monkeypatch, name, config, ["rgb.png"], *argv)["rgb"]

    def check(got, want):
        np.testing.assert_array_equal(got[0], want[2])
        np.testing.assert_array_equal(got[1], want[3])
        assert got[2] == convert_to_sat2graph_format(want[0], want[1])

    key = _key(dict(value=0, grow=2))
    want = _run(net, img, CFG, valid=nodata_ref(img, key, caller))
    got = run("a", CFG, "--nodata", "0", "--nodata-grow", "2", "--valid-masks", "caller.npy")
    check(got, want)
    assert got[3]["SCENE_NODATA"] == {"value": 0, "grow": 2}
    # the key from the YAML, every flag laid over it
    got = run("b", dict(CFG, SCENE_NODATA={"value": 9, "grow": 1}), "--nodata", "0", "0", "0", "--nodata-tolerance", "3", "--nodata-match", "all",
              "--nodata-min-area", "50", "--nodata-grow", "2")
    assert got[3]["SCENE_NODATA"] == {"value": [0, 0, 0], "tolerance": 3, "match": "all", "min_area": 50, "grow": 2}
    check(got, _run(net, img, CFG, valid=nodata_ref(img, _key(FULL))))
    with pytest.raises(ValueError, match="SCENE_NODATA"):
        run("c", CFG, "--nodata", "0", "--nodata-grow", "17")
