"""SCENE_FLOAT (float32 scenes quantised exactly on the device), the GPU-free part: the key and its refusals, the ordered
key, the thresholds and the radix select of sam_road_amd/float_scene.py, the kernels' own per-item code under the host sanitizers, the
resource guard, the ABI, and the orchestration of the scene loops through numpy scene_float_valid / scene_float_hist / scene_float_apply
on a subclass of the CPU stand-in.  The feature is pinned by COMPOSITION: a run with the key on the float scene equals, bit for bit, the
existing pipeline on float_scene_ref's uint8 scene and mask."""
import os
import re
import shutil
import subprocess
import warnings

import numpy as np
import pytest
import torch

from sam_road_amd import Config
from sam_road_amd import float_scene as fs
from sam_road_amd import cli
from sam_road_amd import inferencer as inf
from sam_road_amd.aoi import aoi_ref, scene_aoi_key
from sam_road_amd.inferencer import infer_imgs, infer_one_img, scene_tiles
from sam_road_amd.radiometry import band_lut

import scene_aoi_kit as ak
from scene_kit import E2E_CFG, E2E_SCENE, SceneStandIn, assert_abi_11, compare_worlds, free_port, make_mask, run_cli, same_tuple

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SELECT = [2, 0, 3]                                  # output R, G, B <- raw bands 2, 0, 3 of 4; band 1 is noise nobody may read
SCENE_SEED = 6
F32 = np.float32
INF32 = F32(np.inf)


# ---- the stand-in with the three new methods ---------------------------------------------------------------------------------------------
class FloatStandIn(ak.AoiStandIn):
    """The kit's stand-in (SceneStandIn with the numpy forms of the other scene features) + scene_float_valid / scene_float_hist /
    scene_float_apply from numpy — written here on the bit patterns, not by calling float_scene's reference functions — logged;
    `tables` keeps every applied threshold table."""

    def __init__(self, cfg, features=()):
        super().__init__(cfg, features)
        self.tables = []

    @staticmethod
    def _keys(src):
        b = src.numpy().reshape(-1, src.shape[-1]).view(np.uint32).astype(np.int64)
        b[b == 0x80000000] = 0
        return np.where(b >= 0x80000000, 0xffffffff - b, b + 0x80000000)

    def scene_float_valid(self, src, select, nodata_keys=(), log=False, valid=None):
        assert src.dtype == torch.float32
        self.calls.append(("float_valid", tuple(select), len(nodata_keys), bool(log), valid is not None))
        k = self._keys(src)
        bits = src.numpy().reshape(-1, src.shape[-1]).view(np.uint32)
        ok = np.ones(k.shape[0], bool) if valid is None else valid.numpy().reshape(-1) != 0
        for b in select:
            ok &= (bits[:, b] >> 23) & 0xff != 0xff
            for v in nodata_keys:
                ok &= k[:, b] != int(v)
            if log:
                ok &= k[:, b] > 0x80000000
        return torch.from_numpy(ok.astype(np.uint8).reshape(tuple(src.shape[:-1])))

    def scene_float_hist(self, src, select, valid, targets=None):
        self.calls.append(("float_hist", tuple(select), None if targets is None else tuple(tuple(int(v) for v in t) for t in targets)))
        k = self._keys(src)[valid.numpy().reshape(-1) != 0]
        if targets is None:
            rows = [np.bincount(k[:, b] >> 16, minlength=65536) for b in select]
        else:
            assert 1 <= len(targets) <= 6 and len(set(map(tuple, targets))) == len(targets)
            rows = [np.bincount(k[k[:, b] >> 16 == pre, b] & 0xffff, minlength=65536) for b, pre in targets]
        return torch.from_numpy(np.stack(rows).astype(np.uint32))

    def scene_float_apply(self, src, select, valid, thresholds):
        assert thresholds.dtype == torch.uint32 and tuple(thresholds.shape) == (3, 256)
        self.calls.append(("float_apply", tuple(select)))
        t = thresholds.numpy().astype(np.int64)
        assert (t[:, 255] == 0xffffffff).all() and (np.diff(t, axis=1) >= 0).all()
        self.tables.append(thresholds.numpy().copy())
        k = self._keys(src)
        out = np.stack([np.searchsorted(t[b, :255], k[:, s], side="right") for b, s in enumerate(select)], axis=-1).astype(np.uint8)
        out[valid.numpy().reshape(-1) == 0] = 0
        return torch.from_numpy(out.reshape(tuple(src.shape[:-1]) + (3,)))


def float_calls(calls):
    return [c for c in calls if c[0].startswith("float_")]


def reflectance(u8, select=SELECT, C=4, seed=1):
    """f32 [H,W,C]: band select[b] = channel b of the u8 scene / 255 (so stretch [0, 1] gives the u8 scene back), noise elsewhere."""
    rng = np.random.default_rng(seed)
    raw = rng.normal(size=u8.shape[:2] + (C,)).astype(F32)
    for b, s in enumerate(select):
        raw[..., s] = u8[..., b].astype(F32) / F32(255)
    return raw


def _key(v):
    return fs.scene_float_key(Config(SCENE_FLOAT=v))


# ---- the key --------------------------------------------------------------------------------------------------------------------------
def test_absent_key_is_off_and_every_accepted_form():
    for absent in (Config({}), Config(dict(SCENE_FLOAT=None)), Config(dict(SCENE_FLOAT={}))):
        assert fs.scene_float_key(absent) is None
    k = _key({"stretch": [0, 1]})
    assert k == fs.SceneFloat((0, 1, 2), ((F32(0), F32(1)),) * 3, None, 1.0, False, ())
    k = _key({"select": [0, 0, 0], "stretch": [[-25.0, 0], [0.02, 0.35], [100, 4000]], "gamma": 2.2, "nodata": -9999})
    assert k.select == (0, 0, 0) and k.ranges == ((F32(-25), F32(0)), (F32(0.02), F32(0.35)), (F32(100), F32(4000))) and k.gamma == 2.2
    assert k.nodata == (F32(-9999),) and all(isinstance(v, np.float32) for q in k.ranges for v in q)
    k = _key({"stretch": {"percentile": [2, 98.5]}, "transfer": "log", "nodata": [0, -9999.0, 1e30, -0.0]})
    assert k.percentile == (2.0, 98.5) and k.ranges is None and k.log and len(k.nodata) == 4
    assert _key({"stretch": [1e-3, 10], "transfer": "log"}).log and not _key({"stretch": [0, 1], "transfer": "linear"}).log
    assert _key({"stretch": [0, 1], "nodata": []}).nodata == () and fs.as_key(k) is k
    assert fs.as_key({"stretch": [0, 1]}) == _key({"stretch": [0, 1]})


BAD_KEYS = [
    (7, "mapping"), ([0, 1], "mapping"), ("rgb", "mapping"),
    ({"select": [0, 1, 2]}, "stretch is required"), ({"gamma": 2}, "stretch is required"), ({"stretch": None}, "stretch is required"),
    ({"stretch": [0, 1], "bands": [0, 1, 2]}, "unknown key 'bands'"), ({"stretch": [0, 1], "strech": 1}, "unknown key 'strech'"),
    ({"stretch": [0, 1], "select": [0, 1]}, "select"), ({"stretch": [0, 1], "select": [0, -1, 2]}, "select"), ({"stretch": [0, 1], "select": [0, 1, 16]}, "select"),
    ({"stretch": [0, 1], "select": [0, 1.0, 2]}, "select"), ({"stretch": [0, 1], "select": [0, True, 2]}, "select"), ({"stretch": [0, 1], "select": 3}, "select"),
    ({"stretch": [5, 5]}, "stretch"), ({"stretch": [9, 5]}, "stretch"), ({"stretch": [0, float("inf")]}, "stretch"), ({"stretch": [float("nan"), 1]}, "stretch"),
    ({"stretch": [0, 1e39]}, "stretch"), ({"stretch": [1, 1 + 1e-9]}, "stretch"), ({"stretch": [0, 5, 9]}, "stretch"), ({"stretch": [[0, 5], [0, 5]]}, "stretch"),
    ({"stretch": [[0, 5], [0, 5], [5, 5]]}, "stretch"), ({"stretch": "auto"}, "stretch"), ({"stretch": [0, True]}, "stretch"),
    ({"stretch": [0, 1], "transfer": "log"}, "stretch"), ({"stretch": [-1, 1], "transfer": "log"}, "stretch"),
    ({"stretch": {"percentile": [2, 98], "range": [0, 5]}}, "percentile"), ({"stretch": {"percent": [2, 98]}}, "percentile"),
    ({"stretch": {"percentile": [98, 2]}}, "percentile"), ({"stretch": {"percentile": [5, 5]}}, "percentile"),
    ({"stretch": {"percentile": [-1, 50]}}, "percentile"), ({"stretch": {"percentile": [0, 100.5]}}, "percentile"),
    ({"stretch": {"percentile": [0, float("nan")]}}, "percentile"), ({"stretch": {"percentile": [2]}}, "percentile"),
    ({"stretch": [0, 1], "gamma": 0}, "gamma"), ({"stretch": [0, 1], "gamma": -1.0}, "gamma"), ({"stretch": [0, 1], "gamma": float("inf")}, "gamma"),
    ({"stretch": [0, 1], "gamma": "2.2"}, "gamma"), ({"stretch": [0, 1], "gamma": True}, "gamma"),
    ({"stretch": [0, 1], "transfer": "sqrt"}, "transfer"), ({"stretch": [0, 1], "transfer": 1}, "transfer"),
    ({"stretch": [0, 1], "nodata": float("nan")}, "nodata"), ({"stretch": [0, 1], "nodata": [0, 1, 2, 3, 4]}, "nodata"),
    ({"stretch": [0, 1], "nodata": "none"}, "nodata"), ({"stretch": [0, 1], "nodata": [1e39]}, "nodata"), ({"stretch": [0, 1], "nodata": [0, None]}, "nodata"),
]


class Untouchable(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.w = torch.nn.Parameter(torch.zeros(1))

    def __getattr__(self, name):
        if name.startswith("scene_") or name.startswith("infer_") or name.startswith("mask_"):
            raise AssertionError(f"the model was touched: {name}")
        return super().__getattr__(name)


def _refused_everywhere(net, img, cfg, what, **kw):
    with pytest.raises(ValueError, match=what):
        infer_one_img(net, img, Config(cfg), device="cpu")
    for mode in ({}, dict(tile_sharded=True), dict(tile_sharded=True, pipelined=True)):
        with pytest.raises(ValueError, match=what):
            list(infer_imgs(net, [img], Config(cfg), device="cpu", **mode, **kw))


def test_every_refusal_is_a_value_error_before_the_model_is_touched():
    net = Untouchable()
    H, W = 352, 352
    raw = np.zeros((H, W, 4), F32)
    for v, what in BAD_KEYS:
        with pytest.raises(ValueError, match=what):
            fs.scene_float_key(Config(dict(SCENE_FLOAT=v)))
        _refused_everywhere(net, raw, dict(E2E_CFG, SCENE_FLOAT=v), what)
    ok = {"stretch": [0, 1]}
    # the keys it does not combine with
    _refused_everywhere(net, raw, dict(E2E_CFG, SCENE_FLOAT=ok, SCENE_BANDS={"select": [0, 1, 2]}), "SCENE_FLOAT does not combine with SCENE_BANDS")
    _refused_everywhere(net, raw, dict(E2E_CFG, SCENE_FLOAT=ok, SCENE_NODATA={"value": 0}), "SCENE_FLOAT does not combine with SCENE_NODATA")
    with pytest.raises(ValueError, match="SCENE_FLOAT does not combine with SCENE_GROUP"):
        list(infer_imgs(net, [raw, raw], Config(dict(E2E_CFG, SCENE_FLOAT=ok)), device="cpu", group=2))
    with pytest.raises(ValueError, match="SCENE_FLOAT does not combine with SCENE_GROUP"):
        list(infer_imgs(net, [raw, raw], Config(dict(E2E_CFG, SCENE_FLOAT=ok, SCENE_GROUP=2)), device="cpu"))
    # what depends on the scene
    per_scene = [
        (raw[..., :3], {"select": [0, 1, 3], "stretch": [0, 1]}, "needs more than the 3 band"),
        (np.zeros((H, W), F32), ok, "HxWxC float32"),
        (np.zeros((H, W, 17), F32), ok, "1 <= C <= 16"),
        (np.zeros((H, W, 4), np.float64), ok, "cast it with .astype"),
        (np.zeros((H, W, 4), np.float16), ok, "cast it with .astype"),
        (np.zeros((H, W, 4), np.uint16), ok, "HxWxC float32"),
        (np.zeros((H, W, 3), np.uint8), ok, "HxWxC float32"),
        (np.zeros((0, W, 4), F32), ok, "1 x 1"),
    ]
    for img, v, what in per_scene:
        _refused_everywhere(net, img, dict(E2E_CFG, SCENE_FLOAT=v), what)
        with pytest.raises(ValueError, match=what):
            infer_one_img(net, img, Config(dict(E2E_CFG, SCENE_FLOAT=v)), device="cpu", valid=np.ones(img.shape[:2], bool))
    # without the key: today's messages
    with pytest.raises(ValueError, match="^infer_one_img expects an HxWx3 uint8 scene, got float32"):
        infer_one_img(net, raw[..., :3], Config(E2E_CFG), device="cpu")
    with pytest.raises(ValueError, match="uint8 or uint16"):
        infer_one_img(net, raw, Config(dict(E2E_CFG, SCENE_BANDS={"select": [0, 1, 2]})), device="cpu")
    # the tile plan depends on the shape and the mask only
    assert list(scene_tiles((H, W), Config(dict(E2E_CFG, SCENE_FLOAT=ok)))) == list(scene_tiles((H, W), Config(E2E_CFG)))


# ---- the ordered key --------------------------------------------------------------------------------------------------------------------
def test_ordered_key_is_monotone_and_minus_zero_is_zero():
    rng = np.random.default_rng(0)
    x = rng.integers(0, 2 ** 32, 200000, dtype=np.uint64).astype(np.uint32).view(F32)
    x = np.concatenate([x[np.isfinite(x)], F32([0.0, -0.0, np.inf, -np.inf, 1e-45, -1e-45, 1.17549435e-38, 3.4028235e38, -3.4028235e38])])
    k = fs.float_keys(x)
    order = np.argsort(k, kind="stable")
    assert (np.diff(x[order].astype(np.float64)) >= 0).all()
    a, b = x[order][:-1], x[order][1:]
    assert ((k[order][:-1] == k[order][1:]) == (a == b)).all()                    # equal keys iff equal values (+0 == -0)
    assert fs.float_keys(F32([-0.0]))[0] == fs.float_keys(F32([0.0]))[0] == 0x80000000
    back = fs.keys_to_float(k)
    assert ((back == x) & ((back.view(np.uint32) == x.view(np.uint32)) | (x == 0))).all()


# ---- thresholds, part 1 ----------------------------------------------------------------------------------------------------------------
NARROW = (F32(0.3), (np.array([0.3], F32).view(np.uint32) + np.uint32(85)).view(F32)[0])      # a range only 85 float32 steps wide
SETTINGS = [((0, 1), 1), ((-25, 0), 1), ((0.02, 0.35), 2.2), ((100, 4000), 0.5), (NARROW, 1)]


def _formula(x, lo, hi, gamma):
    lo, hi = np.float64(F32(lo)), np.float64(F32(hi))
    return np.floor(255.0 * np.clip((x.astype(np.float64) - lo) / (hi - lo), 0.0, 1.0) ** (1.0 / gamma) + 0.5).astype(np.int64)


def test_thresholds_are_monotone_and_agree_with_the_float64_formula():
    """Against the formula on random float32 plus every threshold and its two float32 neighbours every disagreement must be ONE level, at a
    value adjacent to a threshold: a condition, not a tolerance (pow may round the other way right at a threshold)."""
    rng = np.random.default_rng(11)
    for (lo, hi), gamma in SETTINGS:
        key = fs.as_key({"stretch": [float(lo), float(hi)], "gamma": gamma})
        T = fs.float_thresholds(key.ranges, key)
        assert T.shape == (3, 255) and T.dtype == F32 and (np.diff(T[0].astype(np.float64)) >= 0).all() and np.array_equal(T[0], T[1])
        lo32, hi32 = key.ranges[0]
        span = np.float64(hi32) - np.float64(lo32)
        x = np.concatenate([(np.float64(lo32) + span * rng.uniform(-0.2, 1.2, 200000)).astype(F32), T[0], np.nextafter(T[0], -INF32), np.nextafter(T[0], INF32),
                            F32([lo32, hi32]), rng.normal(size=1000).astype(F32)])
        got = np.searchsorted(T[0], x, side="right")
        want = _formula(x, lo32, hi32, gamma)
        bad = np.nonzero(got != want)[0]
        print((float(lo), float(hi), gamma), "disagreements:", bad.size)
        assert (np.abs(got[bad] - want[bad]) == 1).all()
        near = np.concatenate([T[0], np.nextafter(T[0], -INF32), np.nextafter(T[0], INF32)])
        assert np.isin(x[bad], near).all()
        assert got[x < lo32].max(initial=0) == 0 and got[x >= hi32].min(initial=255) == 255


def test_thresholds_equal_the_integer_lut_on_cast_uint16():
    v = np.arange(65536).astype(F32)
    for lo, hi in ((0, 510), (0, 255), (100, 4000), (3, 65529), (0, 65535)):
        key = fs.as_key({"stretch": [lo, hi]})
        T = fs.float_thresholds(key.ranges, key)
        np.testing.assert_array_equal(np.searchsorted(T[0], v, side="right"), band_lut(lo, hi, 1, 65536))
    T = fs.float_thresholds(fs.as_key({"stretch": [0, 510]}).ranges, fs.as_key({"stretch": [0, 510]}))
    np.testing.assert_array_equal(T[0], np.arange(1, 511, 2).astype(F32))         # the odd integers, exact in every format


# ---- thresholds, part 2 ----------------------------------------------------------------------------------------------------------------
def test_thresholds_collapsed_denormal_negative_and_log():
    lo = F32(0.75)
    hi = np.nextafter(lo, INF32)
    key = fs.as_key({"stretch": {"percentile": [0, 100]}})
    T = fs.float_thresholds([(lo, hi)] * 3, key)
    assert (T == hi).all()                                                          # every threshold is hi: lo -> 0, hi -> 255
    assert list(np.searchsorted(T[0], F32([lo, hi]), side="right")) == [0, 255]
    # a range of denormals, and one across zero
    d = F32(1e-45)
    for lo, hi in ((F32(0), d * F32(1000)), (-d * F32(500), d * F32(500)), (F32(-3e-39), F32(-1e-39))):
        T = fs.float_thresholds([(lo, hi)] * 3, fs.as_key({"stretch": [0, 1]}))
        assert (np.diff(T[0].astype(np.float64)) >= 0).all() and T[0][0] > lo and T[0][-1] <= hi
        x = np.linspace(np.float64(lo), np.float64(hi), 4001).astype(F32)
        got, want = np.searchsorted(T[0], x, side="right"), _formula(x, lo, hi, 1)
        assert np.abs(got - want).max() <= 1 and got[0] == 0 and got[-1] == 255
    # the keys of the thresholds order as the thresholds do, -0.0 included
    T = fs.float_thresholds([(F32(-1), F32(1))] * 3, fs.as_key({"stretch": [0, 1]}))
    tk = fs.threshold_keys(T)
    assert tk.shape == (3, 256) and tk.dtype == np.uint32 and (tk[:, 255] == 0xffffffff).all() and (np.diff(tk.astype(np.int64), axis=1) >= 0).all()
    # log against linear on log(x): the same levels except next to a threshold
    rng = np.random.default_rng(5)
    klog, klin = fs.as_key({"stretch": [0.001, 10.0], "transfer": "log", "gamma": 1.5}), fs.as_key({"stretch": [np.log(0.001), np.log(10.0)], "gamma": 1.5})
    Tlog = fs.float_thresholds(klog.ranges, klog)[0]
    x = np.exp(rng.uniform(np.log(0.0005), np.log(20.0), 200000)).astype(F32)
    got = np.searchsorted(Tlog, x, side="right")
    lo64, hi64 = np.log(np.float64(klog.ranges[0][0])), np.log(np.float64(klog.ranges[0][1]))
    want = np.floor(255.0 * np.clip((np.log(x.astype(np.float64)) - lo64) / (hi64 - lo64), 0, 1) ** (1 / 1.5) + 0.5).astype(np.int64)
    bad = got != want
    assert np.abs(got - want).max() <= 1 and bad.mean() < 1e-3
    assert (np.diff(Tlog.astype(np.float64)) >= 0).all() and Tlog[0] > klog.ranges[0][0]
    for bad_range in ((F32(1), F32(1)), (F32(2), F32(1)), (F32(0), INF32)):
        with pytest.raises(ValueError):
            fs.float_thresholds([bad_range] * 3, klin)
    with pytest.raises(ValueError):
        fs.float_thresholds([(F32(0), F32(1))] * 3, klog)


# ---- the radix select ---------------------------------------------------------------------------------------------------------------------
def _shapes(rng):
    one = F32(1.0).view(np.uint32)
    return {
        "normal": rng.normal(size=(5001, 3)).astype(F32) * F32(100),
        "constant": np.full((777, 3), F32(0.25)),
        "zeros_and_denormals": rng.choice(F32([0.0, -0.0, 1e-45, -1e-45, 3e-39, -3e-39, 1.2e-38]), size=(2001, 3)),
        "low_mantissa_bits": (one + rng.integers(0, 4000, size=(4097, 3)).astype(np.uint32)).view(F32),          # 1 + k 2^-23: one top-16-bit bucket
        "one_pixel": F32([[3.5, -2.0, 0.0]]),
        "mixed_signs_with_nodata": np.where(rng.random((3001, 3)) < 0.2, F32(-9999), rng.normal(size=(3001, 3)).astype(F32)),
    }


def test_radix_select_equals_sorted_indexing():
    rng = np.random.default_rng(7)
    for name, x in _shapes(rng).items():
        raw = x.reshape(1, -1, 3)
        N0 = raw.shape[1]
        for masked in (False, True):
            valid = (rng.random((1, N0)) < 0.6).astype(np.uint8) if masked and N0 > 1 else None
            for p in ((2, 98), (0, 100), (25, 50), (0.5, 99.5), (33.3, 33.4), (99, 100)):
                key = fs.as_key({"stretch": {"percentile": list(p)}, "select": [2, 0, 2], "nodata": -9999})
                want = fs.float_ranges_ref(raw, key, valid)
                got = fs.radix_select_ref(raw, key, valid)
                # np.sort on the VALUES plus the index, restated here
                ok = fs.float_valid_ref(raw, key, valid) != 0
                for b, (lo, hi) in zip(key.select, want):
                    s = np.sort(raw[..., b][ok])
                    r = [s[int(np.floor(np.float64(q) / 100.0 * (s.size - 1)))] for q in p]
                    assert lo == r[0] and (hi == r[1] if r[1] > r[0] else hi == np.nextafter(F32(r[0]), INF32)), (name, masked, p)
                assert [(a.tobytes(), b.tobytes()) for a, b in got] == [(a.tobytes(), b.tobytes()) for a, b in want], (name, masked, p, got, want)
                assert all(isinstance(v, np.float32) and lo < hi for lo, hi in got for v in (lo, hi))
    # at most 6 de-duplicated targets; repeats of a band share them
    raw = _shapes(rng)["normal"].reshape(1, -1, 3)
    key = fs.as_key({"stretch": {"percentile": [2, 98]}, "select": [1, 1, 1]})
    k = fs.float_keys(raw.reshape(-1, 3))
    hist1 = np.stack([np.bincount(k[:, b] >> 16, minlength=65536) for b in key.select])
    targets, picks = fs.float_hist_targets(hist1, key)
    assert len(targets) == 2 and len(set(targets)) == 2 and picks[0] == picks[1] == picks[2]
    # a valid band constant at the largest finite float32: nextafter would be +inf, so the range steps DOWN (the band comes out as 255)
    big = np.finfo(F32).max
    raw = np.full((1, 9, 3), big, F32)
    key = fs.as_key({"stretch": {"percentile": [2, 98]}})
    want = (np.nextafter(big, -INF32), big)
    assert fs.float_ranges_ref(raw, key) == [want] * 3 == fs.radix_select_ref(raw, key)
    u8, ok = fs.float_scene_ref(raw, key)
    assert ok.all() and (u8 == 255).all()
    # N = 0: no targets, the empty range
    for transfer, want in (("linear", (F32(0), F32(1))), ("log", (F32(1), F32(2)))):
        key = fs.as_key({"stretch": {"percentile": [2, 98]}, "transfer": transfer})
        raw = np.full((4, 5, 3), np.nan, F32)
        assert fs.float_hist_targets(np.zeros((3, 65536), np.uint32), key) == ([], None)
        assert fs.radix_select_ref(raw, key) == [want] * 3 == fs.float_ranges_ref(raw, key)
        u8, ok = fs.float_scene_ref(raw, key)
        assert not u8.any() and not ok.any()


def test_rule_1_and_the_reference_functions():
    raw = np.zeros((2, 6, 3), F32)
    raw[0] = [[0.5, 0.5, 0.5], [np.nan, 0.5, 0.5], [0.5, np.inf, 0.5], [0.5, 0.5, -np.inf], [-9999, 0.5, 0.5], [0.5, -0.0, 0.5]]
    raw[1] = [[0.5, 0.5, 1e-45], [0.5, 0.5, -1e-45], [0.0, 0.5, 0.5], [0.5, 0.5, 0.5], [0.5, 0.5, 0.5], [0.25, 1.0, 2.0]]
    lin = fs.float_valid_ref(raw, {"stretch": [0, 1], "nodata": [-9999, 0]})
    np.testing.assert_array_equal(lin, [[1, 0, 0, 0, 0, 0], [1, 1, 0, 1, 1, 1]])  # -0.0 hits nodata 0
    log = fs.float_valid_ref(raw, {"stretch": [0.1, 1], "transfer": "log"})
    np.testing.assert_array_equal(log, [[1, 0, 0, 0, 0, 0], [1, 0, 0, 1, 1, 1]])
    caller = np.ones((2, 6), np.uint8)
    caller[1, 3:5] = (0, 7)
    np.testing.assert_array_equal(fs.float_valid_ref(raw, {"stretch": [0, 1]}, caller), [[1, 0, 0, 0, 1, 1], [1, 1, 1, 0, 1, 1]])
    # band 1 is not selected: its NaN does not count
    sel = raw.copy()
    sel[..., 1] = np.nan
    assert fs.float_valid_ref(sel, {"stretch": [0, 1], "select": [0, 2, 2]})[1].all()
    u8, ok = fs.float_scene_ref(raw, {"stretch": [0, 1], "nodata": [-9999, 0]})
    assert u8.dtype == np.uint8 and u8.shape == (2, 6, 3) and ok.dtype == np.uint8 and not u8[ok == 0].any()
    np.testing.assert_array_equal(u8[1, 5], [64, 255, 255])
    np.testing.assert_array_equal(u8[0, 0], [128, 128, 128])
    np.testing.assert_array_equal(u8[1, 0], [128, 128, 0])


# ---- the kernels' addressing, on the CPU ------------------------------------------------------------------------------------------------
def test_kernel_addressing_on_the_cpu(tmp_path):
    """tests/scene_float_check.cpp runs every work item of a valid and an apply launch through the kernels' own per-item code
    (csrc/scene_float_piece.hpp) as a stand-alone host program built with the address and undefined-behaviour sanitizers."""
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    cxx = next((c for c in (os.path.join(rocm, "llvm", "bin", "clang++"), os.path.join(rocm, "lib", "llvm", "bin", "clang++")) if os.path.exists(c)), None)
    if cxx is None:
        pytest.skip("no ROCm clang++")
    exe = str(tmp_path / "scene_float_check")
    csrc = os.path.join(ROOT, "sam_road_amd", "csrc")
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", csrc,
                        os.path.join(ROOT, "tests", "scene_float_check.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    assert "scene float OK" in r.stdout


def test_kernels_compile_for_gfx950_without_a_gpu():
    hipcc = next((c for c in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", shutil.which("hipcc")) if c and os.path.exists(c)), None)
    if hipcc is None:
        pytest.skip("hipcc not found")
    from sam_road_amd import build
    assert "scene_float.hip" in build.SOURCES
    r = subprocess.run([hipcc, *build.FLAGS, "-S", "--cuda-device-only", os.path.join(build.CSRC, "scene_float.hip"), "-o", "-"],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    for kernel, lds in (("scene_float_valid_kernel", 0), ("scene_float_apply_kernel", 3072), ("scene_float_hist_kernel", 49152), ("scene_float_hist_low_kernel", 0)):
        m = re.search(r"^(_Z\w*%s\w*):" % kernel, r.stdout, re.M)
        assert m, f"{kernel} is not in the code object"
        meta = r.stdout[r.stdout.index(".amdhsa_kernel " + m.group(1)):]
        meta = meta[:meta.index(".end_amdhsa_kernel")]
        assert int(re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", meta).group(1)) == 0          # no scratch
        assert int(re.search(r"\.amdhsa_group_segment_fixed_size (\d+)", meta).group(1)) == lds
    apply_body = r.stdout[r.stdout.index(re.search(r"^_Z\w*scene_float_apply_kernel\w*:", r.stdout, re.M).group(0)):]
    apply_body = apply_body[:apply_body.index("s_endpgm")]
    assert "ds_read_b32" in apply_body and "flat_load" not in r.stdout              # the binary search reads the LDS copy with DS reads, not flat loads
    assert "global_store_dwordx4" in r.stdout and "global_atomic_add " in r.stdout and "global_atomic_cmpswap" not in r.stdout
    assert not re.search(r"\bv_\w+_f(16|32|64)\b", r.stdout)            # integer compares only: no float instruction


def test_abi_has_the_entries_and_stays_11():
    assert_abi_11([("srh_scene_float_valid", 11), ("srh_scene_float_hist", 10), ("srh_scene_float_apply", 9)])


# ---- the whole loop on the CPU stand-in ----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def standin():
    warnings.simplefilter("ignore")
    torch.set_num_threads(4)
    return FloatStandIn(dict(E2E_CFG), ("valid",))


@pytest.fixture(scope="module")
def scene():
    from oracle.synth import synth_scene
    u8 = synth_scene(E2E_SCENE, seed=SCENE_SEED)
    return u8, reflectance(u8)


def _run(net, img, cfg, **kw):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return infer_one_img(net, img, Config(cfg), device="cpu", **kw)


def _contract(net, raw, key, valid=None, least=(30, 1), base=E2E_CFG, ref_valid=None, **kw):
    """infer_one_img(raw, cfg + SCENE_FLOAT) == infer_one_img(float_scene_ref's scene, cfg, valid = float_scene_ref's mask), bit for bit."""
    u8, ok = fs.float_scene_ref(raw, key, valid if ref_valid is None else ref_valid)
    want = _run(net, u8, base, valid=ok)
    raw_before = raw.copy()
    net.calls.clear()
    net.tables.clear()
    got = _run(net, raw, dict(base, SCENE_FLOAT=key), **({} if valid is None else dict(valid=valid)), **kw)
    assert np.array_equal(raw.view(np.uint32), raw_before.view(np.uint32))
    same_tuple(got, want)
    print(key, "nodes", want[0].shape[0], "edges", want[1].shape[0], "valid", float(ok.mean()))
    assert want[0].shape[0] >= least[0] and want[1].shape[0] >= least[1]
    assert len(net.tables) == 1
    np.testing.assert_array_equal(net.tables[0], fs.threshold_keys(fs.float_thresholds(fs.float_ranges_ref(raw, key, valid if ref_valid is None else ref_valid), fs.as_key(key))))
    return got, u8, ok, list(net.calls)


def test_contract_fixed_range_is_the_stock_scene(standin, scene):
    u8, raw = scene
    got, conv, ok, calls = _contract(standin, raw, {"select": SELECT, "stretch": [0, 1]})
    np.testing.assert_array_equal(conv, u8)                                       # v / 255 under [0, 1] -> v: the converted scene IS the stock one
    assert ok.all()
    same_tuple(got, _run(standin, u8, E2E_CFG))                                   # an all-valid mask changes nothing
    assert got[0].shape[0] > 30 and got[1].shape[0] > 100
    assert [c[0] for c in float_calls(calls)] == ["float_valid", "float_apply"]        # a fixed range counts nothing
    order = [c[0] for c in calls if c[0] in ("float_valid", "float_apply", "tile_valid", "fill", "pass1")]
    assert order == ["float_valid", "float_apply", "tile_valid", "fill", "pass1"]
    _contract(standin, raw, {"select": SELECT, "stretch": [[0.1, 0.9], [0.0, 0.8], [0.05, 1.5]], "gamma": 1.4})


def test_contract_percentile_nan_block_nodata_and_valid(standin, scene):
    u8, raw = scene
    key = {"select": SELECT, "stretch": {"percentile": [2, 98]}}
    _, conv, _, calls = _contract(standin, raw, key)
    hists = [c for c in calls if c[0] == "float_hist"]
    assert len(hists) == 2 and hists[0][2] is None and 1 <= len(hists[1][2]) <= 6 and not np.array_equal(conv, u8)
    assert [c[0] for c in float_calls(calls)] == ["float_valid", "float_hist", "float_hist", "float_apply"]
    # a NaN block that removes a tile (and inf in the band nobody reads, which removes nothing)
    holed = raw.copy()
    holed[:272, :272, SELECT[1]] = np.nan                                          # the whole of the first tile, (16, 16) .. (272, 272)
    holed[300:, :, 1] = np.inf
    n_all = [c for c in calls if c[0] == "pass1"][0][1]
    for k in (key, {"select": SELECT, "stretch": [0, 1]}):
        got, _, ok, calls = _contract(standin, holed, k, least=(10, 1))
        assert not ok[:272, :272].any() and ok[272:].all() and ok[:, 272:].all() and [c for c in calls if c[0] == "pass1"][0][1] == n_all - 1
        assert not got[2][:272, :272].any() and not got[3][:272, :272].any()
    # nodata -9999 in a region, with and without it in the key: other ranges, other masks
    nd = raw.copy()
    nd[250:, 100:300] = -9999
    with_nd = dict(key, nodata=-9999)
    assert fs.float_ranges_ref(nd, with_nd) != fs.float_ranges_ref(nd, key)
    got, _, ok, _ = _contract(standin, nd, with_nd)
    assert not ok[250:, 100:300].any() and ok[:250].all() and not got[3][250:, 100:300].any()
    # valid= given: ANDed into the mask, counted by the histogram
    valid = make_mask("hole", E2E_SCENE, E2E_SCENE)
    nd[~valid] = 1e6
    assert fs.float_ranges_ref(nd, with_nd, valid) != fs.float_ranges_ref(nd, with_nd)
    got, _, ok, calls = _contract(standin, nd, with_nd, valid=valid)
    assert not ok[~valid].any() and [c for c in calls if c[0] == "float_valid"][0] == ("float_valid", tuple(SELECT), 1, False, True)
    # log: x <= 0 is nodata
    lg = raw.copy()
    lg[..., SELECT] = lg[..., SELECT] * F32(100) + F32(0.5)
    lg[300:, :60, SELECT[0]] = 0.0
    got, _, ok, _ = _contract(standin, lg, {"select": SELECT, "stretch": {"percentile": [1, 99]}, "transfer": "log"})
    assert not ok[300:, :60].any() and ok[:300].all()
    # every pixel invalid: the empty result, nothing but the valid kernel, the two empty counts and the apply
    dead = np.full_like(raw, np.nan)
    standin.calls.clear()
    got = _run(standin, dead, dict(E2E_CFG, SCENE_FLOAT=key))
    same_tuple(got, inf._empty_result(E2E_SCENE, E2E_SCENE))
    assert not [c for c in standin.calls if c[0] == "pass1"] and len([c for c in standin.calls if c[0] == "float_hist"]) == 1


def test_contract_with_scene_pad_scene_scale_tta_and_scene_aoi(scene):
    u8, raw = scene
    net = FloatStandIn(dict(E2E_CFG), ("valid", "pad", "tta"))
    aoi = {"include": [[[[20, 30], [340.5, 40], [330, 345.25], [40, 300]]]], "buffer": 2}
    base = dict(E2E_CFG, SCENE_PAD=24, SCENE_SCALE=[3, 2], TTA=["id", "rot90"], INFER_PATCHES_PER_EDGE=4)
    key = {"select": SELECT, "stretch": {"percentile": [2, 98]}, "gamma": 1.2, "nodata": -9999}
    raw = raw.copy()
    raw[100:130, 200:260] = -9999
    area = aoi_ref(raw.shape[:2], scene_aoi_key(Config(SCENE_AOI=aoi)))
    u8c, ok = fs.float_scene_ref(raw, key, area)
    assert 0.3 < ok.mean() < 0.95 and not ok[100:130, 200:260].any()
    want = _run(net, u8c, base, valid=ok)
    net.calls.clear()
    got = _run(net, raw, dict(base, SCENE_FLOAT=key, SCENE_AOI=aoi))
    same_tuple(got, want)
    assert want[0].shape[0] >= 20 and want[1].shape[0] >= 1 and got[2].shape == raw.shape[:2]
    order = [c[0] for c in net.calls if c[0] in ("aoi_fill", "float_valid", "float_hist", "float_apply", "resample", "pad", "tile_valid", "pass1_tta")]
    assert order[:5] == ["aoi_fill", "float_valid", "float_hist", "float_hist", "float_apply"] and "pass1_tta" in order
    assert order.index("float_apply") < min(order.index(n) for n in ("pad", "tile_valid", "pass1_tta"))
    assert [c for c in net.calls if c[0] == "float_valid"][0][4] is True        # the area's mask goes INTO the valid kernel


def test_key_absent_makes_exactly_the_calls_it_made(standin, scene):
    """The stock SceneStandIn has none of the three methods: a run without the key that called one would raise AttributeError.  And on
    the stand-in that has them, the call log of a run without the key holds none of them and equals the stock stand-in's."""
    u8, raw = scene
    plain = SceneStandIn(dict(E2E_CFG), ("valid",))
    assert not any(hasattr(plain, n) for n in ("scene_float_valid", "scene_float_hist", "scene_float_apply"))
    valid = make_mask("hole", E2E_SCENE, E2E_SCENE)
    for kw in ({}, dict(valid=valid)):
        logs = []
        for cfg in (E2E_CFG, dict(E2E_CFG, SCENE_FLOAT=None), dict(E2E_CFG, SCENE_FLOAT={})):
            for net in (plain, standin):
                net.calls.clear()
                res = _run(net, u8, cfg, **kw)
                logs.append((list(net.calls), res))
        assert all(log == logs[0][0] for log, _ in logs) and not [c for c in logs[0][0] if c[0].startswith("float")]
        for _, res in logs[1:]:
            same_tuple(res, logs[0][1])
    with pytest.raises(ValueError, match="^infer_one_img expects an HxWx3 uint8 scene, got float32"):
        _run(plain, raw, E2E_CFG)
    with pytest.raises(AttributeError):                                           # and with the key it does call them
        _run(plain, raw, dict(E2E_CFG, SCENE_FLOAT={"select": SELECT, "stretch": [0, 1]}))


def test_the_scene_loops_inherit_the_feature(standin, scene):
    """infer_imgs (pipelined) and both tile-sharded loops at world 1 over three scenes of different shapes and band counts."""
    u8, raw = scene
    small = np.ascontiguousarray(raw[20:320, 10:330])
    other = reflectance(u8, select=SELECT, C=5, seed=3)
    other[:100, :100] = np.nan
    imgs = [raw, small, other]
    for key in ({"select": SELECT, "stretch": [0, 1]}, {"select": SELECT, "stretch": {"percentile": [2, 98]}}):
        cfg = dict(E2E_CFG, SCENE_FLOAT=key)
        want = [_run(standin, im, cfg) for im in imgs]
        for kw in ({}, dict(tile_sharded=True), dict(tile_sharded=True, pipelined=True)):
            standin.calls.clear()
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                got = list(infer_imgs(standin, iter(imgs), Config(cfg), device="cpu", **kw))
            assert len(got) == 3
            for w, g in zip(want, got):
                same_tuple(g, w)
            assert len([c for c in standin.calls if c[0] == "float_apply"]) == 3
    # valids= travel with their scenes
    valid = make_mask("hole", E2E_SCENE, E2E_SCENE)
    got = list(infer_imgs(standin, iter([raw, other]), Config(cfg), device="cpu", valids=[valid, None]))
    same_tuple(got[0], _run(standin, raw, cfg, valid=valid))
    same_tuple(got[1], want[2])


def test_uint16_cast_to_float_equals_scene_bands(standin):
    """The cross-check that anchors to shipped code: a uint16 scene cast to float32 under SCENE_FLOAT {stretch: [0, 510]} equals the same
    scene under SCENE_BANDS {stretch: [0, 510]}, whole tuple (the thresholds are the odd integers, exact in every format).  The float
    scene is a masked scene with an all-valid mask, which changes nothing."""
    from oracle.synth import synth_scene
    u8 = synth_scene(E2E_SCENE, seed=SCENE_SEED)
    rng = np.random.default_rng(9)
    raw16 = rng.integers(0, 65536, size=u8.shape[:2] + (4,), dtype=np.uint16)
    for b, s in enumerate(SELECT):
        raw16[..., s] = u8[..., b].astype(np.uint16) * 2 + rng.integers(0, 2, size=u8.shape[:2], dtype=np.uint16)
    want = _run(standin, raw16, dict(E2E_CFG, SCENE_BANDS={"select": SELECT, "stretch": [0, 510]}))
    got = _run(standin, raw16.astype(F32), dict(E2E_CFG, SCENE_FLOAT={"select": SELECT, "stretch": [0, 510]}))
    same_tuple(got, want)
    assert got[0].shape[0] > 30 and got[1].shape[0] > 100


# ---- world 2 on gloo -------------------------------------------------------------------------------------------------------------------
def _rank_worker(world, rank, port, out, key):
    """One rank of the serial and the pipelined tile-sharded loop on gloo / CPU with the FloatStandIn: puts (rank, serial result or None,
    pipelined result or None, applied tables)."""
    import torch.distributed as dist
    from oracle.synth import synth_scene
    warnings.simplefilter("ignore")
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from sam_road_amd import distributed as D
        torch.set_num_threads(2)
        D._CHECK_BANDS[0] = True
        net = FloatStandIn(dict(E2E_CFG), ("valid",))
        raw = reflectance(synth_scene(E2E_SCENE, seed=SCENE_SEED))
        valid = make_mask("hole", E2E_SCENE, E2E_SCENE)
        raw[~valid] = np.nan
        cfg = Config(dict(E2E_CFG, SCENE_FLOAT=key))
        serial = infer_one_img(net, raw, cfg, device="cpu")
        piped = list(infer_imgs(net, iter([raw]), Config(dict(cfg, TILE_SHARD_PIPELINE=True)), device="cpu"))[0]
        out.put((rank, None if serial is None else [np.asarray(a) for a in serial], None if piped is None else [np.asarray(a) for a in piped], net.tables))
    except Exception:  # pragma: no cover
        import traceback
        out.put((rank, "ERR " + traceback.format_exc(), None, None))
    finally:
        dist.destroy_process_group()


def test_tile_sharded_world2_serial_and_pipelined(standin, scene):
    """Every rank holds the scene, derives the same mask, counts the same integers and builds the same thresholds — no collective; rank
    0's result is the single-process one under the rule of scene_kit.compare_worlds, and the pipelined loop equals the serial one."""
    import torch.multiprocessing as mp
    key = {"select": SELECT, "stretch": {"percentile": [2, 99]}}
    valid = make_mask("hole", E2E_SCENE, E2E_SCENE)
    raw = scene[1].copy()
    raw[~valid] = np.nan
    one = _run(standin, raw, dict(E2E_CFG, SCENE_FLOAT=key))
    ctx = mp.get_context("spawn")
    port, q = free_port(), ctx.Queue()
    procs = [ctx.Process(target=_rank_worker, args=(2, r, port, q, key)) for r in range(2)]
    for p in procs:
        p.start()
    got = dict((r, (s, pl, t)) for r, s, pl, t in (q.get(timeout=900) for _ in range(2)))
    for p in procs:
        p.join(timeout=60)
    for r, (s, pl, _) in got.items():
        assert not isinstance(s, str), s
        assert (s is None) == (pl is None) == (r != 0)
    assert len(got[0][2]) == len(got[1][2]) == 2
    want = fs.threshold_keys(fs.float_thresholds(fs.float_ranges_ref(raw, key), fs.as_key(key)))
    for r in (0, 1):
        for t in got[r][2]:
            np.testing.assert_array_equal(t, want)                                # identical thresholds on both ranks, in both loops
    same_tuple(got[0][1], got[0][0])
    compare_worlds([one], [got[0][0]], [(E2E_SCENE, E2E_SCENE)], ["hole"], must_be_identical=False)


# ---- CLI -------------------------------------------------------------------------------------------------------------------------------
def test_cli_takes_the_key_and_the_flags(tmp_path, monkeypatch, standin, scene):
    from sam_road_amd.formats import convert_to_sat2graph_format
    u8, raw = scene
    raw = raw.copy()
    raw[300:, 300:] = -9999
    monkeypatch.chdir(tmp_path)
    np.save("raw.npy", raw)

    def run(name, config, *argv):
        return run_cli(cli, standin, tmp_path, monkeypatch, name, config, ["raw.npy"], *argv)["raw"]

    def check(got, want):
        np.testing.assert_array_equal(got[0], want[2])
        np.testing.assert_array_equal(got[1], want[3])
        assert got[2] == convert_to_sat2graph_format(want[0], want[1])

    fixed = {"select": SELECT, "stretch": [0.0, 1.0], "nodata": [-9999.0]}
    want = _run(standin, raw, dict(E2E_CFG, SCENE_FLOAT=fixed))
    assert want[0].shape[0] > 30
    check(run("a", dict(E2E_CFG, SCENE_FLOAT=fixed)), want)                       # the key comes from the YAML
    got = run("b", E2E_CFG, "--float-bands", "2,0,3", "--float-range", "0", "1", "--float-nodata", "-9999")      # the flags set it
    check(got, want)
    assert got[3]["SCENE_FLOAT"] == fixed
    key = {"select": SELECT, "stretch": {"percentile": [2.0, 98.0]}, "gamma": 1.4, "transfer": "log", "nodata": [-9999.0, 0.0]}
    want = _run(standin, raw, dict(E2E_CFG, SCENE_FLOAT=key))
    got = run("c", dict(E2E_CFG, SCENE_FLOAT={"select": [0, 1, 2], "stretch": [5, 9]}), "--float-bands", "2,0,3", "--float-percentile", "2", "98",
              "--float-gamma", "1.4", "--float-transfer", "log", "--float-nodata", "-9999", "0")
    check(got, want)
    assert got[3]["SCENE_FLOAT"] == key
    got = run("d", dict(E2E_CFG, SCENE_FLOAT=key), "--float-range", "0", "1", "--float-transfer", "linear", "--float-gamma", "1", "--float-nodata", "-9999")
    assert got[3]["SCENE_FLOAT"] == dict(fixed, gamma=1.0, transfer="linear")     # one flag keeps the other fields
    check(got, _run(standin, raw, dict(E2E_CFG, SCENE_FLOAT=fixed)))
    assert fs.scene_float_override(Config(dict(SCENE_FLOAT=key)), gamma=2.0) == dict(key, gamma=2.0)
    monkeypatch.setattr(cli, "_build_net", lambda *a: (_ for _ in ()).throw(AssertionError("the model was built")))
    base = ["--config", "b.yaml", "--checkpoint", "none", "--device", "cpu", "--output_dir", "e", "--images", "raw.npy"]
    with pytest.raises(ValueError, match="select"):
        inf.main(base + ["--float-bands", "0,1", "--float-range", "0", "1"])
    with pytest.raises(ValueError, match="stretch is required"):
        inf.main(base + ["--float-gamma", "2"])
    with pytest.raises(ValueError, match="exclude"):
        inf.main(base + ["--float-range", "0", "9", "--float-percentile", "2", "98"])
    with pytest.raises(ValueError, match="SCENE_GROUP"):
        inf.main(base + ["--float-range", "0", "1", "--scene-group", "2"])
    with pytest.raises(ValueError, match="SCENE_BANDS"):
        inf.main(base + ["--float-range", "0", "1", "--bands", "0,1,2"])
