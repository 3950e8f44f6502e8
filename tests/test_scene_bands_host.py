"""SCENE_BANDS (16-bit and multi-band scenes: band selection and a lookup-table stretch on the device), the GPU-free part:
the key and its errors, the table and the percentile rule of sam_road_amd/radiometry.py, the apply kernel's addressing run item by item
on the CPU, and the orchestration of the scene loops through numpy scene_bands_hist / scene_bands_apply on a subclass of the CPU
stand-in of tests/scene_kit.py.  The feature is pinned by COMPOSITION: a run with the key on the raw scene equals, bit for bit, the
existing pipeline on the scene converted with the tables of the definition."""
import os
import shutil
import subprocess
import warnings

import numpy as np
import pytest
import torch

from sam_road_amd import Config
from sam_road_amd import cli
from sam_road_amd import inferencer as inf
from sam_road_amd.inferencer import infer_imgs, infer_one_img, scene_tiles
from sam_road_amd.radiometry import apply_luts, band_lut, band_luts, scene_bands_key, scene_bands_override, stretch_from_hist

from scene_kit import E2E_CFG, E2E_SCENE, SceneStandIn, assert_abi_11, compare_worlds, free_port, make_mask, run_cli
from test_scene_group_host import GroupStandIn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SELECT = [2, 0, 3]                                  # output R, G, B <- raw bands 2, 0, 3 of 4; band 1 is noise nobody may read
SCENE_SEED = 6                                      # the square scene of tests/test_scene_pad_host.py: > 30 nodes, > 100 edges on the stand-in


# ---- the stand-in with the two new methods -------------------------------------------------------------------------------------------
class BandsStandIn(GroupStandIn):
    """SceneStandIn (with the numpy pack and crop of a scene group, tests/test_scene_group_host.py) + scene_bands_hist /
    scene_bands_apply from numpy (np.bincount and a gather), logged; `tables` keeps every applied table set."""

    def __init__(self, cfg, features=()):
        super().__init__(cfg, features)
        self.tables = []

    def scene_bands_hist(self, src, select, valid=None):
        a = src.numpy().reshape(-1, src.shape[-1])
        levels = 256 if a.dtype == np.uint8 else 65536
        keep = slice(None) if valid is None else valid.numpy().reshape(-1) != 0
        self.calls.append(("bands_hist", tuple(select), valid is not None))
        return torch.from_numpy(np.stack([np.bincount(a[keep, b], minlength=levels) for b in select]).astype(np.uint32))

    def scene_bands_apply(self, src, select, lut):
        assert lut.dtype == torch.uint8 and tuple(lut.shape) == (3, 256 if src.dtype == torch.uint8 else 65536)
        self.calls.append(("bands_apply", tuple(select), str(src.dtype)))
        self.tables.append(lut.numpy().copy())
        return torch.from_numpy(np.ascontiguousarray(apply_luts(src.numpy(), list(select), lut.numpy())))


def raw_scene(u8, select=SELECT, C=4, seed=1):
    """u16 [H,W,C]: band select[b] = channel b of the u8 scene times 257 (so the full-range table gives the u8 scene back), noise elsewhere."""
    rng = np.random.default_rng(seed)
    raw = rng.integers(0, 65536, size=u8.shape[:2] + (C,), dtype=np.uint16)
    for b, s in enumerate(select):
        raw[..., s] = u8[..., b].astype(np.uint16) * 257
    return raw


def expected_tables(raw, key, valid=None):
    """The tables of the definition for this scene, from numpy alone (np.percentile where the key asks for one)."""
    levels = 256 if raw.dtype == np.uint8 else 65536
    k = scene_bands_key(Config(dict(SCENE_BANDS=key)))
    if k.percentile is None:
        ranges = k.ranges if k.ranges is not None else [(0, levels - 1)] * 3
    else:
        ranges = []
        for b in k.select:
            x = raw[..., b][np.ones(raw.shape[:2], bool) if valid is None else valid != 0]
            lo, hi = (int(v) for v in np.percentile(x, list(k.percentile), method="lower"))
            ranges.append((lo, hi if hi > lo else lo + 1))
    return np.stack([band_lut(lo, hi, k.gamma, levels) for lo, hi in ranges])


def _same_tuple(a, b):
    assert len(a) == len(b) == 4
    for x, y in zip(a, b):
        x, y = np.asarray(x), np.asarray(y)
        assert x.shape == y.shape and (x.dtype == y.dtype or x.size == 0), (x.shape, y.shape, x.dtype, y.dtype)
        np.testing.assert_array_equal(x, y)


# ---- the key ----------------------------------------------------------------------------------------------------------------------
def test_absent_key_is_off_and_every_accepted_form():
    for absent in (Config({}), Config(dict(SCENE_BANDS=None))):
        assert scene_bands_key(absent) is None
    k = scene_bands_key(Config(dict(SCENE_BANDS={"select": [0, 0, 0]})))
    assert k.select == (0, 0, 0) and k.ranges is None and k.percentile is None and k.gamma == 1.0
    k = scene_bands_key(Config(dict(SCENE_BANDS={"stretch": [10, 4000], "gamma": 2.2})))
    assert k.select == (0, 1, 2) and k.ranges == ((10, 4000),) * 3 and k.gamma == 2.2
    k = scene_bands_key(Config(dict(SCENE_BANDS={"select": [3, 2, 1], "stretch": [[0, 1], [5, 65535], [7, 9]]})))
    assert k.ranges == ((0, 1), (5, 65535), (7, 9))
    k = scene_bands_key(Config(dict(SCENE_BANDS={"stretch": {"percentile": [2, 98.5]}})))
    assert k.percentile == (2.0, 98.5) and k.ranges is None
    assert scene_bands_key(Config(dict(SCENE_BANDS={"stretch": {"percentile": [0, 100]}, "gamma": 0.5}))).percentile == (0.0, 100.0)


BAD_KEYS = [
    (7, "mapping"), ([0, 1, 2], "mapping"), ("rgb", "mapping"),
    ({"bands": [0, 1, 2]}, "unknown key 'bands'"), ({"select": [0, 1, 2], "strech": [0, 9]}, "unknown key 'strech'"),
    ({"select": [0, 1]}, "select"), ({"select": [0, 1, 2, 3]}, "select"), ({"select": [0, -1, 2]}, "select"), ({"select": [0, 1, 16]}, "select"),
    ({"select": [0, 1.0, 2]}, "select"), ({"select": [0, True, 2]}, "select"), ({"select": 3}, "select"),
    ({"stretch": [5, 5]}, "stretch"), ({"stretch": [9, 5]}, "stretch"), ({"stretch": [-1, 5]}, "stretch"), ({"stretch": [0, 65536]}, "stretch"),
    ({"stretch": [0.0, 5]}, "stretch"), ({"stretch": [0, 5, 9]}, "stretch"), ({"stretch": [[0, 5], [0, 5]]}, "stretch"),
    ({"stretch": [[0, 5], [0, 5], [5, 5]]}, "stretch"), ({"stretch": "auto"}, "stretch"),
    ({"stretch": {"percentile": [2, 98], "range": [0, 5]}}, "percentile"), ({"stretch": {"percent": [2, 98]}}, "percentile"),
    ({"stretch": {"percentile": [98, 2]}}, "percentile"), ({"stretch": {"percentile": [5, 5]}}, "percentile"),
    ({"stretch": {"percentile": [-1, 50]}}, "percentile"), ({"stretch": {"percentile": [0, 100.5]}}, "percentile"),
    ({"stretch": {"percentile": [0, float("nan")]}}, "percentile"), ({"stretch": {"percentile": [2]}}, "percentile"),
    ({"gamma": 0}, "gamma"), ({"gamma": -1.0}, "gamma"), ({"gamma": float("inf")}, "gamma"), ({"gamma": float("nan")}, "gamma"),
    ({"gamma": "2.2"}, "gamma"), ({"gamma": True}, "gamma"),
]


class Untouchable(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.w = torch.nn.Parameter(torch.zeros(1))

    def __getattr__(self, name):
        if name.startswith("scene_") or name.startswith("infer_"):
            raise AssertionError(f"the model was touched: {name}")
        return super().__getattr__(name)


def test_every_refusal_is_a_value_error_before_the_model_is_touched():
    net = Untouchable()
    H, W = 352, 352
    raw = np.zeros((H, W, 4), np.uint16)
    for v, what in BAD_KEYS:
        c = Config(dict(E2E_CFG, SCENE_BANDS=v))
        with pytest.raises(ValueError, match=what):
            scene_bands_key(c)
        with pytest.raises(ValueError, match=what):
            infer_one_img(net, raw, c, device="cpu")
        for kw in ({}, dict(tile_sharded=True), dict(tile_sharded=True, pipelined=True)):
            with pytest.raises(ValueError, match=what):
                list(infer_imgs(net, [raw], c, device="cpu", **kw))
    # what depends on the scene: the band count, the dtype, the range against the dtype's levels
    per_scene = [
        (raw[..., :3], {"select": [0, 1, 3]}, "needs more than the 3 band"),
        (np.zeros((H, W), np.uint16), {"select": [0, 0, 0]}, "HxWxC"),
        (np.zeros((H, W, 17), np.uint8), {"select": [0, 1, 2]}, "1 <= C <= 16"),
        (np.zeros((H, W, 4), np.int16), {"select": [0, 1, 2]}, "uint8 or uint16"),
        (np.zeros((H, W, 4), np.float32), {"select": [0, 1, 2]}, "uint8 or uint16"),
        (np.zeros((H, W, 4), np.uint8), {"stretch": [0, 256]}, "256 levels"),
        (np.zeros((H, W, 4), np.uint8), {"stretch": [[0, 255], [0, 255], [3, 1000]]}, "256 levels"),
        (np.zeros((0, W, 4), np.uint16), {"select": [0, 1, 2]}, "1 x 1"),
    ]
    for img, v, what in per_scene:
        c = Config(dict(E2E_CFG, SCENE_BANDS=v))
        with pytest.raises(ValueError, match=what):
            infer_one_img(net, img, c, device="cpu")
        with pytest.raises(ValueError, match=what):
            infer_one_img(net, img, c, device="cpu", valid=np.ones(img.shape[:2], bool))
        with pytest.raises(ValueError, match=what):
            list(infer_imgs(net, [img], c, device="cpu"))
    # a percentile stretch in a scene group: every scene would need its own tables in the middle of the group
    c = Config(dict(E2E_CFG, SCENE_BANDS={"stretch": {"percentile": [2, 98]}}))
    with pytest.raises(ValueError, match="percentile.*SCENE_GROUP|SCENE_GROUP.*percentile"):
        list(infer_imgs(net, [raw, raw], c, device="cpu", group=2))
    # without the key: today's message, for a u16 scene and for a 4-band one
    for img in (np.zeros((H, W, 3), np.uint16), np.zeros((H, W, 4), np.uint8)):
        with pytest.raises(ValueError, match="^infer_one_img expects an HxWx3 uint8 scene, got"):
            infer_one_img(net, img, Config(E2E_CFG), device="cpu")
    # the tile plan depends on the shape and the mask only
    assert list(scene_tiles((H, W), Config(dict(E2E_CFG, SCENE_BANDS={"select": [0, 0, 0]})))) == list(scene_tiles((H, W), Config(E2E_CFG)))


# ---- band_lut ---------------------------------------------------------------------------------------------------------------------------
def test_band_lut_endpoints_monotone_clipped_and_the_257_identity():
    v = np.arange(256)
    full = band_lut(0, 65535, 1, 65536)
    assert full.dtype == np.uint8 and full.shape == (65536,)
    np.testing.assert_array_equal(full[257 * v], v)                               # a u8 scene times 257 converts back to itself
    np.testing.assert_array_equal(band_lut(0, 255, 1, 256), v)
    for lo, hi, gamma, levels in ((0, 255, 1, 256), (17, 200, 1, 256), (100, 4095, 1, 65536), (100, 4095, 2.2, 65536), (3, 4, 0.45, 256),
                                  (65534, 65535, 1, 65536), (0, 65535, 2.2, 65536), (250, 256, 1, 256), (65000, 65536, 2.2, 65536)):
        t = band_lut(lo, hi, gamma, levels)
        assert t.dtype == np.uint8 and t.shape == (levels,)
        assert t[lo] == 0 and (hi >= levels or t[hi] == 255)
        assert (np.diff(t.astype(int)) >= 0).all()
        assert (t[:lo + 1] == 0).all() and (t[hi:] == 255).all()                  # clipped below and above the range
    # gamma 1 against the integer form round-half-up((255 (v - lo)) / (hi - lo))
    rng = np.random.default_rng(3)
    for _ in range(40):
        lo = int(rng.integers(0, 65535))
        hi = int(rng.integers(lo + 1, 65536))
        x = np.arange(65536, dtype=np.int64)
        want = (2 * 255 * np.clip(x - lo, 0, hi - lo) + (hi - lo)) // (2 * (hi - lo))
        np.testing.assert_array_equal(band_lut(lo, hi, 1, 65536), want.astype(np.uint8))
    for bad in ((5, 5, 1, 256), (9, 5, 1, 256), (0, 255, 0, 256), (0, 255, float("nan"), 256)):
        with pytest.raises(ValueError):
            band_lut(*bad)


def test_band_lut_gamma_matches_a_float64_loop():
    import math
    for lo, hi, levels in ((100, 4000, 65536), (0, 255, 256), (30, 31, 256)):
        want = np.empty(levels, np.uint8)
        for x in range(levels):
            t = min(max((x - lo) / (hi - lo), 0.0), 1.0)
            want[x] = int(math.floor(255.0 * t ** (1.0 / 2.2) + 0.5))
        np.testing.assert_array_equal(band_lut(lo, hi, 2.2, levels), want)
    assert not np.array_equal(band_lut(100, 4000, 2.2, 65536), band_lut(100, 4000, 1, 65536))
    t3 = band_luts([(0, 255), (0, 255), (10, 20)], 1, 256)
    assert t3.shape == (3, 256) and t3.dtype == np.uint8 and np.array_equal(t3[0], t3[1]) and not np.array_equal(t3[0], t3[2])


# ---- stretch_from_hist --------------------------------------------------------------------------------------------------------------------
def test_stretch_from_hist_is_the_sorted_index_rule():
    rng = np.random.default_rng(5)
    data = {"random": rng.integers(0, 65536, 5001), "narrow": rng.integers(300, 1800, 4097), "constant": np.full(777, 4242),
            "two_valued": np.where(rng.random(1001) < 0.3, 17, 60000), "u8": rng.integers(0, 256, 2001), "one_pixel": np.array([9])}
    for name, x in data.items():
        levels = 256 if name == "u8" else 65536
        for masked in (False, True):
            xs = x[rng.random(x.size) < 0.6] if masked and x.size > 1 else x
            N = xs.size
            hist = np.bincount(xs, minlength=levels)
            srt = np.sort(xs)
            for p_lo, p_hi in ((2, 98), (0, 100), (25, 50), (0.5, 99.5), (33.3, 33.4), (99, 100)):
                lo, hi = (int(srt[int(np.floor(np.float64(p) / 100.0 * (N - 1)))]) for p in (p_lo, p_hi))
                got = stretch_from_hist(hist, p_lo, p_hi)
                assert got == (lo, hi if hi > lo else lo + 1), (name, masked, p_lo, p_hi, got, lo, hi)
                assert all(isinstance(v, int) for v in got)
    # numpy's own "lower" percentile at p where p / 100 (N - 1) is an integer
    x = rng.integers(0, 4096, 4 * 500 + 1)
    hist = np.bincount(x, minlength=65536)
    for p in (0, 25, 50):
        want = int(np.percentile(x, p, method="lower"))
        assert stretch_from_hist(hist, p, 100)[0] == want
        assert want == int(np.sort(x)[p * 500 // 25])
    assert stretch_from_hist(hist, 0, 100) == (int(x.min()), int(x.max()))
    # a [3, levels] histogram gives three pairs
    h3 = np.stack([np.bincount(data["narrow"], minlength=65536), np.bincount(data["constant"], minlength=65536), np.zeros(65536, np.int64)])
    got = stretch_from_hist(h3.astype(np.uint32), 2, 98)
    assert got[0] == stretch_from_hist(h3[0], 2, 98) and got[1] == (4242, 4243) and got[2] == (0, 65535)


def test_stretch_from_hist_degenerate_cases():
    h = np.zeros(65536, np.int64)
    assert stretch_from_hist(h, 2, 98) == (0, 65535)                              # N = 0
    assert stretch_from_hist(np.zeros(256, np.uint32), 2, 98) == (0, 255)
    h[65535] = 10                                                                 # hi <= lo at the top level: hi = levels
    assert stretch_from_hist(h, 2, 98) == (65535, 65536)
    t = band_lut(65535, 65536, 1, 65536)
    assert t[65535] == 0 and not t.any()
    h = np.zeros(256, np.int64)
    h[[3, 200]] = (1000, 1)                                                       # the top percentile still falls on the lower value
    assert stretch_from_hist(h, 0, 99) == (3, 4)
    assert stretch_from_hist(h, 0, 100) == (3, 200)


# ---- the kernel's addressing, on the CPU ----------------------------------------------------------------------------------------------
def test_kernel_addressing_on_the_cpu(tmp_path):
    """tests/scene_bands_check.cpp runs every work item of an apply launch through the kernel's own per-item code
    (csrc/scene_bands_piece.hpp) as a stand-alone host program built with the address and undefined-behaviour sanitizers: a byte read past
    src or the tables or written outside dst ends it.  u8 at every byte address, u16 at every 2-byte-aligned one, dst at all 16
    misalignments, C in {1, 3, 4, 5, 16}, 1 to 4099 pixels."""
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    cxx = next((c for c in (os.path.join(rocm, "llvm", "bin", "clang++"), os.path.join(rocm, "lib", "llvm", "bin", "clang++")) if os.path.exists(c)), None)
    if cxx is None:
        pytest.skip("no ROCm clang++")
    exe = str(tmp_path / "scene_bands_check")
    csrc = os.path.join(ROOT, "sam_road_amd", "csrc")
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", csrc,
                        os.path.join(ROOT, "tests", "scene_bands_check.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    assert "scene bands OK" in r.stdout


def test_kernels_compile_for_gfx950_without_a_gpu():
    import re
    hipcc = next((c for c in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", shutil.which("hipcc")) if c and os.path.exists(c)), None)
    if hipcc is None:
        pytest.skip("hipcc not found")
    from sam_road_amd import build
    assert "scene_bands.hip" in build.SOURCES
    r = subprocess.run([hipcc, *build.FLAGS, "-S", "--cuda-device-only", os.path.join(build.CSRC, "scene_bands.hip"), "-o", "-"],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    for kernel, lds in (("scene_bands_apply_kernelIh", 0), ("scene_bands_apply_kernelIt", 0), ("scene_bands_hist_u8_kernel", 3072), ("scene_bands_hist_u16_kernel", 0)):
        m = re.search(r"^(_Z\w*%s\w*):" % kernel, r.stdout, re.M)
        assert m, f"{kernel} is not in the code object"
        meta = r.stdout[r.stdout.index(".amdhsa_kernel " + m.group(1)):]
        meta = meta[:meta.index(".end_amdhsa_kernel")]
        assert int(re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", meta).group(1)) == 0          # no scratch
        assert int(re.search(r"\.amdhsa_group_segment_fixed_size (\d+)", meta).group(1)) == lds
    assert "global_store_dwordx4" in r.stdout and "global_atomic_add " in r.stdout and "cmpswap" not in r.stdout


# ---- C ABI surface ------------------------------------------------------------------------------------------------------------------
def test_abi_has_the_entries_and_stays_11():
    from sam_road_amd import _lib
    header, _ = assert_abi_11([("srh_scene_bands_hist", 9), ("srh_scene_bands_apply", 9)])
    assert "SRH_I64 = 4, SRH_U16 = 5" in header and (_lib.SRH_U8, _lib.SRH_U16) == (2, 5)      # appended: the existing codes keep their values


# ---- the whole loop on the CPU stand-in ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def standin():
    warnings.simplefilter("ignore")
    torch.set_num_threads(4)
    return BandsStandIn(dict(E2E_CFG), ("valid",))


@pytest.fixture(scope="module")
def scene():
    from oracle.synth import synth_scene
    u8 = synth_scene(E2E_SCENE, seed=SCENE_SEED)
    return u8, raw_scene(u8)


@pytest.fixture(scope="module")
def stock_run(standin, scene):
    return infer_one_img(standin, scene[0], Config(E2E_CFG), device="cpu")


def _contract(standin, raw, key, valid=None, least=(30, 1)):
    """infer_one_img(raw, cfg + SCENE_BANDS) == infer_one_img(the tables of the definition applied with numpy, cfg), bit for bit."""
    tables = expected_tables(raw, key, valid)
    converted = np.ascontiguousarray(apply_luts(raw, scene_bands_key(Config(dict(SCENE_BANDS=key))).select, tables))
    assert converted.dtype == np.uint8 and converted.shape == raw.shape[:2] + (3,)
    kw = {} if valid is None else dict(valid=valid)
    want = infer_one_img(standin, converted, Config(E2E_CFG), device="cpu", **kw)
    raw_before = raw.copy()
    standin.calls.clear()
    standin.tables.clear()
    got = infer_one_img(standin, raw, Config(dict(E2E_CFG, SCENE_BANDS=key)), device="cpu", **kw)
    np.testing.assert_array_equal(raw, raw_before)
    _same_tuple(got, want)
    print(key, "nodes", want[0].shape[0], "edges", want[1].shape[0])
    assert want[0].shape[0] >= least[0] and want[1].shape[0] >= least[1]
    assert len(standin.tables) == 1
    np.testing.assert_array_equal(standin.tables[0], tables)
    return got, converted, list(standin.calls)


def test_contract_fixed_full_range_is_the_stock_scene(standin, scene, stock_run):
    u8, raw = scene
    got, converted, calls = _contract(standin, raw, {"select": SELECT})
    np.testing.assert_array_equal(converted, u8)                                  # 257 v -> v: the converted scene IS the stock one
    _same_tuple(got, stock_run)
    assert got[0].shape[0] > 30 and got[1].shape[0] > 100
    assert [c[0] for c in calls if c[0].startswith("bands")] == ["bands_apply"]   # a fixed range counts nothing
    # a u8 scene of three bands under the key takes the same path (what an image file does on the command line)
    standin.calls.clear()
    _same_tuple(infer_one_img(standin, u8, Config(dict(E2E_CFG, SCENE_BANDS={"select": [0, 1, 2]})), device="cpu"), stock_run)
    assert ("bands_apply", (0, 1, 2), "torch.uint8") in standin.calls


def test_contract_fixed_narrow_range_and_gamma(standin, scene):
    u8, raw = scene
    _, converted, _ = _contract(standin, raw, {"select": SELECT, "stretch": [[6000, 60000], [4000, 58000], [5000, 62000]], "gamma": 1.4})
    assert not np.array_equal(converted, u8)


def test_contract_percentile(standin, scene):
    u8, raw = scene
    _, converted, calls = _contract(standin, raw, {"select": SELECT, "stretch": {"percentile": [2, 98]}})
    assert [c for c in calls if c[0].startswith("bands")] == [("bands_hist", tuple(SELECT), False), ("bands_apply", tuple(SELECT), "torch.uint16")]
    assert not np.array_equal(converted, u8)


def test_contract_percentile_with_a_mask(standin, scene):
    """The invalid region holds 65535 in every band: a histogram that ignored the mask would put hi at 65535 and give other tables."""
    u8, raw = scene
    valid = make_mask("hole", E2E_SCENE, E2E_SCENE)
    raw = raw.copy()
    raw[~valid] = 65535
    key = {"select": SELECT, "stretch": {"percentile": [2, 99]}}
    assert not np.array_equal(expected_tables(raw, key, valid), expected_tables(raw, key))
    got, _, calls = _contract(standin, raw, key, valid=valid)
    order = [c[0] for c in calls if c[0] in ("bands_hist", "bands_apply", "tile_valid", "fill")]
    assert order == ["bands_hist", "bands_apply", "tile_valid", "fill"]           # histogram and conversion before the selection and the fill
    assert ("bands_hist", tuple(SELECT), True) in calls
    assert not got[2][~valid].any() and not got[3][~valid].any()


def test_key_absent_makes_no_new_call(scene, stock_run):
    """The stock SceneStandIn has neither method: a run without the key that called one would raise AttributeError."""
    plain = SceneStandIn(dict(E2E_CFG))
    assert not hasattr(plain, "scene_bands_hist") and not hasattr(plain, "scene_bands_apply")
    for cfg in (E2E_CFG, dict(E2E_CFG, SCENE_BANDS=None)):
        _same_tuple(infer_one_img(plain, scene[0], Config(cfg), device="cpu"), stock_run)
    with pytest.raises(ValueError, match="^infer_one_img expects an HxWx3 uint8 scene, got uint16"):
        infer_one_img(plain, scene[1], Config(E2E_CFG), device="cpu")
    with pytest.raises(AttributeError):                                           # and with the key it does call them
        infer_one_img(plain, scene[1], Config(dict(E2E_CFG, SCENE_BANDS={"select": SELECT})), device="cpu")


def test_the_scene_loops_and_groups_inherit_the_feature(standin, scene, stock_run):
    """infer_imgs (pipelined), both tile-sharded loops at world 1 and a scene group over [u16 4-band, u16 4-band crop, u8 5-band]: infer_one_img's
    tuples in order.  The group closes before the scene whose dtype and band count differ."""
    u8, raw = scene
    small = np.ascontiguousarray(raw[20:320, 10:330])
    rng = np.random.default_rng(2)
    other = rng.integers(0, 256, size=u8.shape[:2] + (5,), dtype=np.uint8)
    for b, s in enumerate(SELECT):
        other[..., s] = u8[..., b]
    cfg = Config(dict(E2E_CFG, SCENE_BANDS={"select": SELECT}))
    imgs = [raw, small, other]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        want = [infer_one_img(standin, im, cfg, device="cpu") for im in imgs]
        _same_tuple(want[0], stock_run)
        _same_tuple(want[2], stock_run)                                           # the u8 table of the full range is the identity
        for kw in ({}, dict(tile_sharded=True), dict(tile_sharded=True, pipelined=True), dict(group=3)):
            standin.calls.clear()
            got = list(infer_imgs(standin, iter(imgs), cfg, device="cpu", **kw))
            assert len(got) == 3
            for w, g in zip(want, got):
                _same_tuple(g, w)
            applies = [c for c in standin.calls if c[0] == "bands_apply"]
            if "group" in kw:                                                     # one launch for the two u16 scenes, one for the u8 scene alone
                assert applies == [("bands_apply", tuple(SELECT), "torch.uint16"), ("bands_apply", tuple(SELECT), "torch.uint8")]
            else:
                assert len(applies) == 3


# ---- world 2 on gloo -------------------------------------------------------------------------------------------------------------------
def _rank_worker(world, rank, port, out, key, masked):
    """One rank of the serial tile-sharded loop on gloo / CPU with the BandsStandIn: puts (rank, result tuple or None, applied tables)."""
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
        net = BandsStandIn(dict(E2E_CFG), ("valid",))
        raw = raw_scene(synth_scene(E2E_SCENE, seed=SCENE_SEED))
        kw = {}
        if masked:
            valid = make_mask("hole", E2E_SCENE, E2E_SCENE)
            raw[~valid] = 65535
            kw = dict(valid=valid)
        got = infer_one_img(net, raw, Config(dict(E2E_CFG, SCENE_BANDS=key)), device="cpu", **kw)
        out.put((rank, None if got is None else [np.asarray(a) for a in got], net.tables))
    except Exception:  # pragma: no cover
        import traceback
        out.put((rank, "ERR " + traceback.format_exc(), None))
    finally:
        dist.destroy_process_group()


def test_tile_sharded_world2_same_tables_on_both_ranks(standin, scene):
    """Every rank holds the scene and the mask, counts the same integers and builds the same tables — no collective; rank 0's result is
    the single-process one under the rule of scene_kit.compare_worlds."""
    import torch.multiprocessing as mp
    key = {"select": SELECT, "stretch": {"percentile": [2, 99]}}
    valid = make_mask("hole", E2E_SCENE, E2E_SCENE)
    raw = scene[1].copy()
    raw[~valid] = 65535
    one = infer_one_img(standin, raw, Config(dict(E2E_CFG, SCENE_BANDS=key)), device="cpu", valid=valid)
    ctx = mp.get_context("spawn")
    port, q = free_port(), ctx.Queue()
    procs = [ctx.Process(target=_rank_worker, args=(2, r, port, q, key, True)) for r in range(2)]
    for p in procs:
        p.start()
    got = dict((r, (v, t)) for r, v, t in (q.get(timeout=900) for _ in range(2)))
    for p in procs:
        p.join(timeout=60)
    for r, (v, _) in got.items():
        assert not isinstance(v, str), v
        assert (v is None) == (r != 0)
    assert len(got[0][1]) == len(got[1][1]) == 1
    np.testing.assert_array_equal(got[0][1][0], got[1][1][0])                     # identical tables on both ranks
    np.testing.assert_array_equal(got[0][1][0], expected_tables(raw, key, valid))
    compare_worlds([one], [got[0][0]], [(E2E_SCENE, E2E_SCENE)], ["hole"], must_be_identical=False)


# ---- CLI -----------------------------------------------------------------------------------------------------------------------------
def test_cli_takes_the_key_and_the_flags(tmp_path, monkeypatch, standin, scene, stock_run):
    from sam_road_amd.formats import convert_to_sat2graph_format
    u8, raw = scene
    monkeypatch.chdir(tmp_path)
    np.save("raw.npy", raw)

    def run(name, config, *argv):
        return run_cli(cli, standin, tmp_path, monkeypatch, name, config, ["raw.npy"], *argv)["raw"]

    def check(got, want):
        np.testing.assert_array_equal(got[0], want[2])
        np.testing.assert_array_equal(got[1], want[3])
        assert got[2] == convert_to_sat2graph_format(want[0], want[1])

    check(run("a", dict(E2E_CFG, SCENE_BANDS={"select": SELECT})), stock_run)     # the key comes from the YAML
    got = run("b", E2E_CFG, "--bands", "2,0,3")                                   # the flag sets it
    check(got, stock_run)
    assert got[3]["SCENE_BANDS"] == {"select": SELECT}
    key = {"select": SELECT, "stretch": {"percentile": [2.0, 98.0]}, "gamma": 1.4}
    want = infer_one_img(standin, raw, Config(dict(E2E_CFG, SCENE_BANDS=key)), device="cpu")
    got = run("c", dict(E2E_CFG, SCENE_BANDS={"select": [0, 1, 2], "stretch": [5, 9]}), "--bands", "2,0,3", "--stretch-percentile", "2", "98", "--gamma", "1.4")
    check(got, want)
    assert got[3]["SCENE_BANDS"] == key
    got = run("d", dict(E2E_CFG, SCENE_BANDS=key), "--stretch-range", "0", "65535", "--gamma", "1")       # one flag keeps the other fields
    assert got[3]["SCENE_BANDS"] == {"select": SELECT, "stretch": [0, 65535], "gamma": 1.0}
    check(got, stock_run)
    assert scene_bands_override(Config(dict(SCENE_BANDS=key)), gamma=2.0) == dict(key, gamma=2.0)
    monkeypatch.setattr(cli, "_build_net", lambda *a: (_ for _ in ()).throw(AssertionError("the model was built")))
    base = ["--config", "b.yaml", "--checkpoint", "none", "--device", "cpu", "--output_dir", "e", "--images", "raw.npy"]
    with pytest.raises(ValueError, match="select"):
        inf.main(base + ["--bands", "0,1"])
    with pytest.raises(ValueError, match="gamma"):
        inf.main(base + ["--gamma", "0"])
    with pytest.raises(ValueError, match="exclude"):
        inf.main(base + ["--stretch-range", "0", "9", "--stretch-percentile", "2", "98"])
    with pytest.raises(ValueError, match="SCENE_GROUP"):
        inf.main(base + ["--stretch-percentile", "2", "98", "--scene-group", "2"])
