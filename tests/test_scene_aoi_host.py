"""SCENE_AOI without a GPU: the key and its refusals, the rule against two independent restatements (exact rational
arithmetic from the vertices; matplotlib where it is installed), the kernel's own per-item code under the host sanitizers, the ABI, and the
whole loop on the CPU stand-in — a run with the key must equal, exactly, the same loop called with valid = aoi_ref(shape, key, valid)."""
import json
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
from sam_road_amd.aoi import (SceneAoi, aoi_edges, aoi_fill_ref, aoi_key_of, aoi_pack, aoi_ref, read_geojson, scene_aoi_key,
                              scene_aoi_override)
from sam_road_amd.inferencer import _empty_result, infer_imgs, infer_one_img, scene_tiles
from sam_road_amd.nodata import grow_ref, nodata_ref, scene_nodata_key

import scene_aoi_kit as ak
import scene_nodata_kit as nk
from scene_kit import E2E_CFG, HOST_CFG, SCENES, SceneStandIn, assert_abi_11, free_port, rect_scene, run_cli, same_tuple

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOX = [[[2, 3], [2, 9], [5, 9], [5, 3]]]                   # one polygon of one ring: rows [2, 5) x columns [3, 9)


def _key(v):
    return scene_aoi_key(Config(SCENE_AOI=v))


def _q(ring):
    return tuple((int(round(r * 256)), int(round(c * 256))) for r, c in ring)


# ---- the key --------------------------------------------------------------------------------------------------------------------------------------
def test_key_every_accepted_form():
    assert scene_aoi_key(Config()) is None and _key(None) is None and _key({}) is None
    k = _key([BOX])
    assert k == SceneAoi(((_q(BOX[0]),),), (), 0) == _key({"include": [BOX]}) == _key({"include": [BOX], "order": "rc", "buffer": 0, "exclude": []})
    # xy is [col, row]; a repeated closing vertex is dropped; tuples and numpy numbers serve
    xy = [[[3, 2], [9, 2], [9, 5], [3, 5], [3, 2]]]
    assert _key({"include": [xy], "order": " XY "}) == k == _key([tuple(tuple((np.float64(r), np.int64(c)) for r, c in BOX[0]) for _ in (0,))])
    # include absent or empty: the whole scene
    assert _key({"exclude": [BOX]}) == SceneAoi(None, ((_q(BOX[0]),),), 0) == _key({"include": [], "exclude": [BOX]})
    assert _key({"buffer": -16}) == SceneAoi(None, (), -16) and _key({"include": [BOX], "buffer": 16}).buffer == 16
    assert _key([]) == SceneAoi(None, (), 0)
    # quantisation: once, to 1 / 256 px, half to even
    ring = [[0.001953125, 0.005859375], [10, 0.0], [10, 10.00390625]]           # 0.5 / 256 -> 0, 1.5 / 256 -> 2
    assert _key([[ring]]).include[0][0] == ((0, 2), (2560, 0), (2560, 2561))
    assert aoi_key_of(k) is k


def test_geotransform_is_pinned_by_exact_vertices():
    # power-of-two coefficients: X = 1000 + 0.5 col, Y = 2000 - 0.25 row -> col = 2 (X - 1000), row = 4 (2000 - Y)
    gt = [1000.0, 0.5, 0.0, 2000.0, 0.0, -0.25]
    k = _key({"include": [[[[1001.5, 1999.5], [1004.5, 1999.5], [1004.5, 1998.75]]]], "geotransform": gt})
    assert k.include[0][0] == _q([(2, 3), (2, 9), (5, 9)])
    assert _key({"include": [[[[1001.5, 1999.5], [1004.5, 1999.5], [1004.5, 1998.75]]]], "geotransform": gt, "order": "xy"}) == k
    # rotated by 90 degrees with a scale of 2: X = 10 + 2 row, Y = 20 + 2 col -> row = (X - 10) / 2, col = (Y - 20) / 2
    rot = [10.0, 0.0, 2.0, 20.0, 2.0, 0.0]
    k = _key({"exclude": [[[[14, 26], [14, 38], [20, 38]]]], "geotransform": rot})
    assert k.exclude[0][0] == _q([(2, 3), (2, 9), (5, 9)])
    # a rotation by atan(3 / 4) with scale 5: X = 4 col - 3 row, Y = 3 col + 4 row; (row 4, col 3) -> X 0, Y 25
    k = _key({"include": [[[[0, 25], [25, 0], [50, 25]]]], "geotransform": [0, 4, -3, 0, 3, 4]})
    assert k.include[0][0] == _q([(4, 3), (-3, 4), (-2, 11)])


BAD_KEYS = ("x", 1.5, True, 7, {"includes": [BOX]}, {"include": [BOX], "order": "yx"}, {"include": [BOX], "order": 1}, {"include": [BOX], "order": None},
            {"include": [BOX], "order": "rc", "geotransform": [0, 1, 0, 0, 0, 1]}, {"include": [BOX], "geotransform": [0, 1, 2, 0, 2, 4]},
            {"include": [BOX], "geotransform": [0, 1, 0, 0, 0]}, {"include": [BOX], "geotransform": [0, 1, 0, 0, 0, float("nan")]},
            {"include": [BOX], "geotransform": [0, True, 0, 0, 0, 1]}, {"include": [BOX], "buffer": 17}, {"include": [BOX], "buffer": -17},
            {"include": [BOX], "buffer": 1.0}, {"include": [BOX], "buffer": True}, {"include": BOX}, {"include": [[[[0, 0], [1, 1]]]]},
            {"include": [[[[0, 0], [4, 4], [0, 0]]]]}, {"include": [[]]}, {"include": [[[[0, 0], [1, True], [2, 2]]]]}, {"include": [[[[0, 0], [1, "1"], [2, 2]]]]},
            {"include": [[[[0, 0], [1, float("inf")], [2, 2]]]]}, {"include": [[[[0, 0], [1, float("nan")], [2, 2]]]]}, {"include": [[[[0, 0], [1, 2 ** 20 + 1], [2, 2]]]]},
            {"include": [[[[0, 0, 0], [1, 1, 0], [2, 0, 0]]]]}, {"include": 5}, {"exclude": {"a": 1}}, [BOX] * 65, {"include": [BOX] * 40, "exclude": [BOX] * 25},
            [[[[0.0, float(i)] if i % 2 else [9.0, float(i)] for i in range(16386)]]])


class _Untouchable(torch.nn.Module):
    """A model object nothing may be called on: a refusal must come before the device is touched."""

    def __init__(self):
        super().__init__()
        self.w = torch.nn.Parameter(torch.zeros(1))


def test_every_refusal_is_a_value_error_before_the_model_is_touched():
    net, img = _Untouchable(), rect_scene(300, 300, 1)
    for bad in BAD_KEYS:
        with pytest.raises(ValueError, match="SCENE_AOI"):
            _key(bad)
        for call in (lambda cfg: infer_one_img(net, img, cfg, device="cpu"), lambda cfg: list(infer_imgs(net, iter([img]), cfg, device="cpu")),
                     lambda cfg: scene_tiles(img.shape, cfg, net=net)):
            with pytest.raises(ValueError, match="SCENE_AOI"):
                call(Config(dict(HOST_CFG, SCENE_AOI=bad)))
        good = Config(HOST_CFG)
        for call in (lambda: infer_one_img(net, img, good, device="cpu", aoi=bad), lambda: list(infer_imgs(net, iter([img]), good, device="cpu", aois=[bad])),
                     lambda: scene_tiles(img.shape, good, net=net, aoi=bad)):
            with pytest.raises(ValueError, match="SCENE_AOI"):
                call()
    # the limits are met exactly: 64 polygons, 16384 non-horizontal edges
    assert len(_key([BOX] * 64).include) == 64
    ring = [[0.0, float(i)] if i % 2 else [9.0, float(i)] for i in range(16384)]
    assert aoi_edges(_key([[ring]]), 10, 10)[1].tolist() == [0, 16384]
    # SCENE_GROUP > 1: one pixel-frame area for a stream of chips has no meaning
    for kw in (dict(cfg=dict(HOST_CFG, SCENE_AOI=[BOX]), group=2), dict(cfg=dict(HOST_CFG, SCENE_AOI=[BOX], SCENE_GROUP=3)), dict(cfg=dict(HOST_CFG), group=2, aois=[[BOX]])):
        cfg = Config(kw.pop("cfg"))
        with pytest.raises(ValueError, match="SCENE_AOI does not combine with SCENE_GROUP"):
            list(infer_imgs(net, iter([img, img]), cfg, device="cpu", **kw))
    assert len(scene_tiles(img.shape, Config(HOST_CFG))) == 25                   # without the key it is the call it was


def test_cli_flags_lay_over_the_key(tmp_path):
    xy = [[[3, 2], [9, 2], [9, 5], [3, 5]]]
    base = Config(SCENE_AOI={"include": [xy], "order": "xy", "buffer": 2})
    assert scene_aoi_override(base) == {"include": [xy], "order": "xy", "buffer": 2}
    assert scene_aoi_override(base, buffer=-3, exclude=[xy]) == {"include": [xy], "order": "xy", "buffer": -3, "exclude": [xy]}
    assert scene_aoi_override(Config(), include=[xy]) == {"include": [xy], "order": "xy"}
    assert scene_aoi_override(Config(), geotransform=[0, 1, 0, 0, 0, 1], include=[xy]) == {"include": [xy], "order": "xy", "geotransform": [0, 1, 0, 0, 0, 1]}
    assert scene_aoi_override(Config(SCENE_AOI=[BOX]), buffer=1) == {"include": [BOX], "buffer": 1}
    assert scene_aoi_override(Config(SCENE_AOI=[BOX]), include=[xy]) == {"include": [xy], "order": "xy"}      # replaced: nothing in rc is kept
    with pytest.raises(ValueError, match="order rc"):
        scene_aoi_override(Config(SCENE_AOI=[BOX]), exclude=[xy])
    with pytest.raises(ValueError, match="SCENE_AOI"):
        scene_aoi_override(Config(SCENE_AOI="x"), buffer=2)
    # the GeoJSON reader, every geometry type
    poly = {"type": "Polygon", "coordinates": [[[3, 2], [9, 2], [9, 5], [3, 5], [3, 2]]]}
    multi = {"type": "MultiPolygon", "coordinates": [poly["coordinates"], [[[0, 0, 7.5], [4, 0, 7.5], [0, 4, 7.5], [0, 0, 7.5]]]]}
    docs = {"polygon": (poly, 1), "multi": (multi, 2), "feature": ({"type": "Feature", "properties": {}, "geometry": poly}, 1),
            "collection": ({"type": "FeatureCollection", "features": [{"type": "Feature", "geometry": poly}, {"type": "Feature", "geometry": multi},
                                                                      {"type": "Feature", "geometry": None}]}, 3),
            "geometries": ({"type": "GeometryCollection", "geometries": [multi, poly]}, 3)}
    for name, (doc, n) in docs.items():
        path = tmp_path / f"{name}.geojson"
        path.write_text(json.dumps(doc))
        polys = read_geojson(str(path))
        assert len(polys) == n and all(len(p[0][0]) == 2 for p in polys)
        assert _key({"include": polys, "order": "xy"}).include[0 if name != "geometries" else 2] == _key([BOX]).include[0]
    for kind in ("Point", "LineString", "MultiPoint"):
        path = tmp_path / "bad.geojson"
        path.write_text(json.dumps({"type": "FeatureCollection", "features": [{"type": "Feature", "geometry": {"type": kind, "coordinates": [0, 0]}}]}))
        with pytest.raises(ValueError, match=kind):
            read_geojson(str(path))


# ---- the rule against independent restatements ----------------------------------------------------------------------------------------------------------
def test_the_two_rectangles_fill_exactly_their_18_pixels():
    want = np.zeros((8, 12), np.uint8)
    want[2:5, 3:9] = 1
    np.testing.assert_array_equal(aoi_ref((8, 12), _key(ak.menu(8, 12)["rect_int"])), want)
    np.testing.assert_array_equal(aoi_ref((8, 12), _key(ak.menu(8, 12)["rect_half"])), want)
    got = aoi_ref((8, 12, 3), _key([BOX]))
    assert got.dtype == np.uint8 and got.flags.c_contiguous and got.sum() == 18


def test_ref_equals_the_fraction_brute_force_on_random_rings():
    rng = np.random.default_rng(5)
    ties = 0
    for n in range(60):
        H, W = int(rng.integers(5, 15)), int(rng.integers(5, 17))
        nv = int(rng.integers(3, 9))
        if n % 3 == 0:                                    # vertices on pixel centres: every tie rule is exercised
            ring = [[int(rng.integers(-2, H + 2)) + 0.5, int(rng.integers(-2, W + 2)) + 0.5] for _ in range(nv)]
            ties += 1
        elif n % 3 == 1:                                  # multiples of 1 / 4 px: edges that pass exactly through centres are common
            ring = [[int(rng.integers(-8, 4 * H + 8)) / 4, int(rng.integers(-8, 4 * W + 8)) / 4] for _ in range(nv)]
        else:
            ring = [[float(rng.uniform(-3, H + 3)), float(rng.uniform(-3, W + 3))] for _ in range(nv)]
        got = aoi_ref((H, W), _key([[ring]]))
        np.testing.assert_array_equal(got, ak.fraction_ref((H, W), [[ring]]), err_msg=str(ring))
        tab = aoi_edges(_key([[ring]]), H, W)
        np.testing.assert_array_equal(got, ak.table_fill((H, W), *tab), err_msg=str(ring))
    assert ties == 20


def test_ref_equals_matplotlib_on_convex_polygons_without_ties():
    mpath = pytest.importorskip("matplotlib.path")
    rng = np.random.default_rng(9)
    for _ in range(40):
        H, W = int(rng.integers(20, 50)), int(rng.integers(20, 50))
        n = int(rng.integers(3, 9))
        ang = np.sort(rng.uniform(0, 2 * np.pi, n))
        # vertices on a 1 / 256 grid shifted by 1 / 1024: the quantisation is exact and no edge can pass through a centre exactly
        ring = [[(np.rint((H / 2 + 0.45 * H * np.sin(a)) * 256) / 256), (np.rint((W / 2 + 0.45 * W * np.cos(a)) * 256) / 256)] for a in ang]
        yy, xx = np.mgrid[0:H, 0:W]
        centres = np.stack([yy.ravel() + 0.5, xx.ravel() + 0.5], 1)
        inside = mpath.Path(np.asarray(ring)).contains_points(centres).reshape(H, W)
        got = aoi_ref((H, W), _key([[[list(map(float, p)) for p in ring]]])).astype(bool)
        on_edge = np.zeros((H, W), bool)                  # centres ON an edge (possible on the grid) are ties: left to the Fraction test
        for (ya, xa), (yb, xb) in zip(ring, ring[1:] + ring[:1]):
            cross = (centres[:, 0] - ya) * (xb - xa) - (centres[:, 1] - xa) * (yb - ya)
            on_edge |= (cross == 0).reshape(H, W)
        assert ((got != inside) & ~on_edge).sum() == 0


def test_the_menu_on_the_host():
    H, W = 37, 53
    m = {name: aoi_ref((H, W), _key(v)) for name, v in ak.menu(H, W).items()}
    f = lambda name: ak.fraction_ref((H, W), **({"include": ak.menu(H, W)[name]} if isinstance(ak.menu(H, W)[name], list) else
                                                 {k: v for k, v in ak.menu(H, W)[name].items() if k in ("include", "exclude")}))
    for name in ("bowtie", "hole", "union", "exclude", "exclude_only", "sliver", "partly_outside", "wholly_outside", "covers", "centre_vertex", "diagonal"):
        np.testing.assert_array_equal(m[name], f(name), err_msg=name)
    assert 0 < m["bowtie"].sum() < H * W and m["bowtie"][H // 2, 8] == 1 and m["bowtie"][8, W // 2] == 0     # even-odd: a left and a right lobe, above / below the crossing empty
    assert m["hole"][H // 2 - 2, W // 2] == 0 and m["hole"][5, 7] == 1 and m["hole"][0, 0] == 0
    a, b = (aoi_ref((H, W), _key([p])) for p in ak.menu(H, W)["union"])
    np.testing.assert_array_equal(m["union"], a | b)      # a union, not an XOR
    assert (a & b).any()
    inc = aoi_ref((H, W), _key(ak.menu(H, W)["exclude"]["include"]))
    exc = aoi_ref((H, W), _key(ak.menu(H, W)["exclude"]["exclude"]))
    np.testing.assert_array_equal(m["exclude"], inc & (1 - exc))
    assert exc.any() and m["exclude"].any()
    np.testing.assert_array_equal(m["exclude_only"], 1 - aoi_ref((H, W), _key(ak.menu(H, W)["exclude_only"]["exclude"])))
    assert not m["sliver"].any() and not m["wholly_outside"].any() and m["covers"].all() and 0 < m["partly_outside"].sum() < H * W
    assert m["diagonal"][5, 5] == 0 and m["diagonal"][5, 4] == 1 and m["diagonal"][6, 5] == 1     # a centre ON the long edge, a right edge: outside
    # xy is the transpose frame
    np.testing.assert_array_equal(m["xy"], aoi_ref((H, W), _key([[[[0.2 * H, 0.1 * W], [0.3 * H, 0.9 * W], [0.95 * H, 0.5 * W]]]])))
    # edges that cross no row are not in the table, and the table is include-first with running offsets
    e, o, ni, ne = aoi_edges(_key(ak.menu(H, W)["wholly_outside"]), H, W)
    assert e.shape == (0, 4) and e.dtype == np.int32 and o.tolist() == [0, 0, 0] and (ni, ne) == (2, 0)
    e, o, ni, ne = aoi_edges(_key(ak.menu(H, W)["exclude"]), H, W)
    assert o.tolist() == [0, 2, 5] and (ni, ne) == (1, 1) and (e[:, 0] < e[:, 2]).all()
    assert aoi_pack(e, o).tolist() == e.reshape(-1).tolist() + o.tolist() and aoi_pack(e[:0], o[:1]).tolist() == [0, 0, 0, 0, 0]


def test_buffers():
    H, W = 40, 45
    key = ak.menu(H, W)["exclude"]
    base = aoi_ref((H, W), _key(key))
    for b in (1, 16):
        np.testing.assert_array_equal(aoi_ref((H, W), _key(dict(key, buffer=b))), nk.window_max(base, b))
        np.testing.assert_array_equal(aoi_ref((H, W), _key(dict(key, buffer=-b))), 1 - nk.window_max(1 - base, b))
    assert aoi_ref((H, W), _key(dict(key, buffer=1))).sum() > base.sum() > aoi_ref((H, W), _key(dict(key, buffer=-1))).sum() > 0
    # nothing outside the image counts: a whole-scene area stays whole under a negative buffer
    for whole in ({"buffer": -16}, {"include": ak.menu(H, W)["covers"], "buffer": -5}):
        assert aoi_ref((H, W), _key(whole)).all()
    # the caller's mask is ANDed in behind the buffer
    caller = np.ones((H, W), bool)
    caller[:, 30:] = False
    np.testing.assert_array_equal(aoi_ref((H, W), _key(dict(key, buffer=2)), caller), grow_ref(base, 2) & caller)
    with pytest.raises(ValueError, match="shape"):
        aoi_ref((H, W), _key(key), caller[:5])
    np.testing.assert_array_equal(aoi_fill_ref((H, W), _key(dict(key, buffer=9))), base)


# ---- the kernel's own code, on the CPU ----------------------------------------------------------------------------------------------------------------
def test_kernel_addressing_on_the_cpu(tmp_path):
    """tests/scene_aoi_check.cpp runs every item of every phase of whole fill launches through the kernel's own per-item code
    (csrc/scene_aoi_piece.hpp) as a stand-alone host program built with the address and undefined-behaviour sanitizers, against a
    division-free restatement: out at every alignment mod 16, tables / and_with / out / LDS stand-in heap blocks of their exact sizes.  A
    byte read or written outside them ends it."""
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    cxx = next((c for c in (os.path.join(rocm, "llvm", "bin", "clang++"), os.path.join(rocm, "lib", "llvm", "bin", "clang++")) if os.path.exists(c)), None)
    if cxx is None:
        pytest.skip("no ROCm clang++")
    exe = str(tmp_path / "scene_aoi_check")
    csrc = os.path.join(ROOT, "sam_road_amd", "csrc")
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", csrc,
                        os.path.join(ROOT, "tests", "scene_aoi_check.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    assert "scene aoi OK" in r.stdout


def test_kernel_compiles_for_gfx950_without_a_gpu():
    hipcc = next((c for c in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", shutil.which("hipcc")) if c and os.path.exists(c)), None)
    if hipcc is None:
        pytest.skip("hipcc not found")
    from sam_road_amd import build
    assert "scene_aoi.hip" in build.SOURCES
    r = subprocess.run([hipcc, *build.FLAGS, "-S", "--cuda-device-only", os.path.join(build.CSRC, "scene_aoi.hip"), "-o", "-"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    m = re.search(r"^(_Z\w*scene_aoi_fill_kernel\w*):", r.stdout, re.M)
    assert m, "scene_aoi_fill_kernel is not in the code object"
    meta = r.stdout[r.stdout.index(".amdhsa_kernel " + m.group(1)):]
    meta = meta[:meta.index(".end_amdhsa_kernel")]
    assert int(re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", meta).group(1)) == 0              # no scratch
    assert int(re.search(r"\.amdhsa_group_segment_fixed_size (\d+)", meta).group(1)) == 1552             # AOI_LDS_BYTES, whatever W is
    assert int(re.search(r"\.amdhsa_uses_dynamic_stack (\d+)", meta).group(1)) == 0
    body = r.stdout[r.stdout.index(m.group(1) + ":"):r.stdout.index(".amdhsa_kernel " + m.group(1))]
    assert "global_atomic" not in body and "flat_atomic" not in body                                     # LDS atomics only
    assert "ds_xor_b32" in body and "ds_or_b32" in body and "global_load_dwordx4" in body and "global_store_dwordx4" in body


# ---- C ABI surface ----------------------------------------------------------------------------------------------------------------------------------------
def test_abi_has_the_entry_and_stays_11():
    header, lib = assert_abi_11((("srh_scene_aoi_fill", 13),))
    assert "SCENE_AOI" in header
    assert lib.srh_scene_aoi_fill(None, None, None, None, None, 1, 0, 4, 4, None, 0, None, None) == -1      # refused without a context


# ---- the whole loop on the CPU stand-in ---------------------------------------------------------------------------------------------------------------------
H, W, PER_EDGE, SEED = SCENES["401x523"]
CFG = dict(HOST_CFG, INFER_PATCHES_PER_EDGE=PER_EDGE)
TRIANGLE = [[[[-10.0, -10.0], [330.5, -10.0], [-10.0, 420.25]]]]          # over the scene's origin corner: leaves tiles out
HOLED = {"include": [[[[20, 30], [380.5, 60], [390, 500.25], [40, 480]], [[150, 200], [160.5, 330], [260, 320.25], [250, 210]]]], "exclude": [[[[300, 100], [390, 120], [380, 220]]]],
         "buffer": 2}
_NETS = {}


def standin(*features):
    warnings.simplefilter("ignore")
    torch.set_num_threads(4)
    if features not in _NETS:
        _NETS[features] = ak.AoiStandIn(dict(CFG), features)
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
def scene():
    return nk.plain_scene(H, W, SEED)


def test_infer_one_img_equals_the_composition(scene):
    net = standin("valid")
    plain = _run(net, scene, CFG)
    assert not ak.aoi_calls(net)                                                 # with the key absent the new method is never called
    for kw in (TRIANGLE, HOLED, dict(HOLED, buffer=-3), {"exclude": TRIANGLE}):
        key = _key(kw)
        valid = aoi_ref((H, W), key)
        want = _run(net, scene, CFG, valid=valid)
        net.calls.clear()
        got = _run(net, scene, dict(CFG, SCENE_AOI=kw))
        same_tuple(got, want)
        assert not got[2][valid == 0].any() and not got[3][valid == 0].any() and got[3].any() and (got[3] != plain[3]).any()
        names = [c[0] for c in net.calls if c[0] in ("aoi_fill", "nodata_grow", "nodata_match", "mask_clean")]
        assert names == ["aoi_fill"] + ["nodata_grow"] * (key.buffer != 0)       # ONE launch, plus the grow for a buffer
        assert ak.aoi_calls(net)[0][-1] is (key.buffer < 0)                      # the shrink: the fill writes the complement
    # a caller's mask is ANDed in, by the last step
    caller = np.ones((H, W), bool)
    caller[250:, 300:] = False
    for kw in (TRIANGLE, HOLED):
        net.calls.clear()
        got = _run(net, scene, dict(CFG, SCENE_AOI=kw), valid=caller)
        same_tuple(got, _run(net, scene, CFG, valid=aoi_ref((H, W), _key(kw), caller)))
        last = [c for c in net.calls if c[0] in ("aoi_fill", "nodata_grow")][-1]
        assert (last[-2] if last[0] == "aoi_fill" else last[3]) is True and not got[3][250:, 300:].any()
    # aoi= takes the place of the config's key; None means the key
    same_tuple(_run(net, scene, dict(CFG, SCENE_AOI=HOLED), aoi=TRIANGLE), _run(net, scene, CFG, valid=aoi_ref((H, W), _key(TRIANGLE))))
    same_tuple(_run(net, scene, dict(CFG, SCENE_AOI=TRIANGLE), aoi=None), _run(net, scene, CFG, aoi=TRIANGLE))
    # an area that holds no pixel: the empty result, nothing is run
    net.calls.clear()
    same_tuple(_run(net, scene, dict(CFG, SCENE_AOI=ak.menu(H, W)["sliver"])), _empty_result(H, W))
    assert not [c for c in net.calls if c[0] == "pass1"]
    # the plan of scene_tiles is the run's: through the stand-in's device entry with net, through aoi_ref without, and the two agree
    for extra in ({}, dict(MIN_VALID_FRACTION=0.5), dict(SCENE_SCALE=[2, 3])):
        cfg = Config(dict(CFG, SCENE_AOI=TRIANGLE, **extra))
        base = {k: v for k, v in cfg.items() if k != "SCENE_AOI"}
        net = standin("valid")
        tiles = scene_tiles(scene.shape, cfg, net=net)
        assert ak.aoi_calls(net)
        assert list(tiles) == list(scene_tiles(scene.shape, cfg)) == list(scene_tiles(scene.shape, Config(base), valid=aoi_ref((H, W), _key(TRIANGLE)), net=net))
        assert list(tiles) == list(scene_tiles(scene.shape, Config(base), aoi=TRIANGLE)) and 0 < len(tiles) < len(scene_tiles(scene.shape, Config(base)))
        assert (tiles.scale, tiles.model_shape) == (scene_tiles(scene.shape, Config(base)).scale, scene_tiles(scene.shape, Config(base)).model_shape)
    with pytest.raises(ValueError, match="needs the model"):
        scene_tiles(scene.shape, Config(CFG), valid=np.ones((H, W), bool))


def test_the_pipelined_loop_over_the_three_scene_kinds_and_per_scene_aois(scene):
    net = standin("valid")
    wide, small = nk.plain_scene(384, 640, 41), nk.plain_scene(300, 421, 7)
    key = _key(TRIANGLE)
    imgs = [scene, wide, small, scene]
    wants = [_run(net, im, CFG, valid=aoi_ref(im.shape, key)) for im in imgs]
    net.calls.clear()
    res = _loop(net, imgs, dict(CFG, SCENE_AOI=TRIANGLE))
    assert len(res) == 4 and len(ak.aoi_calls(net)) == 4
    for got, want in zip(res, wants):
        same_tuple(got, want)
    # the serial tile-sharded loop (world 1) and the pipelined tile-sharded one inherit it
    for kw in (dict(tile_sharded=True), dict(tile_sharded=True, pipelined=True)):
        for got, want in zip(_loop(net, imgs, dict(CFG, SCENE_AOI=TRIANGLE), **kw), wants):
            same_tuple(got, want)
    # per-scene areas, parallel to the scenes: a value takes the key's place, None is the key, a sliver gives the empty result
    aois = [None, HOLED, ak.menu(300, 421)["sliver"]]                           # shorter than the scenes: the rest is None
    keys = [key, _key(HOLED), _key(aois[2]), key]
    for kw in ({}, dict(tile_sharded=True), dict(tile_sharded=True, pipelined=True)):
        res = _loop(net, imgs, dict(CFG, SCENE_AOI=TRIANGLE), aois=aois, **kw)
        for got, im, k in zip(res, imgs, keys):
            same_tuple(got, _run(net, im, CFG, valid=aoi_ref(im.shape, k)))
        same_tuple(res[2], _empty_result(300, 421))
    # without a key in the config: only the scenes that bring one are masked
    res = _loop(net, imgs[:2], CFG, aois=iter([None, TRIANGLE]), valids=[None, np.ones((384, 640), np.uint8)])
    same_tuple(res[0], _run(net, scene, CFG))
    same_tuple(res[1], wants[1])
    # with the key absent the stand-in's new method is never called, masked or not, and a model without it serves
    net.calls.clear()
    _loop(net, imgs[:2], CFG, valids=[aoi_ref(scene.shape, key), None])
    _loop(net, imgs[:2], dict(CFG, SCENE_AOI=None), aois=[None, None])
    _loop(net, imgs[:1], dict(CFG, SCENE_AOI={}))
    assert not ak.aoi_calls(net) and not [c for c in net.calls if c[0] == "nodata_grow"]
    bare = SceneStandIn(dict(CFG))
    assert not hasattr(bare, "scene_aoi_fill")
    same_tuple(_loop(bare, [scene], CFG)[0], _run(net, scene, CFG))


def test_scene_pad_scene_scale_window_and_tta(scene):
    key = _key(HOLED)
    valid = aoi_ref((H, W), key)
    # SCENE_SCALE [1, 2]: the area is in SCENE pixels; its mask is resampled by the validity rule and kept as zero_where for the way back
    net = standin("valid")
    big = nk.plain_scene(2 * H, 2 * W, SEED)
    doubled = {"include": [[[[2 * r, 2 * c] for r, c in ring] for ring in poly] for poly in HOLED["include"]], "buffer": 3}
    scaled = dict(CFG, SCENE_SCALE=[1, 2])
    vbig = aoi_ref(big.shape, _key(doubled))
    got = _run(net, big, dict(scaled, SCENE_AOI=doubled))
    same_tuple(got, _run(net, big, scaled, valid=vbig))
    assert got[2].shape == (2 * H, 2 * W) and not got[3][vbig == 0].any() and got[3].any()
    # SCENE_PAD 24: the area is in the REAL scene's frame; its mask is padded like a passed one
    net = standin("valid", "pad")
    padded = dict(CFG, SCENE_PAD=24)
    got = _run(net, scene, dict(padded, SCENE_AOI=HOLED))
    same_tuple(got, _run(net, scene, padded, valid=valid))
    assert [c[0] for c in net.calls if c[0] in ("aoi_fill", "pad", "pass1")][:4] == ["aoi_fill", "pad", "pad", "pass1"] and got[3].any()
    assert list(scene_tiles(scene.shape, Config(dict(padded, SCENE_AOI=TRIANGLE)), net=net)) == list(scene_tiles(scene.shape, Config(dict(padded, SCENE_AOI=TRIANGLE))))
    # hann with TTA = [id, rot90]
    net = standin("valid", "window", "tta")
    aug = dict(CFG, FUSE_WINDOW="hann", TTA=["id", "rot90"])
    got = _run(net, scene, dict(aug, SCENE_AOI=HOLED))
    same_tuple(got, _run(net, scene, aug, valid=valid))
    assert got[3].any() and not got[3][valid == 0].any()


def test_scene_nodata_and_scene_aoi_together():
    net = standin("valid")
    img, _ = nk.collar_scene(H, W, SEED)
    nd = dict(value=0, tolerance=3, min_area=50, grow=2)
    far = {"include": [[[[60, 80], [390.5, 100], [395, 510.25], [80, 500]]]], "buffer": -2}      # away from the origin: the collar cuts into it
    caller = np.ones((H, W), np.uint8)
    caller[:, 470:] = 0
    for valid in (None, caller):
        both = nodata_ref(img, scene_nodata_key(Config(SCENE_NODATA=nd)), aoi_ref((H, W), _key(far), valid))
        net.calls.clear()
        got = _run(net, img, dict(CFG, SCENE_NODATA=nd, SCENE_AOI=far), **({} if valid is None else dict(valid=valid)))
        same_tuple(got, _run(net, img, CFG, valid=both))
        order = [c[0] for c in net.calls if c[0] in ("aoi_fill", "nodata_match", "mask_clean", "nodata_grow")]
        assert order == ["aoi_fill", "nodata_grow", "nodata_match", "mask_clean", "nodata_grow"]          # each with its own grow, the AOI in front
        assert got[3].any() and (both != aoi_ref((H, W), _key(far), valid)).any()
    # u16, four bands, a percentile stretch: the histogram counts the pixels of the area
    raw, _ = nk.raw16_scene(H, W, SEED)
    cfg = dict(CFG, SCENE_BANDS=dict(select=[2, 1, 0], stretch=dict(percentile=[2, 98])))
    want = _run(net, raw, cfg, valid=aoi_ref((H, W), _key(far)))
    net.calls.clear()
    got = _run(net, raw, dict(cfg, SCENE_AOI=far))
    same_tuple(got, want)
    order = [c[0] for c in net.calls if c[0] in ("aoi_fill", "nodata_grow", "bands_hist", "bands_apply")]
    assert order == ["aoi_fill", "nodata_grow", "bands_hist", "bands_apply"] and [c for c in net.calls if c[0] == "bands_hist"][0][2] is True


# 512 x 512 in four disjoint tiles, one per batch: every canvas pixel has ONE addend and every tile runs alone in both worlds
GLOO_AOI = {"include": [[[[-5, -5], [400.5, -5], [500, 300.25], [-5, 505]]]], "buffer": 1}
GLOO_CFG = dict(E2E_CFG, SAMPLE_MARGIN=0, INFER_PATCHES_PER_EDGE=2, INFER_BATCH_SIZE=1, SCENE_AOI=GLOO_AOI)


def _rank(world, rank, port, out):
    """One rank of a tile-sharded run on gloo / CPU: puts (rank, infer_one_img's result, its aoi calls)."""
    import torch.distributed as dist
    warnings.simplefilter("ignore")
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        torch.set_num_threads(2)
        net = ak.AoiStandIn(dict(GLOO_CFG), ("valid",))
        res = infer_one_img(net, nk.plain_scene(512, 512, 6), Config(GLOO_CFG), device="cpu")
        out.put((rank, None if res is None else [np.asarray(a) for a in res], [c[0] for c in net.calls if c[0] in ("aoi_fill", "nodata_grow")]))
    except Exception:  # pragma: no cover
        import traceback
        out.put((rank, "ERR " + traceback.format_exc(), None))
    finally:
        dist.destroy_process_group()


def test_tile_sharded_world2_equals_world1_and_every_rank_fills_the_mask():
    import torch.multiprocessing as mp
    warnings.simplefilter("ignore")
    torch.set_num_threads(2)                                                     # as the ranks
    net, img = ak.AoiStandIn(dict(GLOO_CFG), ("valid",)), nk.plain_scene(512, 512, 6)
    one = infer_one_img(net, img, Config(GLOO_CFG), device="cpu")
    unkeyed = {k: v for k, v in GLOO_CFG.items() if k != "SCENE_AOI"}
    same_tuple(one, infer_one_img(net, img, Config(unkeyed), device="cpu", valid=aoi_ref((512, 512), _key(GLOO_AOI))))
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
    # every rank holds the table and fills the same mask: the same two steps on both, no collective
    assert got[1][0] is None and got[0][1] == got[1][1] == ["aoi_fill", "nodata_grow"]
    same_tuple(got[0][0], one)


def test_cli_takes_the_flags(tmp_path, monkeypatch, scene):
    from PIL import Image
    from sam_road_amd.formats import convert_to_sat2graph_format
    net = standin("valid")
    monkeypatch.chdir(tmp_path)
    other = nk.plain_scene(384, 640, 41)
    Image.fromarray(scene).save("a.png")
    Image.fromarray(other).save("b.png")
    xy = lambda polys: [[[[c, r] for r, c in ring] for ring in poly] for poly in polys]
    with open("tri.geojson", "w") as f:
        json.dump({"type": "Feature", "geometry": {"type": "Polygon", "coordinates": xy(TRIANGLE)[0]}}, f)
    with open("holed.geojson", "w") as f:
        json.dump({"type": "MultiPolygon", "coordinates": xy(HOLED["include"])}, f)
    with open("cut.geojson", "w") as f:
        json.dump({"type": "FeatureCollection", "features": [{"type": "Feature", "geometry": {"type": "Polygon", "coordinates": xy(HOLED["exclude"])[0]}}]}, f)
    with open("line.geojson", "w") as f:
        json.dump({"type": "LineString", "coordinates": [[0, 0], [5, 5]]}, f)

    def check(got, want):
        np.testing.assert_array_equal(got[0], want[2])
        np.testing.assert_array_equal(got[1], want[3])
        assert got[2] == convert_to_sat2graph_format(want[0], want[1])

    # one file for every scene, the exclude and the buffer beside it
    got = run_cli(cli, net, tmp_path, monkeypatch, "one", CFG, ["a.png", "b.png"], "--aoi", "holed.geojson", "--aoi-exclude", "cut.geojson", "--aoi-buffer", "2")
    assert _key(got["a"][3]["SCENE_AOI"]) == _key(HOLED)
    check(got["a"], _run(net, scene, CFG, valid=aoi_ref((H, W), _key(HOLED))))
    check(got["b"], _run(net, other, CFG, valid=aoi_ref((384, 640), _key(HOLED))))
    # one file per scene, '-' for a scene without one; the config's buffer stays, the flag's geotransform maps the files
    gt = ["100", "0.5", "0", "50", "0", "0.25"]                                  # X = 100 + col / 2, Y = 50 + row / 4
    with open("tri_map.geojson", "w") as f:
        json.dump({"type": "Polygon", "coordinates": [[[100 + c / 2, 50 + r / 4] for r, c in TRIANGLE[0][0]]]}, f)
    got = run_cli(cli, net, tmp_path, monkeypatch, "per", dict(CFG, SCENE_AOI={"buffer": 1}), ["a.png", "b.png"], "--aoi", "tri_map.geojson", "-", "--aoi-geotransform", *gt)
    check(got["a"], _run(net, scene, CFG, valid=aoi_ref((H, W), _key({"include": TRIANGLE, "buffer": 1}))))
    check(got["b"], _run(net, other, CFG))                                       # no include, no exclude: the whole scene, whatever the buffer
    with pytest.raises(ValueError, match="LineString"):
        run_cli(cli, net, tmp_path, monkeypatch, "bad", CFG, ["a.png"], "--aoi", "line.geojson")
    with pytest.raises(ValueError, match="SCENE_AOI"):
        run_cli(cli, net, tmp_path, monkeypatch, "bad2", CFG, ["a.png"], "--aoi", "tri.geojson", "--aoi-buffer", "17")
    with pytest.raises(ValueError, match="SCENE_GROUP"):
        run_cli(cli, net, tmp_path, monkeypatch, "bad3", CFG, ["a.png", "b.png"], "--aoi", "tri.geojson", "--scene-group", "2")
