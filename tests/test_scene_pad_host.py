"""SCENE_PAD (scenes padded at their borders on the device), the GPU-free part: the key and its errors, the geometry, the
fold against numpy.pad, the kernel's addressing run item by item on the CPU, the C-ABI surface, the CLI, scene_tiles, and the orchestration
of the scene loops through the numpy scene_pad of the CPU stand-in of tests/scene_kit.py.  The feature is pinned by
COMPOSITION: a run with the key equals the existing pipeline on the numpy-padded scene, cropped."""
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
from sam_road_amd.graph_points import extract_graph_points
from sam_road_amd.inferencer import edge_votes, infer_imgs, infer_one_img, scene_pad_key, scene_pad_plan, scene_tiles, votes_to_edges

from scene_kit import E2E_CFG as _E2E_CFG
from scene_kit import E2E_SCENE as _E2E_SCENE
from scene_kit import FILL, SceneStandIn, assert_abi_11, np_pad, run_cli, run_worlds

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODES = ("reflect", "edge", "constant")
GEO = dict(PATCH_SIZE=256, SAMPLE_MARGIN=16, INFER_PATCHES_PER_EDGE=2, MAX_NEIGHBOR_QUERIES=16)      # need = 288


# ---- the definition on the host -----------------------------------------------------------------------------------------------------
def pad_index(i, n, mode):
    """The source index of virtual index i (an int array, relative to the axis' first pixel) on an axis of n pixels — the definition of
    DESIGN.md §6g restated on the host (the kernel's own code is checked against a second restatement in tests/scene_pad_check.cpp):
    reflect: with T = 2 (n - 1), i mod T if that is below n, else T - (i mod T) (n = 1: 0); edge: clamped to [0, n - 1]; constant: -1
    outside [0, n) (the fill colour)."""
    i = np.asarray(i, dtype=np.int64)
    if mode == "reflect":
        if n == 1:
            return np.zeros_like(i)
        T = 2 * (n - 1)
        j = np.mod(i, T)
        return np.where(j < n, j, T - j)
    if mode == "edge":
        return np.clip(i, 0, n - 1)
    if mode == "constant":
        return np.where((i >= 0) & (i < n), i, -1)
    raise ValueError(f"mode must be one of {MODES}, got {mode!r}")


def pad_scene_host(arr, pads, mode, fill=(0, 0, 0)):
    """SAMRoad.scene_pad on the host, from pad_index: arr [H,W] or [H,W,3] -> the padded array."""
    arr = np.asarray(arr)
    top, bottom, left, right = pads
    H, W = arr.shape[:2]
    sy = pad_index(np.arange(-top, H + bottom), H, mode)
    sx = pad_index(np.arange(-left, W + right), W, mode)
    out = arr[np.maximum(sy, 0)][:, np.maximum(sx, 0)]
    outside = (sy < 0)[:, None] | (sx < 0)[None, :]
    if outside.any():
        out[outside] = np.asarray(fill, dtype=arr.dtype)[:arr.shape[2]] if arr.ndim == 3 else np.asarray(fill[0]).astype(arr.dtype)
    return np.ascontiguousarray(out)


# ---- the key ----------------------------------------------------------------------------------------------------------------------
def test_scene_pad_key_every_accepted_form():
    for absent in (Config({}), Config(dict(SCENE_PAD=None)), Config(dict(SCENE_PAD={}))):
        assert scene_pad_key(absent) is None and scene_pad_plan((400, 400, 3), Config(dict(GEO, **absent))) is None
    assert inf.SCENE_PAD_MODES == MODES
    for v, want in ((0, (0, 0, "reflect")), (24, (24, 24, "reflect")), (np.int64(7), (7, 7, "reflect")),
                    ({"border": 24}, (24, 24, "reflect")), ({"border": [8, 40]}, (8, 40, "reflect")), ({"border": (0, 3)}, (0, 3, "reflect")),
                    ({"mode": "edge"}, (0, 0, "edge")), ({"border": 5, "mode": "constant"}, (5, 5, "constant")),
                    ({"border": [1, 2], "mode": " Reflect "}, (1, 2, "reflect")), (Config({"border": 3}), (3, 3, "reflect"))):
        assert scene_pad_key(Config(dict(SCENE_PAD=v))) == want, v


BAD = [(-1, "border"), (True, "mapping"), (2.5, "mapping"), ("24", "mapping"), ([8, 40], "mapping"), ({"border": -3}, "border"),
       ({"border": [8, -1]}, "border"), ({"border": [8]}, "border"), ({"border": [1, 2, 3]}, "border"), ({"border": 2.0}, "border"),
       ({"border": "8"}, "border"), ({"border": [True, 1]}, "border"), ({"border": None}, "border"), ({"border": 8, "mode": "wrap"}, "mode"),
       ({"mode": 1}, "mode"), ({"mode": None}, "mode"), ({"border": 8, "fill": 0}, "unknown key"), ({"borders": 8}, "unknown key")]


def test_every_bad_scene_pad_is_a_value_error_before_the_model_is_touched():
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
    cfg = dict(_E2E_CFG, SAMPLE_MARGIN=0, INFER_PATCHES_PER_EDGE=[3, 5])
    cases = [(dict(SCENE_PAD=v), what) for v, what in BAD]
    cases += [(dict(SCENE_PAD=8, NODATA_FILL=[1, 2]), "NODATA_FILL"), (dict(SCENE_PAD={"mode": "constant"}, NODATA_FILL=[1, 2, 256]), "NODATA_FILL")]
    for extra, what in cases:
        c = Config(dict(cfg, **extra))
        with pytest.raises(ValueError, match=what):
            scene_pad_plan((H, W), c)
        with pytest.raises(ValueError, match=what):
            scene_tiles((H, W), c)
        with pytest.raises(ValueError, match=what):
            infer_one_img(net, img, c, device="cpu")
        with pytest.raises(ValueError, match=what):
            infer_one_img(net, img, c, device="cpu", valid=np.ones((H, W), bool))
        for kw in ({}, dict(tile_sharded=True), dict(tile_sharded=True, pipelined=True)):
            with pytest.raises(ValueError, match=what):
                list(infer_imgs(net, [img], c, device="cpu", **kw))
    # a scene that is too small, the 2^31 limit on the virtual size and an empty scene are refused there too
    with pytest.raises(ValueError, match="2\\^31 - 1 pixels"):
        infer_one_img(net, np.zeros((300, 300, 3), np.uint8), Config(dict(cfg, SCENE_PAD={"border": [40000, 30000]})), device="cpu")
    with pytest.raises(ValueError, match="1 x 1"):
        infer_one_img(net, np.zeros((0, 300, 3), np.uint8), Config(dict(cfg, SCENE_PAD=4)), device="cpu")
    with pytest.raises(ValueError, match="^scene height 200 px is smaller than PATCH_SIZE \\+ 2 \\* SAMPLE_MARGIN = 256.*SCENE_PAD"):
        infer_one_img(net, np.zeros((200, 300, 3), np.uint8), Config(cfg), device="cpu")


# ---- geometry -----------------------------------------------------------------------------------------------------------------------
def test_geometry_border_shortfall_and_both():
    plan = lambda shape, v, **kw: scene_pad_plan(shape, Config(dict(GEO, SCENE_PAD=v, **kw)))
    assert plan((400, 500), 24) == (24, 24, 24, 24, "reflect", FILL)                                   # border only
    assert plan((400, 500, 3), {"border": [8, 40], "mode": "edge"}) == (8, 8, 40, 40, "edge", FILL)
    assert plan((400, 500), 0) == (0, 0, 0, 0, "reflect", FILL)                                        # nothing to do: the plan says so
    assert plan((200, 300), 0) == (44, 44, 0, 0, "reflect", FILL)                                      # shortfall only: 288 - 200 = 88
    assert plan((200, 300), {"border": 0, "mode": "constant"}, NODATA_FILL=[1, 2, 3]) == (44, 44, 0, 0, "constant", (1, 2, 3))
    assert plan((200, 200), 10) == (10 + 34, 10 + 34, 10 + 34, 10 + 34, "reflect", FILL)               # both: 288 - 220 = 68
    assert plan((200, 300), {"border": [50, 0]}) == (50, 50, 0, 0, "reflect", FILL)                    # the border alone is enough
    assert plan((201, 283), 0) == (43, 44, 2, 3, "reflect", FILL)                                      # odd shortfalls 87 and 5: the extra pixel after
    assert plan((1, 1), 3) == (3 + 140, 3 + 141, 3 + 140, 3 + 141, "reflect", FILL)                    # 288 - 7 = 281
    for shape, v in (((200, 300), 0), ((201, 283), 7), ((1, 1), 3), ((37, 900), {"border": [0, 11]})):
        top, bottom, left, right, _, _ = plan(shape, v)
        assert shape[0] + top + bottom >= 288 and shape[1] + left + right >= 288
    # scene_tiles: tiles of the virtual scene, in the frame of the real one, and the four pads
    tiles = scene_tiles((200, 300), Config(dict(GEO, INFER_PATCHES_PER_EDGE=[1, 2], SCENE_PAD=0)))
    assert tiles.pads == (44, 44, 0, 0) and list(tiles) == [(0, (16, 16 - 44), (272, 272 - 44)), (0, (28, 16 - 44), (284, 272 - 44))]
    plain = scene_tiles((401, 523), Config(dict(GEO, INFER_PATCHES_PER_EDGE=4)))
    assert plain.pads == (0, 0, 0, 0) and scene_tiles((401, 523), Config(dict(GEO, INFER_PATCHES_PER_EDGE=4, SCENE_PAD=0))) == plain
    padded = scene_tiles((401, 523), Config(dict(GEO, INFER_PATCHES_PER_EDGE=4, SCENE_PAD=24)))
    virtual = scene_tiles((449, 571), Config(dict(GEO, INFER_PATCHES_PER_EDGE=4)))
    assert padded.pads == (24, 24, 24, 24) and len(padded) == len(plain) == 16                          # the tile count does not change
    assert list(padded) == [(k, (x0 - 24, y0 - 24), (x1 - 24, y1 - 24)) for k, (x0, y0), (x1, y1) in virtual]
    assert min(p[1][0] for p in padded) == 16 - 24 and max(p[2][1] for p in padded) == 401 + 24 - 16    # negative origin, overhang


def test_limits_on_the_virtual_size_and_absent_key():
    cfg = dict(GEO, INFER_PATCHES_PER_EDGE=1)
    with pytest.raises(ValueError, match="^scene height 200 px is smaller than PATCH_SIZE \\+ 2 \\* SAMPLE_MARGIN = 288"):
        scene_tiles((200, 300), Config(cfg))                                     # key absent: today's refusal
    with pytest.raises(ValueError, match="^scene width 287 px is smaller than"):
        scene_tiles((300, 287), Config(dict(cfg, SCENE_PAD=None)))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        assert len(scene_tiles((46340, 46340), Config(cfg))) == 1                # 2^31 - 1 = 2147483647 >= 46340^2 = 2147395600
        assert len(scene_tiles((46300, 46300), Config(dict(cfg, SCENE_PAD=20)))) == 1
        with pytest.raises(ValueError, match="2\\^31 - 1 pixels"):
            scene_tiles((46300, 46300), Config(dict(cfg, SCENE_PAD=21)))         # 46342^2 is over, the real scene is not
        with pytest.raises(ValueError, match="2\\^31 - 1 pixels"):
            scene_tiles((1, 2 ** 23), Config(dict(cfg, SCENE_PAD=0)))            # 288 rows x 2^23 columns
    # the stride warning speaks of the virtual size
    with pytest.warns(UserWarning, match=r"along the width \(648 px\)"):
        scene_tiles((300, 600), Config(dict(cfg, SCENE_PAD=24)))


# ---- the fold -----------------------------------------------------------------------------------------------------------------------
def test_fold_equals_numpy_pad():
    for n in range(1, 8):                                                        # the issue's check: axis lengths 1 to 7, pad widths up to 40
        a = np.arange(n)
        for before in (0, 1, 2, 5, 13, 40):
            for after in (0, 3, 40):
                i = np.arange(-before, n + after)
                np.testing.assert_array_equal(a[pad_index(i, n, "reflect")], np.pad(a, (before, after), mode="reflect"))
                np.testing.assert_array_equal(a[pad_index(i, n, "edge")], np.pad(a, (before, after), mode="edge"))
                c = pad_index(i, n, "constant")
                np.testing.assert_array_equal(np.where(c < 0, -7, a[np.maximum(c, 0)]), np.pad(a, (before, after), mode="constant", constant_values=-7))
    rng = np.random.default_rng(3)
    for (H, W), pads in (((40, 53), (124, 124, 0, 0)), ((1, 64), (2, 3, 70, 9)), ((64, 1), (70, 9, 2, 3)), ((1, 1), (5, 6, 7, 8)),
                         ((37, 53), (80, 3, 120, 0)), ((37, 53), (0, 0, 0, 0))):
        img = rng.integers(0, 256, size=(H, W, 3), dtype=np.uint8)
        mask = rng.random((H, W)) < 0.5
        for mode in MODES:
            got = pad_scene_host(img, pads, mode, FILL)
            np.testing.assert_array_equal(got, np_pad(img, pads, mode))
            assert got.dtype == np.uint8 and got.flags.c_contiguous
            for m in (mask, mask.astype(np.uint8) * 255):
                np.testing.assert_array_equal(pad_scene_host(m, pads, mode, (0, 0, 0)), np_pad(m, pads, mode, (0, 0, 0)))
    with pytest.raises(ValueError, match="mode"):
        pad_index(np.arange(3), 3, "wrap")


# ---- the kernel's addressing, on the CPU ----------------------------------------------------------------------------------------------
def test_kernel_addressing_on_the_cpu(tmp_path):
    """tests/scene_pad_check.cpp runs every work item of a launch through the kernel's own per-item code (csrc/scene_pad_piece.hpp) as a
    stand-alone host program built with the address and undefined-behaviour sanitizers: a byte read outside src or written outside dst
    ends it.  Source and destination at every misalignment, pads several times the axis, axes of length 1, rows of more than one group."""
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    cxx = next((c for c in (os.path.join(rocm, "llvm", "bin", "clang++"), os.path.join(rocm, "lib", "llvm", "bin", "clang++")) if os.path.exists(c)), None)
    if cxx is None:
        pytest.skip("no ROCm clang++")
    exe = str(tmp_path / "scene_pad_check")
    csrc = os.path.join(ROOT, "sam_road_amd", "csrc")
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", csrc,
                        os.path.join(ROOT, "tests", "scene_pad_check.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    assert "scene pad OK" in r.stdout


def test_kernel_compiles_for_gfx950_without_a_gpu():
    hipcc = next((c for c in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", shutil.which("hipcc")) if c and os.path.exists(c)), None)
    if hipcc is None:
        pytest.skip("hipcc not found")
    from sam_road_amd import build
    assert "scene_pad.hip" in build.SOURCES
    r = subprocess.run([hipcc, *build.FLAGS, "-S", "--cuda-device-only", os.path.join(build.CSRC, "scene_pad.hip"), "-o", "-"],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    for c in (1, 3):
        m = re.search(r"^(_Z\w*scene_pad_kernelILi%d\w*):" % c, r.stdout, re.M)
        assert m, f"scene_pad_kernel<{c}> is not in the code object"
        meta = r.stdout[r.stdout.index(".amdhsa_kernel " + m.group(1)):]
        meta = meta[:meta.index(".end_amdhsa_kernel")]
        assert int(re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", meta).group(1)) == 0          # no scratch
        assert int(re.search(r"\.amdhsa_group_segment_fixed_size (\d+)", meta).group(1)) == 0            # no LDS
    assert "global_load_dwordx4" in r.stdout and "global_store_dwordx4" in r.stdout and "atomic" not in r.stdout


# ---- C ABI surface ------------------------------------------------------------------------------------------------------------------
def test_abi_has_the_entry_and_stays_11():
    header, lib = assert_abi_11((("srh_scene_pad", 13),))
    for name, code in _lib.SRH_PAD_MODES.items():
        assert int(re.search(r"#define SRH_PAD_%s (\d+)" % name.upper(), header).group(1)) == code
    assert tuple(_lib.SRH_PAD_MODES) == MODES
    # refused without a context, before anything is launched
    assert lib.srh_scene_pad(None, None, 8, 8, 3, 0, 0, 0, 0, 0, None, None, None) == -1


# ---- the whole loop on the CPU stand-in ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def standin():
    warnings.simplefilter("ignore")
    torch.set_num_threads(4)
    return SceneStandIn(dict(_E2E_CFG), ("pad",))


def _hand_composition(net, cfg, img, pads, mode="reflect"):
    """The padded run from the parts that exist without the key: the existing pipeline on the numpy-padded scene, its masks cropped, the
    graph from those masks and that run's embeddings with the tiles moved to the real scene's frame."""
    top, bottom, left, right = pads
    H, W = img.shape[:2]
    plain = Config({k: v for k, v in cfg.items() if k != "SCENE_PAD"})
    padded = np_pad(img, pads, mode)
    _, infos, xy = inf._scene_plan(padded, plain)
    kp_c, road_c, emb = net.scene_pass1(torch.from_numpy(padded), torch.from_numpy(xy), int(plain.INFER_BATCH_SIZE))
    kp_v, road_v = (m.numpy() for m in net.scene_normalise(kp_c, road_c, torch.from_numpy(xy)))
    whole = infer_one_img(net, padded, plain, device="cpu")
    np.testing.assert_array_equal(whole[2], kp_v)
    np.testing.assert_array_equal(whole[3], road_v)
    kp, road = (np.ascontiguousarray(m[top:top + H, left:left + W]) for m in (kp_v, road_v))
    pts = extract_graph_points(kp, road, plain)
    shifted = [(k, (x0 - left, y0 - top), (x1 - left, y1 - top)) for k, (x0, y0), (x1, y1) in infos]
    edges = np.zeros((0, 2), dtype=np.int32)
    if pts.shape[0]:
        votes = edge_votes(net, emb, pts, shifted, 0, len(shifted), plain, torch.device("cpu"))
        edges = votes_to_edges(*votes, pts.shape[0], plain.TOPO_THRESHOLD)
        # the per-tile scipy queries of the reference agree with the library's on boxes that start below 0 or overhang the scene
        for t, q in enumerate(inf.build_all_patch_queries(pts, shifted, 0, len(shifted), plain)):
            want = inf.build_patch_queries(pts, *shifted[t][1], *shifted[t][2], plain)
            np.testing.assert_array_equal(q[0], want[0])
            np.testing.assert_array_equal(q[1], want[1])
            nbr = lambda x: np.sort(np.where(x[3], x[2][..., 1], -1), axis=1)
            np.testing.assert_array_equal(nbr(q), nbr(want))
    return (pts[:, ::-1], edges, kp, road), whole


def _same_tuple(a, b):
    assert len(a) == len(b) == 4
    for x, y in zip(a, b):
        x, y = np.asarray(x), np.asarray(y)
        assert x.shape == y.shape and (x.dtype == y.dtype or x.size == 0), (x.shape, y.shape, x.dtype, y.dtype)
        np.testing.assert_array_equal(x, y)


def _square_case():
    from oracle.synth import synth_scene
    return synth_scene(_E2E_SCENE, seed=6), dict(_E2E_CFG, SCENE_PAD=24), (24, 24, 24, 24)


def _small_case():
    from oracle.synth import synth_scene
    img = np.ascontiguousarray(synth_scene(_E2E_SCENE, seed=9)[60:260, 100:300])
    return img, dict(_E2E_CFG, INFER_PATCHES_PER_EDGE=1, SCENE_PAD={"border": 0}), (44, 44, 44, 44)


@pytest.fixture(scope="module")
def square_run(standin):
    img, cfg, pads = _square_case()
    want, whole = _hand_composition(standin, cfg, img, pads)
    return img, cfg, pads, want, whole, infer_one_img(standin, img, Config(cfg), device="cpu")


def test_whole_loop_square_scene_with_a_border(standin, square_run):
    img, cfg, pads, want, whole, got = square_run
    assert scene_pad_plan(img.shape, Config(cfg))[:4] == pads
    assert got[2].shape == got[3].shape == img.shape[:2] and got[2].dtype == np.uint8
    _same_tuple(got, want)
    print("nodes", got[0].shape[0], "edges", got[1].shape[0], "| padded-scene run: nodes", whole[0].shape[0])
    assert got[0].shape[0] > 30 and got[1].shape[0] > 100
    assert got[0][:, 0].max() < img.shape[0] and got[0][:, 1].max() < img.shape[1] and got[0].min() >= 0       # (row, col) of the real scene
    # the border does something: the unpadded run has a 16-px frame no tile covers, the padded one predicts there
    plain = infer_one_img(standin, img, Config(_E2E_CFG), device="cpu")
    assert not plain[3][:16].any() and got[3][:16].any()
    # border 0 on a scene that is large enough: the run without the key, and scene_pad is not called
    standin.calls.clear()
    _same_tuple(infer_one_img(standin, img, Config(dict(_E2E_CFG, SCENE_PAD={"border": 0, "mode": "edge"})), device="cpu"), plain)
    assert not [c for c in standin.calls if c[0] == "pad"]


def test_whole_loop_scene_smaller_than_a_tile(standin):
    img, cfg, pads = _small_case()
    assert img.shape == (200, 200, 3) and scene_pad_plan(img.shape, Config(cfg))[:4] == pads
    with pytest.raises(ValueError, match="smaller than"):
        infer_one_img(standin, img, Config({k: v for k, v in cfg.items() if k != "SCENE_PAD"}), device="cpu")
    want, _ = _hand_composition(standin, cfg, img, pads)
    got = infer_one_img(standin, img, Config(cfg), device="cpu")
    assert got[2].shape == got[3].shape == (200, 200)
    _same_tuple(got, want)
    print("nodes", got[0].shape[0], "edges", got[1].shape[0])
    assert got[0].shape[0] > 5 and got[1].shape[0] > 5
    assert got[3][:28].any() and got[3][-28:].any()                               # the one tile covers rows -28 .. 228 of the scene
    for mode in ("edge", "constant"):
        c = dict(cfg, SCENE_PAD={"border": 0, "mode": mode})
        _same_tuple(infer_one_img(standin, img, Config(c), device="cpu"), _hand_composition(standin, c, img, pads, mode)[0])


def test_the_scene_loops_inherit_the_feature(standin, square_run):
    """infer_imgs (pipelined), the serial tile-sharded loop and the pipelined tile-sharded loop (world 1) over [small, square, small]
    yield infer_one_img's tuples, in order: pad and crop live in the one front end."""
    img, cfg, _, _, _, got_sq = square_run
    small, cfg_s, _ = _small_case()
    cfg_all = dict(cfg, INFER_PATCHES_PER_EDGE=3)
    # one config for the three scenes: the small one then runs 3 x 3 tiles, all at the same origin
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        want = [infer_one_img(standin, im, Config(cfg_all), device="cpu") for im in (small, img, small)]
        _same_tuple(want[1], got_sq)
        for kw in ({}, dict(tile_sharded=True), dict(tile_sharded=True, pipelined=True)):
            got = list(infer_imgs(standin, iter([small, img, small]), Config(cfg_all), device="cpu", **kw))
            assert len(got) == 3
            for w, g in zip(want, got):
                _same_tuple(g, w)
    assert want[0][2].shape == (200, 200) and want[1][2].shape == (_E2E_SCENE, _E2E_SCENE)


# ---- world 2 on gloo -------------------------------------------------------------------------------------------------------------------
def test_tile_sharded_world2_matches_single_process(square_run):
    """The serial tile-sharded loop on gloo at world 2: the canvases of the virtual scene are reduced in column bands, rank 0 crops.  The
    f32 sums associate differently across ranks, so the masks may differ by one level (as tests/test_distributed_cpu.py allows at world 3)."""
    one = square_run[5]
    spec = dict(base="e2e", features=("pad",), overrides=dict(SCENE_PAD=24), shapes=[(_E2E_SCENE, _E2E_SCENE)], seeds=[6], mode="serial")
    n2, e2, k2, r2 = run_worlds((2,), spec)[2][0]
    n1, e1, k1, r1 = one
    assert k2.shape == k1.shape == (_E2E_SCENE, _E2E_SCENE)
    assert np.abs(k1.astype(int) - k2.astype(int)).max() <= 1 and np.abs(r1.astype(int) - r2.astype(int)).max() <= 1
    if np.array_equal(k1, k2) and np.array_equal(r1, r2):
        np.testing.assert_array_equal(n1, n2)
        np.testing.assert_array_equal(e1, e2)
    else:
        assert abs(n1.shape[0] - n2.shape[0]) <= 2


# ---- CLI -----------------------------------------------------------------------------------------------------------------------------
def test_cli_takes_the_key_and_the_flags(tmp_path, monkeypatch, standin, square_run):
    from PIL import Image
    from sam_road_amd.formats import convert_to_sat2graph_format
    img, cfg, _, _, _, with_border = square_run
    monkeypatch.chdir(tmp_path)
    Image.fromarray(img).save("rgb.png")
    plain, pad, edge = _E2E_CFG, dict(_E2E_CFG, SCENE_PAD={"border": 24}), dict(_E2E_CFG, SCENE_PAD={"border": 8, "mode": "edge"})

    def run(name, config, *argv):
        return run_cli(cli, standin, tmp_path, monkeypatch, name, config, ["rgb.png"], *argv)["rgb"]

    def check(got, want):
        np.testing.assert_array_equal(got[0], want[2])
        np.testing.assert_array_equal(got[1], want[3])
        assert got[2] == convert_to_sat2graph_format(want[0], want[1])

    check(run("a", pad), with_border)                                     # the key comes from the YAML
    got = run("b", plain, "--scene-pad", "24")                            # the flag sets it
    check(got, with_border)
    assert got[3]["SCENE_PAD"] == {"border": 24, "mode": "reflect"}
    got = run("c", edge, "--scene-pad", "24", "--scene-pad-mode", "reflect")      # both flags override the YAML
    check(got, with_border)
    got = run("d", edge, "--scene-pad-mode", "constant")                  # one flag keeps the other field of the YAML
    assert got[3]["SCENE_PAD"] == {"border": [8, 8], "mode": "constant"}
    check(got, infer_one_img(standin, img, Config(dict(_E2E_CFG, SCENE_PAD={"border": 8, "mode": "constant"})), device="cpu"))
    monkeypatch.setattr(cli, "_build_net", lambda *a: (_ for _ in ()).throw(AssertionError("the model was built")))
    with pytest.raises(ValueError, match="border"):
        inf.main(["--config", "b.yaml", "--checkpoint", "none", "--device", "cpu", "--output_dir", "e", "--images", "rgb.png", "--scene-pad", "-4"])
    with pytest.raises(SystemExit):
        inf.main(["--config", "b.yaml", "--checkpoint", "none", "--device", "cpu", "--output_dir", "e", "--images", "rgb.png", "--scene-pad-mode", "wrap"])
