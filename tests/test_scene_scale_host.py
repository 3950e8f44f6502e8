"""SCENE_SCALE (scenes at another ground resolution, resampled on the device), the GPU-free part: the tables, the rule
against exact rational arithmetic, the key and its errors, the node map, the kernel's addressing run block by block on the CPU, the C-ABI
surface, and the orchestration of the scene loops through a CPU stand-in whose scene_resample IS resample_ref.  The feature is pinned by
COMPOSITION: a run with the key equals the existing pipeline on the numpy-resampled scene, its masks resampled back and its nodes mapped."""
import math
import os
import subprocess
import warnings
from fractions import Fraction

import numpy as np
import pytest
import torch

from sam_road_amd import Config
from sam_road_amd import cli
from sam_road_amd import inferencer as inf
from sam_road_amd import resample as rs
from sam_road_amd.inferencer import infer_imgs, infer_one_img, scene_tiles
from sam_road_amd.resample import axis_tables, map_nodes, resample_ref, scene_scale_key

from scene_kit import E2E_CFG, SceneStandIn, assert_abi_11, make_mask, rect_scene, run_cli

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# every reduced fraction inside the limits: 1 <= p, q <= 16, 1/8 <= p/q <= 4, not 1/1
SCALES = [(p, q) for p in range(1, 17) for q in range(1, 17) if math.gcd(p, q) == 1 and p != q and q <= 8 * p and p <= 4 * q]
NAMED = [(1, 2), (2, 3), (3, 10), (1, 8), (2, 1), (3, 2), (4, 1), (5, 3), (10, 3), (16, 15), (15, 16)]
GEO = dict(PATCH_SIZE=256, SAMPLE_MARGIN=16, INFER_PATCHES_PER_EDGE=2, MAX_NEIGHBOR_QUERIES=16, ITSC_NMS_RADIUS=8, ROAD_NMS_RADIUS=16)


# ---- the tables -------------------------------------------------------------------------------------------------------------------------
def test_tables_of_every_scale():
    assert set(NAMED) <= set(SCALES) and len(SCALES) > 100
    for p, q in SCALES:
        for n in (1, 2, 7, 37, 64):
            n_out = -(-n * p // q)
            s, w, T, D = axis_tables(n, p, q)
            assert s.dtype == np.int32 and w.dtype == np.uint8 and s.shape == (n_out,) and w.shape == (n_out, T)
            assert rs.out_size(n, p, q) == n_out == math.ceil(Fraction(n * p, q))
            assert (T, D) == ((-(-q // p) + 1, q) if p < q else (2, 2 * p)) and D * D <= 1024
            assert (w.astype(np.int64).sum(axis=1) == D).all()               # u8: every weight is >= 0 and fits
            assert (np.diff(s) >= 0).all() and s.min() >= -1
            # every tap with a non-zero weight lies inside the input or is a clamped copy of its border pixel, and within T of the start
            idx = s[:, None].astype(np.int64) + np.arange(T)[None, :]
            assert idx[w > 0].min() >= -1 and (idx[w > 0] - s[:, None].repeat(T, 1)[w > 0]).max() < T
            # the way back from ceil(n p / q) yields exactly n, the clamp catching what overhangs
            sb, wb, Tb, Db = axis_tables(n_out, q, p, n)
            assert sb.shape == (n,) and wb.shape == (n, Tb) and (wb.astype(np.int64).sum(axis=1) == Db).all() and (np.diff(sb) >= 0).all()
            back = resample_ref(np.full((n_out, n_out), 7, np.uint8), q, p, out_shape=(n, n))
            assert back.shape == (n, n) and (back == 7).all()
    for bad in ((0, 1, 2), (5, 0, 2), (5, 2, 0), (5, 3, 3)):
        with pytest.raises(ValueError):
            axis_tables(*bad)
    with pytest.raises(ValueError):
        axis_tables(5, 1, 2, 0)


def test_block_plan_fits_lds_at_every_scale():
    for p, q in SCALES + [(q, p) for p, q in SCALES]:
        for C in (1, 3):
            T = axis_tables(8, p, q)[2]
            bh, bw, win_h, win_w = rs.block_plan(T, T, p, q, C)
            assert 1 <= bh == bw <= 64 and rs.lds_bytes(win_h, win_w, bw, C) <= rs.LDS_BUDGET <= 64 * 1024
            # the window holds the taps of any bh consecutive outputs
            s = axis_tables(4000, p, q)[0].astype(np.int64)
            span = (s[bh - 1:] + T - 1 - s[:len(s) - bh + 1]).max() + 1
            assert span <= win_h, (p, q, span, win_h)
    assert rs.block_plan(9, 9, 1, 8, 3)[0] >= 8 and rs.block_plan(3, 3, 1, 2, 3)[0] >= 32      # (1/8: the 9 x 9 taps of the issue)


# ---- resample_ref against exact rational arithmetic --------------------------------------------------------------------------------------
def _axis_terms(j, n, p, q):
    """[(input index, rational weight)] of output j on an axis of n pixels, weights summing to 1 — the restatement: the area integral over
    [j q/p, (j + 1) q/p) of the edge-extended piecewise-constant signal, or linear interpolation at the output pixel's centre."""
    r = Fraction(q, p)                                        # input pixels per output pixel
    clamp = lambda i: min(max(i, 0), n - 1)
    if p < q:
        lo, hi = j * r, (j + 1) * r
        return [(clamp(i), (min(hi, i + 1) - max(lo, i)) / r) for i in range(math.floor(lo), math.ceil(hi))]
    x = (j + Fraction(1, 2)) * r - Fraction(1, 2)             # the centre of output j in input coordinates
    i0 = math.floor(x)
    return [(clamp(i0), 1 - (x - i0)), (clamp(i0 + 1), x - i0)]


def _exact(arr, p, q, out_shape=None):
    H, W = arr.shape[:2]
    Ho, Wo = out_shape or (math.ceil(Fraction(H * p, q)), math.ceil(Fraction(W * p, q)))
    a3 = arr.reshape(H, W, -1)
    out = np.zeros((Ho, Wo, a3.shape[2]), dtype=arr.dtype)
    for y in range(Ho):
        ty = _axis_terms(y, H, p, q)
        for x in range(Wo):
            tx = _axis_terms(x, W, p, q)
            for c in range(a3.shape[2]):
                v = sum(wy * wx * int(a3[iy, ix, c]) for iy, wy in ty for ix, wx in tx)
                out[y, x, c] = math.floor(v + Fraction(1, 2))        # rounded half up, once
    return out.reshape((Ho, Wo) + arr.shape[2:])


def test_resample_ref_equals_the_rational_restatement():
    rng = np.random.default_rng(5)
    img, row = rng.integers(0, 256, size=(5, 7, 3), dtype=np.uint8), rng.integers(0, 256, size=(1, 9), dtype=np.uint8)
    for p, q in NAMED:
        for arr in (img, row):
            got = resample_ref(arr, p, q)
            assert got.dtype == np.uint8 and got.flags.c_contiguous
            np.testing.assert_array_equal(got, _exact(arr, p, q), err_msg=f"{p}/{q} {arr.shape}")
            # the way back to the array's own size, from the resampled one
            np.testing.assert_array_equal(resample_ref(got, q, p, out_shape=arr.shape[:2]), _exact(got, q, p, arr.shape[:2]))
        const = np.full((6, 11, 3), 201, np.uint8)
        assert (resample_ref(const, p, q) == 201).all() and (resample_ref(const[..., 0], p, q, out_shape=(9, 4)) == 201).all()
    with pytest.raises(ValueError):
        resample_ref(img.astype(np.float32), 1, 2)
    with pytest.raises(ValueError):
        resample_ref(img, 1, 2, zero_where=np.ones((2, 2), np.uint8))


def test_validity_rule_and_zero_where_on_hand_made_masks():
    m = np.ones((4, 8), bool)
    m[1, 5] = False
    # 1/2: output (y, x) covers the 2 x 2 block (2y.., 2x..) — the third tap of T = 3 has weight 0 and does not count
    got = resample_ref(m, 1, 2, valid_rule=True)
    want = np.ones((2, 4), bool)
    want[0, 2] = False
    assert got.dtype == bool
    np.testing.assert_array_equal(got, want)
    u8 = resample_ref(m.astype(np.uint8) * 200, 1, 2, valid_rule=True)
    assert u8.dtype == np.uint8
    np.testing.assert_array_equal(u8, want.astype(np.uint8))              # a u8 mask comes out with value 1
    # 2/1: output j reads inputs floor((2j - 1) / 4), + 1 with weights (4 - f, f), f = 1 or 3: both taps count, except at the clamped border
    line = np.array([[1, 1, 0, 1]], bool)
    np.testing.assert_array_equal(resample_ref(line, 2, 1, valid_rule=True), np.array([[1, 1, 1, 0, 0, 0, 0, 1]] * 2, bool))
    # an all-valid mask stays all valid, at every scale; nothing is valid where nothing was
    for p, q in NAMED:
        assert resample_ref(np.ones((9, 13), bool), p, q, valid_rule=True).all()
        assert not resample_ref(np.zeros((9, 13), np.uint8), p, q, valid_rule=True).any()
    # zero_where: 0 wherever it is 0, untouched elsewhere
    img = np.full((2, 4), 90, np.uint8)
    zw = np.array([[1, 0, 1, 1, 0, 1, 1, 1]] * 4, bool)
    back = resample_ref(img, 2, 1, out_shape=(4, 8), zero_where=zw)
    np.testing.assert_array_equal(back, np.where(zw, 90, 0).astype(np.uint8))
    np.testing.assert_array_equal(resample_ref(img, 2, 1, out_shape=(4, 8), zero_where=zw.astype(np.uint8) * 255), back)


# ---- the key ------------------------------------------------------------------------------------------------------------------------------
def test_scene_scale_key_every_accepted_form():
    key = lambda v, **kw: scene_scale_key(Config(dict(GEO, SCENE_SCALE=v, **kw)))
    for absent in (Config(GEO), Config(dict(GEO, SCENE_SCALE=None)), Config(dict(GEO, SCENE_SCALE={}))):
        assert scene_scale_key(absent) is None
    assert key([1, 2]) == key([2, 4]) == key((8, 16)) == (1, 2) and key([3, 3]) is None and key([16, 16]) is None
    assert key([4, 1]) == (4, 1) and key([1, 8]) == (1, 8) and key([np.int64(15), 16]) == (15, 16)
    assert key({"scene_gsd": 0.5, "model_gsd": 1.0}) == key({"scene_gsd": 0.5}) == (1, 2)
    assert key({"scene_gsd": 0.3, "model_gsd": 1.0}) == (3, 10) and key({"scene_gsd": 1.2, "model_gsd": 1.0}) == (6, 5)
    assert key({"scene_gsd": 0.6, "model_gsd": 0.3}) == (2, 1) and key({"scene_gsd": 1, "model_gsd": 1}) is None
    assert key([1, 2], SCENE_GROUP=1) == (1, 2) and key([2, 1], ITSC_NMS_RADIUS=4, ROAD_NMS_RADIUS=4) == (2, 1)      # 4 * 1 >= 2 * 2


BAD = [([1, 9], "reduces to 1/9"), ([5, 1], "reduces to 5/1"), ([17, 16], "17/16"), ([32, 2], "16/1"), ({"scene_gsd": 0.37, "model_gsd": 1.0}, r"\[p, q\]"),
       ({"scene_gsd": 5.0}, "5/1"), ({"scene_gsd": 0.5, "gsd": 1}, "unknown key"), ({"model_gsd": 1.0}, "positive numbers"),
       ({"scene_gsd": -0.5}, "positive numbers"), ({"scene_gsd": "0.5"}, "positive numbers"), ({"scene_gsd": float("nan")}, "positive numbers"),
       ([0, 2], "two ints"), ([1, 2, 3], "two ints"), ([1.0, 2], "two ints"), ([True, 2], "two ints"), (0.5, "two ints"), ("1/2", "two ints")]


def test_every_bad_scene_scale_is_a_value_error_before_the_model_is_touched():
    class Untouchable(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.w = torch.nn.Parameter(torch.zeros(1))

        def __getattr__(self, name):
            if name.startswith("scene_") or name.startswith("infer_"):
                raise AssertionError(f"the model was touched: {name}")
            return super().__getattr__(name)

    net = Untouchable()
    H, W = 600, 700
    img = np.zeros((H, W, 3), np.uint8)
    cases = [(dict(SCENE_SCALE=v), what) for v, what in BAD]
    cases += [(dict(SCENE_SCALE=[4, 1], ITSC_NMS_RADIUS=1), "one scene pixel"), (dict(SCENE_SCALE=[3, 2], ROAD_NMS_RADIUS=2, ITSC_NMS_RADIUS=8), "one scene pixel"),
              (dict(SCENE_SCALE=[1, 2], SCENE_GROUP=2), "SCENE_GROUP")]
    for extra, what in cases:
        c = Config(dict(E2E_CFG, **extra))
        with pytest.raises(ValueError, match=what):
            scene_scale_key(c)
        with pytest.raises(ValueError, match=what):
            scene_tiles((H, W), c)
        with pytest.raises(ValueError, match=what):
            infer_one_img(net, img, c, device="cpu")
        with pytest.raises(ValueError, match=what):
            infer_one_img(net, img, c, device="cpu", valid=np.ones((H, W), bool))
        for kw in ({}, dict(tile_sharded=True), dict(tile_sharded=True, pipelined=True)):
            with pytest.raises(ValueError, match=what):
                list(infer_imgs(net, [img], c, device="cpu", **kw))
    with pytest.raises(ValueError, match="SCENE_GROUP"):                     # the group given as infer_imgs' argument
        list(infer_imgs(net, [img], Config(dict(E2E_CFG, SCENE_SCALE=[1, 2])), device="cpu", group=3))
    # the size limits apply to the model frame: 500 x 500 at 1/2 is 250 x 250, smaller than a tile; at 2/1 it is large enough
    with pytest.raises(ValueError, match="^scene height 250 px is smaller than"):
        infer_one_img(net, np.zeros((500, 500, 3), np.uint8), Config(dict(E2E_CFG, SCENE_SCALE=[1, 2])), device="cpu")
    with pytest.raises(ValueError, match="^scene height 200 px is smaller than"):
        scene_tiles((200, 200), Config(E2E_CFG))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        assert scene_tiles((200, 200), Config(dict(E2E_CFG, SCENE_SCALE=[2, 1]))).model_shape == (400, 400)
        with pytest.raises(ValueError, match="2\\^31 - 1 pixels"):               # 46340^2 fits, four times as many pixels do not
            scene_tiles((46340, 46340), Config(dict(E2E_CFG, SCENE_SCALE=[2, 1])))
        with pytest.raises(ValueError, match="2\\^31 - 1 pixels"):               # the scene itself, whatever the model frame
            scene_tiles((2 ** 16, 2 ** 15), Config(dict(E2E_CFG, SCENE_SCALE=[1, 8])))


def test_absent_key_and_unit_scale_give_the_plan_of_a_run_without_the_key():
    cfg = dict(GEO, INFER_PATCHES_PER_EDGE=4)
    plain = scene_tiles((401, 523), Config(cfg))
    assert plain.scale == (1, 1) and plain.model_shape == (401, 523)
    for v in (None, [3, 3], {"scene_gsd": 2.0, "model_gsd": 2.0}):
        t = scene_tiles((401, 523), Config(dict(cfg, SCENE_SCALE=v)))
        assert t == plain and (t.scale, t.model_shape, t.pads, t.orientations) == ((1, 1), (401, 523), plain.pads, plain.orientations)
    # with the key the plan is the model frame's, pads included
    half = scene_tiles((802, 1046), Config(dict(cfg, SCENE_SCALE=[1, 2])))
    assert half == plain and half.scale == (1, 2) and half.model_shape == (401, 523)
    padded = scene_tiles((801, 1045), Config(dict(cfg, SCENE_SCALE=[2, 4], SCENE_PAD=24)))
    assert padded == scene_tiles((401, 523), Config(dict(cfg, SCENE_PAD=24))) and padded.pads == (24, 24, 24, 24) and padded.model_shape == (401, 523)
    up = scene_tiles((268, 349), Config(dict(cfg, SCENE_SCALE=[3, 2])))
    assert up == scene_tiles((402, 524), Config(cfg)) and up.model_shape == (402, 524)


def test_cli_flags_lay_over_the_key():
    over = rs.scene_scale_override
    assert over(Config({}), scale=[1, 2]) == [1, 2] and over(Config(dict(SCENE_SCALE=[3, 2])), scale=(2, 4)) == [2, 4]
    assert over(Config({}), scene_gsd=0.5) == {"scene_gsd": 0.5, "model_gsd": 1.0}
    assert over(Config(dict(SCENE_SCALE={"scene_gsd": 0.5, "model_gsd": 2.0})), scene_gsd=0.25) == {"scene_gsd": 0.25, "model_gsd": 2.0}
    assert over(Config(dict(SCENE_SCALE={"scene_gsd": 0.5})), model_gsd=2.0) == {"scene_gsd": 0.5, "model_gsd": 2.0}
    assert over(Config(dict(SCENE_SCALE=[1, 2])), scene_gsd=0.3, model_gsd=1.0) == {"scene_gsd": 0.3, "model_gsd": 1.0}
    for kw in (dict(scale=[1, 2], scene_gsd=0.5), dict(model_gsd=1.0)):
        with pytest.raises(ValueError, match="SCENE_SCALE"):
            over(Config({}), **kw)


# ---- the node map ---------------------------------------------------------------------------------------------------------------------------
def test_node_map_lands_inside_the_scene_on_a_tap_of_the_point():
    for p, q in SCALES:
        for n in range(1, 41):
            s, w, T, _ = axis_tables(n, p, q)                 # scene -> model: the taps the validity rule looks at
            n_m = s.shape[0]
            r = np.arange(n_m, dtype=np.int64)
            nodes = map_nodes(np.stack([r, r], 1), (n, n), p, q)
            assert nodes.dtype == np.int64 and nodes.min() >= 0 and nodes.max() <= n - 1
            np.testing.assert_array_equal(nodes[:, 0], np.minimum(n - 1, ((2 * r + 1) * q) // (2 * p)))
            taps = np.clip(s[:, None].astype(np.int64) + np.arange(T)[None, :], 0, n - 1)
            assert ((taps == nodes[:, :1]) & (w > 0)).any(axis=1).all(), (p, q, n)
    # rows and columns are mapped by their own axis, the dtype is kept, an empty array passes through
    got = map_nodes(np.array([[0, 5], [200, 3]], np.int32), (401, 12), 1, 2)
    assert got.dtype == np.int32 and got.tolist() == [[1, 11], [400, 7]]
    assert map_nodes(np.zeros((0, 2), np.int64), (5, 5), 1, 2).shape == (0, 2)
    # two points at least min(NMS radius) apart in the model frame never share a scene pixel when radius * q >= 2 p (the key's condition)
    for p, q in ((4, 1), (3, 2), (10, 3)):
        d = -(-2 * p // q)
        r = np.arange(0, 400, d, dtype=np.int64)
        assert len(set(map_nodes(np.stack([r, r], 1), (10 ** 6, 10 ** 6), p, q)[:, 0].tolist())) == len(r)


# ---- the kernel's addressing, on the CPU ------------------------------------------------------------------------------------------------------
def test_kernel_addressing_on_the_cpu(tmp_path):
    """tests/scene_scale_check.cpp runs every block of a launch through the kernel's own per-item code (csrc/scene_scale_piece.hpp) as a
    stand-alone host program built with the address and undefined-behaviour sanitizers: a byte read outside src or the tables, or written
    outside dst, ends it.  Scales 1/8, 2/3, 3/2, 4 and their ways back; shapes 1 x 64, 64 x 1, 37 x 53, 3 x 6000; every misalignment."""
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    cxx = next((c for c in (os.path.join(rocm, "llvm", "bin", "clang++"), os.path.join(rocm, "lib", "llvm", "bin", "clang++")) if os.path.exists(c)), None)
    if cxx is None:
        pytest.skip("no ROCm clang++")
    exe = str(tmp_path / "scene_scale_check")
    csrc = os.path.join(ROOT, "sam_road_amd", "csrc")
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", csrc,
                        os.path.join(ROOT, "tests", "scene_scale_check.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    assert "scene scale OK" in r.stdout


def test_kernel_compiles_for_gfx950_without_a_gpu():
    import re
    import shutil
    hipcc = next((c for c in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", shutil.which("hipcc")) if c and os.path.exists(c)), None)
    if hipcc is None:
        pytest.skip("hipcc not found")
    from sam_road_amd import build
    r = subprocess.run([hipcc, *build.FLAGS, "-S", "--cuda-device-only", os.path.join(build.CSRC, "scene_scale.hip"), "-o", "-"],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    m = re.search(r"^(_Z\w*scene_scale_kernel\w*):", r.stdout, re.M)
    assert m, "scene_scale_kernel is not in the code object"
    meta = r.stdout[r.stdout.index(".amdhsa_kernel " + m.group(1)):]
    meta = meta[:meta.index(".end_amdhsa_kernel")]
    assert int(re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", meta).group(1)) == 0              # no scratch
    assert int(re.search(r"\.amdhsa_group_segment_fixed_size (\d+)", meta).group(1)) == 0                # LDS is sized per launch
    # the window is staged with 16-byte loads into 16-byte LDS stores, the output leaves as words; no generic-address access, no atomics
    for ins in ("global_load_dwordx4", "ds_write_b128", "ds_read_u16", "global_store_dword "):
        assert ins in r.stdout, ins
    assert "flat_load" not in r.stdout and "flat_store" not in r.stdout and "atomic" not in r.stdout


# ---- C ABI surface --------------------------------------------------------------------------------------------------------------------------
def test_abi_has_the_entry_and_stays_11():
    header, lib = assert_abi_11((("srh_scene_resample", 23),))
    assert "SCENE_SCALE" in header
    from sam_road_amd import build
    assert "scene_scale.hip" in build.SOURCES
    # refused without a context, before anything is launched
    assert lib.srh_scene_resample(None, None, 8, 8, 3, None, 4, 4, None, None, 3, 2, None, None, 3, 2, 0, None, 8, 8, 0, 0, None) == -1


# ---- the whole loop on the CPU stand-in ---------------------------------------------------------------------------------------------------------
class ScaleStandIn(SceneStandIn):
    """The stand-in with the one method this feature adds, its body the rule itself."""

    def scene_resample(self, t, p, q, out_shape=None, valid_rule=False, zero_where=None):
        self.calls.append(("resample", p, q, None if out_shape is None else tuple(out_shape), valid_rule, zero_where is not None))
        return torch.from_numpy(resample_ref(t.numpy(), p, q, out_shape, valid_rule, None if zero_where is None else zero_where.numpy()))


CFG = dict(E2E_CFG, INFER_PATCHES_PER_EDGE=[1, 2])           # the 288 x 416 model frame of a 576 x 832 scene: two tiles side by side
H, W = 576, 832


@pytest.fixture(scope="module")
def standin():
    warnings.simplefilter("ignore")
    torch.set_num_threads(4)
    return ScaleStandIn(dict(CFG), ("valid",))


def _same_tuple(a, b):
    assert len(a) == len(b) == 4
    for x, y in zip(a, b):
        x, y = np.asarray(x), np.asarray(y)
        assert x.shape == y.shape and (x.dtype == y.dtype or x.size == 0), (x.shape, y.shape, x.dtype, y.dtype)
        np.testing.assert_array_equal(x, y)


def _composition(net, img, cfg, p, q, valid=None):
    """The run with the key from the parts that exist without it: the existing pipeline on resample_ref(scene) (and the mask by the
    validity rule), its masks brought back by resample_ref, its nodes mapped, its edges as they are."""
    plain = Config({k: v for k, v in cfg.items() if k != "SCENE_SCALE"})
    small = resample_ref(img, p, q)
    kw = {} if valid is None else dict(valid=resample_ref(valid, p, q, valid_rule=True))
    nodes, edges, kp, road = infer_one_img(net, small, plain, device="cpu", **kw)
    back = lambda m: resample_ref(m, q, p, out_shape=img.shape[:2], zero_where=valid)
    return (map_nodes(nodes, img.shape[:2], p, q), edges, back(kp), back(road)), (nodes, edges, kp, road)


@pytest.fixture(scope="module")
def half_run(standin):
    img = rect_scene(H, W, 61)
    cfg = dict(CFG, SCENE_SCALE=[1, 2])
    want, model = _composition(standin, img, cfg, 1, 2)
    standin.calls.clear()
    got = infer_one_img(standin, img, Config(cfg), device="cpu")
    return img, cfg, want, model, got, list(standin.calls)


def test_whole_loop_at_half_resolution(standin, half_run):
    img, cfg, want, model, got, calls = half_run
    assert got[2].shape == got[3].shape == (H, W) and got[2].dtype == np.uint8 and model[2].shape == (288, 416)
    _same_tuple(got, want)
    print("nodes", got[0].shape[0], "edges", got[1].shape[0])
    assert got[0].shape[0] > 20 and got[1].shape[0] > 20
    assert got[0].min() >= 0 and got[0][:, 0].max() < H and got[0][:, 1].max() < W and got[0][:, 0].max() >= 288      # scene coordinates
    assert len({tuple(n) for n in got[0].tolist()}) == got[0].shape[0]                                                # no duplicate node
    # one resample of the scene forward, two of the masks back, between them the calls of a 288 x 416 scene
    assert [c for c in calls if c[0] == "resample"] == [("resample", 1, 2, None, False, False)] + [("resample", 2, 1, (H, W), False, False)] * 2
    assert [c for c in calls if c[0] == "pass1"] == [("pass1", 2)]
    # a run without the key, and one whose scale reduces to 1/1, never call scene_resample — on a stand-in that does not even have it
    bare = SceneStandIn(dict(CFG))
    small = resample_ref(img, 1, 2)
    plain = infer_one_img(bare, small, Config(CFG), device="cpu")
    _same_tuple(infer_one_img(bare, small, Config(dict(CFG, SCENE_SCALE=[3, 3])), device="cpu"), plain)
    _same_tuple(plain, model)
    assert not hasattr(bare, "scene_resample") and all(c[0] != "resample" for c in bare.calls)


def test_mask_goes_through_the_validity_rule_and_nodes_stay_off_nodata(standin):
    img, valid = rect_scene(H, W, 61), make_mask("band", H, W)
    cfg = dict(CFG, SCENE_SCALE={"scene_gsd": 0.5})
    want, _ = _composition(standin, img, cfg, 1, 2, valid)
    standin.calls.clear()
    got = infer_one_img(standin, img, Config(cfg), device="cpu", valid=valid)
    _same_tuple(got, want)
    assert ("resample", 1, 2, None, True, False) in standin.calls and ("resample", 2, 1, (H, W), False, True) in standin.calls
    assert not got[2][~valid].any() and not got[3][~valid].any() and got[3][valid].any()
    assert got[0].shape[0] > 5 and valid[got[0][:, 0], got[0][:, 1]].all()
    _same_tuple(infer_one_img(standin, img, Config(cfg), device="cpu", valid=valid.astype(np.uint8) * 255), want)


def test_the_scene_loops_inherit_the_feature(standin, half_run):
    """infer_imgs (pipelined), the serial tile-sharded loop and the pipelined tile-sharded loop (world 1) yield infer_one_img's tuples, in
    order, with and without masks: both resample steps live in the one front end."""
    img, cfg, _, _, got, _ = half_run
    other = rect_scene(600, 640, 62)
    imgs, valids = [img, other, img], [None, make_mask("band", 600, 640), None]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        want = [infer_one_img(standin, im, Config(cfg), device="cpu", valid=v) for im, v in zip(imgs, valids)]
        _same_tuple(want[0], got)
        assert want[1][2].shape == (600, 640) and not want[1][3][~valids[1]].any()
        for kw in ({}, dict(tile_sharded=True), dict(tile_sharded=True, pipelined=True)):
            res = list(infer_imgs(standin, iter(imgs), Config(cfg), device="cpu", valids=iter(valids), **kw))
            assert len(res) == 3
            for w, g in zip(want, res):
                _same_tuple(g, w)


def _rank(world, rank, port, out):
    """One rank of a tile-sharded run of the half-resolution scene on gloo / CPU: puts (rank, infer_one_img's result, its resample calls)."""
    import torch.distributed as dist
    warnings.simplefilter("ignore")
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        torch.set_num_threads(2)
        net = ScaleStandIn(dict(CFG), ("valid",))
        res = infer_one_img(net, rect_scene(H, W, 61), Config(dict(CFG, SCENE_SCALE=[1, 2])), device="cpu", valid=make_mask("band", H, W))
        out.put((rank, None if res is None else [np.asarray(a) for a in res], [c for c in net.calls if c[0] == "resample"]))
    except Exception:  # pragma: no cover
        import traceback
        out.put((rank, "ERR " + traceback.format_exc(), None))
    finally:
        dist.destroy_process_group()


def test_tile_sharded_world2_every_rank_resamples_rank0_brings_the_masks_back(standin):
    """The serial tile-sharded loop on gloo at world 2: both ranks resample the scene and the mask (the same integers, no collective), each
    runs one of the two tiles, rank 0 alone resamples the masks back.  The two tiles overlap, so the f32 canvas sums may associate
    differently and the masks may differ from the single-process run by one model-frame level."""
    import torch.multiprocessing as mp
    from scene_kit import free_port
    img, valid = rect_scene(H, W, 61), make_mask("band", H, W)
    one = infer_one_img(standin, img, Config(dict(CFG, SCENE_SCALE=[1, 2])), device="cpu", valid=valid)
    ctx = mp.get_context("spawn")
    port, q = free_port(), ctx.Queue()
    procs = [ctx.Process(target=_rank, args=(2, r, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    got = dict((r, (res, calls)) for r, res, calls in (q.get(timeout=600) for _ in range(2)))
    for p in procs:
        p.join(timeout=60)
    assert not any(isinstance(res, str) for res, _ in got.values()), got
    forward = [("resample", 1, 2, None, False, False), ("resample", 1, 2, None, True, False)]
    assert got[1][0] is None and got[1][1] == forward
    assert got[0][1] == forward + [("resample", 2, 1, (H, W), False, True)] * 2
    n2, e2, k2, r2 = got[0][0]
    assert k2.shape == r2.shape == (H, W) and not k2[~valid].any() and not r2[~valid].any()
    assert np.abs(one[2].astype(int) - k2.astype(int)).max() <= 1 and np.abs(one[3].astype(int) - r2.astype(int)).max() <= 1
    if np.array_equal(one[2], k2) and np.array_equal(one[3], r2):
        np.testing.assert_array_equal(one[0], n2)
        np.testing.assert_array_equal(one[1], e2)
    else:
        assert abs(one[0].shape[0] - n2.shape[0]) <= 2
    assert n2.shape[0] > 5 and valid[n2[:, 0], n2[:, 1]].all()


def test_composes_with_scene_pad(half_run):
    """The border of SCENE_PAD is in model pixels: pad and crop happen between the two resample steps."""
    img = half_run[0]
    net = ScaleStandIn(dict(CFG), ("pad",))
    cfg = dict(CFG, SCENE_SCALE=[1, 2], SCENE_PAD=24)
    want, model = _composition(net, img, cfg, 1, 2)
    net.calls.clear()
    _same_tuple(infer_one_img(net, img, Config(cfg), device="cpu"), want)
    order = [c[0] for c in net.calls if c[0] in ("resample", "pad", "pass1")]
    assert order == ["resample", "pad", "pass1", "resample", "resample"] and model[2].shape == (288, 416)
    assert ("pad", (24, 24, 24, 24), "reflect") in net.calls


def test_cli_takes_the_key_and_the_flags(tmp_path, monkeypatch, standin, half_run):
    from PIL import Image
    from sam_road_amd.formats import convert_to_sat2graph_format
    img, cfg, _, _, want, _ = half_run
    monkeypatch.chdir(tmp_path)
    Image.fromarray(img).save("rgb.png")

    def run(name, config, *argv):
        return run_cli(cli, standin, tmp_path, monkeypatch, name, config, ["rgb.png"], *argv)["rgb"]

    def check(got):
        np.testing.assert_array_equal(got[0], want[2])
        np.testing.assert_array_equal(got[1], want[3])
        assert got[0].shape == (H, W) and got[2] == convert_to_sat2graph_format(want[0], want[1])

    check(run("a", cfg))                                                  # the key comes from the YAML
    got = run("b", CFG, "--scene-scale", "2", "4")                        # the flag sets it
    check(got)
    assert got[3]["SCENE_SCALE"] == [2, 4]
    got = run("c", dict(CFG, SCENE_SCALE=[3, 2]), "--scene-gsd", "0.5")   # a gsd flag replaces a fraction
    check(got)
    assert got[3]["SCENE_SCALE"] == {"scene_gsd": 0.5, "model_gsd": 1.0}
    check(run("d", dict(CFG, SCENE_SCALE={"scene_gsd": 3.0, "model_gsd": 2.0}), "--scene-gsd", "1.0"))      # the other field stays
    monkeypatch.setattr(cli, "_build_net", lambda *a: (_ for _ in ()).throw(AssertionError("the model was built")))
    base = ["--config", "b.yaml", "--checkpoint", "none", "--device", "cpu", "--output_dir", "e", "--images", "rgb.png"]
    with pytest.raises(ValueError, match="reduces to 1/9"):
        inf.main(base + ["--scene-scale", "1", "9"])
    with pytest.raises(ValueError, match=r"\[p, q\]"):
        inf.main(base + ["--scene-gsd", "0.37"])
    with pytest.raises(ValueError, match="SCENE_GROUP"):
        inf.main(base + ["--scene-scale", "1", "2", "--scene-group", "2"])
