"""MASK_CLEAN (small mask components dropped on the device), the GPU-free part: the key and its errors, the CLI flags,
mask_clean_ref against a flood fill written in the tests, the kernels' own per-lane code run item by item on the CPU in several
schedules, the C-ABI surface, and the orchestration of the scene loops through a CPU stand-in whose mask_clean IS mask_clean_ref.  The
feature is pinned by COMPOSITION: a run with the key equals the existing pipeline with its two masks replaced by mask_clean_ref of them
before the point extraction, bit for bit (tests/mask_clean_kit.py)."""
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
from sam_road_amd import mask_clean as mc
from sam_road_amd.inferencer import infer_imgs, infer_one_img, mask_clean_plan, scene_tiles
from sam_road_amd.mask_clean import MaskCleanPlan, MaskRule, mask_clean_ref, mask_clean_stats, mask_clean_table
from sam_road_amd.resample import resample_ref

import mask_clean_kit as kit
from scene_kit import E2E_CFG, HOST_CFG, SCENES, SceneStandIn, _CountOnly, assert_abi_11, make_mask, np_pad, rect_scene, run_cli, same_tuple, thresholds

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GEO = dict(PATCH_SIZE=256, SAMPLE_MARGIN=16, INFER_PATCHES_PER_EDGE=2, MAX_NEIGHBOR_QUERIES=16, ITSC_NMS_RADIUS=8, ROAD_NMS_RADIUS=16,
           ITSC_THRESHOLD=0.5, ROAD_THRESHOLD=0.3)
T_KP, T_ROAD = 128, 77                                    # floor(0.5 * 255) + 1, floor(0.3 * 255) + 1


# ---- the key ------------------------------------------------------------------------------------------------------------------------------
def _plan(v, **kw):
    return mask_clean_plan(Config(dict(GEO, MASK_CLEAN=v, **kw)))


def test_mask_clean_key_every_accepted_form():
    assert mc.level_above(0.5) == 128 and mc.level_above(0.3) == 77 and mc.level_above(0.0) == 1 and mc.level_above(0.999) == 255
    assert mc.level_above(1.0) == 256 and mc.level_above(2.0) == 256 and mc.level_above(-1.0) == 0
    for t in range(0, 256):                               # the pixels points_and_scores_from_mask takes: mask > T * 255
        T = t / 255.0 + 1e-4
        np.testing.assert_array_equal(np.arange(256) >= mc.level_above(T), np.arange(256) > T * 255)
    assert _plan({"road": {"min_area": 200, "min_peak": 0.6}, "keypoint": {"min_peak": 0.55}, "connectivity": 8}) == \
        MaskCleanPlan(MaskRule(T_KP, 1, 141), MaskRule(T_ROAD, 200, 154), 8)
    assert _plan({"road": {"min_area": 200}}) == MaskCleanPlan(MaskRule(T_KP, 1, 0), MaskRule(T_ROAD, 200, 0), 8)
    assert _plan({"keypoint": {"min_area": np.int64(3)}, "connectivity": 4}) == MaskCleanPlan(MaskRule(T_KP, 3, 0), MaskRule(T_ROAD, 1, 0), 4)
    assert _plan({"road": {"min_peak": 0}, "keypoint": None}) is None        # t_peak 1 <= t_on: every component passes
    assert _plan({"road": {"min_peak": 0.3}}) is None and _plan({"road": {"min_peak": 0.31}}).road == MaskRule(T_ROAD, 1, 80)
    assert _plan({"road": {"min_area": 2}}, ROAD_THRESHOLD=1.0) is None      # no foreground at all
    assert _plan({"road": {"min_area": 2}, "keypoint": {"min_area": 2}}, ROAD_THRESHOLD=1.0).road.t_on == 256


def test_absent_and_idle_keys_give_the_plan_of_a_run_without_the_key():
    cfg = dict(GEO, INFER_PATCHES_PER_EDGE=4)
    plain = scene_tiles((401, 523), Config(cfg))
    idle = (None, {}, {"road": {"min_area": 1}}, {"road": {"min_area": 1}, "keypoint": {}, "connectivity": 4}, {"connectivity": 8}, {"road": None})
    for v in idle:
        c = Config(dict(cfg, MASK_CLEAN=v))
        assert mask_clean_plan(c) is None
        t = scene_tiles((401, 523), c)
        assert t == plain and (t.scale, t.model_shape, t.pads, t.orientations) == (plain.scale, plain.model_shape, plain.pads, plain.orientations)
    assert mask_clean_plan(Config(cfg)) is None
    # a model that can count tiles and nothing else is all that the plan of a masked scene needs, with an idle key as without one
    valid = np.zeros((401, 523), bool)
    valid[:, :60] = True                                  # only the first two tile columns hold a valid pixel
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        net = _CountOnly(256)
        kept = scene_tiles((401, 523), Config(cfg), valid=valid, net=net)
        assert 0 < len(kept) < len(plain)
        for v in idle:
            net = _CountOnly(256)
            assert scene_tiles((401, 523), Config(dict(cfg, MASK_CLEAN=v)), valid=valid, net=net) == kept
            assert [c[0] for c in net.calls] == ["tile_valid"] and not hasattr(net, "mask_clean")


BAD = [("road", "must be a mapping"), (5, "must be a mapping"), (True, "must be a mapping"), ([1, 2], "must be a mapping"),
       ({"roads": {}}, "unknown key 'roads'"), ({"road": {"area": 3}}, "unknown key 'area' in road"), ({"road": 200}, "road must be a mapping"),
       ({"road": True}, "road must be a mapping"), ({"road": {"min_area": 0}}, "min_area must be an int >= 1"),
       ({"road": {"min_area": -3}}, "min_area"), ({"road": {"min_area": 2.0}}, "min_area"), ({"road": {"min_area": True}}, "min_area"),
       ({"keypoint": {"min_area": "7"}}, "keypoint.min_area"), ({"road": {"min_peak": 1.0}}, r"min_peak must be a number in \[0, 1\)"),
       ({"road": {"min_peak": -0.1}}, "min_peak"), ({"road": {"min_peak": float("nan")}}, "min_peak"), ({"road": {"min_peak": float("inf")}}, "min_peak"),
       ({"road": {"min_peak": True}}, "min_peak"), ({"keypoint": {"min_peak": "0.5"}}, "keypoint.min_peak"),
       ({"road": {"min_area": 2}, "connectivity": 6}, "connectivity must be 4 or 8"), ({"connectivity": True}, "connectivity"),
       ({"connectivity": 8.0}, "connectivity"), ({"connectivity": "8"}, "connectivity")]


def test_every_bad_key_is_a_value_error_before_the_model_is_touched():
    class Untouchable(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.w = torch.nn.Parameter(torch.zeros(1))

        def __getattr__(self, name):
            if name.startswith("scene_") or name.startswith("infer_") or name.startswith("mask_"):
                raise AssertionError(f"the model was touched: {name}")
            return super().__getattr__(name)

    net = Untouchable()
    img = np.zeros((600, 700, 3), np.uint8)
    for v, what in BAD:
        c = Config(dict(E2E_CFG, MASK_CLEAN=v))
        with pytest.raises(ValueError, match=what):
            mask_clean_plan(c)
        with pytest.raises(ValueError, match=what):
            infer_one_img(net, img, c, device="cpu")
        with pytest.raises(ValueError, match=what):
            infer_one_img(net, img, c, device="cpu", valid=np.ones((600, 700), bool))
        for kw in ({}, dict(group=2), dict(tile_sharded=True), dict(tile_sharded=True, pipelined=True)):
            scenes = iter([img])
            with pytest.raises(ValueError, match=what):
                list(infer_imgs(net, scenes, c, device="cpu", **kw))
            assert next(scenes, None) is img                                     # no scene was read
    scenes = iter([img])                                                         # a group too large for one call of the filter
    with pytest.raises(ValueError, match="at most 2048"):
        list(infer_imgs(net, scenes, Config(dict(E2E_CFG, MASK_CLEAN={"road": {"min_area": 5}})), device="cpu", group=2049))
    assert next(scenes, None) is img
    with pytest.raises(ValueError, match="ROAD_THRESHOLD"):                      # a rule needs the threshold it refers to
        mask_clean_plan(Config(dict(MASK_CLEAN={"road": {"min_area": 5}})))


def test_cli_flags_lay_over_the_key():
    over = mc.mask_clean_override
    assert over(Config({}), min_area=[200]) == {"road": {"min_area": 200}}
    assert over(Config({}), min_area=[200, 9], min_peak=[0.6]) == {"road": {"min_area": 200, "min_peak": 0.6}, "keypoint": {"min_area": 9}}
    key = {"road": {"min_area": 50, "min_peak": 0.7}, "keypoint": {"min_peak": 0.5}, "connectivity": 4}
    assert over(Config(dict(MASK_CLEAN=key)), min_area=[80]) == {"road": {"min_area": 80, "min_peak": 0.7}, "keypoint": {"min_peak": 0.5}, "connectivity": 4}
    assert over(Config(dict(MASK_CLEAN=key)), min_peak=[0.1, 0.2], connectivity=8) == \
        {"road": {"min_area": 50, "min_peak": 0.1}, "keypoint": {"min_peak": 0.2}, "connectivity": 8}
    assert key == {"road": {"min_area": 50, "min_peak": 0.7}, "keypoint": {"min_peak": 0.5}, "connectivity": 4}      # the config's own is not edited
    assert over(Config(dict(MASK_CLEAN={"road": None})), connectivity=4) == {"road": None, "connectivity": 4}
    for kw in (dict(min_area=[1, 2, 3]), dict(min_peak=[])):
        with pytest.raises(ValueError, match="ROAD \\[KEYPOINT\\]"):
            over(Config({}), **kw)
    with pytest.raises(ValueError, match="must be a mapping"):
        over(Config(dict(MASK_CLEAN=7)), min_area=[3])


# ---- mask_clean_ref against a second statement of the rule -----------------------------------------------------------------------------------
def _both(m, *args):
    got = mask_clean_ref(m, *args)
    assert got.dtype == np.uint8 and got.shape == m.shape and got.flags.c_contiguous and got is not m
    np.testing.assert_array_equal(got, kit.flood_clean(m, *args), err_msg=str(args))
    return got


def test_ref_equals_the_flood_fill_on_hand_made_masks():
    # two 2 x 2 blobs that touch only diagonally: one component of 8 pixels under 8, two of 4 under 4
    m = np.zeros((6, 7), np.uint8)
    m[1:3, 1:3] = 200
    m[3:5, 3:5] = 150
    assert _both(m, 100, 5, 0, 8).tolist() == m.tolist() and not _both(m, 100, 5, 0, 4).any()
    assert _both(m, 100, 8, 0, 8).any() and not _both(m, 100, 9, 0, 8).any()         # an area exactly min_area stays, min_area - 1 goes
    assert _both(m, 100, 4, 0, 4).tolist() == m.tolist()
    # a peak exactly t_peak stays, t_peak - 1 goes; under 4 each blob has its own peak
    assert _both(m, 100, 1, 200, 8).tolist() == m.tolist() and not _both(m, 100, 1, 201, 8).any()
    only_first = _both(m, 100, 1, 151, 4)
    assert only_first[1:3, 1:3].all() and not only_first[3:5, 3:5].any()
    # pixels below the threshold are untouched, whether their neighbours go or stay
    m[0, 0], m[2, 3], m[5, 6] = 99, 99, 1
    got = _both(m, 100, 9, 0, 8)
    assert (got[0, 0], got[2, 3], got[5, 6]) == (99, 99, 1) and got.sum() == 199
    # at 99 the corner (0, 0) and the bridge (2, 3) join the blobs: ten pixels, and (5, 6) stays below the threshold
    frozen = m.copy()
    assert _both(m, 99, 10, 0, 8).sum() == m.sum() and _both(m, 99, 11, 0, 8).sum() == 1
    # t_on = 256: no foreground, nothing happens; t_on = 0: the whole array is one component
    np.testing.assert_array_equal(_both(m, 256, 1000, 256, 8), m)
    np.testing.assert_array_equal(_both(m, 0, 42, 0, 4), m)
    assert not _both(m, 0, 43, 0, 4).any()
    np.testing.assert_array_equal(m, frozen)                                         # the input is never written
    with pytest.raises(ValueError):
        mask_clean_ref(m.astype(np.float32), 100)
    with pytest.raises(ValueError):
        mask_clean_ref(m, 100, connectivity=6)


def test_ref_equals_the_flood_fill_on_every_pattern():
    for k, kind in enumerate(kit.PATTERNS):
        for H, W in ((1, 1), (1, 64), (64, 1), (37, 53)):
            m = kit.levels(kit.pattern(kind, H, W, k), 128, k)
            for conn in (8, 4):
                _both(m, 128, 5, 230, conn)
                _both(m, 128, 3, 0, conn)
    assert kit.pattern("spiral", 63, 63).sum() == 2047 and mask_clean_stats(kit.levels(kit.pattern("spiral", 63, 63), 128), 128, 4)[0].tolist() == [2047]
    a8, _ = mask_clean_stats(kit.levels(kit.pattern("checker", 37, 53), 128), 128, 8)
    a4, _ = mask_clean_stats(kit.levels(kit.pattern("checker", 37, 53), 128), 128, 4)
    assert a8.tolist() == [37 * 53 // 2] and (a4 == 1).all() and a4.size == 37 * 53 // 2
    c8, _ = mask_clean_stats(kit.levels(kit.pattern("corner", 37, 300), 128), 128, 8)
    c4, _ = mask_clean_stats(kit.levels(kit.pattern("corner", 37, 300), 128), 128, 4)
    assert c8.size == 4 and (c4 <= 9).all() and c4.size == 4 * 13                 # a chain of blobs per 64-column border; under 4 every blob alone


def test_table_rows_and_running_sums():
    r = MaskRule(128, 5, 200)
    t = mask_clean_table([(0, 5, 70, r), (350, 9, 64, MaskRule(1, 1, 0)), (1000, 1, 130, r)])
    assert t.dtype == np.int64 and t.tolist() == [[0, 5, 70, 128, 5, 200, 0, 0], [350, 9, 64, 1, 1, 0, 350, 10], [1000, 1, 130, 128, 5, 200, 926, 19]]


# ---- the kernels' own code, on the CPU -----------------------------------------------------------------------------------------------------
def test_kernel_code_on_the_cpu_in_several_schedules(tmp_path):
    """tests/mask_clean_check.cpp runs every (segment, lane) item of the five launches through the kernels' own per-lane code
    (csrc/mask_clean_piece.hpp) as a stand-alone host program built with the address and undefined-behaviour sanitizers, over the shapes
    and patterns of the GPU tests, ascending, descending, in a stride permutation and with loads that return old values; each result
    equals a flood fill inside the program, so all of them are identical.  A read or write outside the buffer or a workspace ends it."""
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    cxx = next((c for c in (os.path.join(rocm, "llvm", "bin", "clang++"), os.path.join(rocm, "lib", "llvm", "bin", "clang++")) if os.path.exists(c)), None)
    if cxx is None:
        pytest.skip("no ROCm clang++")
    exe = str(tmp_path / "mask_clean_check")
    csrc = os.path.join(ROOT, "sam_road_amd", "csrc")
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", csrc,
                        os.path.join(ROOT, "tests", "mask_clean_check.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    assert "mask clean OK" in r.stdout


def test_kernels_compile_for_gfx950_without_a_gpu():
    hipcc = next((c for c in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", shutil.which("hipcc")) if c and os.path.exists(c)), None)
    if hipcc is None:
        pytest.skip("hipcc not found")
    from sam_road_amd import build
    assert "mask_clean.hip" in build.SOURCES
    r = subprocess.run([hipcc, *build.FLAGS, "-S", "--cuda-device-only", os.path.join(build.CSRC, "mask_clean.hip"), "-o", "-"],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    for name in ("mask_clean_init_kernel", "mask_clean_merge_kernel", "mask_clean_flatten_kernel", "mask_clean_stats_kernel", "mask_clean_apply_kernel"):
        m = re.search(r"^(_Z\w*%s\w*):" % name, r.stdout, re.M)
        assert m, f"{name} is not in the code object"
        meta = r.stdout[r.stdout.index(".amdhsa_kernel " + m.group(1)):]
        meta = meta[:meta.index(".end_amdhsa_kernel")]
        assert int(re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", meta).group(1)) == 0          # no scratch
        assert int(re.search(r"\.amdhsa_group_segment_fixed_size (\d+)", meta).group(1)) == 0            # no LDS
        assert int(re.search(r"\.amdhsa_uses_dynamic_stack (\d+)", meta).group(1)) == 0


# ---- C ABI surface --------------------------------------------------------------------------------------------------------------------------
def test_abi_has_the_entry_and_stays_11():
    header, lib = assert_abi_11((("srh_mask_clean", 12),))
    assert "MASK_CLEAN" in header
    # refused without a context, before anything is launched
    assert lib.srh_mask_clean(None, None, 64, None, None, 1, 8, None, None, None, 64, None) == -1


# ---- the whole loop on the CPU stand-in ---------------------------------------------------------------------------------------------------------
def _np_stack(ragged, table, C, Ha, Wa, mode, fill):
    out = np.zeros((Ha, Wa, 3) if C == 3 else (Ha, Wa), dtype=ragged.dtype)
    for off, H, W, top, left, Hv, Wv, row0 in np.asarray(table).tolist():
        block = ragged[off:off + H * W * C].reshape((H, W, 3) if C == 3 else (H, W))
        out[row0:row0 + Hv, :Wv] = np_pad(block, (top, Hv - H - top, left, Wv - W - left), mode, fill)
    return out


class CleanStandIn(SceneStandIn):
    """The stand-in with the one method this feature adds, its body the rule itself — and, for the paths it must compose with, the
    numpy bodies of scene_resample (SCENE_SCALE) and of the two group entries (SCENE_GROUP), as their own suites state them."""

    def mask_clean(self, buf, table, table_dev=None, connectivity=8):
        t = torch.as_tensor(table)
        assert buf.dim() == 1 and buf.dtype == torch.uint8 and buf.is_contiguous() and t.dtype == torch.int64 and tuple(t.shape[1:]) == (8,)
        assert table_dev is None or torch.equal(table_dev, t)
        self.calls.append(("mask_clean", [tuple(r[1:6]) for r in t.tolist()], connectivity))
        flat = buf.numpy()                                                   # shares the tensor's memory: in place
        for off, H, W, t_on, min_area, t_peak, _, _ in t.tolist():
            block = flat[off:off + H * W].reshape(H, W)
            block[...] = mask_clean_ref(block.copy(), t_on, min_area, t_peak, connectivity)
        return buf

    def scene_resample(self, t, p, q, out_shape=None, valid_rule=False, zero_where=None):
        self.calls.append(("resample", p, q))
        return torch.from_numpy(resample_ref(t.numpy(), p, q, out_shape, valid_rule, None if zero_where is None else zero_where.numpy()))

    def scene_group_pack(self, ragged, table, C, Ha, Wa, mode="reflect", fill=(0, 0, 0), table_dev=None):
        self.calls.append(("group_pack", int(table.shape[0])))
        return torch.from_numpy(_np_stack(ragged.numpy(), table.numpy(), C, int(Ha), int(Wa), mode, fill))

    def scene_group_crop(self, kp, road, table, table_dev=None):
        self.calls.append(("group_crop", int(table.shape[0])))
        t = table.numpy()
        out = np.full((2, int((t[:, 1] * t[:, 2]).sum())), 0xEE, np.uint8)
        for off, H, W, top, left, _, _, row0 in t.tolist():
            for j, m in enumerate((kp, road)):
                out[j, off:off + H * W] = m.numpy()[row0 + top:row0 + top + H, left:left + W].reshape(-1)
        return torch.from_numpy(out)


H, W, PER_EDGE, SEED = SCENES["401x523"]
CFG = dict(HOST_CFG, INFER_PATCHES_PER_EDGE=PER_EDGE)
_NETS = {}


def standin(*features):
    warnings.simplefilter("ignore")
    torch.set_num_threads(4)
    if features not in _NETS:
        _NETS[features] = CleanStandIn(dict(CFG), features)
    _NETS[features].calls.clear()
    return _NETS[features]


def clean_calls(net):
    return [c for c in net.calls if c[0] == "mask_clean"]


def median_key(kp, road, cfg, connectivity=8):
    """The key whose rules are the medians of the masks' own components: min_area the median area, min_peak the level just below the
    median peak, per mask — so that in each mask some components go and some stay, which is asserted."""
    key = {"connectivity": connectivity}
    for name, m, thr in (("keypoint", kp, cfg["ITSC_THRESHOLD"]), ("road", road, cfg["ROAD_THRESHOLD"])):
        areas, peaks = mask_clean_stats(m, mc.level_above(thr), connectivity)
        assert areas.size >= 4, (name, areas.size)
        key[name] = {"min_area": int(np.median(areas)), "min_peak": (int(np.median(peaks)) - 0.5) / 255.0}
    plan = mask_clean_plan(Config(dict(cfg, MASK_CLEAN=key)))
    for m, rule in ((kp, plan.keypoint), (road, plan.road)):
        areas, peaks = mask_clean_stats(m, rule.t_on, connectivity)
        keep = (areas >= rule.min_area) & (peaks >= rule.t_peak)
        assert keep.any() and not keep.all(), (rule, areas.size)
    return key, plan


@pytest.fixture(scope="module")
def scene_run():
    """The kit's 401 x 523 scene without the key, the key taken from its masks, and what the run with the key must equal."""
    net, img = standin(), rect_scene(H, W, SEED)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        first = infer_one_img(net, img, Config(CFG), device="cpu")
        # at 0.5 the stand-in's road mask is one blob: the kit's percentile thresholds leave scattered components
        cfg = dict(CFG, **thresholds(first[2], first[3]))
        plain = infer_one_img(net, img, Config(cfg), device="cpu")
        assert not clean_calls(net)
        key, plan = median_key(plain[2], plain[3], cfg)
        want = kit.composed(plan, lambda: [infer_one_img(net, img, Config(cfg), device="cpu")])[0]
    return img, cfg, plain, key, plan, want


def test_whole_loop_equals_the_composition(scene_run):
    img, CFG, plain, key, plan, want = scene_run
    net = standin()
    got = infer_one_img(net, img, Config(dict(CFG, MASK_CLEAN=key)), device="cpu")
    same_tuple(got, want)
    print("nodes", plain[0].shape[0], "->", got[0].shape[0], "edges", plain[1].shape[0], "->", got[1].shape[0])
    assert 5 < got[0].shape[0] < plain[0].shape[0] and got[1].shape[0] > 5               # fewer nodes, still a graph
    assert (got[2] != plain[2]).any() and (got[3] != plain[3]).any()
    assert ((got[2] == plain[2]) | (got[2] == 0)).all() and ((got[3] == plain[3]) | (got[3] == 0)).all()
    # ONE call serves both masks, behind the normalise; an unkeyed run and a stand-in without the method make none
    assert clean_calls(net) == [("mask_clean", [(H, W) + tuple(plan.keypoint), (H, W) + tuple(plan.road)], 8)]
    bare = SceneStandIn(dict(CFG))
    assert not hasattr(bare, "mask_clean")
    same_tuple(infer_one_img(bare, img, Config(dict(CFG, MASK_CLEAN={"road": {"min_area": 1}})), device="cpu"), plain)
    # a rule for one mask only: the other one is not in the table and comes out as it went in
    net.calls.clear()
    one = infer_one_img(net, img, Config(dict(CFG, MASK_CLEAN={"road": key["road"], "connectivity": 4})), device="cpu")
    assert clean_calls(net) == [("mask_clean", [(H, W) + tuple(plan.road)], 4)]
    np.testing.assert_array_equal(one[2], plain[2])
    np.testing.assert_array_equal(one[3], mask_clean_ref(plain[3], *plan.road, 4))


def test_the_scene_loops_inherit_the_feature(scene_run):
    """infer_imgs serial (tile-sharded, world 1), pipelined and grouped yield infer_one_img's tuples: the filter lives in the one front end."""
    img, CFG, plain, key, plan, want = scene_run
    net = standin()
    other = rect_scene(384, 640, 41)
    cfg = dict(CFG, MASK_CLEAN=key)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        want_other = kit.composed(plan, lambda: [infer_one_img(net, other, Config(CFG), device="cpu")])[0]
        assert (want_other[3] != infer_one_img(net, other, Config(CFG), device="cpu")[3]).any()
        imgs, wants = [img, other, img], [want, want_other, want]
        for kw in (dict(), dict(tile_sharded=True), dict(tile_sharded=True, pipelined=True), dict(group=2)):
            net.calls.clear()
            res = list(infer_imgs(net, iter(imgs), Config(cfg), device="cpu", **kw))
            assert len(res) == 3
            for g, w in zip(res, wants):
                same_tuple(g, w)
            # a group of two: ONE call over the four masks of its scenes, each an image of its own
            sizes = [len(c[1]) for c in clean_calls(net)]
            assert sizes == ([4, 2] if kw.get("group") else [2, 2, 2]), (kw, sizes)
        rows = clean_calls(net)[0][1]
        assert rows == [(H, W) + tuple(plan.keypoint), (384, 640) + tuple(plan.keypoint), (H, W) + tuple(plan.road), (384, 640) + tuple(plan.road)]


def test_no_component_crosses_from_one_scene_of_a_group_into_the_next():
    """Two scenes whose masks are all foreground, stacked: each is one component of ITS pixel count, so with min_area between the two
    counts the smaller scene is emptied and the larger one stays — a filter that saw the ragged buffer as one image would keep both."""
    plan = MaskCleanPlan(MaskRule(1, 1, 0), MaskRule(100, 5000, 0), 8)
    blocks = [(0, 40, 100), (4000, 80, 100)]
    table = inf._mask_clean_images(plan, blocks, 12000)
    assert table.tolist() == [[12000, 40, 100, 100, 5000, 0, 0, 0], [16000, 80, 100, 100, 5000, 0, 4000, 80]]         # the idle keypoint rule has no row
    buf = torch.full((2, 12000), 200, dtype=torch.uint8)
    standin().mask_clean(buf.view(-1), table, connectivity=8)
    assert (buf[0] == 200).all() and (buf[1, :4000] == 0).all() and (buf[1, 4000:] == 200).all()
    assert inf._mask_clean_images(MaskCleanPlan(MaskRule(256, 9, 0), MaskRule(100, 1, 50), 8), blocks, 12000) is None


def test_composes_with_scene_pad_scene_scale_and_a_validity_mask(scene_run):
    img, CFG, plain, key, plan, _ = scene_run
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        # SCENE_PAD: the masks are cropped first — a component's area counts real pixels only
        net = standin("pad")
        padded = dict(CFG, SCENE_PAD=24)
        want = kit.composed(plan, lambda: [infer_one_img(net, img, Config(padded), device="cpu")])[0]
        net.calls.clear()
        same_tuple(infer_one_img(net, img, Config(dict(padded, MASK_CLEAN=key)), device="cpu"), want)
        order = [c[0] for c in net.calls if c[0] in ("pad", "pass1", "mask_clean")]
        assert order == ["pad", "pass1", "mask_clean"] and clean_calls(net)[0][1][0][:2] == (H, W) and (want[3] != plain[3]).any()
        # a validity mask: the masks are 0 on nodata before the filter sees them
        net, valid = standin("valid"), make_mask("band", H, W)
        want = kit.composed(plan, lambda: [infer_one_img(net, img, Config(CFG), device="cpu", valid=valid)])[0]
        got = infer_one_img(net, img, Config(dict(CFG, MASK_CLEAN=key)), device="cpu", valid=valid)
        same_tuple(got, want)
        assert not got[2][~valid].any() and not got[3][~valid].any() and got[3].any()
        # SCENE_SCALE [1, 2]: the filter runs on the model-frame masks and the scene-frame masks are resampled from the cleaned ones
        net, big = standin(), rect_scene(2 * H, 2 * W, SEED)
        scaled = dict(CFG, SCENE_SCALE=[1, 2])
        seen = []
        with kit.cleaned_before_extraction(plan, seen):
            nodes, edges, _, _ = infer_one_img(net, big, Config(scaled), device="cpu")
        assert len(seen) == 1 and seen[0][0].shape == (H, W)
        net.calls.clear()
        got = infer_one_img(net, big, Config(dict(scaled, MASK_CLEAN=key)), device="cpu")
        same_tuple(got, (nodes, edges) + tuple(resample_ref(m, 2, 1, out_shape=(2 * H, 2 * W)) for m in seen[0]))
        assert [c[0] for c in net.calls if c[0] in ("resample", "mask_clean")] == ["resample", "mask_clean", "resample", "resample"]
        assert clean_calls(net)[0][1][0][:2] == (H, W) and got[2].shape == (2 * H, 2 * W)


# 512 x 512 in four disjoint tiles, one per batch: every canvas pixel has ONE addend and every tile runs alone in both worlds
GLOO_CFG = dict(E2E_CFG, SAMPLE_MARGIN=0, INFER_PATCHES_PER_EDGE=2, INFER_BATCH_SIZE=1,
                MASK_CLEAN={"road": {"min_area": 40, "min_peak": 0.55}, "keypoint": {"min_area": 6}})


def _rank(world, rank, port, out):
    """One rank of a tile-sharded run on gloo / CPU: puts (rank, infer_one_img's result, its mask_clean calls)."""
    import torch.distributed as dist
    warnings.simplefilter("ignore")
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        torch.set_num_threads(2)
        net = CleanStandIn(dict(GLOO_CFG))
        res = infer_one_img(net, rect_scene(512, 512, 6), Config(GLOO_CFG), device="cpu")
        out.put((rank, None if res is None else [np.asarray(a) for a in res], clean_calls(net)))
    except Exception:  # pragma: no cover
        import traceback
        out.put((rank, "ERR " + traceback.format_exc(), None))
    finally:
        dist.destroy_process_group()


def test_tile_sharded_world2_equals_world1_and_only_rank0_filters():
    import torch.multiprocessing as mp
    from scene_kit import free_port
    warnings.simplefilter("ignore")
    torch.set_num_threads(2)                                                     # as the ranks
    net, img = CleanStandIn(dict(GLOO_CFG)), rect_scene(512, 512, 6)
    one = infer_one_img(net, img, Config(GLOO_CFG), device="cpu")
    plain = infer_one_img(net, img, Config({k: v for k, v in GLOO_CFG.items() if k != "MASK_CLEAN"}), device="cpu")
    assert (one[3] != plain[3]).any() and one[3].any() and one[0].shape[0] > 5           # the key drops something and keeps something
    ctx = mp.get_context("spawn")
    port, q = free_port(), ctx.Queue()
    procs = [ctx.Process(target=_rank, args=(2, r, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    got = dict((r, (res, calls)) for r, res, calls in (q.get(timeout=600) for _ in range(2)))
    for p in procs:
        p.join(timeout=60)
    assert not any(isinstance(res, str) for res, _ in got.values()), got
    assert got[1][0] is None and got[1][1] == [] and len(got[0][1]) == 1 and len(got[0][1][0][1]) == 2      # rank 0 alone filters: no collective
    same_tuple(got[0][0], one)


def test_cli_takes_the_key_and_the_flags(tmp_path, monkeypatch, scene_run):
    from PIL import Image
    from sam_road_amd.formats import convert_to_sat2graph_format
    img, CFG, _, key, plan, want = scene_run
    net = standin()
    monkeypatch.chdir(tmp_path)
    Image.fromarray(img).save("rgb.png")

    def run(name, config, *argv):
        return run_cli(cli, net, tmp_path, monkeypatch, name, config, ["rgb.png"], *argv)["rgb"]

    def check(got):
        np.testing.assert_array_equal(got[0], want[2])                         # the PNGs are the cleaned masks
        np.testing.assert_array_equal(got[1], want[3])
        assert got[2] == convert_to_sat2graph_format(want[0], want[1])

    check(run("a", dict(CFG, MASK_CLEAN=key)))                                 # the key comes from the YAML
    area = [str(key["road"]["min_area"]), str(key["keypoint"]["min_area"])]
    peak = [repr(key["road"]["min_peak"]), repr(key["keypoint"]["min_peak"])]
    got = run("b", CFG, "--mask-min-area", *area, "--mask-min-peak", *peak)     # the flags set it
    check(got)
    assert got[3]["MASK_CLEAN"] == {"road": key["road"], "keypoint": key["keypoint"]}
    wrong = {"road": {"min_area": 1, "min_peak": key["road"]["min_peak"]}, "keypoint": key["keypoint"], "connectivity": 4}
    check(run("c", dict(CFG, MASK_CLEAN=wrong), "--mask-min-area", area[0], "--mask-connectivity", "8"))      # a flag replaces its field only
    monkeypatch.setattr(cli, "_build_net", lambda *a: (_ for _ in ()).throw(AssertionError("the model was built")))
    base = ["--config", "b.yaml", "--checkpoint", "none", "--device", "cpu", "--output_dir", "e", "--images", "rgb.png"]
    with pytest.raises(ValueError, match="connectivity must be 4 or 8"):
        inf.main(base + ["--mask-connectivity", "6"])
    with pytest.raises(ValueError, match="min_area must be an int >= 1"):
        inf.main(base + ["--mask-min-area", "0"])
    with pytest.raises(ValueError, match="min_peak must be a number"):
        inf.main(base + ["--mask-min-peak", "0.5", "1.5"])
