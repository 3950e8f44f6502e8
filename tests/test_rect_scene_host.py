"""Rectangular scenes (H x W), the GPU-free part: validation in _scene_plan, the per-axis tile grid, column bands of the tile-sharded
mode for n_x != n_y, the ABI-11 surface, and the tile-sharded loops on gloo / CPU with a stand-in model built on the oracle."""
import re
import warnings

import numpy as np
import pytest

from sam_road_amd import Config, _lib, get_patch_info_one_img
from sam_road_amd import distributed as D
from sam_road_amd.inferencer import _scene_plan
from sam_road_amd.tiling import get_patch_info_hw, patches_per_axis, shard_tiles

from scene_kit import assert_abi_11, compare_worlds, run_worlds

PLAN_CFG = dict(PATCH_SIZE=256, SAMPLE_MARGIN=16, INFER_PATCHES_PER_EDGE=3, MAX_NEIGHBOR_QUERIES=16)


# ---- 5. rejection and early failure ---------------------------------------------------------------------------------------------
def test_scene_plan_rejects_before_the_device():
    ok = np.zeros((384, 640, 3), np.uint8)
    with warnings.catch_warnings():
        warnings.simplefilter("error")                      # a plan that covers the scene warns about nothing
        img, infos, xy = _scene_plan(ok, Config(dict(PLAN_CFG, INFER_PATCHES_PER_EDGE=[3, 5])))
    assert img.shape == (384, 640, 3) and len(infos) == 15 and xy.shape == (15, 2) and xy.dtype == np.int32
    assert xy[:, 0].max() + 256 <= 640 and xy[:, 1].max() + 256 <= 384
    # an axis below P + 2 m = 288, named in the message
    with pytest.raises(ValueError, match="height"):
        _scene_plan(np.zeros((287, 640, 3), np.uint8), Config(PLAN_CFG))
    with pytest.raises(ValueError, match="width"):
        _scene_plan(np.zeros((640, 287, 3), np.uint8), Config(PLAN_CFG))
    _scene_plan(np.zeros((288, 288, 3), np.uint8), Config(dict(PLAN_CFG, INFER_PATCHES_PER_EDGE=1)))
    # INFER_PATCHES_PER_EDGE: an int or two ints
    for bad in ([3, 5, 2], [3], 3.0, [3, 5.0], "3", None, 0, [3, 0], True, [[3, 5]]):
        with pytest.raises(ValueError, match="INFER_PATCHES_PER_EDGE"):
            _scene_plan(ok, Config(dict(PLAN_CFG, INFER_PATCHES_PER_EDGE=bad)))
    assert patches_per_axis((3, 5)) == (3, 5) and patches_per_axis(np.int64(4)) == (4, 4)
    # not u8, not [H, W, 3]
    for bad in (ok.astype(np.float32), ok.astype(np.int16), ok[:, :, :2], ok[:, :, 0]):
        with pytest.raises(ValueError, match="uint8"):
            _scene_plan(bad, Config(PLAN_CFG))


def test_stride_warning_names_axis_and_count():
    """256-px tiles, margin 16, on 384 x 1400: 3 tiles along the width have a stride of 556 px — one warning that names the width and
    the 6 tiles that close the gap; [3, 6] (stride 222.4) does not warn.  The plan is not refused."""
    img = np.zeros((384, 1400, 3), np.uint8)
    with pytest.warns(UserWarning) as rec:
        _, infos, xy = _scene_plan(img, Config(dict(PLAN_CFG, INFER_PATCHES_PER_EDGE=3)))
    assert len(rec) == 1 and "width" in str(rec[0].message) and "height" not in str(rec[0].message)
    assert re.search(r"\b6 tiles", str(rec[0].message))
    assert len(infos) == 9 and sorted(set(xy[:, 0].tolist())) == [16, 572, 1128]
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        _, infos, xy = _scene_plan(img, Config(dict(PLAN_CFG, INFER_PATCHES_PER_EDGE=[3, 6])))
    assert len(infos) == 18 and np.diff(sorted(set(xy[:, 0].tolist()))).max() <= 256
    with pytest.warns(UserWarning, match="height"):          # and the other axis
        _scene_plan(np.ascontiguousarray(img.transpose(1, 0, 2)), Config(dict(PLAN_CFG, INFER_PATCHES_PER_EDGE=[3, 3])))


# ---- 6. host logic ----------------------------------------------------------------------------------------------------------------
def test_per_axis_grid(golden_dir):
    g = np.load(f"{golden_dir}/patch_info.npz")
    i = 0
    while f"case{i}" in g:                                   # square input: the reference's list, element for element
        size, margin, patch, n = (int(v) for v in g[f"case{i}"])
        want = get_patch_info_one_img(0, size, margin, patch, n)
        assert get_patch_info_hw(0, size, size, margin, patch, n) == want
        assert get_patch_info_hw(0, size, size, margin, patch, [n, n]) == want
        np.testing.assert_array_equal(np.array([[p[1][0], p[1][1], p[2][0], p[2][1]] for p in want]), g[f"xy{i}"])
        i += 1
    assert i > 0
    # one small rectangle by hand: H = 100, W = 153, margin 4, 32-px tiles, [n_y, n_x] = [2, 3]
    #   x: linspace(4, 153 - 36 = 117, 3) = 4, 60.5, 117 -> python round (half to even) 4, 60, 117
    #   y: linspace(4, 100 - 36 = 64, 2) = 4, 64;   x outer / y inner
    want = [(7, (4, 4), (36, 36)), (7, (4, 64), (36, 96)), (7, (60, 4), (92, 36)), (7, (60, 64), (92, 96)),
            (7, (117, 4), (149, 36)), (7, (117, 64), (149, 96))]
    assert get_patch_info_hw(7, 100, 153, 4, 32, [2, 3]) == want
    # an int count is the same count on both axes
    info = get_patch_info_hw(0, 401, 523, 16, 256, 4)
    assert len(info) == 16 and sorted({p[1][0] for p in info}) == [16, 94, 173, 251] and sorted({p[1][1] for p in info}) == [16, 54, 91, 129]


@pytest.mark.parametrize("world", [2, 3, 8])
@pytest.mark.parametrize("H,W,per_edge", [(384, 640, [3, 5]), (640, 384, [5, 3]), (384, 1400, [2, 7])])
def test_tile_bands_are_vertical_bands(world, H, W, per_edge):
    P = 256
    infos = get_patch_info_hw(0, H, W, 16, P, per_edge)
    xy = np.array([[p[1][0], p[1][1]] for p in infos])
    bands = D.tile_bands(xy, P, world)
    assert len(bands) == world
    live = [b for b in bands if b[1] > b[0]]
    assert all(0 <= x0 < x1 <= W for x0, x1 in live)                                        # column ranges: bounded by the WIDTH
    assert all(a[0] <= b[0] and a[1] <= b[1] for a, b in zip(live, live[1:]))               # monotone left to right
    covered = 0
    for r, (x0, x1) in enumerate(bands):                     # every tile of a rank's chunk lies inside the rank's band, full height
        lo, hi = shard_tiles(len(infos), world, r)
        assert (hi > lo) == (x1 > x0)
        for x, y in xy[lo:hi]:
            assert x0 <= x and x + P <= x1 and 0 <= y and y + P <= H
        covered += hi - lo
    assert covered == len(infos)
    assert D.canvas_bytes(bands, H) == sum(2 * 4 * H * (x1 - x0) for x0, x1 in bands[1:])   # H rows per band column


def test_abi_11_surface():
    _, lib = assert_abi_11((("srh_scene_pass1_hw", 12), ("srh_scene_normalise_hw", 11)))
    for name in ("srh_scene_pass1", "srh_scene_normalise"):  # the square entries stay exported with their signatures
        assert hasattr(lib, name) and len(_lib.SYMBOLS[name][1]) == len(_lib.SYMBOLS[name + "_hw"][1]) - 1


# ---- 7. tile-sharded loops, CPU / gloo -------------------------------------------------------------------------------------------
# The GPU model is replaced by the CPU stand-in of tests/scene_kit.py (SAMRoad's scene-level interface built on the oracle): what is
# under test is the orchestration in sam_road_amd/inferencer.py and sam_road_amd/distributed.py for H != W, on HOST_CFG's 128-px tiles.
# A disjoint tiling must be IDENTICAL to the single-process run; runs with overlapping tiles are compared the way
# tests/test_distributed_cpu.py compares them (scene_kit.compare_worlds).
_FIVE = [(384, 640), (640, 384), (448, 448), (640, 384), (401, 523)]


@pytest.mark.parametrize("overrides,must_be_identical", [
    (dict(SAMPLE_MARGIN=0, INFER_PATCHES_PER_EDGE=[3, 5]), True),    # 3 x 5 disjoint tiles; 5 tiles per rank = 1 2/3 columns
    (dict(INFER_PATCHES_PER_EDGE=[4, 6]), False),                    # overlapping tiles, 8 per rank = 2 columns
])
def test_serial_tile_sharded_world3_rect(overrides, must_be_identical):
    shapes = [(384, 640)]
    res = run_worlds((1, 3), dict(shapes=shapes, overrides=overrides, mode="serial"))
    compare_worlds(res[1], res[3], shapes, None, must_be_identical)


def test_pipelined_tile_sharded_world2_five_rect_scenes():
    """The pipelined tile-sharded loop on two ranks over five scenes of four shapes (640 x 384 right after 384 x 640): equal to the
    serial tile-sharded loop of the same world exactly (checked inside the ranks), and to the single-process run."""
    res = run_worlds((1, 2), dict(shapes=_FIVE, mode="pipelined"))
    compare_worlds(res[1], res[2], _FIVE, None, False)
