"""Rectangular scenes (H x W), the GPU-free part: validation in _scene_plan, the per-axis tile grid, column bands of the tile-sharded
mode for n_x != n_y, the ABI-11 surface, and the tile-sharded loops on gloo / CPU with a stand-in model built on the oracle."""
import os
import re
import socket
import warnings

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from sam_road_amd import Config, _lib, get_patch_info_one_img
from sam_road_amd import distributed as D
from sam_road_amd.inferencer import _scene_plan
from sam_road_amd.tiling import get_patch_info_hw, patches_per_axis, shard_tiles

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
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
    header = open(os.path.join(ROOT, "include", "samroad_hip.h")).read()
    lib = _lib.load()
    assert lib.srh_abi_version() == _lib.ABI_VERSION == int(re.search(r"#define SRH_ABI_VERSION (\d+)", header).group(1)) == 11
    for name, n_args in (("srh_scene_pass1_hw", 12), ("srh_scene_normalise_hw", 11)):
        assert re.search(r"\bint %s\(" % name, header)
        assert hasattr(lib, name) and len(_lib.SYMBOLS[name][1]) == n_args
    for name in ("srh_scene_pass1", "srh_scene_normalise"):  # the square entries stay exported with their signatures
        assert hasattr(lib, name) and len(_lib.SYMBOLS[name][1]) == len(_lib.SYMBOLS[name + "_hw"][1]) - 1


# ---- 7. tile-sharded loops, CPU / gloo -------------------------------------------------------------------------------------------
# The GPU model is replaced by a CPU stand-in with SAMRoad's scene-level interface built on the oracle (test infrastructure): what is
# under test is the orchestration in sam_road_amd/inferencer.py and sam_road_amd/distributed.py for H != W.  128-px tiles keep the
# oracle at seconds, and 384 x 640 = 3 x 5 such tiles exactly, so a disjoint tiling exists: every canvas pixel then has ONE addend
# and the multi-rank result must be IDENTICAL to the single-process one.  With overlapping tiles the f32 canvas sums are associated
# differently across ranks (distributed.reduce_canvases) and the u8 truncation may turn the last bit into one level on a few pixels:
# those runs are compared the way tests/test_distributed_cpu.py compares them.
_CFG = dict(SAM_VERSION="vit_b", PATCH_SIZE=128, TOPONET_VERSION="normal", SAM_CKPT_PATH="", ENCODER_DEPTH=1,
            ENCODER_GLOBAL_ATTN_INDEXES=[], INFER_BATCH_SIZE=3, SAMPLE_MARGIN=16, INFER_PATCHES_PER_EDGE=5,
            ITSC_THRESHOLD=0.5, ROAD_THRESHOLD=0.5, TOPO_THRESHOLD=0.5, ITSC_NMS_RADIUS=8, ROAD_NMS_RADIUS=16,
            NEIGHBOR_RADIUS=64, MAX_NEIGHBOR_QUERIES=16)
_FIVE = [(384, 640), (640, 384), (448, 448), (640, 384), (401, 523)]


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


class _CpuStandIn(torch.nn.Module):
    """SAMRoad's scene-level interface (scene_pass1 / scene_normalise / infer_toponet) on the CPU oracle, for [H, W] scenes."""

    def __init__(self, cfg):
        super().__init__()
        from oracle.samroad import AttrDict, SAMRoadOracle
        from oracle.synth import synth_state_dict
        self.oracle = SAMRoadOracle(AttrDict(cfg)).eval()
        sd = synth_state_dict(self.oracle, 77)
        sd["map_decoder.7.bias"] = torch.tensor([-0.3, 0.2])
        self.oracle.load_state_dict(sd, strict=True)
        self.P = cfg["PATCH_SIZE"]

    def scene_pass1(self, scene, tile_xy, bs):
        (H, W), P = scene.shape[:2], self.P
        kp, road = torch.zeros((H, W)), torch.zeros((H, W))
        embs = []
        for x0, y0 in tile_xy.tolist():
            s, e = self.oracle.infer_masks_and_img_features(scene[y0:y0 + P, x0:x0 + P].float()[None])
            kp[y0:y0 + P, x0:x0 + P] += s[0, :, :, 0]
            road[y0:y0 + P, x0:x0 + P] += s[0, :, :, 1]
            embs.append(e)
        emb = torch.cat(embs) if embs else torch.zeros((0, 256, P // 16, P // 16))
        return kp, road, emb

    def scene_normalise(self, kp, road, tile_xy):
        cnt = torch.zeros_like(kp)
        for x0, y0 in tile_xy.tolist():
            cnt[y0:y0 + self.P, x0:x0 + self.P] += 1.0
        u8 = lambda t: torch.nan_to_num(t / cnt * 255, nan=0.0).to(torch.uint8)
        return u8(kp), u8(road)

    def infer_toponet(self, emb, points, pairs, valid):
        return self.oracle.infer_toponet(emb, points, pairs.long(), valid.bool())


def _rect_scene(H, W, seed):
    from oracle.synth import synth_scene
    return np.ascontiguousarray(synth_scene(max(H, W), seed=seed)[:H, :W])


def _rank(world, rank, port, out, shapes, overrides, mode):
    warnings.simplefilter("ignore")
    if world > 1:
        os.environ["MASTER_ADDR"] = "127.0.0.1"
        os.environ["MASTER_PORT"] = str(port)
        dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from sam_road_amd.inferencer import infer_imgs, infer_one_img
        torch.set_num_threads(2)
        D._CHECK_BANDS[0] = True                  # every sender asserts that its canvas is zero outside the band it ships
        cfg = dict(_CFG, **(overrides or {}))
        net = _CpuStandIn(cfg)
        imgs = [_rect_scene(h, w, 60 + i) for i, (h, w) in enumerate(shapes)]
        serial = [infer_one_img(net, im, Config(cfg), device="cpu") for im in imgs]
        if mode == "pipelined" and world > 1:
            got = list(infer_imgs(net, iter(imgs), Config(dict(cfg, TILE_SHARD_PIPELINE=True)), device="cpu"))
            for a, b in zip(got, serial):         # same world size: same summation orders, so the two loops agree exactly
                assert (a is None) == (b is None) == (rank != 0)
                if a is not None:
                    for x, y in zip(a, b):
                        np.testing.assert_array_equal(np.asarray(x), np.asarray(y))
                        assert np.asarray(x).dtype == np.asarray(y).dtype
        else:
            got = serial
        out.put((rank, [None if r is None else [np.asarray(a) for a in r] for r in got]))
    except Exception:  # pragma: no cover
        import traceback
        out.put((rank, "ERR " + traceback.format_exc()))
    finally:
        if world > 1:
            dist.destroy_process_group()


def _run_worlds(worlds, shapes, overrides, mode):
    ctx = mp.get_context("spawn")
    results = {}
    for world in worlds:
        port, q = _free_port(), ctx.Queue()
        procs = [ctx.Process(target=_rank, args=(world, r, port, q, shapes, overrides, mode)) for r in range(world)]
        for p in procs:
            p.start()
        got = dict(q.get(timeout=900) for _ in range(world))
        for p in procs:
            p.join(timeout=60)
        for r, v in got.items():
            assert not isinstance(v, str), v
            assert all((x is None) == (r != 0) for x in v)                     # only rank 0 returns the graphs
        results[world] = got[0]
    return results


def _compare(one, many, shapes, must_be_identical):
    assert len(one) == len(many) == len(shapes)
    for (n1, e1, k1, r1), (nw, ew, kw, rw), hw in zip(one, many, shapes):
        assert k1.shape == r1.shape == kw.shape == rw.shape == tuple(hw)
        assert n1.shape[0] > 30 and e1.shape[0] > 100
        assert n1[:, 0].max() < hw[0] and n1[:, 1].max() < hw[1]               # (row, col)
        assert np.abs(k1.astype(int) - kw.astype(int)).max() <= 1 and np.abs(r1.astype(int) - rw.astype(int)).max() <= 1
        same_masks = np.array_equal(k1, kw) and np.array_equal(r1, rw)
        print(hw, "masks identical to single process:", same_masks, "| nodes", n1.shape[0], "edges", e1.shape[0])
        assert same_masks or not must_be_identical
        if same_masks:
            np.testing.assert_array_equal(n1, nw)
            np.testing.assert_array_equal(e1, ew)                              # same edges in the same (insertion) order
        else:
            assert abs(n1.shape[0] - nw.shape[0]) <= 2


@pytest.mark.parametrize("overrides,must_be_identical", [
    (dict(SAMPLE_MARGIN=0, INFER_PATCHES_PER_EDGE=[3, 5]), True),    # 3 x 5 disjoint tiles; 5 tiles per rank = 1 2/3 columns
    (dict(INFER_PATCHES_PER_EDGE=[4, 6]), False),                    # overlapping tiles, 8 per rank = 2 columns
])
def test_serial_tile_sharded_world3_rect(overrides, must_be_identical):
    shapes = [(384, 640)]
    res = _run_worlds((1, 3), shapes, overrides, "serial")
    _compare(res[1], res[3], shapes, must_be_identical)


def test_pipelined_tile_sharded_world2_five_rect_scenes():
    """The pipelined tile-sharded loop on two ranks over five scenes of four shapes (640 x 384 right after 384 x 640): equal to the
    serial tile-sharded loop of the same world exactly (checked inside the ranks), and to the single-process run."""
    res = _run_worlds((1, 2), _FIVE, None, "pipelined")
    _compare(res[1], res[2], _FIVE, False)
