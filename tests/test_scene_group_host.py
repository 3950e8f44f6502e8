"""SCENE_GROUP (the tiles of several small scenes batched into one pass 1), the GPU-free part: the key and its errors, how
groups form, the stack's geometry, the two kernels' addressing run item by item on the CPU, the C-ABI surface, the CLI, and the
orchestration of the grouped loop through a CPU stand-in whose pack and crop are numpy.  The stand-in's model is batch-independent, so
a grouped run must equal infer_one_img scene by scene EXACTLY; on the GPU the same comparison is within a level (tests/test_gpu_scene_group.py)."""
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
from sam_road_amd.inferencer import group_fits, group_geometry, infer_imgs, infer_one_img, scene_group_key

from scene_kit import HOST_CFG, SceneStandIn, assert_abi_11, make_mask, np_pad, rect_grid, rect_scene, run_cli, same_tuple

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(160, 160), (384, 640), (200, 300), (161, 257), (401, 523)]
SMALL = (100, 140)                                       # raises without SCENE_PAD: smaller than PATCH_SIZE + 2 SAMPLE_MARGIN = 160


def np_stack(ragged, table, C, Ha, Wa, mode, fill):
    """The stack of DESIGN.md §6h from numpy.pad: every scene padded by its own pads into zeros."""
    out = np.zeros((Ha, Wa, 3) if C == 3 else (Ha, Wa), dtype=ragged.dtype)
    for off, H, W, top, left, Hv, Wv, row0 in np.asarray(table).tolist():
        block = ragged[off:off + H * W * C].reshape((H, W, 3) if C == 3 else (H, W))
        out[row0:row0 + Hv, :Wv] = np_pad(block, (top, Hv - H - top, left, Wv - W - left), mode, fill)
    return out


class GroupStandIn(SceneStandIn):
    """The kit's stand-in plus the two entries of a scene group, from numpy, logged.  The base class has neither, so every stand-in test
    of the other scene features keeps proving that a run without the key calls neither."""

    def scene_group_pack(self, ragged, table, C, Ha, Wa, mode="reflect", fill=(0, 0, 0), table_dev=None):
        assert ragged.dim() == 1 and table.dtype == torch.int64 and tuple(table.shape[1:]) == (8,)
        assert table_dev is None or torch.equal(table_dev, table)
        self.calls.append(("group_pack", int(table.shape[0]), C, (int(Ha), int(Wa))))
        return torch.from_numpy(np_stack(ragged.numpy(), table.numpy(), C, int(Ha), int(Wa), mode, fill))

    def scene_group_crop(self, kp, road, table, table_dev=None):
        assert table_dev is None or torch.equal(table_dev, table)
        self.calls.append(("group_crop", int(table.shape[0])))
        t = table.numpy()
        total = int((t[:, 1] * t[:, 2]).sum())
        out = np.full((2, total), 0xEE, np.uint8)
        for off, H, W, top, left, _, _, row0 in t.tolist():
            for j, m in enumerate((kp, road)):
                out[j, off:off + H * W] = m.numpy()[row0 + top:row0 + top + H, left:left + W].reshape(-1)
        return torch.from_numpy(out)


_NETS = {}


def standin(*features):
    warnings.simplefilter("ignore")
    torch.set_num_threads(4)
    if features not in _NETS:
        _NETS[features] = GroupStandIn(dict(HOST_CFG), features)
    net = _NETS[features]
    net.calls.clear()
    return net


def stream(extra=()):
    return [rect_scene(h, w, 60 + i) for i, (h, w) in enumerate(SHAPES + list(extra))]


def group_calls(net):
    return [c for c in net.calls if c[0] in ("group_pack", "group_crop")]


# ---- the key ----------------------------------------------------------------------------------------------------------------------
def test_key_forms_and_refusals():
    for absent in (Config({}), Config(dict(SCENE_GROUP=None)), Config(dict(SCENE_GROUP=1)), Config(dict(SCENE_GROUP=np.int64(1)))):
        assert scene_group_key(absent) == 1
    assert scene_group_key(Config(dict(SCENE_GROUP=4))) == 4 and scene_group_key(Config(dict(SCENE_GROUP=4)), group=2) == 2
    assert scene_group_key(Config(dict(SCENE_GROUP=4)), group=1) == 1 and scene_group_key(Config({}), group=np.int32(7)) == 7

    class Untouchable(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.w = torch.nn.Parameter(torch.zeros(1))

        def __getattr__(self, name):
            if name.startswith("scene_") or name.startswith("infer_"):
                raise AssertionError(f"the model was touched: {name}")
            return super().__getattr__(name)

    net, img = Untouchable(), np.zeros((160, 160, 3), np.uint8)
    for bad in (0, -1, True, 2.5, "3", [2], {"n": 2}):
        with pytest.raises(ValueError, match="SCENE_GROUP"):
            scene_group_key(Config(dict(SCENE_GROUP=bad)))
        with pytest.raises(ValueError, match="SCENE_GROUP"):
            list(infer_imgs(net, [img], Config(dict(HOST_CFG, SCENE_GROUP=bad)), device="cpu"))
        with pytest.raises(ValueError, match="SCENE_GROUP"):
            list(infer_imgs(net, [img], Config(HOST_CFG), device="cpu", group=bad))
    # a tile-sharded mode together with the key says so; without the key, or with 1, it is the loop it always was
    for kw in (dict(tile_sharded=True), dict(tile_sharded=True, pipelined=True)):
        with pytest.raises(ValueError, match="tile-sharded"):
            list(infer_imgs(net, [img], Config(dict(HOST_CFG, SCENE_GROUP=2)), device="cpu", **kw))
        with pytest.raises(ValueError, match="tile-sharded"):
            list(infer_imgs(net, [img], Config(HOST_CFG), device="cpu", group=3, **kw))
    # infer_one_img does not read the key
    with pytest.raises(AssertionError, match="the model was touched"):
        infer_one_img(net, img, Config(dict(HOST_CFG, SCENE_GROUP="nonsense")), device="cpu")


# ---- how groups form ----------------------------------------------------------------------------------------------------------------
def test_group_forming(monkeypatch):
    cfg = Config(HOST_CFG)
    imgs = [np.zeros((160 + i, 170, 3), np.uint8) for i in range(7)]
    sizes = lambda groups: [[g.shape[0] - 160 for g in grp] for grp in groups]
    form = lambda n, **kw: sizes(inf._scene_groups(iter(imgs), inf._valid_iter(kw.get("valids")), cfg, n))
    assert form(3) == [[0, 1, 2], [3, 4, 5], [6]] and form(7) == [[0, 1, 2, 3, 4, 5, 6]] and form(2) == [[0, 1], [2, 3], [4, 5], [6]]
    assert form(100) == [list(range(7))]
    # the limit on the stack: (sum H') x (max W') <= 2^31 - 1
    assert group_fits([(46340, 46340), (1, 1)], 4) and not group_fits([(46340, 46340), (2, 1)], 4)              # 46342 x 46340 = 2147488280
    assert group_fits([(1, 2 ** 31 - 1)], 1) and not group_fits([(1, 2 ** 31 - 1), (1, 1)], 2)
    assert group_fits([(30000, 100), (30000, 35791)], 2) and not group_fits([(30000, 100), (30000, 35792)], 2)       # 60000 x 35791 = 2147460000
    assert not group_fits([(160, 160)] * 3, 2)
    # a group closes BEFORE the scene that would pass the limit (here: a stack of at most 500 rows)
    monkeypatch.setattr(inf, "group_fits", lambda s, n: len(s) <= n and sum(h for h, _ in s) <= 500)
    assert form(5) == [[0, 1, 2], [3, 4, 5], [6]] and form(2) == [[0, 1], [2, 3], [4, 5], [6]]
    # valids are read in step with imgs, and a scene that would raise alone raises the same error from the planning step
    masks = [None, np.ones((161, 170), bool), None, None, np.ones((3, 3), bool)]
    got = list(inf._scene_groups(iter(imgs[:4]), inf._valid_iter(masks), cfg, 2))
    assert [[g.valid is not None for g in grp] for grp in got] == [[False, True], [False, False]]
    with pytest.raises(ValueError, match="valid must have the scene's shape"):
        list(inf._scene_groups(iter(imgs[:5]), inf._valid_iter(masks), cfg, 2))
    with pytest.raises(ValueError, match="^scene height 100 px is smaller than PATCH_SIZE"):
        list(inf._scene_groups(iter([imgs[0], np.zeros(SMALL + (3,), np.uint8)]), inf._valid_iter(None), cfg, 2))


# ---- geometry ---------------------------------------------------------------------------------------------------------------------
def test_geometry_against_a_numpy_restatement():
    P, m = HOST_CFG["PATCH_SIZE"], HOST_CFG["SAMPLE_MARGIN"]
    shapes = [(160, 160), (100, 140), (200, 300), (161, 257), (1, 1)]
    for pad_key, per_edge in ((None, 2), ({"border": [8, 24], "mode": "edge"}, [2, 3]), (0, 1)):
        cfg = Config(dict(HOST_CFG, INFER_PATCHES_PER_EDGE=per_edge, **({} if pad_key is None else dict(SCENE_PAD=pad_key))))
        use = [s for s in shapes if pad_key is not None or min(s) >= P + 2 * m]
        masks = [make_mask("band", *s) if i == 1 else None for i, s in enumerate(use)]
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            scenes = [inf._plan_group_scene(np.zeros(s + (3,), np.uint8), v, cfg) for s, v in zip(use, masks)]
        Ha, Wa, tables, xy, first = group_geometry(scenes)
        pads = [(inf.scene_pad_plan(s, cfg) or (0, 0, 0, 0))[:4] for s in use]
        virt = [(h + p[0] + p[1], w + p[2] + p[3]) for (h, w), p in zip(use, pads)]
        row0 = np.concatenate([[0], np.cumsum([v[0] for v in virt])])
        assert (Ha, Wa) == (int(row0[-1]), max(v[1] for v in virt)) and tables.shape == (3, len(use), 8)
        px = np.concatenate([[0], np.cumsum([h * w for h, w in use])])
        want = [[px[k], h, w, pads[k][0], pads[k][2], virt[k][0], virt[k][1], row0[k]] for k, (h, w) in enumerate(use)]
        np.testing.assert_array_equal(tables[1], want)
        np.testing.assert_array_equal(tables[0][:, 1:], tables[1][:, 1:])
        np.testing.assert_array_equal(tables[0][:, 0], 3 * px[:-1])
        # the mask table: the masked scene as it is, an unmasked one as its whole virtual rectangle of ones
        moff = 0
        for k, (h, w) in enumerate(use):
            row = [moff, h, w, pads[k][0], pads[k][2], *virt[k], row0[k]] if masks[k] is not None else [moff, *virt[k], 0, 0, *virt[k], row0[k]]
            np.testing.assert_array_equal(tables[2][k], row)
            moff += h * w if masks[k] is not None else virt[k][0] * virt[k][1]
        # the tiles: every scene's own, by the unchanged rule on its virtual size, moved down by row0, in scene order
        grid = [[(x0, y0 + int(row0[k])) for _, (x0, y0), _ in rect_grid(*virt[k], m, P, per_edge)] for k in range(len(use))]
        np.testing.assert_array_equal(xy, np.concatenate(grid))
        np.testing.assert_array_equal(first, np.concatenate([[0], np.cumsum([len(g) for g in grid])]))
        assert xy.dtype == np.int32 and [s.row0 for s in scenes] == row0[:-1].tolist()
        for k in range(len(use)):                                          # no tile straddles two scenes
            y = xy[first[k]:first[k + 1], 1]
            assert y.min() >= row0[k] and y.max() + P <= row0[k + 1] and xy[first[k]:first[k + 1], 0].max() + P <= virt[k][1]
    assert group_geometry(scenes, any_mask=False)[2].shape == (2, len(use), 8)


def test_children_map_the_kept_list_back_to_the_scenes():
    cfg = Config(dict(HOST_CFG, INFER_PATCHES_PER_EDGE=2, SCENE_PAD=8))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")                                      # two 128-px tiles leave a gap on 316 px: not this test's subject
        scenes = [inf._plan_group_scene(np.zeros(s + (3,), np.uint8), None, cfg) for s in ((160, 160), (200, 300), (161, 257))]
    first = group_geometry(scenes)[4]
    kids = inf._group_children(scenes, first, [1, 2, 8, 9, 11])            # nothing of the middle scene
    assert [(c.lo, c.hi, c.empty, c.mask_off) for c in kids] == [(0, 2, False, 0), (2, 2, True, 160 * 160), (2, 5, False, 160 * 160 + 200 * 300)]
    assert kids[0].infos == inf._shift_infos([scenes[0].infos[i] for i in (1, 2)], scenes[0].pads) and kids[0].pads == (8, 8, 8, 8)
    np.testing.assert_array_equal(kids[2].all_xy, scenes[2].all_xy[[0, 1, 3]])
    assert kids[2].infos[0][1] == (16 - 8, 16 - 8) and kids[1].infos == [] and kids[1].shape == (200, 300)


# ---- the kernels' addressing, on the CPU ------------------------------------------------------------------------------------------------
def _clang():
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    return next((c for c in (os.path.join(rocm, "llvm", "bin", "clang++"), os.path.join(rocm, "lib", "llvm", "bin", "clang++")) if os.path.exists(c)), None)


def test_kernel_addressing_on_the_cpu(tmp_path):
    """tests/scene_group_check.cpp runs every work item of whole pack and crop launches through the kernels' own per-item code
    (csrc/scene_group_piece.hpp) as a stand-alone host program built with the address and undefined-behaviour sanitizers: a byte read
    outside a source or written outside a destination ends it."""
    cxx = _clang()
    if cxx is None:
        pytest.skip("no ROCm clang++")
    exe = str(tmp_path / "scene_group_check")
    csrc = os.path.join(ROOT, "sam_road_amd", "csrc")
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", csrc,
                        os.path.join(ROOT, "tests", "scene_group_check.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    assert "scene group OK" in r.stdout


def test_scene_pad_check_still_passes_unedited(tmp_path):
    """scene_pad_piece.hpp is shared with the group kernels: its own stand-alone check, as committed, still builds and passes."""
    cxx = _clang()
    if cxx is None:
        pytest.skip("no ROCm clang++")
    exe = str(tmp_path / "scene_pad_check")
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "sam_road_amd", "csrc"),
                        os.path.join(ROOT, "tests", "scene_pad_check.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "scene pad OK" in r.stdout, (r.stdout + r.stderr)[-3000:]


def test_kernels_compile_for_gfx950_without_a_gpu():
    hipcc = next((c for c in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", shutil.which("hipcc")) if c and os.path.exists(c)), None)
    if hipcc is None:
        pytest.skip("hipcc not found")
    from sam_road_amd import build
    assert "scene_group.hip" in build.SOURCES
    r = subprocess.run([hipcc, *build.FLAGS, "-S", "--cuda-device-only", os.path.join(build.CSRC, "scene_group.hip"), "-o", "-"],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    for pat in (r"scene_group_pack_kernelILi1", r"scene_group_pack_kernelILi3", r"scene_group_crop_kernel"):
        m = re.search(r"^(_Z\w*%s\w*):" % pat, r.stdout, re.M)
        assert m, f"{pat} is not in the code object"
        meta = r.stdout[r.stdout.index(".amdhsa_kernel " + m.group(1)):]
        meta = meta[:meta.index(".end_amdhsa_kernel")]
        assert int(re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", meta).group(1)) == 0          # no scratch
        assert int(re.search(r"\.amdhsa_group_segment_fixed_size (\d+)", meta).group(1)) == 0            # no LDS
    assert "global_load_dwordx4" in r.stdout and "global_store_dwordx4" in r.stdout and "atomic" not in r.stdout


# ---- C ABI surface ------------------------------------------------------------------------------------------------------------------
def test_abi_has_the_entries_and_stays_11():
    _, lib = assert_abi_11((("srh_scene_group_pack", 13), ("srh_scene_group_crop", 12)))
    # refused without a context, before anything is launched
    assert lib.srh_scene_group_pack(None, None, 0, None, None, 1, 3, 8, 8, 0, None, None, None) == -1
    assert lib.srh_scene_group_crop(None, None, None, 8, 8, None, None, 1, None, None, 0, None) == -1


# ---- the whole loop on the CPU stand-in ------------------------------------------------------------------------------------------------
_WANT = {}


def alone(tag, net, imgs, cfg, valids=None):
    """[infer_one_img(...)] per scene, computed once per option set."""
    if tag not in _WANT:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            _WANT[tag] = [infer_one_img(net, im, Config(cfg), device="cpu", **({} if valids is None else dict(valid=v)))
                          for im, v in zip(imgs, valids or [None] * len(imgs))]
        net.calls.clear()
    return _WANT[tag]


def check_stream(got, want, shapes):
    assert len(got) == len(want) == len(shapes)
    for g, w, hw in zip(got, want, shapes):
        assert len(g) == 4 and g[2].shape == g[3].shape == tuple(hw) and g[2].flags.c_contiguous and g[2].flags.owndata
        same_tuple(g, w)                                                   # nodes and edge order included


def test_whole_loop_group_of_three_equals_scene_by_scene():
    net, imgs = standin(), stream()
    want = alone("plain", net, imgs, HOST_CFG)
    got = list(infer_imgs(net, iter(imgs), Config(HOST_CFG), device="cpu", group=3))
    check_stream(got, want, SHAPES)
    assert sum(w[0].shape[0] for w in want) > 100 and sum(w[1].shape[0] for w in want) > 100       # the graphs are not trivial
    # one pass 1 per group with the group's tile total (25 tiles per scene), one pack, one crop; no nodata call, no pad call
    assert [c for c in net.calls if c[0].startswith("pass1")] == [("pass1", 75), ("pass1", 50)]
    heights = [sum(h for h, _ in SHAPES[:3]), sum(h for h, _ in SHAPES[3:])]
    assert group_calls(net) == [("group_pack", 3, 3, (heights[0], 640)), ("group_crop", 3), ("group_pack", 2, 3, (heights[1], 523)), ("group_crop", 2)]
    # the key in the config does the same; group= overrides it
    net.calls.clear()
    check_stream(list(infer_imgs(net, iter(imgs), Config(dict(HOST_CFG, SCENE_GROUP=3)), device="cpu")), want, SHAPES)
    assert [c for c in net.calls if c[0].startswith("pass1")] == [("pass1", 75), ("pass1", 50)]
    net.calls.clear()
    check_stream(list(infer_imgs(net, iter(imgs[:2]), Config(dict(HOST_CFG, SCENE_GROUP=3)), device="cpu", group=1)), want[:2], SHAPES[:2])
    assert not group_calls(net) and [c for c in net.calls if c[0] == "pass1"] == [("pass1", 25), ("pass1", 25)]


def test_group_of_one_and_absent_key_take_the_old_path():
    """A model object WITHOUT the two entries (the kit's own stand-in) runs: absent key, None, 1, a stream of one scene under group=3, and
    the final group of one of a stream of four."""
    warnings.simplefilter("ignore")
    base, imgs = SceneStandIn(dict(HOST_CFG)), stream()
    assert not hasattr(base, "scene_group_pack") and not hasattr(base, "scene_group_crop")
    want = alone("plain", standin(), imgs, HOST_CFG)
    for kw, cfg in ((dict(), HOST_CFG), (dict(group=1), HOST_CFG), (dict(), dict(HOST_CFG, SCENE_GROUP=None)), (dict(), dict(HOST_CFG, SCENE_GROUP=1))):
        check_stream(list(infer_imgs(base, iter(imgs[:2]), Config(cfg), device="cpu", **kw)), want[:2], SHAPES[:2])
    check_stream(list(infer_imgs(base, iter(imgs[:1]), Config(HOST_CFG), device="cpu", group=3)), want[:1], SHAPES[:1])
    assert list(infer_imgs(base, iter([]), Config(HOST_CFG), device="cpu", group=3)) == []
    net = standin()
    check_stream(list(infer_imgs(net, iter(imgs[:4]), Config(HOST_CFG), device="cpu", group=3)), want[:4], SHAPES[:4])
    assert group_calls(net) == [("group_pack", 3, 3, (744, 640)), ("group_crop", 3)]
    assert [c for c in net.calls if c[0] == "pass1"] == [("pass1", 75), ("pass1", 25)]


def test_whole_loop_with_masks():
    """A band mask on scene 1, an all-nodata mask on scene 3, the others unmasked: the first group packs a mask stack (ones over the
    unmasked scenes), in the second scene 3 keeps no tile and comes out as the empty result while scene 4 runs."""
    net, imgs = standin("valid"), stream()
    valids = [None, make_mask("band", *SHAPES[1]), None, make_mask("none", *SHAPES[3]), None]
    want = alone("masks", net, imgs, HOST_CFG, valids)
    got = list(infer_imgs(net, iter(imgs), Config(HOST_CFG), device="cpu", group=3, valids=iter(valids)))
    check_stream(got, want, SHAPES)
    assert got[3][0].shape == (0, 2) and not got[3][2].any() and not got[3][3].any() and got[4][0].shape[0] > 5
    assert not got[1][2][~valids[1]].any() and got[1][2][valids[1]].any()
    packs = [c for c in net.calls if c[0] == "group_pack"]
    assert [(c[1], c[2]) for c in packs] == [(3, 3), (3, 1), (2, 3), (2, 1)]                 # a second pack per group, for the mask
    assert [c[1] for c in net.calls if c[0] == "tile_valid"] == [75, 50]
    kept = [c[1] for c in net.calls if c[0] == "pass1"]
    assert kept[0] < 75 and kept[1] == 25                                                    # the band dropped tiles; scene 3 dropped all 25
    # a group whose every scene is nodata launches nothing and yields empty results
    net.calls.clear()
    none = list(infer_imgs(net, iter(imgs[:2]), Config(HOST_CFG), device="cpu", group=2, valids=[make_mask("none", *s) for s in SHAPES[:2]]))
    assert all(r[0].shape == (0, 2) and r[1].shape == (0, 2) and r[2].shape == s and not r[2].any() for r, s in zip(none, SHAPES[:2]))
    assert not [c for c in net.calls if c[0].startswith("pass1") or c[0] == "group_crop"]
    # a final group of ONE masked scene takes the single-scene path with its mask
    net.calls.clear()
    band3 = make_mask("band", *SHAPES[3])
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        want3 = infer_one_img(net, imgs[3], Config(HOST_CFG), device="cpu", valid=band3)
    net.calls.clear()
    got4 = list(infer_imgs(net, iter(imgs[:4]), Config(HOST_CFG), device="cpu", group=3, valids=iter(valids[:3] + [band3])))
    check_stream(got4, want[:3] + [want3], SHAPES[:4])
    assert [c[1] for c in net.calls if c[0] == "group_crop"] == [3] and [c[1] for c in net.calls if c[0] == "tile_valid"] == [75, 25]
    # with unmasked groups no nodata call is made
    net.calls.clear()
    list(infer_imgs(net, iter(imgs[:2]), Config(HOST_CFG), device="cpu", group=2, valids=[None, None]))
    assert not [c for c in net.calls if c[0] in ("tile_valid", "fill")] and [c[2] for c in net.calls if c[0] == "group_pack"] == [3]


def test_whole_loop_with_hann():
    net, imgs = standin("window"), stream()
    cfg = dict(HOST_CFG, FUSE_WINDOW="hann")
    want = alone("hann", net, imgs, cfg)
    check_stream(list(infer_imgs(net, iter(imgs), Config(cfg), device="cpu", group=3)), want, SHAPES)
    assert [c for c in net.calls if c[0].startswith("pass1")] == [("pass1_window", 75), ("pass1_window", 50)]


def test_whole_loop_with_tta():
    net, imgs = standin("tta"), stream()
    cfg = dict(HOST_CFG, TTA=["id", "rot90"])
    want = alone("tta", net, imgs, cfg)
    check_stream(list(infer_imgs(net, iter(imgs), Config(cfg), device="cpu", group=3)), want, SHAPES)
    assert [c for c in net.calls if c[0].startswith("pass1")] == [("pass1_tta", 75, (0, 5), False), ("pass1_tta", 50, (0, 5), False)]
    assert [c for c in net.calls if c[0] == "normalise"] == [("normalise", 150), ("normalise", 100)]


def test_whole_loop_with_scene_pad_and_a_scene_smaller_than_a_tile():
    net = standin("pad")
    shapes = SHAPES + [SMALL]
    imgs = stream([SMALL])
    cfg = dict(HOST_CFG, SCENE_PAD={"border": [8, 24], "mode": "edge"})
    with pytest.raises(ValueError, match="smaller than"):
        list(infer_imgs(net, iter(imgs), Config(HOST_CFG), device="cpu", group=3))
    want = alone("pad", net, imgs, cfg)
    got = list(infer_imgs(net, iter(imgs), Config(cfg), device="cpu", group=3))
    check_stream(got, want, shapes)
    assert got[5][2].shape == SMALL and got[5][3].any()
    assert not [c for c in net.calls if c[0] == "pad"]                                       # the pack kernel applies every scene's own pads
    virt = [(h + 16 + max(0, 160 - h - 16), w + 48 + max(0, 160 - w - 48)) for h, w in shapes]
    assert [c[3] for c in net.calls if c[0] == "group_pack"] == [(sum(v[0] for v in virt[:3]), 688), (sum(v[0] for v in virt[3:]), 571)]


def test_results_do_not_depend_on_the_host_pool(monkeypatch):
    net, imgs = standin(), stream()
    want = alone("plain", net, imgs, HOST_CFG)
    for n in (1, 4):
        monkeypatch.setattr(inf, "worker_threads", lambda cap=8, n=n: n)
        assert inf._group_pool_threads(5) == n and inf._group_pool_threads(1) == 1
        check_stream(list(infer_imgs(net, iter(imgs), Config(HOST_CFG), device="cpu", group=5)), want, SHAPES)


def test_host_stages_take_a_thread_count():
    from sam_road_amd.graph_points import extract_graph_points
    want = alone("plain", standin(), stream(), HOST_CFG)[4]
    for nt in (None, 1, 3):
        np.testing.assert_array_equal(extract_graph_points(want[2], want[3], Config(HOST_CFG), **({} if nt is None else dict(n_threads=nt)))[:, ::-1], want[0])


# ---- CLI -----------------------------------------------------------------------------------------------------------------------------
def test_cli_scene_group_gives_the_files_of_a_run_without_it(tmp_path, monkeypatch):
    from PIL import Image
    net, imgs = standin(), stream()[:3]
    monkeypatch.chdir(tmp_path)
    names = []
    for i, im in enumerate(imgs):
        names.append(f"chip{i}.png")
        Image.fromarray(im).save(names[-1])
    plain = run_cli(cli, net, tmp_path, monkeypatch, "a", HOST_CFG, names)
    assert not group_calls(net)
    grouped = run_cli(cli, net, tmp_path, monkeypatch, "b", HOST_CFG, names, "--scene-group", "2")
    assert [c[:2] for c in group_calls(net)] == [("group_pack", 2), ("group_crop", 2)]
    by_key = run_cli(cli, net, tmp_path, monkeypatch, "c", dict(HOST_CFG, SCENE_GROUP=3), names)
    for stem in plain:
        for other in (grouped, by_key):
            np.testing.assert_array_equal(plain[stem][0], other[stem][0])
            np.testing.assert_array_equal(plain[stem][1], other[stem][1])
            assert plain[stem][2] == other[stem][2]
    assert grouped["chip0"][3]["SCENE_GROUP"] == 2 and "SCENE_GROUP" not in plain["chip0"][3]
    monkeypatch.setattr(cli, "_build_net", lambda *a: (_ for _ in ()).throw(AssertionError("the model was built")))
    with pytest.raises(ValueError, match="SCENE_GROUP"):
        inf.main(["--config", "a.yaml", "--checkpoint", "none", "--device", "cpu", "--output_dir", "e", "--images", *names, "--scene-group", "0"])
