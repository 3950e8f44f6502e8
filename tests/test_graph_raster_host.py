"""GRAPH_RASTER without a GPU: the rule against two independent restatements (exact rationals; float64 away from the
boundary), the span bound, hand-counted cases, the properties of the comparison, the key and the CLI flags on the CPU stand-in, the kernels'
own per-item code under the host sanitizers, the cross-compile and the ABI."""
import json
import os
import pickle
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
from sam_road_amd.formats import convert_to_sat2graph_format
from sam_road_amd.graph_raster import (EDGE_COLOR, MAX_COORD, MAX_SPAN, NODE_COLOR, VIZ_DEFAULT, GraphRaster, VizStyle, check_graph, compare_ref,
                                       composite_ref, graph_mask_ref, graph_raster_key, graph_raster_key_of, graph_raster_override, graph_raster_ref,
                                       metrics, read_gt_graph, render, total_metrics)

import graph_raster_kit as gk
from scene_kit import HOST_CFG, assert_abi_11, rect_scene, run_cli

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _key(v):
    return graph_raster_key(Config(GRAPH_RASTER=v))


# ---- 1. the rule against a brute force in exact rationals ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("t", range(1, 13))
def test_ref_equals_the_fraction_brute_force(t):
    """Random graphs in images of at most 40 x 40, both marks, zero-length edges, nodes outside the image."""
    rng = np.random.default_rng(100 + t)
    shapes = [(1, 1), (40, 40) if t % 4 == 0 else (int(rng.integers(2, 30)), int(rng.integers(2, 30))), (int(rng.integers(5, 20)), int(rng.integers(20, 40)))]
    covered = 0
    for k, (H, W) in enumerate(shapes):
        nodes, edges = gk.random_graph(rng, H, W, 6, 5, margin=7)
        mark, r = ("square", "disc", "none")[(t + k) % 3], int(rng.integers(0, 5))
        want = gk.brute_raster(nodes, edges, (H, W), t, mark, r)
        np.testing.assert_array_equal(graph_raster_ref(nodes, edges, (H, W), t, mark, r), want, err_msg=f"t {t} {H}x{W} {mark} {r}")
        covered += int((want == 1).sum())
    assert covered > 0
    # a float node array is truncated toward zero, as the reference's int() does
    f = np.array([[2.9, -1.7], [7.2, 9.99]])
    np.testing.assert_array_equal(graph_raster_ref(f, [[0, 1]], (12, 12), t, "disc", 2), graph_raster_ref([[2, -1], [7, 9]], [[0, 1]], (12, 12), t, "disc", 2))


# ---- 2. the rule against float64, away from the boundary ---------------------------------------------------------------------------------------------
def test_ref_equals_float64_away_from_the_boundary():
    rng = np.random.default_rng(7)
    checked = 0
    for t in (1, 2, 3, 4, 7, 10, 31, 255):
        H, W = int(rng.integers(40, 120)), int(rng.integers(40, 120))
        nodes, edges = gk.random_graph(rng, H, W, 12, 14, margin=30)
        dist = gk.float_distance(nodes, edges, (H, W))
        sure = np.abs(dist - t / 2) > 1e-6
        got = graph_raster_ref(nodes, edges, (H, W), t) != 0
        np.testing.assert_array_equal(got[sure], (dist <= t / 2)[sure], err_msg=f"t {t}")
        checked += int(sure.sum())
        assert 0 < got.sum()
    assert checked > 20000


# ---- 3. the extremes of the span bound ---------------------------------------------------------------------------------------------------------------
def test_products_at_the_extremes_fit_64_bits_and_a_longer_edge_is_refused():
    S, t = MAX_SPAN, 255
    g = (t + 1) // 2
    worst = 0
    for dr, dc in ((S, S), (S, -S), (-S, S), (S, 0), (0, S), (S, 1)):
        L = dr * dr + dc * dc
        for pr in (-g, g, dr - g if dr < 0 else dr + g, -(S + g), S + g):
            for pc in (-g, g, dc - g if dc < 0 else dc + g, -(S + g), S + g):
                u, cross = pr * dr + pc * dc, pr * dc - pc * dr
                for v in (u, L, cross, 4 * (pr * pr + pc * pc), 4 * ((pr - dr) ** 2 + (pc - dc) ** 2), 4 * cross * cross, t * t * L, dc * (S + g)):
                    worst = max(worst, abs(v))
    assert worst < 2 ** 63 and worst == 4 * (2 * S * (S + g)) ** 2 < 2 ** 62
    assert 2 * S * (S + g) < 2 ** 30 and 2 * S * S < 2 ** 29 and S * S < 2 ** 31          # what the device keeps in 32 bits
    # the bound itself is accepted on both axes and in both directions, one pixel more is refused; so are far coordinates and bad indices
    for nodes in ([[0, 0], [S, S]], [[S, 5], [0, 5 + S]], [[-MAX_COORD, MAX_COORD - S], [-MAX_COORD + S, MAX_COORD]]):
        check_graph(nodes, [[0, 1]])
    assert graph_raster_ref([[0, 0], [0, S]], [[0, 1]], (2, S + 1), 1).sum() == S + 1
    for nodes in ([[0, 0], [S + 1, 0]], [[0, S + 1], [0, 0]], [[3, 3], [3 - S - 1, 3]]):
        with pytest.raises(ValueError, match="spans"):
            check_graph(nodes, [[0, 1]])
        check_graph(nodes, [])                             # nodes alone may lie anywhere
    for nodes, edges in (([[0, MAX_COORD + 1]], []), ([[-MAX_COORD - 1, 0]], []), ([[0, 0]], [[0, 1]]), ([[0, 0]], [[-1, 0]]), ([[0.0, float("nan")]], []),
                         ([[0, 0, 0]], []), ([[0, 0]], [[0.0, 0.0]]), ([[0, 0]], [[0, 0, 0]]), ([], [[0, 0]])):
        with pytest.raises(ValueError, match="GRAPH_RASTER"):
            check_graph(nodes, edges)
    for bad in (dict(width=0), dict(width=256), dict(width=2.0), dict(width=True), dict(mark="circle"), dict(radius=128), dict(radius=-1), dict(mark=None)):
        with pytest.raises(ValueError, match="GRAPH_RASTER"):
            graph_raster_ref([[0, 0]], [], (4, 4), **dict(dict(width=1, mark="disc", radius=1), **bad))
    for shape in ((0, 4), (4, 0), (65536, 32768)):
        with pytest.raises(ValueError, match="GRAPH_RASTER"):
            graph_raster_ref([[0, 0]], [], shape, 1)


# ---- 4. hand-counted cases -------------------------------------------------------------------------------------------------------------------------------
def test_hand_counted_cases():
    # a horizontal edge of 5 pixels at width 1: exactly its 5 pixels, an 8-connected line
    got = graph_raster_ref([[2, 1], [2, 5]], [[0, 1]], (5, 7), 1)
    want = np.zeros((5, 7), np.uint8)
    want[2, 1:6] = 1
    np.testing.assert_array_equal(got, want)
    # a vertical edge from (1, 2) to (4, 2) at width 2: the pixels within 1 of it — a 4 x 3 block and the two caps
    got = graph_raster_ref([[1, 2], [4, 2]], [[0, 1]], (6, 5), 2)
    want = np.array([[0, 0, 1, 0, 0],
                     [0, 1, 1, 1, 0],
                     [0, 1, 1, 1, 0],
                     [0, 1, 1, 1, 0],
                     [0, 1, 1, 1, 0],
                     [0, 0, 1, 0, 0]], np.uint8)
    np.testing.assert_array_equal(got, want)
    # a width-1 diagonal is the 8-connected staircase of its own pixels
    np.testing.assert_array_equal(graph_raster_ref([[0, 0], [3, 3]], [[0, 1]], (4, 4), 1), np.eye(4, dtype=np.uint8))
    # marks: a square of half-side 1 has 9 pixels, a disc of radius 1 has 5, a disc of radius 2 has 13; a node mark wins over an edge
    assert (graph_raster_ref([[3, 3]], [], (7, 7), 1, "square", 1) == 2).sum() == 9
    assert (graph_raster_ref([[3, 3]], [], (7, 7), 1, "disc", 1) == 2).sum() == 5
    assert (graph_raster_ref([[3, 3]], [], (7, 7), 1, "disc", 2) == 2).sum() == 13
    both = graph_raster_ref([[3, 1], [3, 5]], [[0, 1]], (7, 7), 1, "square", 0)
    assert both[3].tolist() == [0, 2, 1, 1, 1, 2, 0] and both.sum() == 7
    # clipped: a node at a corner outside the image, E = 0 and N = 0
    assert (graph_raster_ref([[-1, -1]], [], (4, 4), 1, "square", 2) == 2).sum() == 4
    assert not graph_raster_ref([], [], (3, 3), 4, "disc", 4).any() and not graph_raster_ref([[9, 9], [30, 9]], [[0, 1]], (5, 5), 3).any()
    # the mask product: 0 / 255, width 2 rho, squares of half-side rho
    m = graph_mask_ref([[3, 3], [3, 8]], [[0, 1]], (7, 12), 1)
    assert set(np.unique(m)) == {0, 255} and (m != 0).sum() == 3 * 8


# ---- 5. properties of the comparison ---------------------------------------------------------------------------------------------------------------------
def test_properties_of_the_comparison():
    rng = np.random.default_rng(11)
    H, W = 90, 120
    a = gk.random_graph(rng, H, W, 14, 18, margin=10)
    for thin, wide in ((1, 1), (1, 5), (2, 3), (5, 5), (3, 60)):
        lo, hi = graph_mask_ref(*a, (H, W), thin), graph_mask_ref(*a, (H, W), wide)
        assert not (lo & ~hi).any() and lo.any()                                        # thin is a subset of wide
        m, image = compare_ref(a, a, (H, W), thin, wide)
        assert m["n_fp"] == m["n_missed"] == 0 and m["precision"] == m["recall"] == 1.0 and m["n_pred"] == m["n_gt"] == (lo != 0).sum()
        assert not image.any()                                                          # nothing to paint on black
    with pytest.raises(ValueError, match="thin <= wide"):
        compare_ref(a, a, (H, W), 3, 2)
    # disjoint graphs: everything is a false positive and everything is missed
    left = (np.array([[10, 5], [80, 20]]), np.array([[0, 1]]))
    right = (np.array([[10, 100], [80, 110]]), np.array([[0, 1]]))
    m, image = compare_ref(left, right, (H, W), 1, 5)
    assert m["precision"] == m["recall"] == 0.0 and m["n_fp"] == m["n_pred"] > 0 and m["n_missed"] == m["n_gt"] > 0
    assert (image[..., 2] == 255).sum() == m["n_fp"] and (image[..., 0] == 255).sum() == m["n_missed"]
    # an empty side: the ratio with a zero denominator is None
    me, _ = compare_ref(([], []), right, (H, W), 1, 5)
    assert me["precision"] is None and me["recall"] == 0.0 and me["n_pred"] == 0
    assert metrics((0, 0, 0, 0)) == dict(n_pred=0, n_fp=0, n_gt=0, n_missed=0, precision=None, recall=None)
    # the counts respect valid, and so does the paint
    valid = np.zeros((H, W), np.uint8)
    valid[:, :60] = 3
    mv, iv = compare_ref(left, right, (H, W), 1, 5, valid=valid)
    assert mv["n_gt"] == mv["n_missed"] == 0 and mv["recall"] is None and mv["n_pred"] == mv["n_fp"] == m["n_pred"]
    assert not iv[:, 60:].any()
    # red wins over blue where both hold, and the scene shows through elsewhere
    img = rng.integers(0, 255, (H, W, 3), dtype=np.uint8)
    b = gk.random_graph(rng, H, W, 14, 18, margin=10)
    m, image = compare_ref(a, b, (H, W), 1, 2, img=img)
    pt, pw, gt, gw = (graph_mask_ref(*g, (H, W), r) != 0 for g, r in ((a, 1), (a, 2), (b, 1), (b, 2)))
    counts, want = gk.np_compare(pt, pw, gt, gw, img=img)
    assert [m[k] for k in ("n_pred", "n_fp", "n_gt", "n_missed")] == counts and 0 < m["n_fp"] < m["n_pred"]
    np.testing.assert_array_equal(image, want)
    t = total_metrics([m, mv])
    assert t["n_pred"] == m["n_pred"] + mv["n_pred"] and t["precision"] == 1 - (m["n_fp"] + mv["n_fp"]) / t["n_pred"]


# ---- 6. the key and the CLI --------------------------------------------------------------------------------------------------------------------------------
def test_key_every_accepted_form():
    assert graph_raster_key(Config()) is None
    for off in (None, {}, {"viz": None}, {"viz": False, "mask": None, "diff": False}, {"diff": {}}):
        assert _key(off) is None
    assert _key({"viz": True}) == GraphRaster(VIZ_DEFAULT, None, None) == _key({"viz": {"width": 4, "mark": " Disc ", "radius": 4}})
    assert VIZ_DEFAULT == VizStyle(4, "disc", 4, (253, 160, 15), (255, 255, 0)) == VizStyle(4, "disc", 4, EDGE_COLOR, NODE_COLOR)
    k = _key({"viz": {"width": 255, "mark": "square", "radius": 0, "edge_color": [1, 2, 3], "node_color": (0, 0, 255)}, "mask": 3, "diff": True})
    assert k == GraphRaster(VizStyle(255, "square", 0, (1, 2, 3), (0, 0, 255)), 3, (1, 5))
    assert _key({"mask": {"radius": 127}}).mask == 127 and _key({"mask": np.int64(1)}).mask == 1
    assert _key({"diff": {"thin": 2}}).diff == (2, 5) and _key({"diff": {"wide": 9}}).diff == (1, 9) and _key({"diff": {"thin": 4, "wide": 4}}).diff == (4, 4)
    assert _key({"viz": {"mark": "none", "radius": 127}}).viz.mark == "none"
    assert graph_raster_key_of(k) is k


BAD_KEYS = ("x", 3, True, [1], {"vis": True}, {"viz": 1}, {"viz": "yes"}, {"viz": {"colour": [1, 2, 3]}}, {"viz": {"width": 0}}, {"viz": {"width": 256}},
            {"viz": {"width": 4.0}}, {"viz": {"width": True}}, {"viz": {"mark": "circle"}}, {"viz": {"mark": 1}}, {"viz": {"radius": 128}}, {"viz": {"radius": -1}},
            {"viz": {"edge_color": [1, 2]}}, {"viz": {"edge_color": [1, 2, 256]}}, {"viz": {"node_color": [1, 2, -1]}}, {"viz": {"node_color": [1.0, 2, 3]}},
            {"viz": {"node_color": "red"}}, {"mask": 0}, {"mask": 128}, {"mask": 2.5}, {"mask": True}, {"mask": {"radius": 0}}, {"mask": {"rho": 3}},
            {"mask": {"radius": 3, "x": 1}}, {"diff": 1}, {"diff": [1, 5]}, {"diff": {"thin": 0}}, {"diff": {"wide": 128}}, {"diff": {"thin": 3, "wide": 2}},
            {"diff": {"thin": 1.0}}, {"diff": {"thick": 2}}, {"viz": True, "masks": 3})


def test_every_refusal_is_a_value_error_before_the_model_is_touched(tmp_path, monkeypatch):
    import yaml
    for bad in BAD_KEYS:
        with pytest.raises(ValueError, match="GRAPH_RASTER"):
            _key(bad)
    # the CLI refuses before it builds the model
    monkeypatch.chdir(tmp_path)

    def untouchable(*a, **k):
        raise AssertionError("the model was built")
    monkeypatch.setattr(cli, "_build_net", untouchable)
    for n, (bad, argv) in enumerate([(b, ()) for b in BAD_KEYS[:8]] + [(None, ("--graph-mask", "0")), (None, ("--graph-mask", "128")), (None, ("--diff", "3", "2")),
                                                                        (None, ("--diff", "1")), (None, ("--diff", "0", "5")), ({"viz": {"width": 0}}, ("--viz",)),
                                                                        (None, ("--diff",))]):     # the last: --images without --gt-graphs
        with open(f"bad{n}.yaml", "w") as f:
            yaml.safe_dump(dict(HOST_CFG, DATASET="cityscale", **({} if bad is None else {"GRAPH_RASTER": bad})), f)
        with pytest.raises(ValueError, match="GRAPH_RASTER"):
            inf.main(["--config", f"bad{n}.yaml", "--checkpoint", "none", "--device", "cpu", "--output_dir", "bad", *argv, "--images", "a.png"])
    with open("good.yaml", "w") as f:
        yaml.safe_dump(dict(HOST_CFG, DATASET="cityscale"), f)
    with pytest.raises(SystemExit):                        # --gt-graphs must be parallel to --images
        inf.main(["--config", "good.yaml", "--checkpoint", "none", "--device", "cpu", "--diff", "--gt-graphs", "a.p", "b.p", "--images", "a.png"])
    assert not os.path.exists("save")


def test_cli_flags_lay_over_the_key():
    assert graph_raster_override(Config()) == {}
    assert graph_raster_override(Config(), viz=True) == {"viz": True}
    assert graph_raster_override(Config(), mask=3, diff=True) == {"mask": {"radius": 3}, "diff": True}
    assert graph_raster_override(Config(), diff=[2, 7]) == {"diff": {"thin": 2, "wide": 7}}
    styled = Config(GRAPH_RASTER={"viz": {"width": 2, "mark": "square"}, "mask": 5, "diff": {"thin": 2, "wide": 3}})
    assert graph_raster_override(styled, viz=True, diff=True) == styled.GRAPH_RASTER                 # the config's style and radii stay
    assert graph_raster_override(styled, mask=1, diff=[1, 1]) == dict(styled.GRAPH_RASTER, mask={"radius": 1}, diff={"thin": 1, "wide": 1})
    assert graph_raster_override(Config(GRAPH_RASTER={"viz": False}), viz=True) == {"viz": True}
    for kw in (dict(mask=0), dict(diff=[3, 2]), dict(diff=[1]), dict(diff=[1, 2, 3])):
        with pytest.raises(ValueError, match="GRAPH_RASTER"):
            graph_raster_override(Config(), **kw)
    with pytest.raises(ValueError, match="GRAPH_RASTER"):
        graph_raster_override(Config(GRAPH_RASTER="x"), viz=True)


H, W, SEED = 300, 340, 43
CFG = dict(HOST_CFG, INFER_PATCHES_PER_EDGE=2)
GT = (np.array([[20, 30], [150, 60], [280, 300], [-10, 200], [40, 339]]), np.array([[0, 1], [1, 2], [3, 4], [1, 4]]))


def _files(root):
    return sorted(os.path.relpath(os.path.join(d, f), root) for d, _, fs in os.walk(root) for f in fs)


def test_cli_writes_the_renders_of_the_returned_graph(tmp_path, monkeypatch):
    """The flags on the CPU stand-in (the kernels themselves are checked on the GPU): every file is the host composition of the graph the run
    returned, a scene without a ground truth gets no diff, the products run on the stand-in's three methods, and a run without the flags
    writes exactly the files it wrote before and calls none of them."""
    from PIL import Image
    warnings.simplefilter("ignore")
    torch.set_num_threads(4)
    net = gk.RasterStandIn(dict(CFG), ("valid",))
    monkeypatch.chdir(tmp_path)
    a, b = rect_scene(H, W, SEED), rect_scene(H, W, SEED + 1)
    Image.fromarray(a).save("a.png")
    Image.fromarray(b).save("b.png")
    valid = np.ones((H, W), np.uint8)
    valid[:, 200:] = 0
    np.save("va.npy", valid)
    with open("gt.p", "wb") as f:
        pickle.dump(convert_to_sat2graph_format(*GT), f)
    gt = read_gt_graph("gt.p")
    np.testing.assert_array_equal(graph_mask_ref(*gt, (H, W), 2), graph_mask_ref(*GT, (H, W), 2))          # the pickle round trip keeps the graph
    sp = read_gt_graph("gt.p", spacenet=True)[0]
    assert sorted(map(tuple, sp.tolist())) == sorted((400 - r, c) for r, c in GT[0].tolist())              # inferencer.py:289-292

    plain = run_cli(cli, net, tmp_path, monkeypatch, "plain", CFG, ["a.png", "b.png"])
    assert not gk.raster_calls(net)
    assert _files("save/plain") == ["config.yaml", "graph/a.p", "graph/b.p", "inference_time.txt", "mask/a_itsc.png", "mask/a_road.png", "mask/b_itsc.png", "mask/b_road.png"]
    got = run_cli(cli, net, tmp_path, monkeypatch, "all", CFG, ["a.png", "b.png"], "--viz", "--graph-mask", "3", "--diff", "--gt-graphs", "gt.p", "-",
                  "--valid-masks", "va.npy", "-")
    assert got["a"][3]["GRAPH_RASTER"] == {"viz": True, "mask": {"radius": 3}, "diff": True}
    assert _files("save/all") == sorted(_files("save/plain") + ["viz/a.png", "viz/b.png", "graph_mask/a.png", "graph_mask/b.png", "diff/a.png", "diff/metrics.json"])
    assert plain["b"][2] == got["b"][2] and np.array_equal(plain["b"][1], got["b"][1])                    # the run itself is the run it was
    report = json.load(open("save/all/diff/metrics.json"))
    assert set(report) == {"thin", "wide", "scenes", "total"} and (report["thin"], report["wide"]) == (1, 5) and list(report["scenes"]) == ["a"]
    for stem, img, v in (("a", a, valid), ("b", b, None)):
        nodes, edges = read_gt_graph(f"save/all/graph/{stem}.p")
        assert nodes.shape[0] > 0
        cls = graph_raster_ref(nodes, edges, (H, W), 4, "disc", 4)
        np.testing.assert_array_equal(np.array(Image.open(f"save/all/viz/{stem}.png")), composite_ref(cls, img))
        np.testing.assert_array_equal(np.array(Image.open(f"save/all/graph_mask/{stem}.png")), graph_mask_ref(nodes, edges, (H, W), 3))
        if stem == "a":
            m, image = compare_ref((nodes, edges), GT, (H, W), 1, 5, valid=v, img=img)
            np.testing.assert_array_equal(np.array(Image.open("save/all/diff/a.png")), image)
            assert report["scenes"]["a"] == m == report["total"] and m["n_gt"] > 0
    assert {c[0] for c in gk.raster_calls(net)} == {"graph_raster", "graph_composite", "graph_compare"}
    # the key in the config alone does the same; a flag replaces its part
    net.calls.clear()
    keyed = dict(CFG, GRAPH_RASTER={"viz": {"width": 2, "mark": "square", "radius": 1, "edge_color": [9, 8, 7]}, "mask": 9})
    got = run_cli(cli, net, tmp_path, monkeypatch, "keyed", keyed, ["a.png"], "--graph-mask", "2")
    assert got["a"][3]["GRAPH_RASTER"]["mask"] == {"radius": 2} and _files("save/keyed")[-1] == "viz/a.png" and "graph_mask/a.png" in _files("save/keyed")
    nodes, edges = read_gt_graph("save/keyed/graph/a.p")
    np.testing.assert_array_equal(np.array(Image.open("save/keyed/viz/a.png")), composite_ref(graph_raster_ref(nodes, edges, (H, W), 2, "square", 1), a, (9, 8, 7)))
    np.testing.assert_array_equal(np.array(Image.open("save/keyed/graph_mask/a.png")), graph_mask_ref(nodes, edges, (H, W), 2))
    # render(): without a key nothing, with a scene that is not uint8 RGB the graph on black
    assert render(None, nodes, edges, (H, W), net=net) == {}
    raw = np.zeros((H, W, 4), np.uint16)
    np.testing.assert_array_equal(render(_key({"viz": True}), nodes, edges, (H, W), img=raw, net=net)["viz"], composite_ref(graph_raster_ref(nodes, edges, (H, W), 4, "disc", 4)))


# ---- 7. the kernels' own code, on the CPU ------------------------------------------------------------------------------------------------------------------
def test_kernel_addressing_on_the_cpu(tmp_path):
    """tests/graph_raster_check.cpp runs every item of whole launches through the kernels' own per-item code
    (csrc/graph_raster_piece.hpp) as a stand-alone host program built with the address and undefined-behaviour sanitizers, against a scalar
    loop over the rule in 128-bit integers: 1 x 1, 1 x 16384 and 16384 x 2 images with a maximum-span edge, out at odd byte addresses, edges
    crossing the image with both ends outside, every block of its exact size.  A byte read or written outside them ends it."""
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    cxx = next((c for c in (os.path.join(rocm, "llvm", "bin", "clang++"), os.path.join(rocm, "lib", "llvm", "bin", "clang++")) if os.path.exists(c)), None)
    if cxx is None:
        pytest.skip("no ROCm clang++")
    exe = str(tmp_path / "graph_raster_check")
    csrc = os.path.join(ROOT, "sam_road_amd", "csrc")
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", csrc,
                        os.path.join(ROOT, "tests", "graph_raster_check.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    assert "graph raster OK" in r.stdout


# ---- 8. the cross-compile ------------------------------------------------------------------------------------------------------------------------------------
def test_kernels_compile_for_gfx950_without_a_gpu():
    hipcc = next((c for c in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", shutil.which("hipcc")) if c and os.path.exists(c)), None)
    if hipcc is None:
        pytest.skip("hipcc not found")
    from sam_road_amd import build
    assert "graph_raster.hip" in build.SOURCES
    r = subprocess.run([hipcc, *build.FLAGS, "-S", "--cuda-device-only", os.path.join(build.CSRC, "graph_raster.hip"), "-o", "-"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    for kernel, lds in (("graph_clear_kernel", 0), ("graph_edges_kernel", 0), ("graph_nodes_kernel", 0), ("graph_composite_kernel", 0), ("graph_counts_zero_kernel", 0),
                        ("graph_compare_kernel", 64)):
        m = re.search(r"^(_Z\w*%s\w*):" % kernel, r.stdout, re.M)
        assert m, f"{kernel} is not in the code object"
        meta = r.stdout[r.stdout.index(".amdhsa_kernel " + m.group(1)):]
        meta = meta[:meta.index(".end_amdhsa_kernel")]
        assert int(re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", meta).group(1)) == 0, kernel      # no scratch
        assert int(re.search(r"\.amdhsa_group_segment_fixed_size (\d+)", meta).group(1)) == lds, kernel
        assert int(re.search(r"\.amdhsa_uses_dynamic_stack (\d+)", meta).group(1)) == 0, kernel
        body = r.stdout[r.stdout.index(m.group(1) + ":"):r.stdout.index(".amdhsa_kernel " + m.group(1))]
        assert ("global_atomic_add_x2" in body) == (kernel == "graph_compare_kernel"), kernel                 # the 64-bit sums of the counts
        assert "atomic" not in body or kernel == "graph_compare_kernel", kernel                               # and no atomic anywhere else
        if kernel == "graph_clear_kernel":
            assert "global_store_dwordx4" in body


# ---- 9. C ABI surface ------------------------------------------------------------------------------------------------------------------------------------------
def test_abi_has_the_entries_and_stays_11():
    header, lib = assert_abi_11((("srh_graph_raster", 16), ("srh_graph_composite", 10), ("srh_graph_compare", 12)))
    assert "GRAPH_RASTER" in header and "#define SRH_GRAPH_MAX_SPAN 16383" in header
    out = (torch.zeros(4, dtype=torch.uint8))
    assert lib.srh_graph_raster(None, None, None, 0, None, None, 0, 2, 2, 1, 0, 0, 1, 2, out.data_ptr(), None) == -1      # refused without a context
    assert lib.srh_graph_composite(None, None, None, 2, 2, None, None, None, None, None) == -1
    assert lib.srh_graph_compare(None, None, None, None, None, None, None, 2, 2, None, None, None) == -1
    assert not out.any()
