"""ROAD_WIDTH without a GPU: the separable statement of the distance map pinned three ways (scipy's exact transform, a brute
force, the mask without background), the statistics against an independent restatement, hand-made bars, the 32-bit bound, the keep rule,
the key and the CLI flags on the CPU stand-in, the kernels' own per-item code under the host sanitizers, the cross-compile and the ABI."""
import json
import math
import os
import pickle
import re
import shutil
import subprocess
import warnings
from fractions import Fraction

import numpy as np
import pytest
import torch

from sam_road_amd import Config
from sam_road_amd import cli
from sam_road_amd import inferencer as inf
from sam_road_amd import road_width as rw
from sam_road_amd.edge_support import edge_attrs, edge_support_ref, graph_geojson
from sam_road_amd.formats import convert_to_sat2graph_format
from sam_road_amd.graph_raster import MAX_SPAN
from sam_road_amd.road_width import (MAX_COVERED, MAX_Q, MAX_RADIUS, RoadWidth, road_dist_ref, road_width_key, road_width_key_of, road_width_override, road_width_ref,
                                     width_attrs, width_keep)

import road_width_kit as wk
from scene_kit import HOST_CFG, assert_abi_11, rect_scene, run_cli

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _key(v, **kw):
    return road_width_key(Config(ROAD_WIDTH=v, **kw))


# ---- 1. the separable form, pinned three ways ------------------------------------------------------------------------------------------------------
SCIPY_CASES = [((1, 1), 3), ((37, 53), 5), ((64, 64), 32), ((40, 300), 254), ((33, 2), 1), ((1, 70), 33), ((70, 1), 2)]


@pytest.mark.parametrize("shape,R", SCIPY_CASES)
def test_dist_equals_scipy_on_every_mask_with_a_background_pixel(shape, R):
    H, W = shape
    rng = np.random.default_rng(H * 1000 + W + R)
    capped = below = 0
    masks = [(wk.random_mask(rng, H, W, level, d), level) for level, d in ((127, 0.9), (0, 0.99), (254, 0.5), (200, 0.97))]
    masks += [(wk.solid_with_holes(H, W, 127), 127), (np.zeros((H, W), np.uint8), 127), (np.full((H, W), 255, np.uint8), 255)]
    masks += [(wk.shape_mask(kind, half, H, W), 127) for kind in ("bars", "disc", "cross") for half in (R - 1, R, R + 1) if H > 1 and W > 1]
    for mask, level in masks:
        if (mask > level).all():                          # a random mask of a tiny shape may have none: the third pin covers it
            mask = mask.copy()
            mask[0, 0] = level
        got = road_dist_ref(mask, level, R)
        assert got.dtype == np.uint16 and got.shape == (H, W)
        np.testing.assert_array_equal(got, wk.scipy_dist(mask, level, R), err_msg=f"{shape} R {R} level {level}")
        capped += int((got == R * R).sum())
        below += int(((got > 0) & (got < R * R)).sum())
    assert below > 0 or R == 1 or H * W == 1              # at R = 1 every road pixel is at the cap; one pixel with a background pixel is that pixel
    assert capped > 0 or max(H, W) <= R                   # no pixel of such a shape is R away from another


@pytest.mark.parametrize("R", [1, 2, 3, 7])
def test_dist_equals_the_brute_force_on_small_masks(R):
    rng = np.random.default_rng(40 + R)
    for H, W in [(1, 1), (1, 9), (8, 1), (7, 11), (12, 12), (5, 17)]:
        for level, d in ((127, 0.85), (0, 0.95), (255, 0.5), (254, 1.0)):
            mask = wk.random_mask(rng, H, W, level, d)
            np.testing.assert_array_equal(road_dist_ref(mask, level, R), wk.brute_dist(mask, level, R), err_msg=f"{H}x{W} R {R} level {level}")


def test_dist_of_a_mask_without_background_is_all_capped():
    for (H, W), R in SCIPY_CASES:
        assert (road_dist_ref(np.full((H, W), 255, np.uint8), 254, R) == R * R).all()
        assert (road_dist_ref(np.full((H, W), 1, np.uint8), 0, R) == R * R).all()
        assert not road_dist_ref(np.full((H, W), 255, np.uint8), 255, R).any()      # nothing is above 255
    # pixels outside the image are not background: a bar that runs off both ends of the scene keeps its half-width to the very edge
    m = np.zeros((21, 50), np.uint8)
    m[7:14] = 255
    d = road_dist_ref(m, 127, 32)
    assert (d[10] == 16).all() and (d[7] == 1).all() and (d[13] == 1).all() and not d[:7].any() and not d[14:].any()
    for bad in (dict(mask=m.astype(np.int32)), dict(mask=m[0]), dict(R=0), dict(R=255), dict(R=2.0), dict(R=True), dict(on_level=256), dict(on_level=0.5)):
        with pytest.raises(ValueError):
            road_dist_ref(**dict(dict(mask=m, on_level=127, R=3), **bad))


# ---- 2. the statistics -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R", [1, 3, 32])
def test_widths_equal_the_brute_force(R):
    """Random graphs in images of at most 24 x 24, zero-length edges, nodes outside the image."""
    rng = np.random.default_rng(500 + R)
    covered = partly = 0
    for H, W in [(1, 1), (24, 24), (int(rng.integers(2, 20)), int(rng.integers(2, 24))), (9, 20)]:
        nodes, edges = wk.random_graph(rng, H, W, 6, 5, margin=7)
        mask = wk.random_mask(rng, H, W, 127, 0.8)
        d2 = road_dist_ref(mask, 127, R)
        want = wk.brute_widths(nodes, edges, d2, R)
        got = road_width_ref(nodes, edges, mask, 127, R)
        assert got.dtype == np.int32 and got.shape == (5, 8) and not got[:, 6:].any()
        np.testing.assert_array_equal(got, want, err_msg=f"R {R} {H}x{W}")
        np.testing.assert_array_equal(road_width_ref(nodes, edges, mask, 127, R, d2=d2), want)
        # n is EDGE_SUPPORT's n at width 1, and n_in its n_on over the map's support
        es = edge_support_ref(nodes, edges, (d2 > 0).astype(np.uint8), 1, 0)
        np.testing.assert_array_equal(got[:, :2], es[:, [0, 2]])
        covered += int(want[:, 0].sum())
        partly += int(((want[:, 1] > 0) & (want[:, 1] < want[:, 0])).sum())
    assert covered > 0 and partly > 0
    assert road_width_ref([], [], np.zeros((3, 3), np.uint8), 0, R).shape == (0, 8)
    assert road_width_ref([[0, 0], [1, 1]], [], np.zeros((3, 3), np.uint8), 0, R).shape == (0, 8)
    with pytest.raises(ValueError):
        road_width_ref([[0, 0], [1, 1]], [[0, 2]], np.zeros((3, 3), np.uint8), 0, R)                 # check_graph validates the graph as it is
    with pytest.raises(ValueError, match="ROAD_WIDTH"):
        road_width_ref([[0, 0], [1, 1]], [[0, 1]], np.zeros((3, 3), np.uint8), 0, R, d2=np.zeros((3, 3), np.int32))


@pytest.mark.parametrize("k", [0, 1, 3, 10])
def test_a_bar_of_thickness_2k_plus_1_is_that_wide(k):
    """A horizontal bar with an edge along its axis, far from the bar's ends: every pixel of the centre line has D2 = (k + 1)^2, Q = 16 (k + 1),
    and width_px = 2 * 16 (k + 1) n / (16 n) - 1 = 2 k + 1 exactly."""
    H, W = 2 * k + 31, 200
    m = np.zeros((H, W), np.uint8)
    m[H // 2 - k:H // 2 + k + 1] = 255
    nodes, edges = [[H // 2, 50], [H // 2, 150], [H // 2 - k - 3, 60], [H // 2 + k + 3, 60], [2, 2], [2, 40]], [[0, 1], [2, 3], [4, 5], [1, 1]]
    st = road_width_ref(nodes, edges, m, 127, 32)
    np.testing.assert_array_equal(st[0], [101, 101, 16 * (k + 1) * 101, 0, (k + 1) ** 2, (k + 1) ** 2, 0, 0])
    a = width_attrs(nodes, edges, st)
    assert a[0] == dict(width_px=2 * k + 1, width_min_px=2 * k + 1, width_max_px=2 * k + 1, in_frac=1.0, width_capped=False, length_px=100.0)
    assert isinstance(a[0]["width_px"], float) and a[0]["width_px"] == 2 * k + 1
    # across the bar: 2 k + 7 pixels, 2 k + 1 of them on the road, the widest in the middle
    assert st[1, 0] == 2 * k + 7 and st[1, 1] == 2 * k + 1 and st[1, 4] == 1 and st[1, 5] == (k + 1) ** 2
    assert a[1]["in_frac"] == (2 * k + 1) / (2 * k + 7) and a[1]["width_min_px"] == 1.0 and a[1]["width_max_px"] == 2 * k + 1
    # off the road: no width
    np.testing.assert_array_equal(st[2], [39, 0, 0, 0, 0, 0, 0, 0])
    assert a[2] == dict(width_px=None, width_min_px=None, width_max_px=None, in_frac=0.0, width_capped=False, length_px=38.0)
    assert a[3]["width_px"] == 2 * k + 1 and a[3]["length_px"] == 0.0
    # capped: with R = k the centre line is at the cap and the width is a lower bound
    if k:
        st = road_width_ref(nodes, edges, m, 127, k)
        assert st[0, 3] == 101 and st[0, 5] == k * k and width_attrs(nodes, edges, st)[0]["width_capped"] is True
        assert width_attrs(nodes, edges, st)[0]["width_px"] == 2 * k - 1
    # an edge wholly outside the image: n = 0
    st = road_width_ref([[-5, -5], [-9, -20]], [[0, 1]], m, 127, 32)
    assert not st.any() and width_attrs([[-5, -5], [-9, -20]], [[0, 1]], st)[0]["in_frac"] is None
    with pytest.raises(ValueError, match="ROAD_WIDTH"):
        width_attrs(nodes, edges, st)


def test_the_32_bit_bound():
    """The longest edges the graph check admits stay below MAX_COVERED pixels, and MAX_Q * MAX_COVERED fits int32."""
    assert MAX_Q == math.isqrt(256 * MAX_RADIUS ** 2) == 4064 and MAX_Q * MAX_COVERED < 2 ** 31
    assert (rw.q_table()[[0, 1, 2, 64516]] == [0, 16, 22, 4064]).all() and rw.q_table().dtype == np.uint16 and rw.q_table(3).shape == (10,)
    assert all(int(q) == math.isqrt(256 * v) for v, q in enumerate(rw.q_table(40).tolist()))
    S = MAX_SPAN
    l = S * math.sqrt(2)
    assert l + math.pi / 4 + (2 * l + math.pi) / 2 + 1 < MAX_COVERED
    full = np.full((1, S + 1), 255, np.uint8)
    st = road_width_ref([[0, 0], [0, S]], [[0, 1]], full, 254, 254)
    np.testing.assert_array_equal(st[0], [S + 1, S + 1, 4064 * (S + 1), S + 1, 64516, 64516, 0, 0])
    assert st[0, 0] <= MAX_COVERED and 4064 * MAX_COVERED == 188337952
    d = wk.brute_widths([[0, 0], [20, 20]], [[0, 1]], np.full((21, 21), 64516, np.uint16), 254)      # the diagonal is one pixel per row
    assert d[0, 0] == 21


# ---- 3. the keep rule ------------------------------------------------------------------------------------------------------------------------------
def test_width_keep_every_condition_and_no_evidence():
    #                n   n_in  s_q   n_cap d2_min d2_max
    rows = np.array([[10, 10, 480, 0, 9, 9, 0, 0],          # width 5 exactly: 2 * 480 / 160 - 1
                     [10, 5, 160, 0, 4, 4, 0, 0],           # half on the road, width 3
                     [10, 0, 0, 0, 0, 0, 0, 0],             # off the road: n_in = 0
                     [0, 0, 0, 0, 0, 0, 0, 0],              # outside the image: n = 0
                     [7, 7, 7 * 4064, 7, 64516, 64516, 0, 0]], np.int32)
    assert width_keep(rows, None).all() and width_keep(rows, {}).all()
    assert width_keep(rows, {"max_radius": 5}).all()                                          # a key without a condition filters nothing
    assert width_keep(rows, {"min_width": 5}).tolist() == [True, False, False, False, True]   # >= : exactly 5 is kept
    assert width_keep(rows, {"min_width": 5.000001}).tolist() == [False, False, False, False, True]
    assert width_keep(rows, {"max_width": 5}).tolist() == [True, True, False, False, False]
    assert width_keep(rows, {"max_width": 4.999999}).tolist() == [False, True, False, False, False]
    assert width_keep(rows, {"min_width": 0}).tolist() == [True, True, False, False, True]    # n_in = 0 and n = 0 fail every stated condition
    assert width_keep(rows, {"max_width": 1e9}).tolist() == [True, True, False, False, True]
    assert width_keep(rows, {"min_in": 0}).tolist() == [True, True, True, False, True]
    assert width_keep(rows, {"min_in": 0.5}).tolist() == [True, True, False, False, True]
    assert width_keep(rows, {"min_in": 0.5000001}).tolist() == [True, False, False, False, True]
    assert width_keep(rows, {"min_width": 3, "max_width": 5, "min_in": 0.6}).tolist() == [True, False, False, False, False]
    # exact in rationals where a float product would round: 2 s_q >= 16 (w + 1) n_in with w + 1 one ulp above 3
    w = float(np.nextafter(2.0, 3.0))
    assert Fraction(w) + 1 > 3 and width_keep([[10, 10, 240, 0, 4, 4, 0, 0]], {"min_width": w}).tolist() == [False]
    assert width_keep([[10, 10, 240, 0, 4, 4, 0, 0]], {"min_width": 2.0}).tolist() == [True]
    assert width_keep([], {"min_width": 1}).shape == (0,)
    for bad in (np.zeros((3, 4), np.int32), np.zeros((3, 8), np.float32)):
        with pytest.raises(ValueError, match="ROAD_WIDTH"):
            width_keep(bad, {"min_in": 0.5})


# ---- 4. the key ------------------------------------------------------------------------------------------------------------------------------------
def test_key_every_accepted_form():
    assert _key(None) is None and _key({}) is None and road_width_key(Config()) is None
    assert _key({"max_radius": 32}) == RoadWidth(127, 32, None, None, None, False)
    assert _key({"drop_isolated": True}) == RoadWidth(127, 32, None, None, None, True)        # no condition: valid, attributes only
    assert not rw.filters(_key({"on": 0.25})) and rw.filters(_key({"min_in": 0})) and not rw.filters(None)
    assert _key({"on": 0.25, "max_radius": 254, "min_width": 2, "max_width": 2, "min_in": 1, "drop_isolated": False}) == RoadWidth(63, 254, 2.0, 2.0, 1.0, False)
    assert _key({"max_radius": 1}, ROAD_THRESHOLD=0.3).on_level == 76 and _key({"on": 1.0}).on_level == 255 and _key({"on": 0}).on_level == 0
    assert _key({"max_radius": np.int64(7), "min_width": np.float32(1.5)}) == RoadWidth(127, 7, 1.5, None, None, False)
    k = _key({"min_width": 0})
    assert road_width_key_of(k) is k and k.min_width == 0.0


BAD_KEYS = ("x", 3, [1], {"radius": 3}, {"width": 3}, {"max_radius": 0}, {"max_radius": 255}, {"max_radius": 3.0}, {"max_radius": True}, {"on": -0.1}, {"on": 1.5},
            {"on": True}, {"on": "0.5"}, {"min_width": -1}, {"min_width": True}, {"min_width": float("nan")}, {"max_width": -0.5}, {"max_width": float("inf")},
            {"min_width": 5, "max_width": 4.5}, {"min_in": 1.5}, {"min_in": -0.1}, {"min_in": False}, {"drop_isolated": 1}, {"drop_isolated": "yes"})


def test_every_refusal_is_a_value_error_before_the_model_is_touched(tmp_path, monkeypatch):
    import yaml
    for bad in BAD_KEYS:
        with pytest.raises(ValueError, match="ROAD_WIDTH"):
            _key(bad)
        with pytest.raises(ValueError, match="ROAD_WIDTH"):
            road_width_key_of(bad)
    monkeypatch.chdir(tmp_path)

    def untouchable(*a, **k):
        raise AssertionError("the model was built")
    monkeypatch.setattr(cli, "_build_net", untouchable)
    cases = [(b, ()) for b in BAD_KEYS[:7]] + [(None, ("--road-width-radius", "0")), (None, ("--road-width", "--road-width-radius", "255")),
                                               (None, ("--road-width-on", "1.5")), (None, ("--road-min-width", "-1")), (None, ("--road-max-width", "-2")),
                                               (None, ("--road-min-in", "2")), (None, ("--road-min-width", "5", "--road-max-width", "4")),
                                               ({"max_width": 3}, ("--road-min-width", "3.5")), ({"drop_isolated": 1}, ("--road-width",))]
    for n, (bad, argv) in enumerate(cases):
        with open(f"bad{n}.yaml", "w") as f:
            yaml.safe_dump(dict(HOST_CFG, DATASET="cityscale", **({} if bad is None else {"ROAD_WIDTH": bad})), f)
        with pytest.raises(ValueError, match="ROAD_WIDTH"):
            inf.main(["--config", f"bad{n}.yaml", "--checkpoint", "none", "--device", "cpu", "--output_dir", "bad", *argv, "--images", "a.png"])
    assert not os.path.exists("save")


def test_cli_flags_lay_over_the_key():
    assert road_width_override(Config(), enable=True) == {"max_radius": 32}
    assert road_width_override(Config(), min_in=0.5) == {"min_in": 0.5}
    assert road_width_override(Config(), True, 0.25, 64, 2.0, 9.0, 0.75, True) == \
        {"on": 0.25, "max_radius": 64, "min_width": 2.0, "max_width": 9.0, "min_in": 0.75, "drop_isolated": True}
    keyed = Config(ROAD_WIDTH={"max_radius": 5, "min_width": 3, "drop_isolated": True})
    assert road_width_override(keyed) == keyed.ROAD_WIDTH and road_width_override(keyed, enable=True) == keyed.ROAD_WIDTH      # the config's fields stay
    assert road_width_override(keyed, max_radius=9, max_width=8) == dict(keyed.ROAD_WIDTH, max_radius=9, max_width=8)
    for kw in (dict(max_radius=0), dict(min_in=1.5), dict(min_width=-2), dict(on=2.0), dict(min_width=4, max_width=3)):
        with pytest.raises(ValueError, match="ROAD_WIDTH"):
            road_width_override(Config(), **kw)
    with pytest.raises(ValueError, match="ROAD_WIDTH"):
        road_width_override(keyed, max_width=2)                                                   # below the config's min_width
    with pytest.raises(ValueError, match="ROAD_WIDTH"):
        road_width_override(Config(ROAD_WIDTH="x"), min_in=0.5)


# ---- 5. runs without and with the key --------------------------------------------------------------------------------------------------------------------
H, W, SEED = 300, 340, 43
CFG = dict(HOST_CFG, INFER_PATCHES_PER_EDGE=2)


def _files(root):
    return sorted(os.path.relpath(os.path.join(d, f), root) for d, _, fs in os.walk(root) for f in fs)


def test_apply_equals_apply_ref_on_the_stand_in():
    rng = np.random.default_rng(9)
    net = wk.WidthStandIn(dict(CFG), ())
    nodes, edges = wk.grid_graph(120, 150)
    road = wk.shape_mask("bars", 4, 120, 150) | wk.random_mask(rng, 120, 150, 127, 0.05)
    result = (nodes, edges, np.zeros_like(road), road)
    assert rw.apply(None, result, net=net) == (result, None) and rw.apply(None, result, net=net, return_keep=True) == (result, None, None)
    assert rw.apply_ref(None, result) == (result, None) and not wk.width_calls(net)
    st = road_width_ref(nodes, edges, road, 127, 32)
    assert ((st[:, 1] > 0) & (st[:, 1] < st[:, 0])).any()
    w_med = float(np.median([a["width_px"] for a in width_attrs(nodes, edges, st) if a["width_px"] is not None]))
    for extra in ({}, {"min_width": w_med}, {"max_width": w_med, "drop_isolated": True}, {"min_in": 0.5, "max_radius": 3}, {"min_width": 1, "max_width": w_med, "min_in": 0.2, "on": 0.9}):
        key = _key(dict({"max_radius": 32}, **extra))
        net.calls.clear()
        (n1, e1, k1, r1), a1, keep = rw.apply(key, result, net=net, return_keep=True)
        (n2, e2, _, _), a2 = rw.apply_ref(key, result)
        assert np.array_equal(n1, n2) and np.array_equal(e1, e2) and a1 == a2 and k1 is result[2] and r1 is road and len(a1) == e1.shape[0] == int(keep.sum())
        assert wk.width_calls(net) == [("road_dist", (120, 150), key.on_level, key.max_radius), ("graph_edge_widths", (120, 150), key.max_radius)]
        if rw.filters(key):
            assert 0 < e1.shape[0] < edges.shape[0]
        else:
            assert np.array_equal(e1, edges) and keep.all()
    # a graph without edges calls nothing
    net.calls.clear()
    (_, e0, _, _), a0 = rw.apply(_key({"min_in": 0.5}), (nodes, np.zeros((0, 2), np.int64), road, road), net=net)
    assert e0.shape == (0, 2) and a0 == [] and not wk.width_calls(net)


def test_cli_without_the_key_is_the_run_it_was_and_with_it_writes_the_widths(tmp_path, monkeypatch):
    from PIL import Image
    warnings.simplefilter("ignore")
    torch.set_num_threads(4)
    net = wk.WidthStandIn(dict(CFG), ("valid",))
    monkeypatch.chdir(tmp_path)
    img = rect_scene(H, W, SEED)
    Image.fromarray(img).save("a.png")

    # without the key: no call, and the files of a run in which the new code is out of the way, byte for byte
    plain = run_cli(cli, net, tmp_path, monkeypatch, "plain", CFG, ["a.png"], "--viz")
    assert not wk.width_calls(net) and not wk.ek.support_calls(net)
    assert _files("save/plain") == ["config.yaml", "graph/a.p", "inference_time.txt", "mask/a_itsc.png", "mask/a_road.png", "viz/a.png"]
    with monkeypatch.context() as mp:
        def never(*a, **k):
            raise AssertionError("the new code ran")
        mp.setattr(cli, "road_width_key", lambda *a, **k: None)
        mp.setattr(cli, "apply_road_width", never)
        run_cli(cli, net, tmp_path, mp, "bypassed", CFG, ["a.png"], "--viz")
    assert _files("save/bypassed") == _files("save/plain")
    for f in _files("save/plain"):
        if f != "inference_time.txt":
            assert open(f"save/plain/{f}", "rb").read() == open(f"save/bypassed/{f}", "rb").read(), f
    assert "ROAD_WIDTH" not in plain["a"][3]

    # with the key alone: length_px and the width attributes, nothing filtered
    res = inf.infer_one_img(net, img, Config(CFG), device="cpu")
    nodes, edges, _, road = res
    assert edges.shape[0] > 3
    net.calls.clear()
    got = run_cli(cli, net, tmp_path, monkeypatch, "attrs", CFG, ["a.png"], "--road-width", "--graph-geojson", "--viz")["a"]
    assert got[3]["ROAD_WIDTH"] == {"max_radius": 32} and [c[0] for c in wk.width_calls(net)] == ["road_dist", "graph_edge_widths"] and not wk.ek.support_calls(net)
    assert _files("save/attrs") == sorted(_files("save/plain") + ["graph_geojson/a.geojson"])
    st = road_width_ref(nodes, edges, road, 127, 32)
    attrs = width_attrs(nodes, edges, st)
    assert json.load(open("save/attrs/graph_geojson/a.geojson")) == json.loads(json.dumps(graph_geojson(nodes, edges, attrs)))
    assert set(attrs[0]) == {"width_px", "width_min_px", "width_max_px", "in_frac", "width_capped", "length_px"}
    assert np.array_equal(got[1], road) and got[2] == convert_to_sat2graph_format(nodes, edges)
    for f in ("mask/a_itsc.png", "mask/a_road.png", "viz/a.png", "graph/a.p"):
        assert open(f"save/attrs/{f}", "rb").read() == open(f"save/plain/{f}", "rb").read(), f

    # a condition: the threshold is the median in_frac of the reference on this scene, so the reference decides
    f_med = float(np.median([a["in_frac"] for a in attrs]))
    key = road_width_key(Config(CFG, ROAD_WIDTH={"min_in": f_med, "max_radius": 7, "drop_isolated": True}))
    (want_nodes, want_edges, _, _), want_attrs = rw.apply_ref(key, res)
    if not 0 < want_edges.shape[0] < edges.shape[0]:      # every edge at the median: use the strict side of it
        f_med = float(np.nextafter(f_med, 2.0))
        key = road_width_key(Config(CFG, ROAD_WIDTH={"min_in": f_med, "max_radius": 7, "drop_isolated": True}))
        (want_nodes, want_edges, _, _), want_attrs = rw.apply_ref(key, res)
    assert want_edges.shape[0] < edges.shape[0]
    got = run_cli(cli, net, tmp_path, monkeypatch, "kept", CFG, ["a.png"], "--road-min-in", repr(f_med), "--road-width-radius", "7", "--drop-isolated-nodes", "--graph-geojson")["a"]
    assert got[3]["ROAD_WIDTH"] == {"min_in": f_med, "max_radius": 7, "drop_isolated": True} and "EDGE_SUPPORT" not in got[3]
    assert got[2] == convert_to_sat2graph_format(want_nodes, want_edges)                         # the pickle
    assert json.load(open("save/kept/graph_geojson/a.geojson")) == json.loads(json.dumps(graph_geojson(want_nodes, want_edges, want_attrs)))

    # behind EDGE_SUPPORT, on the graph it kept; the properties of both keys side by side
    from sam_road_amd import edge_support as es
    on = [a["on_frac"] for a in edge_attrs(nodes, edges, edge_support_ref(nodes, edges, road, 1, 127))]
    o_med = float(np.median(on))
    skey = es.edge_support_key(Config(CFG, EDGE_SUPPORT={"min_on": o_med}))
    mid, mid_attrs = es.apply_ref(skey, res)
    wkey = road_width_key(Config(CFG, ROAD_WIDTH={"max_radius": 32, "min_in": 0.0}))
    (want_nodes, want_edges, _, _), want_w = rw.apply_ref(wkey, mid)
    assert 0 < mid[1].shape[0] < edges.shape[0] and np.array_equal(want_edges, mid[1])
    net.calls.clear()
    got = run_cli(cli, net, tmp_path, monkeypatch, "both", CFG, ["a.png"], "--edge-min-on", repr(o_med), "--road-min-in", "0", "--graph-geojson")["a"]
    assert [c[0] for c in net.calls if c[0].startswith(("graph_edge", "road_"))] == ["graph_edge_stats", "road_dist", "graph_edge_widths"]
    assert got[2] == convert_to_sat2graph_format(want_nodes, want_edges)
    doc = json.load(open("save/both/graph_geojson/a.geojson"))
    assert doc == json.loads(json.dumps(graph_geojson(want_nodes, want_edges, [dict(a, **w) for a, w in zip(mid_attrs, want_w)])))
    assert {"n", "mean", "on_frac", "n_invalid", "length_px", "width_px", "in_frac", "width_capped"} <= set(doc["features"][0]["properties"])
    assert pickle.load(open("save/both/graph/a.p", "rb")) == got[2]


# ---- 6. the kernels' own code, on the CPU ----------------------------------------------------------------------------------------------------------------
def test_kernel_addressing_on_the_cpu(tmp_path):
    """tests/road_width_check.cpp runs every item of whole launches of the three kernels through their own per-item code
    (csrc/road_width_piece.hpp) as a stand-alone host program built with the address and undefined-behaviour sanitizers, against scalar
    loops over ALL pixels: shapes on and one off the chunk, strip and segment sizes, every kind of mask, maximum-span edges, every block
    of its exact size.  A byte read or written outside them ends it."""
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    cxx = next((c for c in (os.path.join(rocm, "llvm", "bin", "clang++"), os.path.join(rocm, "lib", "llvm", "bin", "clang++")) if os.path.exists(c)), None)
    if cxx is None:
        pytest.skip("no ROCm clang++")
    exe = str(tmp_path / "road_width_check")
    csrc = os.path.join(ROOT, "sam_road_amd", "csrc")
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", csrc,
                        os.path.join(ROOT, "tests", "road_width_check.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    assert "road width OK" in r.stdout
    # the tiling the tests' shapes are built around is the kernels'
    piece = open(os.path.join(csrc, "road_width_piece.hpp")).read()
    assert int(re.search(r"RW_COL_ROWS = (\d+)", piece).group(1)) == wk.COL_ROWS and int(re.search(r"RW_COL_THREADS = (\d+)", piece).group(1)) == wk.COL_STRIP
    assert int(re.search(r"RW_ROW_THREADS = (\d+)", piece).group(1)) * int(re.search(r"RW_QUAD = (\d+)", piece).group(1)) == wk.ROW_SEG


# ---- 7. the cross-compile ----------------------------------------------------------------------------------------------------------------------------------
def test_kernels_compile_for_gfx950_without_a_gpu():
    hipcc = next((c for c in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", shutil.which("hipcc")) if c and os.path.exists(c)), None)
    if hipcc is None:
        pytest.skip("hipcc not found")
    from sam_road_amd import build
    assert "road_width.hip" in build.SOURCES and "road_width.hip" in os.listdir(build.CSRC)      # in the library and in its build id
    r = subprocess.run([hipcc, *build.FLAGS, "-S", "--cuda-device-only", os.path.join(build.CSRC, "road_width.hip"), "-o", "-"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    lds = {}
    for kernel, stores in (("road_dist_cols_kernel", ("global_store_byte",)), ("road_dist_rows_kernel", ("global_store_dwordx2", "global_store_short")),
                           ("graph_edge_widths_kernel", ("global_store_dwordx4",))):
        names = set(re.findall(r"^(_Z\w*%s\w*):" % kernel, r.stdout, re.M))
        assert len(names) == 1, f"{kernel} is not in the code object: {names}"
        name = names.pop()
        meta = r.stdout[r.stdout.index(".amdhsa_kernel " + name):]
        meta = meta[:meta.index(".end_amdhsa_kernel")]
        assert int(re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", meta).group(1)) == 0, name      # no scratch
        assert int(re.search(r"\.amdhsa_uses_dynamic_stack (\d+)", meta).group(1)) == 0, name
        lds[kernel] = int(re.search(r"\.amdhsa_group_segment_fixed_size (\d+)", meta).group(1))
        body = r.stdout[r.stdout.index(name + ":"):r.stdout.index(".amdhsa_kernel " + name)]
        assert ".amdhsa_kernel" not in body and "s_endpgm" in body, name                            # this kernel's own code
        assert "atomic" not in body and all(s in body for s in stores), name
    assert lds == {"road_dist_cols_kernel": 32 * 256, "road_dist_rows_kernel": 1024 + 2 * 254,"graph_edge_widths_kernel": 0}
    body = r.stdout[r.stdout.index("graph_edge_widths_kernel"):]
    assert body[:body.index(".end_amdhsa_kernel")].count("global_store_dwordx4") == 2               # the edge's 32 bytes, two stores


# ---- 8. C ABI surface ----------------------------------------------------------------------------------------------------------------------------------------
def test_abi_has_the_entries_and_stays_11():
    header, lib = assert_abi_11((("srh_road_dist", 8), ("srh_graph_edge_widths", 13)))
    assert "ROAD_WIDTH" in header and "#define SRH_ROAD_MAX_RADIUS 254" in header
    out = torch.zeros(16, dtype=torch.int32)
    assert lib.srh_road_dist(None, None, 2, 2, 0, 1, out.data_ptr(), None) == -1                  # refused without a context
    assert lib.srh_graph_edge_widths(None, None, None, 0, None, None, 0, 2, 2, None, 1, out.data_ptr(), None) == -1
    assert not out.any()
