"""EDGE_SUPPORT without a GPU: the statistics against an independent restatement in exact rationals and against the
rasteriser's own reference, hand-counted cases, the 32-bit bound, the keep rule, the key and the CLI flags on the CPU stand-in, the GeoJSON
export, the kernel's own per-item code under the host sanitizers, the cross-compile and the ABI."""
import json
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
from sam_road_amd import edge_support as es
from sam_road_amd import cli
from sam_road_amd import inferencer as inf
from sam_road_amd.aoi import aoi_key_of
from sam_road_amd.edge_support import (MAX_COVERED, EdgeSupport, edge_attrs, edge_keep, edge_support_key, edge_support_key_of, edge_support_override,
                                       edge_support_ref, filter_graph, graph_geojson)
from sam_road_amd.formats import convert_to_sat2graph_format
from sam_road_amd.graph_raster import MAX_SPAN, MAX_WIDTH, composite_ref, graph_raster_ref

import edge_support_kit as ek
from scene_kit import HOST_CFG, assert_abi_11, rect_scene, run_cli

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _key(v, **kw):
    return edge_support_key(Config(EDGE_SUPPORT=v, **kw))


# ---- 1. the rule against a brute force in exact rationals ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("t", range(1, 13))
def test_ref_equals_the_brute_force(t):
    """Random graphs in images of at most 24 x 24, zero-length edges, nodes outside the image, valid present and absent."""
    rng = np.random.default_rng(300 + t)
    covered = 0
    for k, (H, W) in enumerate([(1, 1), (24, 24) if t % 4 == 0 else (int(rng.integers(2, 20)), int(rng.integers(2, 24))), (int(rng.integers(5, 12)), int(rng.integers(12, 24)))]):
        nodes, edges = ek.random_graph(rng, H, W, 6, 5, margin=7)
        mask = rng.integers(0, 256, (H, W), dtype=np.uint8)
        valid = (rng.integers(0, 3, (H, W)) != 0) if (t + k) % 2 else None
        level = int(rng.integers(0, 256))
        want = ek.brute_stats(nodes, edges, mask, t, level, valid)
        got = edge_support_ref(nodes, edges, mask, t, level, valid)
        assert got.dtype == np.int32 and got.shape == (5, 4)
        np.testing.assert_array_equal(got, want, err_msg=f"t {t} {H}x{W}")
        covered += int(want[:, 0].sum())
    assert covered > 0


def test_ref_equals_the_raster_of_the_single_edge_on_300x517():
    rng = np.random.default_rng(17)
    H, W = 300, 517
    nodes, edges = ek.random_graph(rng, H, W, 30, 40, margin=60, zero_length=3)
    nodes, edges = np.concatenate([nodes, [[-300, -300], [-280, -400]]]), np.concatenate([edges, [[30, 31]]])      # an edge wholly outside at every width
    mask = rng.integers(0, 256, (H, W), dtype=np.uint8)
    valid = (rng.integers(0, 4, (H, W)) * 60).astype(np.uint8)
    for t, level in ((1, 127), (4, 0), (31, 254), (255, 200)):
        got = edge_support_ref(nodes, edges, mask, t, level, valid)
        bare = edge_support_ref(nodes, edges, mask, t, level)
        for k, e in enumerate(edges.tolist()):
            cov = graph_raster_ref(nodes, [e], (H, W), t) == 1
            assert got[k].tolist() == [int(cov.sum()), int(mask[cov].sum(dtype=np.int64)), int((mask[cov] > level).sum()), int((valid[cov] == 0).sum())], (t, k)
        np.testing.assert_array_equal(bare[:, :3], got[:, :3])
        assert not bare[:, 3].any() and got[:, 3].any() and (got[:, 0] == 0).any() and (got[:, 0] > 0).any()


def test_hand_counted_cases():
    # a horizontal 10-px edge on a 1 x 10 mask: all ten pixels
    mask = np.arange(10, dtype=np.uint8)[None] * 20                                    # 0, 20, .. 180
    assert edge_support_ref([[0, 0], [0, 9]], [[0, 1]], mask, 1, 99).tolist() == [[10, 900, 5, 0]]
    # valid cutting it in half
    valid = np.array([[1, 1, 1, 1, 1, 0, 0, 0, 0, 0]], np.uint8)
    assert edge_support_ref([[0, 0], [0, 9]], [[0, 1]], mask, 1, 99, valid).tolist() == [[10, 900, 5, 5]]
    assert edge_support_ref([[0, 0], [0, 9]], [[0, 1]], mask, 1, 99, valid != 0).tolist() == [[10, 900, 5, 5]]
    # a width-1 diagonal is its own four pixels; > on_level is strict
    m = np.full((4, 4), 7, np.uint8)
    m[np.arange(4), np.arange(4)] = (10, 20, 30, 40)
    assert edge_support_ref([[0, 0], [3, 3]], [[0, 1]], m, 1, 20).tolist() == [[4, 100, 2, 0]]
    # an edge wholly outside: no evidence; a zero-length edge is the disc around its node
    assert edge_support_ref([[9, 9], [30, 9], [2, 2]], [[0, 1], [2, 2]], m, 3, 0).tolist() == [[0, 0, 0, 0], [9, 7 * 6 + 20 + 30 + 40, 9, 0]]      # at width 3 the 3 x 3 block around it
    assert edge_support_ref([[2, 2]], [[0, 0]], m, 1, 29).tolist() == [[1, 30, 1, 0]]
    # E = 0, and what is refused
    assert edge_support_ref([[0, 0]], [], m, 1, 0).shape == (0, 4)
    for bad in (dict(width=0), dict(width=256), dict(width=True), dict(on_level=-1), dict(on_level=256), dict(on_level=1.0), dict(mask=m.astype(np.int32)),
                dict(mask=m[0]), dict(valid=np.ones((4, 5), np.uint8)), dict(valid=np.ones((4, 4), np.int32))):
        with pytest.raises(ValueError):
            edge_support_ref(**dict(dict(nodes=[[0, 0], [3, 3]], edges=[[0, 1]], mask=m, width=1, on_level=0), **bad))


# ---- 2. the 32-bit bound, the keep rule ----------------------------------------------------------------------------------------------------------------
def test_the_32_bit_bound_in_python_ints():
    """A + P / 2 + 1 of the stadium at span 16383 on both axes and t = 255, in Python ints (rounded up where irrational), against the
    module's constant; the diagonal and the axis-parallel extremes counted exactly stay below it; a longer edge is refused."""
    S, t = MAX_SPAN, MAX_WIDTH
    assert (S, t) == (16383, 255)
    length = 23170
    assert (length - 1) ** 2 < 2 * S * S <= length ** 2                                 # ceil(S sqrt 2)
    cap_area, half_turn = 51071, 401                                                    # ceil(pi t^2 / 4), ceil(pi t / 2)
    assert Fraction(355, 113) > Fraction(3141592653589794, 10 ** 15)                    # 355 / 113 > pi
    assert cap_area >= Fraction(355, 113) * t * t / 4 and half_turn >= Fraction(355, 113) * t / 2
    bound = length * t + cap_area + length + half_turn + 1
    assert bound == MAX_COVERED == 5982993 and bound < 6 * 10 ** 6 and 255 * bound == 1525663215 < 2 ** 31
    # the axis-parallel extreme, counted exactly: rows within t / 2 of the segment, plus the two caps
    inside = sum(1 for r in range(-t, t + 1) if 4 * r * r <= t * t)
    caps = 2 * sum(1 for r in range(-t, t + 1) for c in range(1, t + 1) if 4 * (r * r + c * c) <= t * t)
    assert inside * (S + 1) + caps <= bound
    got = edge_support_ref([[200, 0], [200, S]], [[0, 1]], np.full((401, S + 1), 255, np.uint8), t, 0)[0].tolist()
    assert got == [inside * (S + 1), 255 * inside * (S + 1), inside * (S + 1), 0]       # the image clips the caps; the largest sum the reference is asked for here
    with pytest.raises(ValueError, match="spans"):
        edge_support_ref([[0, 0], [0, S + 1]], [[0, 1]], np.zeros((1, 4), np.uint8), 1, 0)


def test_edge_keep_every_condition_and_no_evidence():
    stats = np.array([[10, 2550, 10, 0],      # all on
                      [10, 1275, 5, 0],       # mean exactly 0.5, half on
                      [10, 1276, 4, 3],       # mean just above 0.5
                      [0, 0, 0, 0],           # wholly outside: no evidence
                      [4, 0, 0, 4]], np.int32)
    k = lambda **kw: EdgeSupport(**dict(dict(width=1, on_level=127, min_mean=None, min_on=None, max_invalid=None, drop_isolated=False), **kw))
    assert edge_keep(stats, k()).tolist() == [True] * 5 and edge_keep(stats, None).tolist() == [True] * 5
    assert edge_keep(stats, k(min_mean=0.5)).tolist() == [True, False, True, False, False]         # s > m 255 n is strict
    assert edge_keep(stats, k(min_mean=0.0)).tolist() == [True, True, True, False, False]
    assert edge_keep(stats, k(min_mean=1.0)).tolist() == [False] * 5
    assert edge_keep(stats, k(min_on=0.5)).tolist() == [True, True, False, False, False]           # n_on >= f n is not
    assert edge_keep(stats, k(min_on=0.0)).tolist() == [True, True, True, False, True]
    assert edge_keep(stats, k(min_on=1.0)).tolist() == [True, False, False, False, False]
    assert edge_keep(stats, k(max_invalid=0)).tolist() == [True, True, False, True, False]         # n = 0 passes max_invalid
    assert edge_keep(stats, k(max_invalid=3)).tolist() == [True, True, True, True, False]
    assert edge_keep(stats, k(min_mean=0.5, min_on=0.375, max_invalid=3)).tolist() == [True, False, True, False, False]
    assert edge_keep(stats, {"min_on": 0.5}).tolist() == [True, True, False, False, False]         # a mapping is validated first
    assert edge_keep(np.zeros((0, 4), np.int32), k(min_on=0.5)).shape == (0,)
    # exact: 0.1 is not 1 / 10 — the float is a little above it, so 1 of 10 pixels does not reach it
    assert Fraction(0.1) > Fraction(1, 10) and edge_keep(np.array([[10, 0, 1, 0]]), k(min_on=0.1)).tolist() == [False]
    # at the extreme of the bound the products leave 64 bits for some floats; Python ints do not
    big = np.array([[MAX_COVERED, 255 * MAX_COVERED, MAX_COVERED, 0]], np.int32)
    assert edge_keep(big, k(min_mean=1e-300, min_on=1.0)).tolist() == [True] and edge_keep(big, k(min_mean=1.0)).tolist() == [False]
    # monotone: raising min_mean (min_on) never keeps more edges
    rng = np.random.default_rng(5)
    n = rng.integers(0, 50, 200)
    s = rng.integers(0, 255 * n + 1)
    stats = np.stack([n, s, rng.integers(0, n + 1), rng.integers(0, 5, 200)], 1).astype(np.int32)
    last_mean = last_on = np.ones(200, bool)
    for v in np.linspace(0, 1, 41):
        a, b = edge_keep(stats, k(min_mean=float(v))), edge_keep(stats, k(min_on=float(v)))
        assert not (a & ~last_mean).any() and not (b & ~last_on).any()
        last_mean, last_on = a, b
    assert not last_mean.any() and 0 < last_on.sum() < 200


def test_filter_graph_and_attrs():
    nodes = np.array([[0, 0], [3, 4], [9, 9], [5, 5], [7, 1]], np.int64)
    edges = np.array([[0, 1], [1, 2], [3, 1], [4, 4]], np.int64)
    keep = np.array([True, False, True, False])
    n, e, idx = filter_graph(nodes, edges, keep)
    assert n is not None and np.array_equal(n, nodes) and e.tolist() == [[0, 1], [3, 1]] and idx.tolist() == [0, 1, 2, 3, 4]
    n, e, idx = filter_graph(nodes, edges, keep, drop_isolated=True)                  # nodes 2 and 4 go, the order stays, indices are renumbered
    assert n.tolist() == [[0, 0], [3, 4], [5, 5]] and e.tolist() == [[0, 1], [2, 1]] and idx.tolist() == [0, 1, 3] and e.dtype == edges.dtype
    n, e, idx = filter_graph(nodes, edges, np.zeros(4, bool), drop_isolated=True)
    assert n.shape == (0, 2) and e.shape == (0, 2) and idx.size == 0
    n, e, _ = filter_graph(np.zeros((0, 2), np.int64), np.zeros((0, 2), np.int64), np.zeros(0, bool), True)
    assert n.shape == (0, 2) and e.shape == (0, 2)
    with pytest.raises(ValueError):
        filter_graph(nodes, edges, keep[:3])
    attrs = edge_attrs(nodes, edges, [[5, 500, 2, 1], [0, 0, 0, 0], [4, 1020, 4, 0], [1, 9, 0, 0]])
    assert attrs[0] == dict(n=5, mean=100.0, on_frac=0.4, n_invalid=1, length_px=5.0)
    assert attrs[1]["mean"] is None and attrs[1]["on_frac"] is None and attrs[1]["n"] == 0 and attrs[1]["length_px"] == float(np.sqrt(np.float64(61)))
    assert attrs[2]["mean"] == 255.0 and attrs[3]["length_px"] == 0.0 and isinstance(attrs[3]["length_px"], float)
    json.dumps(attrs)


# ---- 3. the key and the CLI flags ----------------------------------------------------------------------------------------------------------------------
def test_key_every_accepted_form():
    assert edge_support_key(Config()) is None and _key(None) is None and _key({}) is None
    assert _key({"min_on": 0.5}) == EdgeSupport(1, 127, None, 0.5, None, False)
    assert _key({"min_on": 0.5}, ROAD_THRESHOLD=0.2) == EdgeSupport(1, 51, None, 0.5, None, False)          # on defaults to ROAD_THRESHOLD
    assert _key({"min_on": 1, "on": 0.3}, ROAD_THRESHOLD=0.2).on_level == 76                                # floor(0.3 * 255)
    assert _key({"width": 255, "on": 1.0, "min_mean": 0, "min_on": 1.0, "max_invalid": 0, "drop_isolated": True}) == EdgeSupport(255, 255, 0.0, 1.0, 0, True)
    assert _key({"width": np.int64(3), "max_invalid": np.int32(7), "on": 0}) == EdgeSupport(3, 0, None, None, 7, False)
    assert _key({"min_mean": np.float32(0.25), "min_on": None, "max_invalid": None}).min_mean == 0.25
    k = _key({"max_invalid": 2})
    assert edge_support_key_of(k) is k
    # no condition: for attributes only
    assert edge_support_key(Config(EDGE_SUPPORT={"width": 3}), attributes_only=True) == EdgeSupport(3, 127, None, None, None, False)
    assert edge_support_key_of({"drop_isolated": True}, attributes_only=True).drop_isolated is True


BAD_KEYS = ("x", 3, True, [1], {"widht": 2, "min_on": 0.5}, {"width": 0, "min_on": 0.5}, {"width": 256, "min_on": 0.5}, {"width": 2.0, "min_on": 0.5},
            {"width": True, "min_on": 0.5}, {"on": -0.1, "min_on": 0.5}, {"on": 1.5, "min_on": 0.5}, {"on": True, "min_on": 0.5}, {"on": "0.5", "min_on": 0.5},
            {"on": float("nan"), "min_on": 0.5}, {"min_mean": -0.01}, {"min_mean": 1.01}, {"min_mean": True}, {"min_mean": "1"}, {"min_on": 2}, {"min_on": False},
            {"min_on": float("inf")}, {"max_invalid": -1}, {"max_invalid": 1.0}, {"max_invalid": True}, {"min_on": 0.5, "drop_isolated": 1},
            {"min_on": 0.5, "drop_isolated": "yes"}, {"width": 3}, {"drop_isolated": True}, {"on": 0.5})      # the last three state no condition


def test_every_refusal_is_a_value_error_before_the_model_is_touched(tmp_path, monkeypatch):
    import yaml
    for bad in BAD_KEYS:
        with pytest.raises(ValueError, match="EDGE_SUPPORT"):
            _key(bad)
        with pytest.raises(ValueError, match="EDGE_SUPPORT"):
            edge_support_key_of(bad)
    monkeypatch.chdir(tmp_path)

    def untouchable(*a, **k):
        raise AssertionError("the model was built")
    monkeypatch.setattr(cli, "_build_net", untouchable)
    cases = [(b, ()) for b in BAD_KEYS[:6]] + [(None, ("--edge-support-width", "0")), (None, ("--edge-support-width", "256", "--edge-min-on", "0.5")),
                                               (None, ("--edge-on", "1.5", "--edge-min-on", "0.5")), (None, ("--edge-min-mean", "-1")), (None, ("--edge-min-on", "2")),
                                               (None, ("--edge-max-invalid", "-1")), (None, ("--edge-support-width", "3")), (None, ("--drop-isolated-nodes",)),
                                               ({"min_on": 0.5, "drop_isolated": 1}, ("--edge-min-mean", "0.5"))]
    for n, (bad, argv) in enumerate(cases):
        with open(f"bad{n}.yaml", "w") as f:
            yaml.safe_dump(dict(HOST_CFG, DATASET="cityscale", **({} if bad is None else {"EDGE_SUPPORT": bad})), f)
        with pytest.raises(ValueError, match="EDGE_SUPPORT"):
            inf.main(["--config", f"bad{n}.yaml", "--checkpoint", "none", "--device", "cpu", "--output_dir", "bad", *argv, "--images", "a.png"])
    assert not os.path.exists("save")


def test_cli_flags_lay_over_the_key():
    assert edge_support_override(Config(), min_on=0.5) == {"min_on": 0.5}
    assert edge_support_override(Config(), width=3, on=0.25, min_mean=0.5, min_on=0.75, max_invalid=4, drop_isolated=True) == \
        {"width": 3, "on": 0.25, "min_mean": 0.5, "min_on": 0.75, "max_invalid": 4, "drop_isolated": True}
    keyed = Config(EDGE_SUPPORT={"width": 5, "min_mean": 0.3, "drop_isolated": True})
    assert edge_support_override(keyed) == keyed.EDGE_SUPPORT                                       # the config's fields stay
    assert edge_support_override(keyed, width=2, max_invalid=0) == dict(keyed.EDGE_SUPPORT, width=2, max_invalid=0)
    assert edge_support_override(Config(EDGE_SUPPORT={"width": 3}), min_on=0.5) == {"width": 3, "min_on": 0.5}      # an attributes-only key gains a condition
    assert edge_support_override(Config(), width=3, attributes_only=True) == {"width": 3}
    for kw in (dict(width=3), dict(width=0, min_on=0.5), dict(min_on=1.5), dict(max_invalid=-2), dict(on=2.0, min_on=0.5)):
        with pytest.raises(ValueError, match="EDGE_SUPPORT"):
            edge_support_override(Config(), **kw)
    with pytest.raises(ValueError, match="EDGE_SUPPORT"):
        edge_support_override(Config(EDGE_SUPPORT="x"), min_on=0.5)


# ---- 4. the GeoJSON export -----------------------------------------------------------------------------------------------------------------------------
def test_geojson_export_and_the_round_trip_through_the_aoi_frame():
    nodes = np.array([[0, 0], [7, 3], [120, 45], [-4, 60], [33, 2000]])
    edges = np.array([[0, 1], [1, 2], [3, 4], [2, 2]])
    doc = graph_geojson(nodes, edges)
    assert doc["type"] == "FeatureCollection" and len(doc["features"]) == 4
    for k, (f, (a, b)) in enumerate(zip(doc["features"], edges.tolist())):
        assert f["type"] == "Feature" and f["geometry"]["type"] == "LineString" and f["properties"] == {"edge": k}
        assert f["geometry"]["coordinates"] == [[nodes[a][1] + 0.5, nodes[a][0] + 0.5], [nodes[b][1] + 0.5, nodes[b][0] + 0.5]]      # [x, y] = [col + 1/2, row + 1/2]
    assert graph_geojson(nodes, edges, geotransform=[0, 1, 0, 0, 0, 1]) == doc                     # the identity
    attrs = edge_attrs(nodes, edges, [[5, 500, 2, 1], [0, 0, 0, 0], [4, 1020, 4, 0], [1, 9, 0, 0]])
    with_attrs = json.loads(json.dumps(graph_geojson(nodes, edges, attrs)))
    assert [f["properties"] for f in with_attrs["features"]] == [dict({"edge": k}, **a) for k, a in enumerate(attrs)]
    assert graph_geojson([], [])["features"] == [] and graph_geojson(nodes, [])["features"] == []
    # through a geotransform and back through aoi.py with the same one: every node lands on the centre of its own pixel
    for gt in ([440720.0, 0.5, 0.0, 3751320.0, 0.0, -0.5], [100.0, 0.3, 0.1, -50.0, -0.2, 0.4]):
        doc = json.loads(json.dumps(graph_geojson(nodes, edges, geotransform=gt)))
        ring = [f["geometry"]["coordinates"][0] for f in doc["features"][:3]] + [doc["features"][2]["geometry"]["coordinates"][1]]
        x, y = nodes[0][1] + 0.5, nodes[0][0] + 0.5
        assert ring[0] == [gt[0] + x * gt[1] + y * gt[2], gt[3] + x * gt[4] + y * gt[5]]
        back = aoi_key_of({"include": [[ring]], "geotransform": gt}).include[0][0]                  # (row, col) in 1 / 256 px
        assert [(r // 256, c // 256) for r, c in back] == [tuple(nodes[i].tolist()) for i in (0, 1, 3, 4)]
        assert all(abs(r % 256 - 128) <= 1 and abs(c % 256 - 128) <= 1 for r, c in back)
    for bad in ([1, 2, 3], [0, 1, 0, 0, 0, float("nan")], "x", [0, 1, 0, 0, 0, True]):
        with pytest.raises(ValueError, match="EDGE_SUPPORT"):
            graph_geojson(nodes, edges, geotransform=bad)
    with pytest.raises(ValueError, match="EDGE_SUPPORT"):
        graph_geojson(nodes, edges, attrs[:2])


# ---- 5. runs without and with the key --------------------------------------------------------------------------------------------------------------------
H, W, SEED = 300, 340, 43
CFG = dict(HOST_CFG, INFER_PATCHES_PER_EDGE=2)


def _files(root):
    return sorted(os.path.relpath(os.path.join(d, f), root) for d, _, fs in os.walk(root) for f in fs)


def test_cli_without_the_key_is_the_run_it_was_and_with_it_writes_the_filtered_graph(tmp_path, monkeypatch):
    from PIL import Image
    warnings.simplefilter("ignore")
    torch.set_num_threads(4)
    net = ek.SupportStandIn(dict(CFG), ("valid",))
    monkeypatch.chdir(tmp_path)
    img = rect_scene(H, W, SEED)
    Image.fromarray(img).save("a.png")
    valid = np.ones((H, W), np.uint8)
    valid[:, 250:] = 0
    np.save("va.npy", valid)

    # without the key: no call, and the files of a run in which the new code is out of the way, byte for byte
    plain = run_cli(cli, net, tmp_path, monkeypatch, "plain", CFG, ["a.png"], "--viz")
    assert not ek.support_calls(net) and es.apply(None, plain, net=None) == (plain, None)
    assert _files("save/plain") == ["config.yaml", "graph/a.p", "inference_time.txt", "mask/a_itsc.png", "mask/a_road.png", "viz/a.png"]
    with monkeypatch.context() as mp:
        def never(*a, **k):
            raise AssertionError("the new code ran")
        mp.setattr(cli, "edge_support_key", lambda *a, **k: None)
        mp.setattr(cli, "apply_edge_support", never)
        mp.setattr(cli, "write_geojson", never)
        run_cli(cli, net, tmp_path, mp, "bypassed", CFG, ["a.png"], "--viz")
    assert _files("save/bypassed") == _files("save/plain")
    for f in _files("save/plain"):
        if f != "inference_time.txt":
            assert open(f"save/plain/{f}", "rb").read() == open(f"save/bypassed/{f}", "rb").read(), f

    # with the key: the threshold is the median on_frac of the reference on this scene, so the reference decides
    res = inf.infer_one_img(net, img, Config(CFG), device="cpu", valid=valid)
    nodes, edges, _, road = res
    assert edges.shape[0] > 3
    frac = [a["on_frac"] for a in edge_attrs(nodes, edges, edge_support_ref(nodes, edges, road, 1, 127))]
    f_med = float(np.median(frac))
    key = edge_support_key(Config(CFG, EDGE_SUPPORT={"min_on": f_med, "drop_isolated": True}))
    (want_nodes, want_edges, _, want_road), want_attrs = es.apply_ref(key, res, valid)
    assert 0 < want_edges.shape[0] < edges.shape[0] and want_road is road                        # at least one edge dropped, at least one kept
    net.calls.clear()
    (got_nodes, got_edges, _, _), got_attrs = es.apply(key, res, valid=valid, net=net)           # apply on the stand-in is the host statement
    assert np.array_equal(got_nodes, want_nodes) and np.array_equal(got_edges, want_edges) and got_attrs == want_attrs
    assert ek.support_calls(net) == [("graph_edge_stats", (H, W), 1, 127, True)]
    net.calls.clear()
    gt = [10.0, 2.0, 0.0, 500.0, 0.0, -2.0]
    got = run_cli(cli, net, tmp_path, monkeypatch, "kept", CFG, ["a.png"], "--edge-min-on", repr(f_med), "--drop-isolated-nodes", "--viz", "--graph-geojson",
                  "--geotransform", *[str(g) for g in gt], "--valid-masks", "va.npy")["a"]
    assert got[3]["EDGE_SUPPORT"] == {"min_on": f_med, "drop_isolated": True} and len(ek.support_calls(net)) == 1
    assert _files("save/kept") == sorted(_files("save/plain") + ["graph_geojson/a.geojson"])
    assert np.array_equal(got[1], road)                                                          # the masks are what they were
    assert got[2] == convert_to_sat2graph_format(want_nodes, want_edges)                         # the pickle
    np.testing.assert_array_equal(np.array(Image.open("save/kept/viz/a.png")), composite_ref(graph_raster_ref(want_nodes, want_edges, (H, W), 4, "disc", 4), img))
    doc = json.load(open("save/kept/graph_geojson/a.geojson"))
    assert doc == json.loads(json.dumps(graph_geojson(want_nodes, want_edges, want_attrs, gt)))
    assert len(doc["features"]) == want_edges.shape[0] and all(f["properties"]["on_frac"] >= f_med for f in doc["features"])
    # --graph-geojson alone: the unfiltered graph, geometry only, in pixel coordinates; no call
    net.calls.clear()
    run_cli(cli, net, tmp_path, monkeypatch, "export", CFG, ["a.png"], "--graph-geojson", "--valid-masks", "va.npy")
    assert not ek.support_calls(net)
    assert json.load(open("save/export/graph_geojson/a.geojson")) == json.loads(json.dumps(graph_geojson(nodes, edges)))
    # a key without a condition and --graph-geojson: attributes, nothing filtered
    run_cli(cli, net, tmp_path, monkeypatch, "attrs", CFG, ["a.png"], "--graph-geojson", "--edge-support-width", "3", "--geotransform", *[str(g) for g in gt],
            "--valid-masks", "va.npy")
    want = graph_geojson(nodes, edges, edge_attrs(nodes, edges, edge_support_ref(nodes, edges, road, 3, 127, valid)), gt)
    assert json.load(open("save/attrs/graph_geojson/a.geojson")) == json.loads(json.dumps(want))
    assert pickle.load(open("save/attrs/graph/a.p", "rb")) == pickle.load(open("save/export/graph/a.p", "rb"))


# ---- 6. the kernel's own code, on the CPU ----------------------------------------------------------------------------------------------------------------
def test_kernel_addressing_on_the_cpu(tmp_path):
    """tests/edge_support_check.cpp runs every item of whole launches through the kernel's own per-item code
    (csrc/edge_support_piece.hpp) as a stand-alone host program built with the address and undefined-behaviour sanitizers, against a scalar
    loop over ALL pixels in 128-bit integers: 1 x 1, 1 x 16384 and 16384 x 2 images with maximum-span edges, edges with both ends outside,
    coordinates at +-2^28, valid present and absent, every block of its exact size.  A byte read or written outside them ends it."""
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    cxx = next((c for c in (os.path.join(rocm, "llvm", "bin", "clang++"), os.path.join(rocm, "lib", "llvm", "bin", "clang++")) if os.path.exists(c)), None)
    if cxx is None:
        pytest.skip("no ROCm clang++")
    exe = str(tmp_path / "edge_support_check")
    csrc = os.path.join(ROOT, "sam_road_amd", "csrc")
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", csrc,
                        os.path.join(ROOT, "tests", "edge_support_check.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    assert "edge support OK" in r.stdout


# ---- 7. the cross-compile ----------------------------------------------------------------------------------------------------------------------------------
def test_kernel_compiles_for_gfx950_without_a_gpu():
    hipcc = next((c for c in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", shutil.which("hipcc")) if c and os.path.exists(c)), None)
    if hipcc is None:
        pytest.skip("hipcc not found")
    from sam_road_amd import build
    assert "edge_support.hip" in build.SOURCES
    r = subprocess.run([hipcc, *build.FLAGS, "-S", "--cuda-device-only", os.path.join(build.CSRC, "edge_support.hip"), "-o", "-"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    names = re.findall(r"^(_Z\w*graph_edge_stats_kernel\w*):", r.stdout, re.M)
    assert len(set(names)) == 2, f"graph_edge_stats_kernel (16 lanes and 64 lanes per edge) is not in the code object: {names}"
    for name in names:
        meta = r.stdout[r.stdout.index(".amdhsa_kernel " + name):]
        meta = meta[:meta.index(".end_amdhsa_kernel")]
        assert int(re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", meta).group(1)) == 0, name      # no scratch
        assert int(re.search(r"\.amdhsa_group_segment_fixed_size (\d+)", meta).group(1)) == 0, name        # no LDS
        assert int(re.search(r"\.amdhsa_uses_dynamic_stack (\d+)", meta).group(1)) == 0, name
        body = r.stdout[r.stdout.index(name + ":"):r.stdout.index(".amdhsa_kernel " + name)]
        assert ".amdhsa_kernel" not in body and "s_endpgm" in body, name                            # this kernel's own code
        assert "atomic" not in body and "global_store_dwordx4" in body, name                        # the edge's 16 bytes, one store


# ---- 8. C ABI surface ----------------------------------------------------------------------------------------------------------------------------------------
def test_abi_has_the_entry_and_stays_11():
    header, lib = assert_abi_11((("srh_graph_edge_stats", 15),))
    assert "EDGE_SUPPORT" in header
    out = torch.zeros(8, dtype=torch.int32)
    assert lib.srh_graph_edge_stats(None, None, None, 0, None, None, 0, 2, 2, 1, None, None, 0, out.data_ptr(), None) == -1      # refused without a context
    assert not out.any()
