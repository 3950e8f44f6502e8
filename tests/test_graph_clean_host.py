"""GRAPH_CLEAN without a GPU: the rule against an independent statement with networkx (components from networkx, chains
from the line graph over the degree-2 nodes), hand-built cases with their answers literally, the key and the thresholds through Fraction,
the kept graph and its renumbering, the polylines and their GeoJSON, the CLI on the CPU stand-in, the kernels' own per-item code under the
host sanitizers, the cross-compile and the ABI."""
import json
import math
import os
import pickle
import shutil
import subprocess
import warnings
from fractions import Fraction

import networkx as nx
import numpy as np
import pytest
import torch

from sam_road_amd import Config
from sam_road_amd import cli
from sam_road_amd import graph_clean as gc
from sam_road_amd import inferencer as inf
from sam_road_amd.edge_support import filter_graph, graph_geojson
from sam_road_amd.formats import convert_to_sat2graph_format
from sam_road_amd.graph_clean import (GraphClean, apply_ref, chains, clean_attrs, graph_clean_key, graph_clean_key_of, graph_clean_override,
                                      graph_clean_ref, kept_graph, polylines_geojson, threshold_q, thresholds_q)

import graph_clean_kit as gk
from scene_kit import HOST_CFG, assert_abi_11, rect_scene, run_cli

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- 1. the rule against networkx ------------------------------------------------------------------------------------------------------------------
def nx_clean(nodes, edges, spur_q, comp_q, rounds):
    """The rule stated with networkx.MultiGraph: components by nx.connected_components, chains as the components of the graph whose
    vertices are the live edges and whose links join the two edge-ends of every node of degree 2."""
    nodes, edges = np.asarray(nodes, np.int64), np.asarray(edges, np.int64)
    E = edges.shape[0]
    d = nodes[edges[:, 1]] - nodes[edges[:, 0]]
    len_q = [math.isqrt(256 * int(r * r + c * c)) for r, c in d]
    live = set(range(E))
    state = np.zeros(E, np.uint8)

    def analyse():
        g = nx.MultiGraph()
        g.add_nodes_from(range(nodes.shape[0]))
        for k in sorted(live):
            g.add_edge(int(edges[k, 0]), int(edges[k, 1]), key=k)
        deg = dict(g.degree())                                           # a self-loop counts 2
        comp = {}
        for cc in nx.connected_components(g):
            ks = [k for _, _, k in g.edges(cc, keys=True)]
            for k in ks:
                comp[k] = (min(cc), sum(len_q[j] for j in set(ks)))
        line = nx.Graph()
        line.add_nodes_from(live)
        for v in g.nodes:
            if deg[v] == 2:
                ends = [k for a, b, k in g.edges(v, keys=True) for _ in range(2 if a == b else 1)]
                assert len(ends) == 2
                line.add_edge(ends[0], ends[1])
        chain = {}
        for cc in nx.connected_components(line):
            ends = [deg[int(v)] for k in cc for v in edges[k] if deg[int(v)] != 2]
            assert len(ends) in (0, 2)
            for k in cc:
                chain[k] = (min(cc), sum(len_q[j] for j in cc), sum(x == 1 for x in ends), sum(x >= 3 for x in ends))
        return chain, comp

    for r in range(1, rounds + 1):
        chain, comp = analyse()
        for k in sorted(live):
            _, cl, n_leaf, n_junc = chain[k]
            spur = spur_q > 0 and n_leaf == 1 and n_junc == 1 and cl < spur_q
            small = comp_q > 0 and comp[k][1] < comp_q
            if spur or small:
                state[k] = 4 * r + spur + 2 * small
                live.discard(k)
    chain, comp = analyse()
    out = np.tile(np.array(gk.DEAD, np.int32), (E, 1))
    for k in live:
        out[k] = (chain[k][0], comp[k][0], min(chain[k][1], gk.CLAMP), min(comp[k][1], gk.CLAMP))
    return state, out


@pytest.mark.parametrize("block", range(8))
def test_ref_equals_the_networkx_statement(block):
    """30 random multigraphs per block (240 in all) of at most 40 nodes and 60 edges with self-loops and parallel edges, 1 to 3 rounds;
    the thresholds come from the graph's own dead-end and component lengths (graph_clean_kit.draw_thresholds), so a few per cent of the
    edges drop."""
    rng = np.random.default_rng(900 + block)
    dropped = total = multi = 0
    for _ in range(30):
        nodes, edges = gk.random_multigraph(rng)
        E = edges.shape[0]
        spur_q, comp_q = gk.draw_thresholds(rng, nodes, edges)
        rounds = int(rng.integers(1, 4))
        want = nx_clean(nodes, edges, spur_q, comp_q, rounds)
        got = graph_clean_ref(nodes, edges, spur_q, comp_q, rounds)
        assert got[0].dtype == np.uint8 and got[1].dtype == np.int32 and got[1].shape == (E, 4)
        np.testing.assert_array_equal(got[0], want[0])
        np.testing.assert_array_equal(got[1], want[1])
        dropped += int((got[0] != 0).sum())
        total += E
        multi += int((edges[:, 0] == edges[:, 1]).sum())
    assert 0.01 * total < dropped < 0.15 * total and multi > 0, (dropped, total)


# ---- 2. exact answers ----------------------------------------------------------------------------------------------------------------------------------
CASES = gk.hand_cases()


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_hand_built_cases(case):
    key = graph_clean_key_of(case["key"])
    state, out = graph_clean_ref(case["nodes"], case["edges"], *thresholds_q(key), key.rounds)
    np.testing.assert_array_equal(state, case["state"])
    np.testing.assert_array_equal(out, case["out"])


def test_the_long_chain_passes_2_31_and_is_decided_in_64_bits():
    case = CASES[-1]
    len_q = gc.edge_len_q(case["nodes"], case["edges"])
    assert int(len_q.max()) == gc.MAX_LEN_Q == 370704 and int(len_q[:6000].sum()) == 2224224000 > 2 ** 31
    assert int(np.int32(np.uint32(2224224000 % 2 ** 32))) < 0                                    # what a 32-bit sum would have compared
    assert thresholds_q(graph_clean_key_of(case["key"])) == (2 ** 24, 2 ** 24)


# ---- 3. the key --------------------------------------------------------------------------------------------------------------------------------------
def _key(v):
    return graph_clean_key(Config(GRAPH_CLEAN=v))


def test_key_every_accepted_form():
    assert _key(None) is None and _key({}) is None and graph_clean_key(Config()) is None
    assert _key({"min_spur": 12}) == GraphClean(12, None, 1, False)
    assert _key({"min_component": 30.5, "rounds": 8, "drop_isolated": True}) == GraphClean(None, 30.5, 8, True)
    assert _key({"rounds": 2}) == GraphClean(None, None, 2, False) and not gc.filters(_key({"rounds": 2}))      # attributes and polylines only
    assert _key({"drop_isolated": True}) == GraphClean(None, None, 1, True)
    assert gc.filters(_key({"min_spur": 2 ** 20})) and _key({"min_spur": np.float32(2.5)}).min_spur == 2.5
    k = _key({"min_spur": 3})
    assert graph_clean_key_of(k) is k


BAD_KEYS = ("x", 3, [1], {"spur": 3}, {"min_spur": 0}, {"min_spur": -1}, {"min_spur": 2 ** 20 + 1}, {"min_spur": True}, {"min_spur": "3"},
            {"min_spur": float("nan")}, {"min_component": float("inf")}, {"min_component": 0.0}, {"rounds": 0}, {"rounds": 9}, {"rounds": 1.0},
            {"rounds": True}, {"min_spur": 3, "drop_isolated": 1}, {"min_spur": 3, "drop_isolated": "yes"})


def test_every_refusal_is_a_value_error_before_the_model_is_touched(tmp_path, monkeypatch):
    import yaml
    for bad in BAD_KEYS:
        with pytest.raises(ValueError, match="GRAPH_CLEAN"):
            _key(bad)
    monkeypatch.chdir(tmp_path)

    def untouchable(*a, **k):
        raise AssertionError("the model was built")
    monkeypatch.setattr(cli, "_build_net", untouchable)
    cases = [(b, ()) for b in BAD_KEYS[:6]] + [(None, ("--graph-min-spur", "0")), (None, ("--graph-min-component", "-2")), (None, ("--graph-clean-rounds", "9")),
                                               (None, ("--graph-min-spur", "2000000")), ({"rounds": 0}, ("--graph-polylines",))]
    for n, (bad, argv) in enumerate(cases):
        with open(f"bad{n}.yaml", "w") as f:
            yaml.safe_dump(dict(HOST_CFG, DATASET="cityscale", **({} if bad is None else {"GRAPH_CLEAN": bad})), f)
        with pytest.raises(ValueError, match="GRAPH_CLEAN"):
            inf.main(["--config", f"bad{n}.yaml", "--checkpoint", "none", "--device", "cpu", "--output_dir", "bad", *argv, "--images", "a.png"])
    assert not os.path.exists("save")


def test_cli_flags_lay_over_the_key():
    assert graph_clean_override(Config(), min_spur=12.5) == {"min_spur": 12.5}
    assert graph_clean_override(Config(), min_spur=4, min_component=50, rounds=3, drop_isolated=True) == \
        {"min_spur": 4, "min_component": 50, "rounds": 3, "drop_isolated": True}
    keyed = Config(GRAPH_CLEAN={"min_spur": 7, "rounds": 2})
    assert graph_clean_override(keyed) == keyed.GRAPH_CLEAN and graph_clean_override(keyed, enable=True) == keyed.GRAPH_CLEAN
    assert graph_clean_override(keyed, min_component=9, rounds=1) == {"min_spur": 7, "rounds": 1, "min_component": 9}
    assert graph_clean_override(Config()) == {} and graph_clean_override(Config(), drop_isolated=True) == {}      # the shared flag alone turns nothing on
    assert graph_clean_override(Config(), enable=True) == {"rounds": 1}                             # --graph-polylines alone: attributes only
    assert graph_clean_override(Config(), enable=True, drop_isolated=True) == {"drop_isolated": True}
    for kw in (dict(min_spur=0), dict(min_component=-1), dict(rounds=9), dict(min_spur=2.0 ** 21)):
        with pytest.raises(ValueError, match="GRAPH_CLEAN"):
            graph_clean_override(Config(), **kw)
    with pytest.raises(ValueError, match="GRAPH_CLEAN"):
        graph_clean_override(Config(GRAPH_CLEAN="x"), min_spur=3)


def test_thresholds_are_rounded_up_exactly():
    assert threshold_q(None) == 0 and threshold_q(10) == 160 and threshold_q(10.0) == 160 and threshold_q(10.0625) == 161
    assert threshold_q(9.9375) == 159 and threshold_q(2 ** 20) == 2 ** 24
    assert threshold_q(0.1) == 2 and threshold_q(1e-9) == 1 and threshold_q(5e-324) == 1            # any stated threshold is at least 1
    for v in (0.3, 12.01, 1 / 3, 7.999999999999999, 65536.00000000001):
        q = threshold_q(v)
        assert isinstance(q, int) and Fraction(q - 1, 16) < Fraction(v) <= Fraction(q, 16)       # x < 16 v  <=>  x < q for every integer x
    below = np.nextafter(10.0, 0)
    assert threshold_q(below) == 160 and threshold_q(np.nextafter(10.0, 11)) == 161
    assert thresholds_q(GraphClean(10.0625, None, 1, False)) == (161, 0)
    for bad in ((-1, 0, 1), (0, -1, 1), (1.5, 0, 1), (0, 0, 0), (0, 0, 9)):
        with pytest.raises(ValueError, match="GRAPH_CLEAN"):
            graph_clean_ref([[0, 0], [0, 1]], [[0, 1]], *bad)


# ---- 4. the kept graph, the attributes, the polylines ----------------------------------------------------------------------------------------------------
def test_kept_graph_renumbers_chains_and_components():
    # an isolated node 0, a dead pair 1 - 2 (small), then the Y of the kit shifted by three nodes
    y = next(c for c in CASES if c["name"] == "Y, two rounds")
    nodes = np.concatenate([[[50, 50], [60, 60], [60, 61]], y["nodes"]])
    edges = np.concatenate([[[1, 2]], y["edges"] + 3])
    state, out = graph_clean_ref(nodes, edges, 192, 100, 2)
    np.testing.assert_array_equal(state, [6, 5, 5, 9, 0, 0])
    np.testing.assert_array_equal(out[4:], [[4, 6, 3200, 3200]] * 2)
    n1, e1, keep, table = kept_graph(nodes, edges, state, out)
    assert np.array_equal(n1, nodes) and np.array_equal(e1, edges[4:]) and keep.tolist() == [False] * 4 + [True] * 2
    np.testing.assert_array_equal(table, [[0, 6, 3200, 3200]] * 2)                                  # chain 4 -> kept edge 0; the nodes stay
    n2, e2, keep2, table2 = kept_graph(nodes, edges, state, out, drop_isolated=True)
    want_n, want_e, _ = filter_graph(nodes, edges, keep, True)
    assert np.array_equal(n2, want_n) and np.array_equal(e2, want_e) and np.array_equal(keep2, keep)
    assert n2.tolist() == nodes[[6, 7, 8]].tolist() and e2.tolist() == [[0, 1], [0, 2]]
    np.testing.assert_array_equal(table2, [[0, 0, 3200, 3200]] * 2)                                 # node 6 -> kept node 0
    assert clean_attrs(table2) == [dict(chain=0, chain_length_px=200.0, component=0, component_length_px=200.0)] * 2
    assert np.array_equal(gc.table_of(clean_attrs(table2)), table2)
    # every chain id of a kept graph is the smallest kept edge of its chain, every component id its smallest kept node
    rng = np.random.default_rng(5)
    for _ in range(20):
        nodes, edges = gk.random_multigraph(rng)
        state, out = graph_clean_ref(nodes, edges, 300, 200, 2)
        for drop in (False, True):
            n3, e3, _, t3 = kept_graph(nodes, edges, state, out, drop)
            s3, o3 = graph_clean_ref(n3, e3)                                                        # the kept graph analysed on its own
            assert not s3.any()
            np.testing.assert_array_equal(o3, t3)
    empty = kept_graph(nodes, np.zeros((0, 2), np.int32), np.zeros(0, np.uint8), np.zeros((0, 4), np.int32))
    assert empty[1].shape == (0, 2) and empty[3].shape == (0, 4) and clean_attrs(empty[3]) == []


def _walk_ok(nodes, edges, ids):
    got = chains(nodes, edges, ids)
    used = []
    deg = np.bincount(np.asarray(edges).reshape(-1), minlength=len(nodes))
    by_pair = {}
    for k, (a, b) in enumerate(np.asarray(edges).tolist()):
        by_pair.setdefault((min(a, b), max(a, b)), []).append(k)
    assert [c for c, _ in got] == sorted(set(np.asarray(ids).tolist()))
    for c, seq in got:
        members = set(np.flatnonzero(np.asarray(ids) == c).tolist())
        assert len(seq) == len(members) + 1
        mine = []
        for a, b in zip(seq[:-1], seq[1:]):                              # every step is an edge of the chain not used before
            free = [k for k in by_pair[(min(a, b), max(a, b))] if k in members and k not in mine]
            assert free, (c, seq)
            mine.append(free[0])
        assert set(mine) == members
        used += mine
        inner, ends = seq[1:-1], (seq[0], seq[-1])
        assert all(deg[v] == 2 for v in inner)
        if deg[ends[0]] == 2 or deg[ends[1]] == 2:                       # a ring: closed, from its smallest node, along the smaller edge
            assert ends[0] == ends[1] == min(seq) and all(deg[v] == 2 for v in seq)
            first = sorted(k for k in members if ends[0] in np.asarray(edges)[k])[0]
            assert set(np.asarray(edges)[first].tolist()) == {seq[0], seq[1]}
        else:
            assert ends[0] <= ends[1]
    assert sorted(used) == list(range(len(edges)))                       # every edge once, in exactly one chain
    return got


def test_chains_fixed_cases_literally():
    by = {c["name"]: c for c in CASES}

    def run(name):
        c = by[name]
        state, out = graph_clean_ref(c["nodes"], c["edges"], *thresholds_q(graph_clean_key_of(c["key"])), c["key"]["rounds"])
        n, e, _, t = kept_graph(c["nodes"], c["edges"], state, out)
        return _walk_ok(n, e, t[:, 0]), (n, e, t)

    assert run("single edge")[0] == [(0, [0, 1])]
    assert run("self-loop alone")[0] == [(0, [0, 0])]
    assert run("self-loop on a junction, s = 10")[0] == [(0, [0, 0]), (1, [0, 1])]
    assert run("two parallel edges")[0] == [(0, [0, 1, 0])]
    assert run("path of 3")[0] == [(0, [0, 1, 2, 3])]
    assert run("ring")[0] == [(0, [0, 1, 2, 3, 0])]                       # node 0's incident edges are 0 (to node 1) and 3: along edge 0
    assert run("lollipop, tail of exactly s")[0] == [(0, [3, 2, 1, 0, 3]), (4, [3, 4])]      # both ends at node 3: along edge 2, not edge 3
    assert run("lollipop, tail below s")[0] == [(0, [0, 1, 2, 3, 0])]     # the tail gone, the loop is a ring
    assert run("star, s = 10")[0] == [(0, [1, 0, 4])]                     # arms A and C through the centre, from the smaller end
    assert run("star, s = 10 - 1/16")[0] == [(0, [0, 1]), (1, [0, 2, 3]), (3, [0, 4])]
    assert run("Y, two rounds")[0] == [(0, [4, 3, 5])]
    # a path given against its orientation and out of order still starts at its smaller end
    assert chains([[0, 0], [0, 1], [0, 2], [0, 3]], [[2, 3], [1, 0], [2, 1]], [0, 0, 0]) == [(0, [0, 1, 2, 3])]
    assert chains([[0, 0]], [], []) == [] and chains([], [], []) == []
    five = [[0, 0], [0, 1], [0, 2], [0, 3], [5, 5]]
    for bad_edges, bad_ids in (([[0, 1], [1, 2], [2, 3]], [0, 0, 1]),     # a chain cut in two
                               ([[0, 1], [1, 2], [1, 4]], [0, 0, 0]),     # three chains at a junction given as one
                               ([[0, 1], [1, 2], [2, 3]], [0, 0])):       # one id short
        with pytest.raises(ValueError, match="GRAPH_CLEAN"):
            chains(five, bad_edges, bad_ids)


def test_chains_on_random_multigraphs_use_every_edge_once():
    rng = np.random.default_rng(11)
    for _ in range(60):
        nodes, edges = gk.random_multigraph(rng)
        state, out = graph_clean_ref(nodes, edges, 200, 0, 1)
        n, e, _, t = kept_graph(nodes, edges, state, out, drop_isolated=bool(rng.integers(0, 2)))
        _walk_ok(n, e, t[:, 0])
    nodes, edges = gk.jittered_grid(rng, side=30)
    state, out = graph_clean_ref(nodes, edges, 160, 800, 2)
    n, e, _, t = kept_graph(nodes, edges, state, out)
    assert 0 < e.shape[0] < edges.shape[0] and len(_walk_ok(n, e, t[:, 0])) < e.shape[0]


def test_polylines_geojson_with_and_without_a_geotransform():
    c = next(c for c in CASES if c["name"] == "star, s = 10 - 1/16")
    state, out = graph_clean_ref(c["nodes"], c["edges"], 159, 0, 1)
    n, e, _, t = kept_graph(c["nodes"], c["edges"], state, out)
    doc = polylines_geojson(n, e, t)
    assert doc["type"] == "FeatureCollection" and [f["geometry"]["type"] for f in doc["features"]] == ["LineString"] * 3
    xy = lambda i: [n[i][1] + 0.5, n[i][0] + 0.5]                        # [x, y] = [col + 1/2, row + 1/2], graph_geojson's
    assert [f["geometry"]["coordinates"] for f in doc["features"]] == [[xy(0), xy(1)], [xy(0), xy(2), xy(3)], [xy(0), xy(4)]]
    assert [f["properties"] for f in doc["features"]] == [
        dict(chain=0, n_edges=1, length_px=10.0, component=0, component_length_px=1119 / 16, deg_start=3, deg_end=1),
        dict(chain=1, n_edges=2, length_px=159 / 16, component=0, component_length_px=1119 / 16, deg_start=3, deg_end=1),
        dict(chain=3, n_edges=1, length_px=50.0, component=0, component_length_px=1119 / 16, deg_start=3, deg_end=1)]
    assert polylines_geojson(n, e, t, [0, 1, 0, 0, 0, 1]) == doc
    gt = [440720.0, 0.5, 0.0, 3751320.0, 0.0, -0.5]
    moved = json.loads(json.dumps(polylines_geojson(n, e, t, gt)))
    edge_doc = graph_geojson(n, e, geotransform=gt)                        # the same points as the per-edge export
    assert moved["features"][1]["geometry"]["coordinates"][:2] == edge_doc["features"][1]["geometry"]["coordinates"]
    assert moved["features"][1]["geometry"]["coordinates"][1:] == edge_doc["features"][2]["geometry"]["coordinates"]
    assert [f["properties"] for f in moved["features"]] == [f["properties"] for f in doc["features"]]
    assert polylines_geojson([], [], np.zeros((0, 4)))["features"] == []
    with pytest.raises(ValueError, match="EDGE_SUPPORT"):
        polylines_geojson(n, e, t, [1, 2, 3])
    with pytest.raises(ValueError, match="GRAPH_CLEAN"):
        polylines_geojson(n, e, t[:2])


# ---- 5. runs without and with the key --------------------------------------------------------------------------------------------------------------------
H, W, SEED = 300, 340, 43
CFG = dict(HOST_CFG, INFER_PATCHES_PER_EDGE=2)


def _files(root):
    return sorted(os.path.relpath(os.path.join(d, f), root) for d, _, fs in os.walk(root) for f in fs)


def test_cli_without_the_key_is_the_run_it_was_and_with_it_writes_the_cleaned_graph(tmp_path, monkeypatch):
    from PIL import Image
    warnings.simplefilter("ignore")
    torch.set_num_threads(4)
    net = gk.CleanStandIn(dict(CFG), ("valid",))
    monkeypatch.chdir(tmp_path)
    img = rect_scene(H, W, SEED)
    Image.fromarray(img).save("a.png")

    # without the key: no call, and the files of a run in which the new code is out of the way, byte for byte
    plain = run_cli(cli, net, tmp_path, monkeypatch, "plain", CFG, ["a.png"], "--viz", "--graph-geojson")
    assert not gk.clean_calls(net) and gc.apply(None, plain, net=None) == (plain, None) and gc.apply(None, plain, return_keep=True) == (plain, None, None)
    plain_files = ["config.yaml", "graph/a.p", "graph_geojson/a.geojson", "inference_time.txt", "mask/a_itsc.png", "mask/a_road.png", "viz/a.png"]
    assert _files("save/plain") == plain_files and "GRAPH_CLEAN" not in plain["a"][3]
    with monkeypatch.context() as mp:
        def never(*a, **k):
            raise AssertionError("the new code ran")
        mp.setattr(cli, "graph_clean_key", lambda *a, **k: None)
        mp.setattr(cli, "graph_clean_override", never)
        mp.setattr(cli, "apply_graph_clean", lambda key, res, **k: (res, None, None) if key is None else never())
        mp.setattr(cli, "write_polylines", never)
        mp.setattr(cli, "clean_table_of", never)
        run_cli(cli, net, tmp_path, mp, "bypassed", CFG, ["a.png"], "--viz", "--graph-geojson")
    assert _files("save/bypassed") == plain_files
    for f in plain_files:
        if f != "inference_time.txt":
            assert open(f"save/plain/{f}", "rb").read() == open(f"save/bypassed/{f}", "rb").read(), f

    # with the key: thresholds from the graph's own lengths, so that the reference decides and something goes
    res = inf.infer_one_img(net, img, Config(CFG), device="cpu")
    nodes, edges, _, road = res
    assert edges.shape[0] > 3
    n32, e32 = gc.check_graph(nodes, edges)
    _, _, _, chain_len, comp_len, n_leaf, n_junc = gc.analyse(n32.shape[0], e32, gc.edge_len_q(n32, e32), np.ones(e32.shape[0], bool))
    dead_ends = chain_len[(n_leaf == 1) & (n_junc == 1)]
    s_px = float(np.median(dead_ends)) / 16 if dead_ends.size else 5.0
    c_px = float(np.median(comp_len)) / 16
    key = graph_clean_key(Config(CFG, GRAPH_CLEAN={"min_spur": s_px, "min_component": c_px, "rounds": 2, "drop_isolated": True}))
    (want_nodes, want_edges, _, want_road), want_attrs = apply_ref(key, res)
    assert 0 < want_edges.shape[0] < edges.shape[0] and want_road is road                        # at least one edge dropped, at least one kept
    net.calls.clear()
    (got_nodes, got_edges, _, _), got_attrs, keep = gc.apply(key, res, net=net, return_keep=True)      # apply on the stand-in is the host statement
    assert np.array_equal(got_nodes, want_nodes) and np.array_equal(got_edges, want_edges) and got_attrs == want_attrs
    assert keep.shape == (edges.shape[0],) and int(keep.sum()) == want_edges.shape[0]
    assert gk.clean_calls(net) == [("graph_clean", edges.shape[0], *thresholds_q(key), 2)]
    net.calls.clear()
    gt = [10.0, 2.0, 0.0, 500.0, 0.0, -2.0]
    got = run_cli(cli, net, tmp_path, monkeypatch, "kept", CFG, ["a.png"], "--graph-min-spur", repr(s_px), "--graph-min-component", repr(c_px),
                  "--graph-clean-rounds", "2", "--drop-isolated-nodes", "--viz", "--graph-geojson", "--graph-polylines", "--geotransform", *[str(g) for g in gt])["a"]
    assert got[3]["GRAPH_CLEAN"] == {"min_spur": s_px, "min_component": c_px, "rounds": 2, "drop_isolated": True} and len(gk.clean_calls(net)) == 1
    assert "EDGE_SUPPORT" not in got[3]                                                          # the shared flag reached this key alone
    assert _files("save/kept") == sorted(plain_files + ["graph_polylines/a.geojson"])
    assert np.array_equal(got[1], road)                                                          # the masks are what they were
    assert got[2] == convert_to_sat2graph_format(want_nodes, want_edges)                         # the pickle holds apply_ref's graph
    doc = json.load(open("save/kept/graph_geojson/a.geojson"))
    assert doc == json.loads(json.dumps(graph_geojson(want_nodes, want_edges, want_attrs, gt)))  # per-edge features with the four attributes
    assert set(doc["features"][0]["properties"]) == {"edge", "chain", "chain_length_px", "component", "component_length_px"}
    lines = json.load(open("save/kept/graph_polylines/a.geojson"))
    assert lines == json.loads(json.dumps(polylines_geojson(want_nodes, want_edges, gc.table_of(want_attrs), gt)))
    assert 0 < len(lines["features"]) <= want_edges.shape[0] and sum(f["properties"]["n_edges"] for f in lines["features"]) == want_edges.shape[0]
    # --graph-polylines alone: an attributes-only key, nothing filtered, the pickle of the plain run
    net.calls.clear()
    only = run_cli(cli, net, tmp_path, monkeypatch, "lines", CFG, ["a.png"], "--graph-polylines")["a"]
    assert only[3]["GRAPH_CLEAN"] == {"rounds": 1} and gk.clean_calls(net) == [("graph_clean", edges.shape[0], 0, 0, 1)]
    assert open("save/lines/graph/a.p", "rb").read() == open("save/plain/graph/a.p", "rb").read()
    state, out = graph_clean_ref(nodes, edges)
    n0, e0, _, t0 = kept_graph(nodes, edges, state, out)
    assert json.load(open("save/lines/graph_polylines/a.geojson")) == json.loads(json.dumps(polylines_geojson(n0, e0, t0)))
    # behind EDGE_SUPPORT and ROAD_WIDTH: the attributes of all three on the edges all three keep
    from sam_road_amd import edge_support as es, road_width as rw
    chained = run_cli(cli, net, tmp_path, monkeypatch, "chained", CFG, ["a.png"], "--edge-min-on", "0.3", "--road-width", "--graph-min-spur", repr(s_px),
                      "--graph-geojson")["a"]
    k1 = es.edge_support_key(Config(CFG, EDGE_SUPPORT={"min_on": 0.3}))
    k2 = rw.road_width_key(Config(CFG, ROAD_WIDTH={"max_radius": 32}))
    k3 = graph_clean_key(Config(GRAPH_CLEAN={"min_spur": s_px}))
    r1, a1 = es.apply_ref(k1, res)
    r2, a2 = rw.apply_ref(k2, r1)
    r3, a3, keep3 = apply_ref(k3, r2, return_keep=True)
    assert chained[2] == convert_to_sat2graph_format(r3[0], r3[1])
    merged = [dict(a1[k], **a2[k], **c) for k, c in zip(np.flatnonzero(keep3).tolist(), a3)]
    assert json.load(open("save/chained/graph_geojson/a.geojson")) == json.loads(json.dumps(graph_geojson(r3[0], r3[1], merged)))


# ---- 6. the kernels' own code, on the CPU ----------------------------------------------------------------------------------------------------------------
def test_kernel_items_on_the_cpu(tmp_path):
    """tests/graph_clean_check.cpp runs every item of whole calls through the kernels' own per-item code (csrc/graph_clean_piece.hpp) as a
    stand-alone host program built with the address and undefined-behaviour sanitizers, in four schedules (one with stale parent loads),
    against a breadth-first restatement: N and E at 1, 2, 63 .. 65, 255 .. 257 and 1000, 1 to 8 rounds, the 6000-edge chain past 2^31,
    coordinates at +-2^28; workspace and outputs end at their heap block's end behind guard bytes.  A byte outside them ends it."""
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    cxx = next((c for c in (os.path.join(rocm, "llvm", "bin", "clang++"), os.path.join(rocm, "lib", "llvm", "bin", "clang++")) if os.path.exists(c)), None)
    if cxx is None:
        pytest.skip("no ROCm clang++")
    exe = str(tmp_path / "graph_clean_check")
    csrc = os.path.join(ROOT, "sam_road_amd", "csrc")
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", csrc,
                        os.path.join(ROOT, "tests", "graph_clean_check.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    assert "graph clean OK" in r.stdout


# ---- 7. the cross-compile ----------------------------------------------------------------------------------------------------------------------------------
def test_kernels_compile_for_gfx950_without_a_gpu():
    import re
    hipcc = next((c for c in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", shutil.which("hipcc")) if c and os.path.exists(c)), None)
    if hipcc is None:
        pytest.skip("hipcc not found")
    from sam_road_amd import build
    assert "graph_clean.hip" in build.SOURCES
    r = subprocess.run([hipcc, *build.FLAGS, "-S", "--cuda-device-only", os.path.join(build.CSRC, "graph_clean.hip"), "-o", "-"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    for step in ("init", "edges", "chains", "sums", "decide"):
        names = re.findall(r"^(_Z\w*graph_clean_%s_kernel\w*):" % step, r.stdout, re.M)
        assert len(names) == 1, (step, names)
        meta = r.stdout[r.stdout.index(".amdhsa_kernel " + names[0]):]
        meta = meta[:meta.index(".end_amdhsa_kernel")]
        assert int(re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", meta).group(1)) == 0, step      # no scratch
        assert int(re.search(r"\.amdhsa_group_segment_fixed_size (\d+)", meta).group(1)) == 0, step        # no LDS
        assert int(re.search(r"\.amdhsa_uses_dynamic_stack (\d+)", meta).group(1)) == 0, step


# ---- 8. C ABI surface ----------------------------------------------------------------------------------------------------------------------------------------
def test_abi_has_the_entry_and_stays_11():
    header, lib = assert_abi_11((("srh_graph_clean", 13),))
    assert "GRAPH_CLEAN" in header
    out = torch.zeros(8, dtype=torch.int32)
    state = torch.zeros(2, dtype=torch.uint8)
    assert lib.srh_graph_clean(None, None, None, 0, None, None, 0, 0, 0, 1, state.data_ptr(), out.data_ptr(), None) == -1      # refused without a context
    assert not out.any() and not state.any()
