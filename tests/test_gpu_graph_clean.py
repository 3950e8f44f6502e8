"""GRAPH_CLEAN (spur and small-component pruning, chains and components of the road graph) on the HIP path.  Run on an
MI355X: pytest -m gpu.

state and out of the device must equal graph_clean_ref at every size at which the kernels' loops and the two forests can go wrong; the
kept graph, the attributes and the polylines work on those integers on the host.  There is no tolerance anywhere."""
import ctypes
import threading

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import graph_clean_kit as gk
import road_width_kit as wk
from scene_kit import kernel_rows

from sam_road_amd import edge_support as es
from sam_road_amd import graph_clean as gc
from sam_road_amd import road_width as rw
from sam_road_amd.graph_clean import graph_clean_key_of, graph_clean_ref, thresholds_q
from sam_road_amd.graph_raster import MAX_SPAN

GUARD = 64                                                # bytes on either side of state and out: out stays 16-byte aligned
ROWS = {"graph_clean_init", "graph_clean_edges", "graph_clean_chains", "graph_clean_sums", "graph_clean_decide"}
CASES = gk.hand_cases()
EDGE_SIZES = (1, 63, 64, 65, 255, 256, 257)               # the wave and workgroup edges of the grid-stride loops


def _ops():
    from sam_road_amd.model import DeviceGraphOps
    return DeviceGraphOps("cuda")


def _ctx():
    from sam_road_amd import _lib
    return _lib.Context.get(torch.cuda.current_device())


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _device(nodes, edges, spur_q, comp_q, rounds):
    state, out = _ops().graph_clean(nodes, edges, spur_q=spur_q, comp_q=comp_q, rounds=rounds)
    return state.cpu().numpy(), out.cpu().numpy()


def _same(got, want, what=""):
    assert got[0].dtype == np.uint8 and got[1].dtype == np.int32 and got[1].shape == want[1].shape
    np.testing.assert_array_equal(got[0], want[0], err_msg=f"state {what}")
    np.testing.assert_array_equal(got[1], want[1], err_msg=f"out {what}")


def _entry(nodes, edges, spur_q, comp_q, rounds):
    """srh_graph_clean itself, state and out between guard bytes of 0xA5 inside larger tensors: (return code, state, out)."""
    ctx = _ctx()
    N, E = nodes.shape[0], edges.shape[0]
    sbuf = torch.full((2 * GUARD + E,), 0xA5, dtype=torch.uint8, device="cuda")
    obuf = torch.full((2 * GUARD + 16 * E,), 0xA5, dtype=torch.uint8, device="cuda")
    assert (obuf.data_ptr() + GUARD) % 16 == 0
    n_h, e_h = torch.from_numpy(nodes), torch.from_numpy(edges)
    n_d, e_d = n_h.cuda(), e_h.cuda()
    rc = ctx.lib.srh_graph_clean(ctx.handle, n_h.data_ptr(), n_d.data_ptr(), N, e_h.data_ptr(), e_d.data_ptr(), E, spur_q, comp_q, rounds,
                                 sbuf.data_ptr() + GUARD, obuf.data_ptr() + GUARD, _stream())
    torch.cuda.synchronize()
    s, o = sbuf.cpu().numpy(), obuf.cpu().numpy()
    for host, n in ((s, E), (o, 16 * E)):
        assert (host[:GUARD] == 0xA5).all() and (host[GUARD + n:] == 0xA5).all()                # nothing else is written
    assert np.array_equal(n_d.cpu().numpy(), nodes) and np.array_equal(e_d.cpu().numpy(), edges)      # and the tables are not
    return rc, s[GUARD:GUARD + E].copy(), o[GUARD:GUARD + 16 * E].copy().view(np.int32).reshape(E, 4)


# ---- 1. exact answers --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_hand_built_cases(case):
    """The literal answers of the kit, the 6000-edge chain past 2^31 included, through the entry with guard bytes around both outputs."""
    key = graph_clean_key_of(case["key"])
    rc, state, out = _entry(case["nodes"], case["edges"], *thresholds_q(key), key.rounds)
    assert rc == 0
    _same((state, out), (case["state"], case["out"]), case["name"])
    _same(gc.clean(case["nodes"], case["edges"], key), (case["state"], case["out"]), case["name"])      # and through the module


# ---- 2. sizes ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", EDGE_SIZES)
def test_sizes_at_the_wave_and_workgroup_edges(N):
    """Every E of the list at this N (and N at this E): random sparse multigraphs with thresholds from their own lengths, 1 to 3 rounds."""
    rng = np.random.default_rng(40 + N)
    dropped = 0
    for E in EDGE_SIZES:
        nodes, edges = gk.sized_graph(rng, N, E)
        spur_q, comp_q = gk.draw_thresholds(rng, nodes, edges)
        rounds = int(rng.integers(1, 4))
        want = graph_clean_ref(nodes, edges, spur_q, comp_q, rounds)
        rc, state, out = _entry(nodes, edges, spur_q, comp_q, rounds)
        assert rc == 0
        _same((state, out), want, f"N {N} E {E}")
        dropped += int((want[0] != 0).sum())
    assert N < 63 or dropped > 0


def test_random_multigraphs_equal_the_reference():
    rng = np.random.default_rng(77)
    ops = _ops()
    for _ in range(40):
        nodes, edges = gk.random_multigraph(rng)
        spur_q, comp_q = gk.draw_thresholds(rng, nodes, edges)
        rounds = int(rng.integers(1, 4))
        state, out = ops.graph_clean(nodes, edges, spur_q=spur_q, comp_q=comp_q, rounds=rounds)
        _same((state.cpu().numpy(), out.cpu().numpy()), graph_clean_ref(nodes, edges, spur_q, comp_q, rounds))


# ---- 3. deep trees, one root, a large component -----------------------------------------------------------------------------------------------------------
def test_a_shuffled_chain_of_5000_edges():
    """One path with shuffled node and edge indices: deep trees in both forests and every sum on one root.  Not a spur (two leaf ends); at
    a component threshold one sixteenth above its length it goes, at its length it stays."""
    rng = np.random.default_rng(3)
    nodes, edges = gk.shuffled_chain(rng, 5000)
    total = int(gc.edge_len_q(nodes, edges).sum())
    for spur_q, comp_q in ((2 ** 24, total), (2 ** 24, total + 1), (0, 0)):
        want = graph_clean_ref(nodes, edges, spur_q, comp_q, 1)
        assert bool(want[0].any()) == (comp_q == total + 1)
        _same(_device(nodes, edges, spur_q, comp_q, 1), want, f"comp_q {comp_q}")
    assert (want[1][:, 0] == 0).all() and (want[1][:, 1] == 0).all() and (want[1][:, 2] == total).all()


@pytest.mark.parametrize("rounds", (1, 3))
def test_a_jittered_grid_of_20000_edges_twice_with_identical_bytes(rounds):
    rng = np.random.default_rng(21)
    nodes, edges = gk.jittered_grid(rng, side=100)
    assert 19000 < edges.shape[0] < 22000
    spur_q, comp_q = 16 * 9, 16 * 60
    want = graph_clean_ref(nodes, edges, spur_q, comp_q, rounds)
    kept = want[1][want[0] == 0]
    biggest = np.bincount(kept[:, 1]).max()
    assert biggest > 15000 and 100 < int((want[0] != 0).sum()) < 5000 and ((want[0] & 3) == 1).any() and ((want[0] & 2) == 2).any()
    assert rounds == 1 or (want[0] >= 8).any()                           # something falls only in a later round
    first = _device(nodes, edges, spur_q, comp_q, rounds)
    _same(first, want)
    second = _device(nodes, edges, spur_q, comp_q, rounds)
    assert first[0].tobytes() == second[0].tobytes() and first[1].tobytes() == second[1].tobytes()


# ---- 4. the launch contract -------------------------------------------------------------------------------------------------------------------------------
def test_launch_contract():
    ops, ctx = _ops(), _ctx()
    rng = np.random.default_rng(8)
    nodes, edges = gk.jittered_grid(rng, side=20)
    result = (nodes, edges, np.zeros((4, 4), np.uint8), np.zeros((4, 4), np.uint8))
    with kernel_rows(ctx) as rows:
        ops.graph_clean(nodes, edges, spur_q=100)
        assert rows() == ROWS
        s, o = ops.graph_clean(nodes, [], spur_q=100)
        assert tuple(s.shape) == (0,) and tuple(o.shape) == (0, 4) and rows() == set()                   # E = 0
        assert gc.apply(None, result, net=ops) == (result, None) and rows() == set()                     # a None key
        (n2, e2, _, _), attrs = gc.apply(graph_clean_key_of({"min_spur": 9}), result, net=ops)
        assert rows() == ROWS and 0 < e2.shape[0] < edges.shape[0] and len(attrs) == e2.shape[0]
    ctx.profile_read()
    ctx.profile_enable(True)
    try:
        for r, (g_nodes, g_edges) in ((1, (nodes, edges)), (3, (nodes, edges)), (8, (nodes[:2], edges[:1] * 0 + [[0, 1]])), (2, gk.shuffled_chain(rng, 300))):
            ops.graph_clean(g_nodes, g_edges, spur_q=150, comp_q=900, rounds=r)
            torch.cuda.synchronize()                                     # 5 (rounds + 1) launches whatever the graph holds
            assert {x["name"]: x["launches"] for x in ctx.profile_read() if x["launches"]} == {name: r + 1 for name in ROWS}
    finally:
        ctx.profile_enable(False)


def test_entry_rejects_bad_arguments_and_launches_nothing():
    from sam_road_amd import _lib
    ctx = _ctx()
    lib, s = ctx.lib, _stream()
    nodes = np.array([[1, 1], [6, 5], [3, 7]], np.int32)
    edges = np.array([[0, 1], [1, 2]], np.int32)
    buf = torch.full((256,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    out = buf[16:24]                                      # [2, 4]
    state = buf[64:65]                                    # 4 bytes, 2 used

    def edit(a, i, v):
        a = a.copy()
        a.reshape(-1)[i] = v
        return a

    def call(n=nodes, e=edges, N=None, E=None, spur_q=100, comp_q=100, rounds=1, state_p=state.data_ptr(), out_p=out.data_ptr(), n_host=True, n_dev=True,
             e_host=True, e_dev=True, dev_off=0, out_is=None, state_is=None, c=ctx.handle):
        nh, eh = torch.from_numpy(np.ascontiguousarray(n)), torch.from_numpy(np.ascontiguousarray(e))
        nd, ed = nh.cuda(), eh.cuda()
        if out_is is not None:                            # an output overlapping a table
            out_p = {"nodes": nd, "edges": ed}[out_is].data_ptr()
        if state_is is not None:
            state_p = {"nodes": nd, "edges": ed}[state_is].data_ptr() + 3
        return lib.srh_graph_clean(c, nh.data_ptr() if n_host else None, nd.data_ptr() + dev_off if n_dev else None, n.shape[0] if N is None else N,
                                   eh.data_ptr() if e_host else None, ed.data_ptr() if e_dev else None, e.shape[0] if E is None else E, spur_q, comp_q, rounds,
                                   state_p, out_p, s)

    S = MAX_SPAN
    assert call() == 0                                    # the workspace exists from here on: an output inside it can be named
    torch.cuda.synchronize()
    host = buf.cpu().numpy()
    want = graph_clean_ref(nodes, edges, 100, 100, 1)
    np.testing.assert_array_equal(host[16:24].reshape(2, 4), want[1])
    np.testing.assert_array_equal(host[64:65].view(np.uint8)[:2], want[0])
    assert (host[:16] == 0x5A5A5A5A).all() and (host[24:64] == 0x5A5A5A5A).all() and (host[65:] == 0x5A5A5A5A).all()
    assert host[64:65].view(np.uint8)[2:].tolist() == [0x5A, 0x5A]
    buf.fill_(0x5A5A5A5A)
    bad = (dict(c=None), dict(n_host=False), dict(n_dev=False), dict(e_host=False), dict(e_dev=False), dict(N=-1), dict(E=-1), dict(N=0), dict(dev_off=2),
           dict(N=2 ** 26 + 1), dict(E=2 ** 26 + 1),
           dict(e=edit(edges, 1, 3)), dict(e=edit(edges, 2, -1)), dict(n=edit(nodes, 0, 2 ** 28 + 1)), dict(n=edit(nodes, 5, -2 ** 28 - 1)),
           dict(n=edit(nodes, 2, 1 + S + 1)), dict(n=edit(nodes, 3, 1 - S - 1)),                         # what srh_graph_edge_stats refuses of its tables
           dict(rounds=0), dict(rounds=9), dict(rounds=-1), dict(spur_q=-1), dict(comp_q=-1), dict(comp_q=-2 ** 62),
           dict(state_p=None), dict(out_p=None), dict(out_p=out.data_ptr() + 4), dict(out_p=out.data_ptr() + 8),
           dict(out_is="nodes"), dict(out_is="edges"), dict(state_is="nodes"), dict(state_is="edges"),
           dict(state_p=out.data_ptr() + 5), dict(state_p=out.data_ptr() + 31), dict(out_p=state.data_ptr() - 16))      # the outputs overlap each other
    for kw in bad:
        assert call(**kw) == -1, kw
    torch.cuda.synchronize()
    assert (buf.cpu().numpy() == 0x5A5A5A5A).all()        # nothing was launched: state and out are unchanged
    with kernel_rows(ctx) as rows:                        # E = 0 is SRH_OK and launches nothing, with or without tables and outputs
        assert call(E=0) == 0 and call(N=0, E=0, n_host=False, n_dev=False, e_host=False, e_dev=False, state_p=None, out_p=None) == 0
        assert rows() == set()
        for kw in bad[1:]:                                # and a refused call launches nothing
            assert call(**kw) == -1
        assert rows() == set()
    assert (buf.cpu().numpy() == 0x5A5A5A5A).all()
    with pytest.raises(_lib.SrhError, match="rounds"):
        ctx.check(call(rounds=9), "srh_graph_clean")
    with pytest.raises(_lib.SrhError, match="16-byte"):
        ctx.check(call(out_p=out.data_ptr() + 8), "srh_graph_clean")
    with pytest.raises(_lib.SrhError, match="overlap"):
        ctx.check(call(state_p=out.data_ptr() + 5), "srh_graph_clean")
    # the shim refuses on the host, with ValueError
    ops = _ops()
    for fn in (lambda: ops.graph_clean(nodes, edit(edges, 1, 3)), lambda: ops.graph_clean(nodes, edges, rounds=0), lambda: ops.graph_clean(nodes, edges, rounds=9),
               lambda: ops.graph_clean(nodes, edges, spur_q=-1), lambda: ops.graph_clean(nodes, edges, comp_q=1.5), lambda: ops.graph_clean(nodes, edges, spur_q=True),
               lambda: ops.graph_clean(nodes, edges, state=torch.zeros(2, dtype=torch.uint8)), lambda: ops.graph_clean(nodes, edges, out=torch.zeros((2, 4), device="cuda")),
               lambda: gc.clean(nodes, edges, None), lambda: gc.clean(nodes, edges, {"min_spur": 0})):
        with pytest.raises(ValueError):
            fn()
    torch.cuda.synchronize()


def test_two_threads_on_two_streams_get_their_own_results():
    """The workspace belongs to the context: two calls in flight at once must not share it.  Each thread runs its own graph on its own
    stream, several times, and every result equals the reference of ITS graph."""
    rng = np.random.default_rng(5)
    graphs = [gk.jittered_grid(rng, side=60), gk.jittered_grid(rng, side=45, gap=0.2, stub=0.3)]
    params = [(16 * 9, 16 * 60, 2), (16 * 7, 16 * 200, 3)]
    wants = [graph_clean_ref(n, e, *p) for (n, e), p in zip(graphs, params)]
    assert not np.array_equal(wants[0][0][:1000], wants[1][0][:1000])
    ops = _ops()
    ops.graph_clean(*graphs[0], spur_q=1)                 # the workspace at its full size before the threads start
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    got, errors = [[], []], []
    start = threading.Barrier(2)

    def work(k):
        try:
            with torch.cuda.stream(streams[k]):
                start.wait(timeout=30)
                for _ in range(6):
                    state, out = ops.graph_clean(*graphs[k], spur_q=params[k][0], comp_q=params[k][1], rounds=params[k][2])
                    got[k].append((state, out))
                streams[k].synchronize()
        except Exception as exc:                          # noqa: BLE001
            errors.append(exc)

    threads = [threading.Thread(target=work, args=(k,)) for k in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(timeout=120)
    assert not errors, errors
    torch.cuda.synchronize()
    for k in range(2):
        assert len(got[k]) == 6
        for state, out in got[k]:
            _same((state.cpu().numpy(), out.cpu().numpy()), wants[k], f"thread {k}")


# ---- 5. end to end ----------------------------------------------------------------------------------------------------------------------------------------
def test_apply_on_the_device_equals_apply_ref_behind_the_two_other_steps():
    rng = np.random.default_rng(9)
    ops = _ops()
    nodes, edges = wk.grid_graph(260, 300)
    road = wk.shape_mask("bars", 4, 260, 300) | wk.random_mask(rng, 260, 300, 127, 0.05)
    result = (nodes, edges, np.zeros_like(road), road)
    k1 = es.edge_support_key_of({"min_on": 0.1})
    k2 = rw.road_width_key_of({"max_radius": 32, "min_in": 0.05})
    d1, a1 = es.apply(k1, result, net=ops)
    h1, b1 = es.apply_ref(k1, result)
    d2, a2, keep_d = rw.apply(k2, d1, net=ops, return_keep=True)
    h2, b2 = rw.apply_ref(k2, h1)
    assert np.array_equal(d2[1], h2[1]) and 3 < d2[1].shape[0] < edges.shape[0]
    for extra in ({}, {"min_spur": 40}, {"min_component": 100}, {"min_spur": 40, "min_component": 100, "rounds": 3}, {"min_spur": 25.5, "drop_isolated": True},
                  {"rounds": 8}):
        key = graph_clean_key_of(dict({"rounds": 1}, **extra))
        (n1, e1, k_1, r1), c1, keep1 = gc.apply(key, d2, net=ops, return_keep=True)
        (n2, e2, _, _), c2, keep2 = gc.apply_ref(key, h2, return_keep=True)
        assert np.array_equal(n1, n2) and np.array_equal(e1, e2) and c1 == c2 and np.array_equal(keep1, keep2) and k_1 is result[2] and r1 is road, extra
        assert gc.apply(key, d2, net=ops)[1] == c1
        assert (0 < e1.shape[0] < d2[1].shape[0]) if gc.filters(key) else np.array_equal(e1, d2[1]), extra
        lines = gc.polylines_geojson(n1, e1, gc.table_of(c1))
        assert sum(f["properties"]["n_edges"] for f in lines["features"]) == e1.shape[0]
