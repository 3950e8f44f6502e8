"""EDGE_SUPPORT (the road mask under every edge, counted on the device) on the HIP path.  Run on an MI355X: pytest -m gpu.

The four counters of every edge must equal edge_support_ref as integers at every shape at which the kernel's addressing can go wrong;
the filter and the export work on those integers on the host.  There is no tolerance anywhere."""
import ctypes
import json
import os
import warnings

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import edge_support_kit as ek
from scene_kit import CFG, kernel_rows, pair, rect_scene, run_cli, thresholds  # noqa: F401

from sam_road_amd import edge_support as es
from sam_road_amd.edge_support import edge_attrs, edge_support_key, edge_support_ref, graph_geojson
from sam_road_amd.formats import convert_to_sat2graph_format
from sam_road_amd.graph_raster import MAX_SPAN, composite_ref, graph_raster_ref

GUARD = 16                                                # int32 words on either side of out: 64 bytes, so out stays 16-byte aligned
WIDTHS = (1, 2, 5, 16, 255)


def _ops():
    from sam_road_amd.model import DeviceGraphOps
    return DeviceGraphOps("cuda")


def _ctx():
    from sam_road_amd import _lib
    return _lib.Context.get(torch.cuda.current_device())


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _entry(nodes, edges, mask, t, level, valid=None):
    """srh_graph_edge_stats itself, out between guard words of 0xA5A5A5A5 inside a larger tensor: (return code, int32 [E, 4] host array)."""
    from sam_road_amd.graph_raster import check_graph
    ctx = _ctx()
    n, e = check_graph(nodes, edges)
    E = e.shape[0]
    buf = torch.full((2 * GUARD + 4 * E,), -0x5A5A5A5B, dtype=torch.int32, device="cuda")
    out = buf[GUARD:GUARD + 4 * E]
    assert out.data_ptr() % 16 == 0
    n_h, e_h = torch.from_numpy(n), torch.from_numpy(e)
    n_d, e_d, m_d = n_h.cuda(), e_h.cuda(), _dev(mask)
    v_d = None if valid is None else _dev(valid)
    H, W = mask.shape
    rc = ctx.lib.srh_graph_edge_stats(ctx.handle, n_h.data_ptr(), n_d.data_ptr(), n.shape[0], e_h.data_ptr(), e_d.data_ptr(), E, H, W, t, m_d.data_ptr(),
                                      None if v_d is None else v_d.data_ptr(), level, out.data_ptr(), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    host = buf.cpu().numpy()
    assert (host[:GUARD] == -0x5A5A5A5B).all() and (host[GUARD + 4 * E:] == -0x5A5A5A5B).all()      # nothing else is written
    return rc, host[GUARD:GUARD + 4 * E].reshape(E, 4)


# ---- 1. parity with the reference -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(1, 1), (37, 53), (64, 64), (300, 517)])
def test_stats_equal_the_reference(shape):
    """Random graphs with zero-length edges and edges wholly or partly outside the image, random masks, with and without valid, every width
    of {1, 2, 5, 16, 255}; through the entry with guard words around out, and through the shim and the module's function."""
    H, W = shape
    rng = np.random.default_rng(H * 1000 + W + 7)
    nodes, edges = ek.random_graph(rng, H, W, 40, 61, margin=max(20, H // 3), zero_length=4)
    far = np.array([[-50, -60], [-20, -300], [H + 30, W + 5], [H + 200, W + 90], [H // 2, -40], [H // 2 + 3, W + 40]])      # two edges wholly outside, one across
    nodes = np.concatenate([nodes, far])
    edges = np.concatenate([edges, [[40, 41], [42, 43], [44, 45]]])          # 64 edges: 16 workgroups, the last wave of the last one included
    mask = rng.integers(0, 256, (H, W), dtype=np.uint8)
    valid = (rng.integers(0, 4, (H, W)) * 60).astype(np.uint8)
    ops, covered = _ops(), 0
    for k, t in enumerate(WIDTHS):
        level = (0, 127, 200, 254, 255)[k]
        for v in (None, valid):
            want = edge_support_ref(nodes, edges, mask, t, level, v)
            rc, got = _entry(nodes, edges, mask, t, level, v)
            assert rc == 0
            np.testing.assert_array_equal(got, want, err_msg=f"{shape} t {t} valid {v is not None}")
            assert H == 1 or t == 255 or (want[:, 0] == 0).any()
            covered += int(want[:, 0].sum())
        out = ops.graph_edge_stats(nodes, edges, _dev(mask), width=t, on_level=level, valid=_dev(valid != 0))      # device tensors, a bool valid
        assert out.is_cuda and out.dtype == torch.int32 and tuple(out.shape) == (64, 4)
        np.testing.assert_array_equal(out.cpu().numpy(), want)
    assert covered > 0                                    # neither all nor nothing: a kernel that ignores the graph cannot pass
    got = es.edge_stats(nodes[:40], edges[:7], mask, 2, 100, valid=valid, device="cuda")                           # numpy in, a host array out; E below a workgroup
    assert isinstance(got, np.ndarray) and got.dtype == np.int32
    np.testing.assert_array_equal(got, edge_support_ref(nodes[:40], edges[:7], mask, 2, 100, valid))
    # a float node array is truncated toward zero
    np.testing.assert_array_equal(es.edge_stats(nodes + 0.75, edges, mask, 2, 100, device="cuda"), edge_support_ref(np.trunc(nodes + 0.75), edges, mask, 2, 100))


def test_stats_a_star_of_500_edges_and_maximum_span_edges():
    rng = np.random.default_rng(23)
    nodes, edges = ek.star(64, 64, 500)
    mask = rng.integers(0, 256, (64, 64), dtype=np.uint8)
    valid = rng.integers(0, 2, (64, 64)).astype(np.uint8)
    for t in (1, 4):
        rc, got = _entry(nodes, edges, mask, t, 127, valid)
        want = edge_support_ref(nodes, edges, mask, t, 127, valid)
        assert rc == 0 and want[:, 0].min() > 0
        np.testing.assert_array_equal(got, want)
    S = MAX_SPAN
    for shape, nd in (((1, 16384), [[0, 0], [0, S]]), ((1, 16384), [[0, S], [0, 0]]), ((16384, 2), [[0, 1], [S, 0]]), ((16384, 2), [[S - 7000, 0], [-7000, 1]])):
        mask = rng.integers(0, 256, shape, dtype=np.uint8)
        valid = rng.integers(0, 2, shape).astype(np.uint8)
        for t in (1, 16, 255):
            rc, got = _entry(nd, [[0, 1]], mask, t, 100, valid)
            want = edge_support_ref(nd, [[0, 1]], mask, t, 100, valid)
            assert rc == 0 and want[0, 0] >= 9000
            np.testing.assert_array_equal(got, want, err_msg=f"{shape} {nd} t {t}")


def test_stats_of_a_full_mask_at_the_largest_width():
    H, W = 300, 517
    rng = np.random.default_rng(31)
    nodes, edges = ek.random_graph(rng, H, W, 30, 40, margin=100)
    got = es.edge_stats(nodes, edges, np.full((H, W), 255, np.uint8), 255, 254, device="cuda")
    np.testing.assert_array_equal(got, edge_support_ref(nodes, edges, np.full((H, W), 255, np.uint8), 255, 254))
    assert (got[:, 1] == 255 * got[:, 0]).all() and (got[:, 2] == got[:, 0]).all() and not got[:, 3].any() and got[:, 0].max() > 50000


# ---- 2. the launch contract -------------------------------------------------------------------------------------------------------------------------------
def test_launch_contract():
    ops, ctx = _ops(), _ctx()
    nodes, edges = ek.grid_graph(100, 100)
    mask = _dev(np.full((100, 100), 200, np.uint8))
    key = edge_support_key({"EDGE_SUPPORT": {"min_on": 0.5}})
    result = (nodes, edges, mask.cpu().numpy(), mask.cpu().numpy())
    with kernel_rows(ctx) as rows:
        ops.graph_edge_stats(nodes, edges, mask)
        assert rows() == {"graph_edge_stats"}
        ops.graph_edge_stats(nodes, edges, mask, width=255, on_level=0, valid=mask)
        assert rows() == {"graph_edge_stats"}
        assert tuple(ops.graph_edge_stats(nodes, [], mask).shape) == (0, 4) and rows() == set()          # E = 0
        assert es.apply(None, result, net=ops) == (result, None) and rows() == set()                     # a None key
        (n2, e2, _, _), attrs = es.apply(key, result, net=ops)
        assert rows() == {"graph_edge_stats"} and np.array_equal(e2, edges) and len(attrs) == edges.shape[0] and attrs[0]["mean"] == 200.0
    ctx.profile_read()
    ctx.profile_enable(True)
    try:
        ops.graph_edge_stats(nodes, edges, mask)
        torch.cuda.synchronize()
        assert {r["name"]: r["launches"] for r in ctx.profile_read() if r["launches"]} == {"graph_edge_stats": 1}          # exactly one launch per call
    finally:
        ctx.profile_enable(False)


def test_entry_rejects_bad_arguments_and_launches_nothing():
    from sam_road_amd import _lib
    ctx = _ctx()
    lib, s = ctx.lib, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    H = W = 8
    nodes = np.array([[1, 1], [6, 5], [3, 7]], np.int32)
    edges = np.array([[0, 1], [1, 2]], np.int32)
    buf = torch.full((64,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    out = buf[16:24]
    mask = torch.ones(H * W + 64, dtype=torch.uint8, device="cuda")
    valid = torch.ones(H * W, dtype=torch.uint8, device="cuda")

    def edit(a, i, v):
        a = a.copy()
        a.reshape(-1)[i] = v
        return a

    def call(n=nodes, e=edges, N=None, E=None, H=H, W=W, t=1, mask_p=mask.data_ptr(), valid_p=valid.data_ptr(), level=127, out_p=out.data_ptr(), n_host=True, n_dev=True,
             e_host=True, e_dev=True, dev_off=0, out_is=None):
        nh, eh = torch.from_numpy(np.ascontiguousarray(n)), torch.from_numpy(np.ascontiguousarray(e))
        nd, ed = nh.cuda(), eh.cuda()
        if out_is is not None:                            # out overlapping a table
            out_p = {"nodes": nd, "edges": ed}[out_is].data_ptr()
        return lib.srh_graph_edge_stats(ctx.handle, nh.data_ptr() if n_host else None, nd.data_ptr() + dev_off if n_dev else None, n.shape[0] if N is None else N,
                                        eh.data_ptr() if e_host else None, ed.data_ptr() if e_dev else None, e.shape[0] if E is None else E, H, W, t, mask_p, valid_p,
                                        level, out_p, s)

    S = MAX_SPAN
    bad = (dict(n_host=False), dict(n_dev=False), dict(e_host=False), dict(e_dev=False), dict(N=-1), dict(E=-1), dict(H=0), dict(W=0), dict(H=-3), dict(H=65536, W=32768),
           dict(t=0), dict(t=256), dict(dev_off=2), dict(e=edit(edges, 1, 3)), dict(e=edit(edges, 2, -1)), dict(n=edit(nodes, 0, 2 ** 28 + 1)),
           dict(n=edit(nodes, 5, -2 ** 28 - 1)), dict(n=edit(nodes, 2, 1 + S + 1)), dict(n=edit(nodes, 3, 1 - S - 1)), dict(N=0),      # what srh_graph_raster refuses
           dict(level=-1), dict(level=256), dict(mask_p=None), dict(out_p=None), dict(out_p=out.data_ptr() + 4), dict(out_p=out.data_ptr() + 8),
           dict(mask_p=out.data_ptr() - 40), dict(valid_p=out.data_ptr() + 16), dict(out_is="nodes"), dict(out_is="edges"))
    for kw in bad:
        assert call(**kw) == -1, kw
    assert lib.srh_graph_edge_stats(None, None, None, 0, None, None, 0, H, W, 1, mask.data_ptr(), None, 0, out.data_ptr(), s) == -1
    torch.cuda.synchronize()
    assert (buf.cpu().numpy() == 0x5A5A5A5A).all()        # nothing was launched: out is unchanged
    with kernel_rows(ctx) as rows:                        # E = 0 is SRH_OK and launches nothing, with or without tables, mask and out
        assert call(E=0) == 0 and call(N=0, E=0, n_host=False, n_dev=False, e_host=False, e_dev=False, mask_p=None, out_p=None) == 0
        assert rows() == set()
    assert (buf.cpu().numpy() == 0x5A5A5A5A).all()
    assert call() == 0 and call(valid_p=None) == 0        # and the good calls run
    torch.cuda.synchronize()
    host = buf.cpu().numpy()
    assert (host[:16] == 0x5A5A5A5A).all() and (host[24:] == 0x5A5A5A5A).all()
    np.testing.assert_array_equal(host[16:24].reshape(2, 4), edge_support_ref(nodes, edges, np.ones((H, W), np.uint8), 1, 127))
    with pytest.raises(_lib.SrhError, match="on_level"):
        ctx.check(call(level=256), "srh_graph_edge_stats")
    # the shim refuses on the host, with ValueError
    ops, m2 = _ops(), mask[:H * W].view(H, W)
    for fn in (lambda: ops.graph_edge_stats(nodes, edit(edges, 1, 3), m2), lambda: ops.graph_edge_stats(nodes, edges, m2, width=0), lambda: ops.graph_edge_stats(nodes, edges, m2, on_level=256),
               lambda: ops.graph_edge_stats(nodes, edges, m2, on_level=0.5), lambda: ops.graph_edge_stats(nodes, edges, m2.cpu()), lambda: ops.graph_edge_stats(nodes, edges, m2.int()),
               lambda: ops.graph_edge_stats(nodes, edges, m2, valid=valid[:32].view(4, 8)), lambda: ops.graph_edge_stats(nodes, edges, np.ones((H, W), np.float32)),
               lambda: ops.graph_edge_stats(nodes, edges, m2[:, ::2])):
        with pytest.raises(ValueError):
            fn()
    torch.cuda.synchronize()


# ---- 3. end to end ----------------------------------------------------------------------------------------------------------------------------------------
def _files(root):
    return sorted(os.path.relpath(os.path.join(d, f), root) for d, _, fs in os.walk(root) for f in fs)


def test_apply_and_the_cli_end_to_end(pair, tmp_path, monkeypatch):
    """apply on a real infer_one_img result equals the host statement on the returned masks; the CLI with --edge-min-on, --viz and
    --graph-geojson writes the filtered pickle, the viz and the GeoJSON of exactly that graph, and leaves the masks as they were."""
    from PIL import Image
    from sam_road_amd import Config
    from sam_road_amd import cli, inferencer as inf
    _, net = pair
    monkeypatch.chdir(tmp_path)
    H, W = 401, 523
    img = rect_scene(H, W, 43)
    Image.fromarray(img).save("rgb.png")
    valid = np.ones((H, W), np.uint8)
    valid[:, 400:] = 0
    np.save("valid.npy", valid)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        base = dict(CFG, INFER_PATCHES_PER_EDGE=4)
        _, _, kp0, road0 = inf.infer_one_img(net, img, Config(base), valid=valid)
        cfg = dict(base, **thresholds(kp0, road0))
        res = next(iter(inf.infer_imgs(net, iter([img]), Config(cfg), device=torch.device("cuda"), valids=iter([valid]))))      # the loop the CLI runs
        nodes, edges, _, road = res
        assert edges.shape[0] > 5
        level = es.on_level_of(cfg["ROAD_THRESHOLD"])
        ref = edge_support_ref(nodes, edges, road, 1, level, valid)
        np.testing.assert_array_equal(net.graph_edge_stats(nodes, edges, road, 1, level, valid).cpu().numpy(), ref)
        f_med = float(np.median([a["on_frac"] for a in edge_attrs(nodes, edges, ref)]))
        for extra in ({"min_on": f_med, "drop_isolated": True}, {"width": 5, "min_mean": 0.1, "max_invalid": 0}):
            key = edge_support_key(Config(cfg, EDGE_SUPPORT=extra))
            (n1, e1, k1, r1), a1 = es.apply(key, res, valid=valid, net=net)
            (n2, e2, _, _), a2 = es.apply_ref(key, res, valid)
            assert np.array_equal(n1, n2) and np.array_equal(e1, e2) and a1 == a2 and k1 is res[2] and r1 is road
        key = edge_support_key(Config(cfg, EDGE_SUPPORT={"min_on": f_med, "drop_isolated": True}))
        (want_nodes, want_edges, _, _), want_attrs = es.apply_ref(key, res, valid)
        assert 0 < want_edges.shape[0] < edges.shape[0]                              # at least one edge dropped, at least one kept
        before = run_cli(cli, net, tmp_path, monkeypatch, "before", cfg, ["rgb.png"], "--device", "cuda", "--valid-masks", "valid.npy")["rgb"]
        got = run_cli(cli, net, tmp_path, monkeypatch, "kept", cfg, ["rgb.png"], "--device", "cuda", "--valid-masks", "valid.npy", "--edge-min-on", repr(f_med),
                      "--drop-isolated-nodes", "--viz", "--graph-geojson")["rgb"]
    plain_files = ["config.yaml", "graph/rgb.p", "inference_time.txt", "mask/rgb_itsc.png", "mask/rgb_road.png"]
    assert _files("save/before") == plain_files and _files("save/kept") == sorted(plain_files + ["viz/rgb.png", "graph_geojson/rgb.geojson"])
    for f in plain_files[3:]:
        assert open(f"save/kept/{f}", "rb").read() == open(f"save/before/{f}", "rb").read(), f
    assert before[2] == convert_to_sat2graph_format(nodes, edges) and got[2] == convert_to_sat2graph_format(want_nodes, want_edges)
    np.testing.assert_array_equal(np.array(Image.open("save/kept/viz/rgb.png")), composite_ref(graph_raster_ref(want_nodes, want_edges, (H, W), 4, "disc", 4), img))
    assert json.load(open("save/kept/graph_geojson/rgb.geojson")) == json.loads(json.dumps(graph_geojson(want_nodes, want_edges, want_attrs)))
