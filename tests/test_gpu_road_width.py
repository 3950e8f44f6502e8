"""ROAD_WIDTH (an exact distance map of the road mask and the road width under every edge) on the HIP path.  Run on an MI355X:
pytest -m gpu.

The distance map must equal road_dist_ref and the eight integers of every edge road_width_ref, at every shape at which the kernels'
addressing can go wrong; the attributes, the filter and the export work on those integers on the host.  There is no tolerance anywhere."""
import ctypes
import json
import os
import warnings

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import road_width_kit as wk
from scene_kit import CFG, kernel_rows, pair, rect_scene, run_cli, thresholds  # noqa: F401

from sam_road_amd import road_width as rw
from sam_road_amd.edge_support import graph_geojson
from sam_road_amd.formats import convert_to_sat2graph_format
from sam_road_amd.graph_raster import MAX_SPAN, check_graph
from sam_road_amd.road_width import road_dist_ref, road_width_key, road_width_ref, width_attrs

GUARD = 32                                                # bytes on either side of D2 and out: D2 stays 8-byte, out 16-byte aligned
RADII = (1, 2, 5, 32, 33, 254)
LEVELS = (0, 127, 254, 255)
# the issue's shapes, and one on either side of the column pass's chunk (32 rows) and strip (256 columns) and of the row pass's segment
# (1024 pixels); odd widths give every row another misalignment of its quads
SHAPES = [(1, 1), (1, 70), (70, 1), (37, 53), (64, 64), (131, 260), (300, 517), (31, 255), (33, 257), (3, 1023), (2, 1025)]
assert wk.COL_ROWS == 32 and wk.COL_STRIP == 256 and wk.ROW_SEG == 1024


def _ops():
    from sam_road_amd.model import DeviceGraphOps
    return DeviceGraphOps("cuda")


def _ctx():
    from sam_road_amd import _lib
    return _lib.Context.get(torch.cuda.current_device())


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _entry_dist(mask, level, R):
    """srh_road_dist itself, D2 between guard bytes of 0xA5 inside a larger tensor: (return code, uint16 [H, W] host array)."""
    ctx = _ctx()
    H, W = mask.shape
    buf = torch.full((2 * GUARD + 2 * H * W,), 0xA5, dtype=torch.uint8, device="cuda")
    ptr = buf.data_ptr() + GUARD
    assert ptr % 8 == 0
    m_d = _dev(mask)
    rc = ctx.lib.srh_road_dist(ctx.handle, m_d.data_ptr(), H, W, level, R, ptr, _stream())
    torch.cuda.synchronize()
    host = buf.cpu().numpy()
    assert (host[:GUARD] == 0xA5).all() and (host[GUARD + 2 * H * W:] == 0xA5).all()      # nothing else is written
    assert np.array_equal(m_d.cpu().numpy(), mask)                                          # and the mask is not
    return rc, host[GUARD:GUARD + 2 * H * W].copy().view(np.uint16).reshape(H, W)


def _entry_widths(nodes, edges, d2, R):
    """srh_graph_edge_widths itself, out between guard words inside a larger tensor: (return code, int32 [E, 8] host array)."""
    ctx = _ctx()
    n, e = check_graph(nodes, edges)
    E = e.shape[0]
    g = GUARD // 4
    buf = torch.full((2 * g + 8 * E,), -0x5A5A5A5B, dtype=torch.int32, device="cuda")
    out = buf[g:g + 8 * E]
    assert out.data_ptr() % 16 == 0
    n_h, e_h = torch.from_numpy(n), torch.from_numpy(e)
    n_d, e_d, d_d = n_h.cuda(), e_h.cuda(), _dev(d2)
    H, W = d2.shape
    rc = ctx.lib.srh_graph_edge_widths(ctx.handle, n_h.data_ptr(), n_d.data_ptr(), n.shape[0], e_h.data_ptr(), e_d.data_ptr(), E, H, W, d_d.data_ptr(), R, out.data_ptr(), _stream())
    torch.cuda.synchronize()
    host = buf.cpu().numpy()
    assert (host[:g] == -0x5A5A5A5B).all() and (host[g + 8 * E:] == -0x5A5A5A5B).all()      # nothing else is written
    return rc, host[g:g + 8 * E].reshape(E, 8)


def _count(d2, R, tally):
    tally[0] += int((d2 == R * R).sum())
    tally[1] += int(((d2 > 0) & (d2 < R * R)).sum())


# ---- 1. the distance map ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES)
def test_dist_equals_the_reference(shape):
    """Every R of {1, 2, 5, 32, 33, 254}, the levels {0, 127, 254, 255} dealt over them; a random mask at density 0.9, all road, all
    background and a solid mask with single background pixels at the corners, the centre and the boundaries of both passes' tiling."""
    H, W = shape
    si = SHAPES.index(shape)
    rng = np.random.default_rng(H * 1000 + W)
    tally = [0, 0]
    for ri, R in enumerate(RADII):
        level = LEVELS[(ri + si) % 4]
        bg, road = wk.level_values(level)
        masks = {"random": wk.random_mask(rng, H, W, level, 0.9), "road": np.full((H, W), 255, np.uint8), "background": np.full((H, W), bg, np.uint8),
                 "holes": wk.solid_with_holes(H, W, level)}
        for name, mask in masks.items():
            want = road_dist_ref(mask, level, R)
            rc, got = _entry_dist(mask, level, R)
            assert rc == 0
            np.testing.assert_array_equal(got, want, err_msg=f"{shape} R {R} level {level} {name}")
            _count(want, R, tally)
            if name == "background" or (name == "road" and road is None):
                assert not got.any()                      # all background: every pixel 0
            elif name == "road":
                assert (got == R * R).all()               # no background: every pixel at the cap
    assert tally[0] > 0 and (tally[1] > 0 or max(H, W) <= 2)          # neither all capped nor none: a kernel that caps everything or nothing cannot pass
    mask, level = wk.random_mask(rng, H, W, 127, 0.9), 127            # the shim, from a device tensor and from numpy, and the module's function
    want = road_dist_ref(mask, 127, 5)
    ops = _ops()
    for out in (ops.road_dist(_dev(mask), on_level=127, radius=5), ops.road_dist(mask, 127, 5), rw.distance_map(mask, 127, 5, device="cuda")):
        assert out.is_cuda and out.dtype == torch.uint16 and tuple(out.shape) == shape
        np.testing.assert_array_equal(out.cpu().numpy(), want)


@pytest.mark.parametrize("R", RADII)
def test_dist_of_bars_a_disc_and_a_cross_around_the_cap(R):
    """Half-widths R - 1, R and R + 1: the largest distance (half + 1) lies just below the cap, exactly on it and behind it."""
    S = 2 * R + 13
    tally = [0, 0]
    kinds = ("bars", "disc", "cross") if R < 33 else ("cross",)
    cases = [(kind, half) for kind in kinds for half in (R - 1, R, R + 1)] + ([("disc", R + 1), ("bars", R)] if R >= 33 else [])
    for k, (kind, half) in enumerate(cases):
        H, W = (S, S + 5) if k % 2 else (S + 3, S)
        mask = wk.shape_mask(kind, half, H, W)
        want = road_dist_ref(mask, 127, R)
        rc, got = _entry_dist(mask, 127, R)
        assert rc == 0
        np.testing.assert_array_equal(got, want, err_msg=f"{kind} half {half} R {R}")
        if kind == "cross":                               # the centre of the cross: the road's half-width, or the cap
            assert got[H // 2, 2] == min(half + 1, R) ** 2
        _count(want, R, tally)
    assert tally[0] > 0 and (tally[1] > 0 or R == 1)


# ---- 2. the edge statistics -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(1, 1), (37, 53), (64, 64), (300, 517)])
def test_widths_equal_the_reference(shape):
    """Random graphs with zero-length edges and edges wholly or partly outside the image, on a random mask, a solid mask with holes and a
    cross; 64 edges (whole workgroups), 61 (a ragged last workgroup) and 1; through the entry with guard words around out, and through
    the shim and the module's function, whose map is the device's."""
    H, W = shape
    rng = np.random.default_rng(H * 1000 + W + 11)
    nodes, edges = wk.random_graph(rng, H, W, 40, 61, margin=max(20, H // 3), zero_length=4)
    far = np.array([[-50, -60], [-20, -300], [H + 30, W + 5], [H + 200, W + 90], [H // 2, -40], [H // 2 + 3, W + 40]])      # two edges wholly outside, one across
    nodes = np.concatenate([nodes, far])
    edges = np.concatenate([edges, [[40, 41], [42, 43], [44, 45]]])
    ops, covered, partly = _ops(), 0, 0
    cases = ((1, 0, wk.random_mask(rng, H, W, 0, 0.9)), (5, 127, wk.solid_with_holes(H, W, 127)), (32, 254, wk.shape_mask("cross", 9, H, W)),
             (254, 200, wk.random_mask(rng, H, W, 200, 0.97)), (33, 255, wk.random_mask(rng, H, W, 255, 0.9)))      # at 255 nothing is road: n_in = 0
    for R, level, mask in cases:
        d2 = road_dist_ref(mask, level, R)
        for E in (64, 61, 1):
            want = road_width_ref(nodes, edges[:E], mask, level, R, d2=d2)
            rc, got = _entry_widths(nodes, edges[:E], d2, R)
            assert rc == 0
            np.testing.assert_array_equal(got, want, err_msg=f"{shape} R {R} E {E}")
        want = road_width_ref(nodes, edges, mask, level, R, d2=d2)
        covered += int(want[:, 0].sum())
        partly += int(((want[:, 1] > 0) & (want[:, 1] < want[:, 0])).sum())
        out = ops.graph_edge_widths(nodes, edges, ops.road_dist(_dev(mask), level, R), radius=R)
        assert out.is_cuda and out.dtype == torch.int32 and tuple(out.shape) == (64, 8)
        np.testing.assert_array_equal(out.cpu().numpy(), want)
        got = rw.edge_widths(nodes[:40], edges[:7], mask, level, R, device="cuda")                 # numpy in, a host array out; E below a workgroup
        assert isinstance(got, np.ndarray) and got.dtype == np.int32
        np.testing.assert_array_equal(got, road_width_ref(nodes[:40], edges[:7], mask, level, R))
    assert covered > 0 and (partly > 0 or H == 1)         # some edge lies partly on the road: n_in is neither 0 nor n


def test_widths_a_star_of_500_edges_and_maximum_span_edges():
    rng = np.random.default_rng(29)
    nodes, edges = wk.star(64, 64, 500)
    mask = wk.random_mask(rng, 64, 64, 127, 0.9)
    for R in (2, 32):
        d2 = road_dist_ref(mask, 127, R)
        rc, got = _entry_widths(nodes, edges, d2, R)
        want = road_width_ref(nodes, edges, mask, 127, R, d2=d2)
        assert rc == 0 and want[:, 0].min() > 0 and ((want[:, 1] > 0) & (want[:, 1] < want[:, 0])).any()
        np.testing.assert_array_equal(got, want)
    S = MAX_SPAN
    for shape, nd in (((1, 16384), [[0, 0], [0, S]]), ((1, 16384), [[0, S], [0, 0]]), ((16384, 2), [[0, 1], [S, 0]]), ((16384, 2), [[S - 7000, 0], [-7000, 1]])):
        for R in (3, 254):                                # any map with values up to R^2 is an input of the gather: every value of the square root's domain
            d2 = np.where(rng.random(shape) < 0.3, 0, rng.integers(1, R * R + 1, shape)).astype(np.uint16)
            d2[rng.random(shape) < 0.2] = R * R
            rc, got = _entry_widths(nd, [[0, 1]], d2, R)
            want = road_width_ref(nd, [[0, 1]], np.zeros(shape, np.uint8), 0, R, d2=d2)
            assert rc == 0 and want[0, 0] >= 9000 and 0 < want[0, 1] < want[0, 0] and want[0, 3] > 0
            np.testing.assert_array_equal(got, want, err_msg=f"{shape} {nd} R {R}")
    # the whole chain on a road that is all cap, at the largest radius: s_q = 4064 n
    full = np.full((1, 16384), 255, np.uint8)
    got = rw.edge_widths([[0, 0], [0, S]], [[0, 1]], full, 254, 254, device="cuda")
    np.testing.assert_array_equal(got, [[S + 1, S + 1, 4064 * (S + 1), S + 1, 64516, 64516, 0, 0]])


# ---- 3. the launch contract -------------------------------------------------------------------------------------------------------------------------------
def test_launch_contract():
    ops, ctx = _ops(), _ctx()
    nodes, edges = wk.grid_graph(100, 100)
    half = np.zeros((100, 100), np.uint8)
    half[:, :50] = 255                                    # the edges on the left are on the road, those on the right are not
    mask = _dev(half)
    key = road_width_key({"ROAD_WIDTH": {"min_in": 0.5}})
    result = (nodes, edges, mask.cpu().numpy(), mask.cpu().numpy())
    with kernel_rows(ctx) as rows:
        d2 = ops.road_dist(mask)
        assert rows() == {"road_dist_cols", "road_dist_rows"}
        ops.graph_edge_widths(nodes, edges, d2)
        assert rows() == {"graph_edge_widths"}
        assert tuple(ops.graph_edge_widths(nodes, [], d2).shape) == (0, 8) and rows() == set()           # E = 0
        assert rw.apply(None, result, net=ops) == (result, None) and rows() == set()                     # a None key
        (n2, e2, _, _), attrs = rw.apply(key, result, net=ops)
        assert rows() == {"road_dist_cols", "road_dist_rows", "graph_edge_widths"} and 0 < e2.shape[0] < edges.shape[0] and len(attrs) == e2.shape[0]
    ctx.profile_read()
    ctx.profile_enable(True)
    try:
        for m in (mask, torch.zeros_like(mask), torch.full_like(mask, 255)):       # the launch count does not depend on what the mask holds
            ops.graph_edge_widths(nodes, edges, ops.road_dist(m, radius=254), radius=254)
            torch.cuda.synchronize()
            assert {r["name"]: r["launches"] for r in ctx.profile_read() if r["launches"]} == {"road_dist_cols": 1, "road_dist_rows": 1, "graph_edge_widths": 1}
    finally:
        ctx.profile_enable(False)


def test_entries_reject_bad_arguments_and_launch_nothing():
    from sam_road_amd import _lib
    ctx = _ctx()
    lib, s = ctx.lib, _stream()
    H = W = 8
    nodes = np.array([[1, 1], [6, 5], [3, 7]], np.int32)
    edges = np.array([[0, 1], [1, 2]], np.int32)
    buf = torch.full((256,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    out = buf[16:32]                                      # [2, 8]
    d2 = buf[64:96]                                       # 128 bytes: u16 [8, 8]
    mask = torch.full((H * W + 64,), 255, dtype=torch.uint8, device="cuda")

    def dist(mask_p=mask.data_ptr(), H=H, W=W, level=127, R=3, d2_p=d2.data_ptr(), c=ctx.handle):
        return lib.srh_road_dist(c, mask_p, H, W, level, R, d2_p, s)

    for kw in (dict(c=None), dict(mask_p=None), dict(d2_p=None), dict(H=0), dict(W=0), dict(H=-3), dict(H=65536, W=32768), dict(level=-1), dict(level=256), dict(R=0),
               dict(R=255), dict(R=-1), dict(d2_p=d2.data_ptr() + 2), dict(d2_p=d2.data_ptr() + 4), dict(d2_p=mask.data_ptr()), dict(d2_p=mask.data_ptr() + 56),
               dict(mask_p=d2.data_ptr() + 100)):
        assert dist(**kw) == -1, kw

    def edit(a, i, v):
        a = a.copy()
        a.reshape(-1)[i] = v
        return a

    def widths(n=nodes, e=edges, N=None, E=None, H=H, W=W, d2_p=d2.data_ptr(), R=3, out_p=out.data_ptr(), n_host=True, n_dev=True, e_host=True, e_dev=True, dev_off=0,
               out_is=None):
        nh, eh = torch.from_numpy(np.ascontiguousarray(n)), torch.from_numpy(np.ascontiguousarray(e))
        nd, ed = nh.cuda(), eh.cuda()
        if out_is is not None:                            # out overlapping a table
            out_p = {"nodes": nd, "edges": ed}[out_is].data_ptr()
        return lib.srh_graph_edge_widths(ctx.handle, nh.data_ptr() if n_host else None, nd.data_ptr() + dev_off if n_dev else None, n.shape[0] if N is None else N,
                                         eh.data_ptr() if e_host else None, ed.data_ptr() if e_dev else None, e.shape[0] if E is None else E, H, W, d2_p, R, out_p, s)

    S = MAX_SPAN
    bad = (dict(n_host=False), dict(n_dev=False), dict(e_host=False), dict(e_dev=False), dict(N=-1), dict(E=-1), dict(H=0), dict(W=0), dict(H=-3), dict(H=65536, W=32768),
           dict(dev_off=2), dict(e=edit(edges, 1, 3)), dict(e=edit(edges, 2, -1)), dict(n=edit(nodes, 0, 2 ** 28 + 1)), dict(n=edit(nodes, 5, -2 ** 28 - 1)),
           dict(n=edit(nodes, 2, 1 + S + 1)), dict(n=edit(nodes, 3, 1 - S - 1)), dict(N=0),                                     # what srh_graph_edge_stats refuses
           dict(R=0), dict(R=255), dict(d2_p=None), dict(d2_p=d2.data_ptr() + 1), dict(out_p=None), dict(out_p=out.data_ptr() + 4), dict(out_p=out.data_ptr() + 8),
           dict(d2_p=out.data_ptr() - 40), dict(d2_p=out.data_ptr() + 32), dict(out_is="nodes"), dict(out_is="edges"))
    for kw in bad:
        assert widths(**kw) == -1, kw
    assert lib.srh_graph_edge_widths(None, None, None, 0, None, None, 0, H, W, d2.data_ptr(), 3, out.data_ptr(), s) == -1
    torch.cuda.synchronize()
    assert (buf.cpu().numpy() == 0x5A5A5A5A).all()        # nothing was launched: D2 and out are unchanged
    with kernel_rows(ctx) as rows:                        # E = 0 is SRH_OK and launches nothing, with or without tables, map and out
        assert widths(E=0) == 0 and widths(N=0, E=0, n_host=False, n_dev=False, e_host=False, e_dev=False, d2_p=None, out_p=None) == 0
        assert rows() == set()
    assert (buf.cpu().numpy() == 0x5A5A5A5A).all()
    assert dist() == 0 and widths() == 0                  # and the good calls run
    torch.cuda.synchronize()
    host = buf.cpu().numpy()
    assert (host[:16] == 0x5A5A5A5A).all() and (host[32:64] == 0x5A5A5A5A).all() and (host[96:] == 0x5A5A5A5A).all()
    full = np.full((H, W), 255, np.uint8)
    np.testing.assert_array_equal(host[64:96].view(np.uint16).reshape(H, W), road_dist_ref(full, 127, 3))
    np.testing.assert_array_equal(host[16:32].reshape(2, 8), road_width_ref(nodes, edges, full, 127, 3))
    with pytest.raises(_lib.SrhError, match="radius"):
        ctx.check(dist(R=255), "srh_road_dist")
    with pytest.raises(_lib.SrhError, match="8-byte"):
        ctx.check(dist(d2_p=d2.data_ptr() + 4), "srh_road_dist")
    # the shim refuses on the host, with ValueError
    ops, m2 = _ops(), mask[:H * W].view(H, W)
    good = ops.road_dist(m2, radius=3)
    for fn in (lambda: ops.road_dist(m2, radius=0), lambda: ops.road_dist(m2, radius=255), lambda: ops.road_dist(m2, on_level=256), lambda: ops.road_dist(m2, on_level=0.5),
               lambda: ops.road_dist(m2.cpu()), lambda: ops.road_dist(m2.int()), lambda: ops.road_dist(np.ones((H, W), np.float32)), lambda: ops.road_dist(m2[:, ::2]),
               lambda: ops.graph_edge_widths(nodes, edit(edges, 1, 3), good), lambda: ops.graph_edge_widths(nodes, edges, good, radius=0),
               lambda: ops.graph_edge_widths(nodes, edges, good.cpu()), lambda: ops.graph_edge_widths(nodes, edges, m2), lambda: ops.graph_edge_widths(nodes, edges, good[:, ::2]),
               lambda: ops.graph_edge_widths(nodes, edges, good.cpu().numpy())):
        with pytest.raises(ValueError):
            fn()
    torch.cuda.synchronize()


# ---- 4. end to end ----------------------------------------------------------------------------------------------------------------------------------------
def test_apply_on_the_device_equals_apply_ref_with_and_without_each_condition():
    rng = np.random.default_rng(9)
    ops = _ops()
    nodes, edges = wk.grid_graph(260, 300)
    road = wk.shape_mask("bars", 4, 260, 300) | wk.random_mask(rng, 260, 300, 127, 0.05)
    result = (nodes, edges, np.zeros_like(road), road)
    st = road_width_ref(nodes, edges, road, 127, 32)
    assert ((st[:, 1] > 0) & (st[:, 1] < st[:, 0])).any()
    w_med = float(np.median([a["width_px"] for a in width_attrs(nodes, edges, st) if a["width_px"] is not None]))
    for extra in ({}, {"min_width": w_med}, {"max_width": w_med}, {"min_in": 0.5}, {"drop_isolated": True, "min_in": 0.5}, {"max_radius": 3, "on": 0.9},
                  {"min_width": 1, "max_width": w_med, "min_in": 0.2, "max_radius": 254}):
        key = road_width_key({"ROAD_WIDTH": dict({"max_radius": 32}, **extra)})
        (n1, e1, k1, r1), a1 = rw.apply(key, result, net=ops)
        (n2, e2, _, _), a2 = rw.apply_ref(key, result)
        assert np.array_equal(n1, n2) and np.array_equal(e1, e2) and a1 == a2 and k1 is result[2] and r1 is road, extra
        assert (0 < e1.shape[0] < edges.shape[0]) if rw.filters(key) else np.array_equal(e1, edges)


def _files(root):
    return sorted(os.path.relpath(os.path.join(d, f), root) for d, _, fs in os.walk(root) for f in fs)


def test_the_cli_end_to_end(pair, tmp_path, monkeypatch):
    """The CLI with --road-width --graph-geojson writes the GeoJSON whose every property is width_attrs of road_width_ref on the written
    masks, and leaves the pickle and the masks as they were; a run without the flag writes the files of a run in which the new code is
    out of the way, byte for byte."""
    from PIL import Image
    from sam_road_amd import Config
    from sam_road_amd import cli, inferencer as inf
    _, net = pair
    monkeypatch.chdir(tmp_path)
    H, W = 401, 523
    img = rect_scene(H, W, 43)
    Image.fromarray(img).save("rgb.png")
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        base = dict(CFG, INFER_PATCHES_PER_EDGE=4)
        _, _, kp0, road0 = inf.infer_one_img(net, img, Config(base))
        cfg = dict(base, **thresholds(kp0, road0))
        plain = run_cli(cli, net, tmp_path, monkeypatch, "plain", cfg, ["rgb.png"], "--device", "cuda")["rgb"]
        with monkeypatch.context() as mp:
            def never(*a, **k):
                raise AssertionError("the new code ran")
            mp.setattr(cli, "road_width_key", lambda *a, **k: None)
            mp.setattr(cli, "apply_road_width", never)
            run_cli(cli, net, tmp_path, mp, "bypassed", cfg, ["rgb.png"], "--device", "cuda")
        got = run_cli(cli, net, tmp_path, monkeypatch, "width", cfg, ["rgb.png"], "--device", "cuda", "--road-width", "--graph-geojson")["rgb"]
    plain_files = ["config.yaml", "graph/rgb.p", "inference_time.txt", "mask/rgb_itsc.png", "mask/rgb_road.png"]
    assert _files("save/plain") == _files("save/bypassed") == plain_files and _files("save/width") == sorted(plain_files + ["graph_geojson/rgb.geojson"])
    for f in plain_files:
        if f != "inference_time.txt":
            assert open(f"save/plain/{f}", "rb").read() == open(f"save/bypassed/{f}", "rb").read(), f
    for f in ("graph/rgb.p", "mask/rgb_itsc.png", "mask/rgb_road.png"):                             # attributes only: nothing is filtered
        assert open(f"save/width/{f}", "rb").read() == open(f"save/plain/{f}", "rb").read(), f
    road = got[1]
    res = next(iter(inf.infer_imgs(net, iter([img]), Config(cfg), device=torch.device("cuda"))))      # the loop the CLI runs
    nodes, edges = res[0], res[1]
    assert edges.shape[0] > 5 and got[2] == convert_to_sat2graph_format(nodes, edges) and np.array_equal(res[3], road)
    level = int(np.floor(cfg["ROAD_THRESHOLD"] * 255))
    st = road_width_ref(nodes, edges, road, level, 32)
    assert (st[:, 1] > 0).any()
    want = width_attrs(nodes, edges, st)
    doc = json.load(open("save/width/graph_geojson/rgb.geojson"))
    assert len(doc["features"]) == edges.shape[0]
    for k, (f, a) in enumerate(zip(doc["features"], want)):
        assert f["properties"] == dict({"edge": k}, **a), k                                        # each property, exactly
    assert doc == json.loads(json.dumps(graph_geojson(nodes, edges, want)))
