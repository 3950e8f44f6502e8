"""GRAPH_RASTER (the road graph rasterised on the device) on the HIP path.  Run on an MI355X: pytest -m gpu.

The reference draws with cv2 on the host and its bytes are not reproduced, so the behaviour is pinned by the rule: the class map must equal
graph_raster_ref byte for byte at every shape at which the kernels' addressing can go wrong, the composition and the comparison must
equal numpy's, and the CLI's files must be the host composition of the graph the run returned.  There is no tolerance anywhere."""
import json
import os
import pickle
import warnings

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import graph_raster_kit as gk
from scene_kit import CFG, pair, rect_scene, run_cli, thresholds  # noqa: F401

from sam_road_amd.graph_raster import (MAX_SPAN, compare_graphs, compare_ref, composite_ref, graph_mask_ref, graph_raster_ref, rasterize_graph,
                                       read_gt_graph, render_mask, render_viz)

GUARD = 64
STYLES = ((1, "none", 0), (2, "square", 1), (4, "disc", 4), (10, "square", 127), (255, "disc", 0), (4, "disc", 127), (1, "square", 0), (2, "disc", 1),
          (10, "none", 4), (255, "square", 4))            # every t of {1, 2, 4, 10, 255} and every r of {0, 1, 4, 127} with both marks, and none


def _ops():
    from sam_road_amd.model import DeviceGraphOps
    return DeviceGraphOps("cuda")


def _guarded(n, offset=1):
    """(buffer of 0xA5, its view of n bytes that starts GUARD + offset bytes in): out at an odd offset inside a larger tensor."""
    buf = torch.full((n + 2 * GUARD + 16,), 0xA5, dtype=torch.uint8, device="cuda")
    return buf, buf[GUARD + offset:GUARD + offset + n]


def _guards_ok(buf, off, n):
    b = buf.cpu().numpy()
    return (b[:GUARD + off] == 0xA5).all() and (b[GUARD + off + n:] == 0xA5).all()


def _raster(shape, nodes, edges, t, mark, r, off=1, values=(1, 2)):
    H, W = shape
    buf, out = _guarded(H * W, off)
    got = _ops().graph_raster(shape, nodes, edges, t, mark, r, values=values, out=out)
    assert got.data_ptr() == out.data_ptr()
    assert _guards_ok(buf, off, H * W)                    # the other bytes of the larger tensor are unchanged
    return out.cpu().numpy().reshape(H, W)


# ---- 1. srh_graph_raster against the reference --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(1, 1), (37, 53), (64, 64), (300, 517)])
def test_raster_equals_the_reference(shape):
    """Random graphs with zero-length edges and edges wholly or partly outside the image, every style, out at the offsets 1, 2, 3, 4 (mod 4:
    every alignment) between 0xA5 guards."""
    H, W = shape
    rng = np.random.default_rng(H * 1000 + W)
    nodes, edges = gk.random_graph(rng, H, W, 40, 60, margin=max(20, H // 3), zero_length=4)
    far = np.array([[-50, -60], [-20, -300], [H + 30, W + 5], [H + 200, W + 90], [H // 2, -40], [H // 2 + 3, W + 40]])      # two edges wholly outside, one across
    nodes = np.concatenate([nodes, far])
    edges = np.concatenate([edges, [[40, 41], [42, 43], [44, 45]]])
    partial = 0
    for k, (t, mark, r) in enumerate(STYLES):
        want = graph_raster_ref(nodes, edges, shape, t, mark, r)
        np.testing.assert_array_equal(_raster(shape, nodes, edges, t, mark, r, off=1 + (k & 3)), want, err_msg=f"{shape} t {t} {mark} {r}")
        partial += 0 < (want != 0).sum() < H * W
    assert partial >= (5 if H > 1 else 0)                 # neither all nor nothing: a kernel that ignores the graph cannot pass
    # other class bytes (the mask product), E = 0, N = 0
    np.testing.assert_array_equal(_raster(shape, nodes, edges, 6, "square", 3, values=(255, 255)), graph_mask_ref(nodes, edges, shape, 3))
    np.testing.assert_array_equal(_raster(shape, nodes, [], 4, "disc", 4), graph_raster_ref(nodes, [], shape, 4, "disc", 4))
    assert not _raster(shape, [], [], 4, "disc", 4).any()
    assert not _raster(shape, nodes, edges[-3:-1], 4, "none", 0).any()                    # only the edges wholly outside
    # a float node array is truncated toward zero
    np.testing.assert_array_equal(_raster(shape, nodes + 0.75, edges, 2, "disc", 1), graph_raster_ref(np.trunc(nodes + 0.75), edges, shape, 2, "disc", 1))


def test_raster_a_star_of_500_edges_and_a_maximum_span_edge():
    # many writers on the pixels around one node
    nodes, edges = gk.star(64, 64, 500)
    for t, mark, r in ((1, "none", 0), (4, "disc", 4)):
        want = graph_raster_ref(nodes, edges, (64, 64), t, mark, r)
        assert 0 < (want == 1).sum() < 64 * 64
        np.testing.assert_array_equal(_raster((64, 64), nodes, edges, t, mark, r), want)
    # a maximum-span edge on a 2 x 16384 image, along it and from corner to corner; and one across a tall image
    S = MAX_SPAN
    for shape, nd in (((2, 16384), [[0, 0], [0, S]]), ((2, 16384), [[1, S], [0, 0]]), ((2, 16384), [[-7000, 3], [S - 7000, S + 3]]), ((16384, 2), [[0, 1], [S, 0]])):
        for t, mark, r in ((1, "square", 1), (4, "disc", 4), (255, "none", 0)):
            want = graph_raster_ref(nd, [[0, 1]], shape, t, mark, r)
            assert (want != 0).any()
            np.testing.assert_array_equal(_raster(shape, nd, [[0, 1]], t, mark, r, off=3), want, err_msg=f"{shape} {nd} t {t}")
    # the module's functions: a device tensor, the mask product
    nodes, edges = gk.grid_graph(120, 150)
    got = rasterize_graph(nodes, edges, (120, 150), 4, "disc", 4, device="cuda")
    assert got.is_cuda and got.dtype == torch.uint8
    np.testing.assert_array_equal(got.cpu().numpy(), graph_raster_ref(nodes, edges, (120, 150), 4, "disc", 4))
    np.testing.assert_array_equal(render_mask(nodes, edges, (120, 150), 5, device="cuda").cpu().numpy(), graph_mask_ref(nodes, edges, (120, 150), 5))


# ---- 2. srh_graph_composite -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(1, 1), (37, 53), (64, 64), (300, 517)])
def test_composite_equals_numpy(shape):
    H, W = shape
    rng = np.random.default_rng(H + W)
    nodes, edges = gk.random_graph(rng, H, W, 30, 40)
    cls = graph_raster_ref(nodes, edges, shape, 4, "disc", 4)
    img = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    ops = _ops()
    for off in (0, 1, 2, 3):                              # the class map, the image and the output at every alignment: words and bytes
        cbuf, cview = _guarded(H * W, off)
        cview.copy_(torch.from_numpy(cls).cuda().reshape(-1))
        ibuf, iview = _guarded(3 * H * W, off)
        iview.copy_(torch.from_numpy(img).cuda().reshape(-1))
        for with_img in (True, False):
            obuf, oview = _guarded(3 * H * W, off)
            got = ops.graph_composite(cview.view(H, W), iview.view(H, W, 3) if with_img else None, (253, 160, 15), (255, 255, 0), (1, 2, 3), out=oview.view(H, W, 3))
            assert got.data_ptr() == oview.data_ptr() and _guards_ok(obuf, off, 3 * H * W)
            np.testing.assert_array_equal(got.cpu().numpy(), composite_ref(cls, img if with_img else None, (253, 160, 15), (255, 255, 0), (1, 2, 3)), err_msg=f"off {off} img {with_img}")
        np.testing.assert_array_equal(cbuf.cpu().numpy()[GUARD + off:GUARD + off + H * W], cls.reshape(-1))          # the inputs are not written
        np.testing.assert_array_equal(ibuf.cpu().numpy()[GUARD + off:GUARD + off + 3 * H * W], img.reshape(-1))
    # render_viz: the reference's defaults, from a numpy scene
    np.testing.assert_array_equal(render_viz(img, nodes, edges, device="cuda").cpu().numpy(), composite_ref(cls, img))
    np.testing.assert_array_equal(render_viz(None, nodes, edges, shape=shape, device="cuda").cpu().numpy(), composite_ref(cls))


# ---- 3. srh_graph_compare ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(1, 1), (37, 53), (64, 64), (300, 517)])
def test_compare_equals_numpy(shape):
    H, W = shape
    rng = np.random.default_rng(3 * H + W)
    pred, gt = gk.random_graph(rng, H, W, 30, 40), gk.random_graph(rng, H, W, 30, 40)
    img = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    valid = (rng.integers(0, 4, (H, W)) * 60).astype(np.uint8)
    maps = [graph_mask_ref(*g, shape, r) for g, r in ((pred, 1), (pred, 3), (gt, 1), (gt, 3))]
    ops = _ops()
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    for with_valid in (False, True):
        for with_img in (False, True):
            counts, image = ops.graph_compare(*[dev(m) for m in maps], valid=dev(valid) if with_valid else None, img=dev(img) if with_img else None, diff=True)
            want_counts, want_image = gk.np_compare(*maps, valid if with_valid else None, img if with_img else None)
            assert counts.dtype == torch.int64 and counts.is_cuda and counts.cpu().tolist() == want_counts, (with_valid, with_img)
            np.testing.assert_array_equal(image.cpu().numpy(), want_image)
        counts, image = ops.graph_compare(*[dev(m) for m in maps], valid=dev(valid != 0) if with_valid else None)      # a bool mask, no image
        assert image is None and counts.cpu().tolist() == gk.np_compare(*maps, valid if with_valid else None)[0]
    # unaligned maps take the byte path
    views = []
    for m in maps:
        _, v = _guarded(H * W, 3)
        v.copy_(dev(m).reshape(-1))
        views.append(v.view(H, W))
    counts, image = ops.graph_compare(*views, diff=True)
    want_counts, want_image = gk.np_compare(*maps)
    assert counts.cpu().tolist() == want_counts
    np.testing.assert_array_equal(image.cpu().numpy(), want_image)
    # compare_graphs: the product from the two graphs; a graph against itself has nothing to report
    for v, im in ((None, None), (valid, img)):
        m, image = compare_graphs(pred, gt, shape, 1, 3, valid=v, img=im, device="cuda")
        want_m, want_image = compare_ref(pred, gt, shape, 1, 3, valid=v, img=im)
        assert m == want_m and (image is None) == (im is None)
        if im is not None:
            np.testing.assert_array_equal(image.cpu().numpy(), want_image)
    m, image = compare_graphs(pred, pred, shape, 2, 2, diff=True, device="cuda")
    assert m["n_fp"] == m["n_missed"] == 0 and m["n_pred"] == m["n_gt"] == (graph_mask_ref(*pred, shape, 2) != 0).sum() and not image.any()
    assert m["precision"] == m["recall"] == (1.0 if m["n_pred"] else None)


# ---- 4. the launch contract -------------------------------------------------------------------------------------------------------------------------------
def _launches(ctx, fn):
    ctx.profile_read()
    ctx.profile_enable(True)
    try:
        out = fn()
        torch.cuda.synchronize()
        return out, {r["name"]: r["launches"] for r in ctx.profile_read() if r["launches"]}
    finally:
        ctx.profile_enable(False)


def test_launch_contract(pair):
    from sam_road_amd import Config, _lib
    from sam_road_amd.inferencer import infer_one_img
    _, net = pair
    img = rect_scene(401, 523, 43)
    ctx = _lib.Context.get(torch.cuda.current_device())
    ecfg = dict(CFG, INFER_PATCHES_PER_EDGE=4)

    def run(cfg):
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            return infer_one_img(net, img, Config(cfg))

    # a run without the key calls none of the three; nor does one with it: the render is a separate step applied to a result
    res, base = _launches(ctx, lambda: run(ecfg))
    assert base and not [k for k in base if k.startswith("graph_")]
    _, keyed = _launches(ctx, lambda: run(dict(ecfg, GRAPH_RASTER={"viz": True, "mask": 3, "diff": True})))
    assert keyed == base
    # the launches of the three entries: clear always, edges with E > 0, nodes with N > 0 and a mark
    nodes, edges = gk.grid_graph(100, 100)
    _, rows = _launches(ctx, lambda: net.graph_raster((100, 100), nodes, edges, 4, "disc", 4))
    assert rows == {"graph_clear": 1, "graph_edges": 1, "graph_nodes": 1}
    _, rows = _launches(ctx, lambda: net.graph_raster((100, 100), nodes, edges, 4, "none", 4))
    assert rows == {"graph_clear": 1, "graph_edges": 1}
    _, rows = _launches(ctx, lambda: net.graph_raster((100, 100), nodes, [], 4, "square", 4))
    assert rows == {"graph_clear": 1, "graph_nodes": 1}
    _, rows = _launches(ctx, lambda: net.graph_raster((100, 100), [], [], 4, "square", 4))
    assert rows == {"graph_clear": 1}
    cls = net.graph_raster((100, 100), nodes, edges, 4, "disc", 4)
    _, rows = _launches(ctx, lambda: net.graph_composite(cls))
    assert rows == {"graph_composite": 1}
    _, rows = _launches(ctx, lambda: net.graph_compare(cls, cls, cls, cls, diff=True))
    assert rows == {"graph_counts_zero": 1, "graph_compare": 1}


def test_entries_reject_bad_arguments_and_launch_nothing():
    import ctypes
    from sam_road_amd import _lib
    ctx = _lib.Context.get(torch.cuda.current_device())
    lib, s = ctx.lib, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    H = W = 8
    buf, out = _guarded(3 * H * W, 1)
    nodes = np.array([[1, 1], [6, 5], [3, 7]], np.int32)
    edges = np.array([[0, 1], [1, 2]], np.int32)

    def edit(a, i, v):
        a = a.copy()
        a.reshape(-1)[i] = v
        return a

    def raster(n=nodes, e=edges, N=None, E=None, H=H, W=W, t=4, mark=2, r=4, ev=1, nv=2, out_p=out.data_ptr(), n_host=True, n_dev=True, e_host=True, e_dev=True, dev_off=0):
        nh, eh = torch.from_numpy(np.ascontiguousarray(n)), torch.from_numpy(np.ascontiguousarray(e))
        nd, ed = nh.cuda(), eh.cuda()
        return lib.srh_graph_raster(ctx.handle, nh.data_ptr() if n_host else None, nd.data_ptr() + dev_off if n_dev else None, n.shape[0] if N is None else N,
                                    eh.data_ptr() if e_host else None, ed.data_ptr() if e_dev else None, e.shape[0] if E is None else E, H, W, t, mark, r, ev, nv, out_p, s)

    S = MAX_SPAN
    bad = (dict(n_host=False), dict(n_dev=False), dict(e_host=False), dict(e_dev=False), dict(out_p=None), dict(N=-1), dict(E=-1), dict(H=0), dict(W=0), dict(H=-3),
           dict(H=65536, W=32768), dict(t=0), dict(t=256), dict(mark=-1), dict(mark=3), dict(r=-1), dict(r=128), dict(ev=0), dict(ev=256), dict(nv=0), dict(nv=256),
           dict(dev_off=2), dict(e=edit(edges, 1, 3)), dict(e=edit(edges, 2, -1)), dict(n=edit(nodes, 0, 2 ** 28 + 1)), dict(n=edit(nodes, 5, -2 ** 28 - 1)),
           dict(n=edit(nodes, 2, 1 + S + 1)), dict(n=edit(nodes, 3, 1 - S - 1)), dict(N=0))
    for kw in bad:
        assert raster(**kw) == -1, kw
    assert lib.srh_graph_raster(None, None, None, 0, None, None, 0, H, W, 4, 0, 0, 1, 2, out.data_ptr(), s) == -1

    cls = torch.ones(H * W, dtype=torch.uint8, device="cuda")
    img = torch.ones(3 * H * W, dtype=torch.uint8, device="cuda")
    col = lambda *v: (ctypes.c_int32 * 3)(*v)
    black, c1, c2 = col(0, 0, 0), col(253, 160, 15), col(255, 255, 0)

    def composite(cls_p=cls.data_ptr(), img_p=img.data_ptr(), H=H, W=W, bg=black, e=c1, n=c2, out_p=out.data_ptr()):
        return lib.srh_graph_composite(ctx.handle, cls_p, img_p, H, W, bg, e, n, out_p, s)

    for kw in (dict(cls_p=None), dict(out_p=None), dict(H=0), dict(W=-1), dict(H=65536, W=32768), dict(bg=None), dict(e=None), dict(n=None), dict(e=col(256, 0, 0)),
               dict(n=col(0, -1, 0)), dict(bg=col(0, 0, 300)), dict(cls_p=out.data_ptr() + 5), dict(img_p=out.data_ptr() + 64), dict(img_p=out.data_ptr() - 100)):
        assert composite(**kw) == -1, kw
    assert lib.srh_graph_composite(None, cls.data_ptr(), None, H, W, black, c1, c2, out.data_ptr(), s) == -1

    counts = torch.full((5,), 0x5A5A5A5A, dtype=torch.int64, device="cuda")
    maps = [torch.ones(H * W, dtype=torch.uint8, device="cuda") for _ in range(4)]

    def compare(m=None, valid_p=None, img_p=None, H=H, W=W, counts_p=counts.data_ptr(), diff_p=out.data_ptr()):
        m = [t.data_ptr() for t in maps] if m is None else m
        return lib.srh_graph_compare(ctx.handle, *m, valid_p, img_p, H, W, counts_p, diff_p, s)

    ptrs = [t.data_ptr() for t in maps]
    for kw in ([dict(m=ptrs[:k] + [None] + ptrs[k + 1:]) for k in range(4)] +
               [dict(counts_p=None), dict(counts_p=counts.data_ptr() + 4), dict(H=0), dict(W=0), dict(H=65536, W=32768), dict(m=[out.data_ptr() + 8] + ptrs[1:]),
                dict(valid_p=out.data_ptr() + 100), dict(img_p=out.data_ptr()), dict(m=ptrs[:3] + [counts.data_ptr()], diff_p=None), dict(diff_p=counts.data_ptr() - 8 * 20)]):
        assert compare(**kw) == -1, kw
    assert lib.srh_graph_compare(None, *ptrs, None, None, H, W, counts.data_ptr(), None, s) == -1
    torch.cuda.synchronize()
    assert (buf.cpu().numpy() == 0xA5).all() and (counts.cpu().numpy() == 0x5A5A5A5A).all()      # nothing was launched: the outputs are unchanged
    # and the good calls run
    assert raster() == 0 and raster(N=0, E=0, n_host=False, n_dev=False, e_host=False, e_dev=False) == 0 and composite() == 0 and composite(img_p=None) == 0
    assert compare() == 0 and compare(diff_p=None, valid_p=cls.data_ptr(), img_p=img.data_ptr()) == 0
    torch.cuda.synchronize()
    assert _guards_ok(buf, 1, 3 * H * W) and counts.cpu().tolist()[:4] == [H * W, 0, H * W, 0] and counts.cpu().tolist()[4] == 0x5A5A5A5A
    with pytest.raises(_lib.SrhError, match="inconsistent table"):
        ctx.check(raster(e=edit(edges, 1, 3)), "srh_graph_raster")
    # the shim refuses on the host, with ValueError
    ops = _ops()
    for call in (lambda: ops.graph_raster((0, 5), nodes, edges, 4), lambda: ops.graph_raster((8, 8), nodes, edit(edges, 1, 3), 4), lambda: ops.graph_raster((8, 8), nodes, edges, 0),
                 lambda: ops.graph_raster((8, 8), nodes, edges, 4, "circle"), lambda: ops.graph_raster((8, 8), nodes, edges, 4, "disc", 128),
                 lambda: ops.graph_raster((8, 8), nodes, edges, 4, values=(0, 2)), lambda: ops.graph_raster((8, 8), nodes, edges, 4, out=out[:10]),
                 lambda: ops.graph_composite(cls.view(8, 8), img.view(8, 8, 3)[:4]), lambda: ops.graph_composite(cls.view(8, 8), None, (1, 2, 256)),
                 lambda: ops.graph_composite(cls.cpu().view(8, 8)), lambda: ops.graph_compare(cls.view(8, 8), cls.view(8, 8), cls.view(8, 8), cls.view(4, 16))):
        with pytest.raises(ValueError):
            call()
    torch.cuda.synchronize()


# ---- 5. the CLI, end to end -------------------------------------------------------------------------------------------------------------------------------
def _files(root):
    return sorted(os.path.relpath(os.path.join(d, f), root) for d, _, fs in os.walk(root) for f in fs)


def test_cli_end_to_end(pair, tmp_path, monkeypatch):
    """--viz --graph-mask 3 --diff --gt-graphs on the kit's tiny model: the PNGs decode to the host composition of the graph the run wrote,
    metrics.json holds the numpy counts; the same under SCENE_SCALE [1, 2] and SCENE_PAD, where the renders are in the scene's own frame; and
    the same run without the flags writes exactly the files it wrote before, with the same bytes."""
    from PIL import Image
    from sam_road_amd import Config
    from sam_road_amd import cli, inferencer as inf
    from sam_road_amd.formats import convert_to_sat2graph_format
    _, net = pair
    monkeypatch.chdir(tmp_path)
    flags = ("--device", "cuda", "--viz", "--graph-mask", "3", "--diff", "--gt-graphs", "gt.p")
    for name, (H, W), extra in (("plain", (401, 523), {}), ("framed", (600, 640), dict(SCENE_SCALE=[1, 2], SCENE_PAD=24))):
        img = rect_scene(H, W, 43)
        Image.fromarray(img).save("rgb.png")
        gt = gk.grid_graph(H, W, step=70, jitter=20, seed=9)
        gt[0][0] = (-15, 30)                                                          # a ground-truth node outside the scene
        with open("gt.p", "wb") as f:
            pickle.dump(convert_to_sat2graph_format(*gt), f)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            base = dict(CFG, INFER_PATCHES_PER_EDGE=4, **extra)
            _, _, kp0, road0 = inf.infer_one_img(net, img, Config(base))
            cfg = dict(base, **thresholds(kp0, road0))
            before = run_cli(cli, net, tmp_path, monkeypatch, f"{name}_before", cfg, ["rgb.png"], "--device", "cuda")["rgb"]
            got = run_cli(cli, net, tmp_path, monkeypatch, name, cfg, ["rgb.png"], *flags)["rgb"]
        plain_files = ["config.yaml", "graph/rgb.p", "inference_time.txt", "mask/rgb_itsc.png", "mask/rgb_road.png"]
        assert _files(f"save/{name}_before") == plain_files
        assert _files(f"save/{name}") == sorted(plain_files + ["viz/rgb.png", "graph_mask/rgb.png", "diff/rgb.png", "diff/metrics.json"])
        for f in plain_files[1:2] + plain_files[3:]:                                  # the run itself is the run it was: the same bytes
            assert open(f"save/{name}/{f}", "rb").read() == open(f"save/{name}_before/{f}", "rb").read(), f
        assert got[2] == before[2] and got[0].shape == (H, W)
        nodes, edges = read_gt_graph(f"save/{name}/graph/rgb.p")
        assert nodes.shape[0] > 5 and edges.shape[0] > 0 and nodes[:, 0].max() >= H // 2 + 1       # the scene's frame, beyond the model frame of a scaled scene
        cls = graph_raster_ref(nodes, edges, (H, W), 4, "disc", 4)
        np.testing.assert_array_equal(np.array(Image.open(f"save/{name}/viz/rgb.png")), composite_ref(cls, img))
        np.testing.assert_array_equal(np.array(Image.open(f"save/{name}/graph_mask/rgb.png")), graph_mask_ref(nodes, edges, (H, W), 3))
        m, image = compare_ref((nodes, edges), gt, (H, W), 1, 5, img=img)
        np.testing.assert_array_equal(np.array(Image.open(f"save/{name}/diff/rgb.png")), image)
        report = json.load(open(f"save/{name}/diff/metrics.json"))
        assert report == {"thin": 1, "wide": 5, "scenes": {"rgb": m}, "total": m} and m["n_gt"] > 0 and m["n_pred"] > 0
