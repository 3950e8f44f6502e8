"""GEOTIFF (GeoTIFF scenes decoded on the device) on the HIP path.  Run on an MI355X: pytest -m gpu.

srh_tiff_assemble must equal tiff_read_ref bit for bit — floats as bit patterns — at every shape at which the kernel's addressing can go
wrong, and the guard bytes around its output must come back unchanged.  There is no tolerance anywhere."""
import ctypes
import warnings

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import geotiff_kit as gk
from scene_kit import CFG, kernel_rows, rect_scene, thresholds
from scene_kit import net_for as _net_for
from test_scene_bands_host import SELECT, raw_scene
from test_scene_float_host import reflectance

from sam_road_amd import _lib
from sam_road_amd import geotiff as gt

GUARD = 32                                                # bytes on either side of the raster: it stays 16-byte aligned
CH = gk.CHUNK
assert CH == 4096                                         # the kernel's row chunk (TIF_CHUNK): the wide shapes are built around it
P = CFG["PATCH_SIZE"]
STRIP_SHAPES = [(1, 1), (1, 70), (70, 1), (37, 53), (3, CH - 1), (2, CH + 1), (2, 2 * CH + 3)]
TILE_SHAPES = [(37, 53), (16, 16)]
TILES = [(16, 16), (32, 16)]
LAYOUTS = [("strips", s, r) for s in STRIP_SHAPES for r in (1, 5, "H")] + [("tiles", s, t) for s in TILE_SHAPES for t in TILES]
# C x sample type x predictor x planar configuration x byte order
FORMATS = [(C, d, p, planar, be) for C in (1, 3, 4, 16) for d, preds in (("uint8", (1, 2)), ("uint16", (1, 2)), ("float32", (1, 3))) for p in preds
           for planar in (1, 2) for be in (False, True)]
T_DTYPE = {"uint8": (torch.uint8, _lib.SRH_U8), "uint16": (torch.uint16, _lib.SRH_U16), "float32": (torch.float32, _lib.SRH_F32)}


def _ctx():
    return _lib.Context.get(torch.cuda.current_device())


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _launch(sc, flat, table):
    """srh_tiff_assemble itself, the raster between guard bytes of 0xA5 inside a larger tensor: (return code, the whole buffer on the
    device, the raster's bytes)."""
    ctx = _ctx()
    H, W, C = sc.shape
    n = H * W * C * sc.dtype.itemsize
    buf = torch.full((2 * GUARD + n,), 0xA5, dtype=torch.uint8, device="cuda")
    ptr = buf.data_ptr() + GUARD
    flat_d, t_h = torch.from_numpy(flat).cuda(), torch.from_numpy(table)
    t_d = t_h.cuda()
    assert flat_d.data_ptr() % 16 == 0
    rc = ctx.lib.srh_tiff_assemble(ctx.handle, flat_d.data_ptr(), flat_d.numel(), t_h.data_ptr(), t_d.data_ptr(), table.shape[0], ptr, H, W, C,
                                   T_DTYPE[str(sc.dtype)][1], sc.predictor, 0 if sc.little else 1, _stream())
    return rc, buf, n, (flat_d, t_d)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8).reshape(-1)


@pytest.mark.parametrize("layout", LAYOUTS, ids=[f"{k}-{s[0]}x{s[1]}-{v if not isinstance(v, tuple) else f'{v[0]}x{v[1]}'}" for k, s, v in LAYOUTS])
def test_assemble_equals_the_reference(tmp_path, layout):
    """Every C x sample type x predictor x planar configuration x byte order at this shape and layout; the launches are queued and read
    back after ONE wait.  Float data holds NaNs (two payloads), +-inf, -0.0 and denormals."""
    kind, (H, W), v = layout
    kw = dict(tile=v) if kind == "tiles" else dict(rows_per_strip=H if v == "H" else v)
    queued = []
    for i, (C, dtype, pred, planar, be) in enumerate(FORMATS):
        a = gk.sample((H, W, C), dtype, 1000 * H + W + i)
        p = gk.write_tiff(str(tmp_path / "t.tif"), a, predictor=pred, planar=planar, big_endian=be, **kw)
        sc = gt.open_scene(p)
        want = gt.tiff_read_ref(sc)
        flat, table = sc.segments()
        if sc.is_raster:                                      # nothing to launch: the flat array is the raster
            assert np.array_equal(_bits(flat), _bits(want))
            flat, table = sc.segments(aligned=True)           # and the launch does the same file all the same
        rc, buf, n, keep = _launch(sc, flat, table)
        assert rc == 0, (C, dtype, pred, planar, be)
        queued.append((buf, n, want, keep, (C, dtype, pred, planar, be)))
    torch.cuda.synchronize()
    for buf, n, want, _, what in queued:
        host = buf.cpu().numpy()
        assert (host[:GUARD] == 0xA5).all() and (host[GUARD + n:] == 0xA5).all(), what      # nothing else is written
        assert np.array_equal(host[GUARD:GUARD + n], _bits(want)), what
    if (H, W) == (37, 53) and kind == "tiles":
        assert any(np.isnan(w).any() for _, _, w, _, f in queued if f[1] == "float32")


def test_bad_arguments_are_refused_and_nothing_is_written(tmp_path):
    a = gk.sample((37, 53, 3), "uint16", 1)
    sc = gt.open_scene(gk.write_tiff(str(tmp_path / "t.tif"), a, tile=(16, 16), predictor=2))
    flat, table = sc.segments()
    ctx = _ctx()
    bad_tables = []
    for col, val in ((0, 8), (0, flat.size), (1, 10), (2, 37), (2, -1), (3, 53), (4, 0), (5, 0), (6, 3), (6, -2)):
        t = table.copy()
        t[1, col] = val
        bad_tables.append(t)
    for t in bad_tables:
        rc, buf, n, _ = _launch(sc, flat, t)
        torch.cuda.synchronize()
        assert rc == -1 and (buf.cpu().numpy() == 0xA5).all(), t[1]
    H, W, C = sc.shape
    out = torch.full((H * W * C,), 7, dtype=torch.uint16, device="cuda")
    flat_d, t_h = torch.from_numpy(flat).cuda(), torch.from_numpy(table)
    t_d = t_h.cuda()
    call = lambda **k: ctx.lib.srh_tiff_assemble(ctx.handle, k.get("flat", flat_d.data_ptr()), k.get("nflat", flat_d.numel()), t_h.data_ptr(), t_d.data_ptr(), k.get("n", table.shape[0]),
                                                 k.get("out", out.data_ptr()), k.get("H", H), W, k.get("C", C), k.get("dtype", _lib.SRH_U16), k.get("pred", 2), k.get("be", 0), _stream())
    for k in (dict(flat=None), dict(out=None), dict(n=0), dict(H=0), dict(C=17), dict(C=0), dict(dtype=_lib.SRH_F16), dict(pred=3), dict(pred=0), dict(be=2),
              dict(dtype=_lib.SRH_F32, pred=2), dict(flat=flat_d.data_ptr() + 8), dict(out=out.data_ptr() + 1), dict(out=flat_d.data_ptr()), dict(nflat=flat.size - 1)):
        assert call(**k) == -1, k
    torch.cuda.synchronize()
    assert (out == 7).all()
    assert call() == 0
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy().reshape(a.shape), a)


def test_fast_path_launches_nothing(tmp_path):
    from sam_road_amd import inferencer as inf
    net = _net_for(P)
    ctx = _ctx()
    a = gk.sample((37, 53, 4), "uint16", 3)
    io = inf._BlockingIO(torch.device("cuda"))
    with kernel_rows(ctx) as rows:
        got = inf._upload_scene(net, io, gt.open_scene(gk.write_tiff(str(tmp_path / "fast.tif"), a, rows_per_strip=5)))
        assert "tiff_assemble" not in rows()
        assert got.dtype == torch.uint16 and np.array_equal(got.cpu().numpy(), a)
        for kw in (dict(big_endian=True), dict(tile=(16, 16)), dict(planar=2), dict(predictor=2), dict(compression="deflate"), dict(compression="lzw", predictor=2, tile=(16, 32))):
            got = inf._upload_scene(net, io, gt.open_scene(gk.write_tiff(str(tmp_path / "slow.tif"), a, **kw)))
            assert rows() == {"tiff_assemble"}, kw
            assert np.array_equal(got.cpu().numpy(), a), kw
        f = gk.sample((37, 53, 2), "float32", 3)
        got = inf._upload_scene(net, io, gt.open_scene(gk.write_tiff(str(tmp_path / "f.tif"), f, compression="deflate", predictor=3, tile=(16, 16))))
        assert rows() == {"tiff_assemble"} and gk.same_bits(got.cpu().numpy(), f)
        got = inf._upload_scene(net, io, a)                   # an array goes as it always went
        assert not rows() and np.array_equal(got.cpu().numpy(), a)


# ---- end to end on the real model ---------------------------------------------------------------------------------------------------------
H0, W0, PER_EDGE, SEED = 300, 340, 2, 43
E2E = {"uint8": (lambda u8: u8, dict(compression="deflate", predictor=2, tile=(64, 48)), {}),
       "uint16": (raw_scene, dict(compression="lzw", predictor=2, planar=2, big_endian=True, rows_per_strip=64), dict(SCENE_BANDS={"select": SELECT, "stretch": {"percentile": [2, 98]}})),
       "float32": (reflectance, dict(compression="deflate", predictor=3, tile=(32, 64)), dict(SCENE_FLOAT={"select": SELECT, "stretch": [0.0, 1.0]}))}


@pytest.mark.parametrize("dtype", sorted(E2E))
def test_end_to_end_key_equals_the_run_on_the_reference_array(tmp_path, dtype):
    from sam_road_amd import Config
    from sam_road_amd.inferencer import infer_imgs, infer_one_img
    make, kw, keys = E2E[dtype]
    arr = make(rect_scene(H0, W0, SEED))
    p = gk.write_tiff(str(tmp_path / "a.tif"), arr, geo=gk.GEO, **kw)
    ref = gt.tiff_read_ref(p)
    assert gk.same_bits(ref, arr) and str(ref.dtype) == dtype
    net = _net_for(P)
    ctx = _ctx()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        base = Config(dict(CFG, INFER_PATCHES_PER_EDGE=PER_EDGE, **keys))
        _, _, kp0, road0 = infer_one_img(net, ref, base)
        plain = Config(dict(base, **thresholds(kp0, road0)))
        want = infer_one_img(net, ref, plain)
        with kernel_rows(ctx) as rows:
            got = infer_one_img(net, gt.open_scene(p), Config(dict(plain, GEOTIFF=True)))
            assert "tiff_assemble" in rows()
        piped = list(infer_imgs(net, iter([gt.open_scene(p).load(4), gt.open_scene(p)]), Config(dict(plain, GEOTIFF=True))))
    print(dtype, "nodes", want[0].shape[0], "edges", want[1].shape[0])
    assert want[0].shape[0] >= 30 and want[1].shape[0] >= 1
    for res in [got] + piped:
        assert len(res) == 4
        for a, b in zip(res, want):
            assert a.dtype == b.dtype and np.array_equal(a, b)
