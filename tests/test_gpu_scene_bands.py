"""SCENE_BANDS (16-bit and multi-band scenes) on the HIP path.  Run on an MI355X: pytest -m gpu.

Nothing here has a tolerance.  The apply kernel must equal LUT[b][src[..., select[b]]] byte for byte and the histogram np.bincount count
for count; a run with the key on a raw scene must equal, bit for bit, the existing pipeline on the scene converted with numpy and the
tables of sam_road_amd/radiometry.py (np.percentile where the key asks for a percentile).
"""
import ctypes
import warnings

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from scene_kit import CFG, assert_abi_11, kernel_rows, make_mask, rect_scene
from scene_kit import net_for as _net_for
from scene_kit import same_bits as _same
from scene_kit import thresholds as _thresholds
from test_scene_bands_host import expected_tables, raw_scene

P = CFG["PATCH_SIZE"]
SELECT = [2, 0, 3]
SHAPES = [(37, 53), (401, 523), (3, 6000), (1, 1)]
CS = (1, 3, 4, 5, 16)
DTYPES = {np.uint8: (torch.uint8, 256, (1, 3)), np.uint16: (torch.uint16, 65536, (2, 6))}      # torch dtype, levels, byte offsets of the source view


def _selections(C):
    perm = [C - 1, 0, C // 2]                            # a permutation where C >= 3, repeats below
    return [perm, [0, 0, 0]]


def _view_at(arr, off):
    """arr on the device as a view at byte offset `off` of a larger allocation filled with 0xA5: (the big u8 tensor, the view)."""
    t_dtype = DTYPES[arr.dtype.type][0]
    big = torch.full((arr.nbytes + 16,), 0xA5, dtype=torch.uint8, device="cuda")
    v = big[off:off + arr.nbytes].view(t_dtype).view(arr.shape)
    v.copy_(torch.from_numpy(arr))
    assert v.data_ptr() == big.data_ptr() + off
    return big, v


# ---- 1. the apply kernel ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=[f"{h}x{w}" for h, w in SHAPES])
def test_apply_equals_the_numpy_gather(shape):
    from sam_road_amd.radiometry import band_luts
    net = _net_for(P)
    dev = torch.device("cuda")
    ctx, _ = net._weights(dev)
    H, W = shape
    rng = np.random.default_rng(H * 1000 + W)
    for np_dtype, (t_dtype, levels, offsets) in DTYPES.items():
        luts = [rng.integers(0, 256, size=(3, levels), dtype=np.uint8), band_luts([(3, levels - 7), (0, levels - 1), (levels // 3, levels // 2)], 2.2, levels)]
        for C in CS:
            src = rng.integers(0, levels, size=(H, W, C), dtype=np_dtype)
            for k, sel in enumerate(_selections(C)):
                lut = luts[k]
                lut_d = torch.from_numpy(lut).cuda()
                want = np.stack([lut[b][src[..., sel[b]]] for b in range(3)], -1)
                big, v = _view_at(src, offsets[k])
                before = big.cpu().numpy().copy()
                out = net.scene_bands_apply(v, sel, lut_d)
                assert out.dtype == torch.uint8 and tuple(out.shape) == (H, W, 3)
                np.testing.assert_array_equal(out.cpu().numpy(), want, err_msg=f"{np_dtype.__name__} C {C} select {sel}")
                np.testing.assert_array_equal(big.cpu().numpy(), before)         # the source (and the bytes around it) are untouched
                # dst at an odd address inside guard bytes: the C entry itself
                for dst_off in (0, 5, 15):
                    guard = torch.full((3 * H * W + 48,), 0x5A, dtype=torch.uint8, device=dev)
                    sel_c = (ctypes.c_int32 * 3)(*sel)
                    rc = ctx.lib.srh_scene_bands_apply(ctx.handle, v.data_ptr(), 2 if np_dtype is np.uint8 else 5, H * W, C, sel_c, lut_d.data_ptr(),
                                                       guard.data_ptr() + 16 + dst_off, net._stream(dev))
                    assert rc == 0
                    g = guard.cpu().numpy()
                    np.testing.assert_array_equal(g[16 + dst_off:16 + dst_off + 3 * H * W], want.reshape(-1))
                    assert (g[:16 + dst_off] == 0x5A).all() and (g[16 + dst_off + 3 * H * W:] == 0x5A).all()


@pytest.mark.parametrize("gamma", [1, 2.2])
def test_apply_on_every_level(gamma):
    """256 x 256 scenes that hold every one of the 65536 (256) values in every selected band: the judge of anything that computes instead of
    gathering, and of every table entry."""
    from sam_road_amd.radiometry import band_luts
    net = _net_for(P)
    rng = np.random.default_rng(11)
    for np_dtype, (t_dtype, levels, _) in DTYPES.items():
        src = np.stack([rng.permutation(65536) % levels for _ in range(4)], -1).reshape(256, 256, 4).astype(np_dtype)
        for ranges in ([(0, levels - 1)] * 3, [(levels // 64, levels // 3), (1, levels - 2), (levels - 2, levels - 1)]):
            lut = band_luts(ranges, gamma, levels)
            for sel in ([3, 1, 0], [2, 2, 2]):
                assert all(np.array_equal(np.sort(src[..., s].reshape(-1))[::65536 // levels], np.arange(levels)) for s in sel)
                out = net.scene_bands_apply(torch.from_numpy(src).cuda(), sel, torch.from_numpy(lut).cuda())
                np.testing.assert_array_equal(out.cpu().numpy(), np.stack([lut[b][src[..., sel[b]]] for b in range(3)], -1))


# ---- 2. the histogram ---------------------------------------------------------------------------------------------------------------------
def _hist_data(kind, np_dtype, H, W, C, rng):
    levels = 256 if np_dtype is np.uint8 else 65536
    if kind == "uniform":
        return rng.integers(0, levels, size=(H, W, C), dtype=np_dtype)
    if kind == "constant":                               # the worst contention: every pixel adds to the same three counters
        return np.full((H, W, C), levels - 3, np_dtype)
    return rng.integers(levels // 400, levels // 16, size=(H, W, C), dtype=np_dtype)            # "narrow": 12-bit data in a u16 container


@pytest.mark.parametrize("shape", SHAPES + [(256, 256)], ids=[f"{h}x{w}" for h, w in SHAPES + [(256, 256)]])
def test_hist_equals_bincount(shape):
    net = _net_for(P)
    dev = torch.device("cuda")
    ctx, _ = net._weights(dev)
    H, W = shape
    rng = np.random.default_rng(H * 7 + W)
    mask = rng.random((H, W)) < 0.6
    for np_dtype, (t_dtype, levels, offsets) in DTYPES.items():
        for C in (1, 4, 16):
            for kind in ("uniform", "constant", "narrow"):
                src = _hist_data(kind, np_dtype, H, W, C, rng)
                sel = _selections(C)[0]
                _, v = _view_at(src, offsets[1])
                for valid in (None, mask, (mask * 200).astype(np.uint8)):
                    keep = np.ones((H, W), bool) if valid is None else valid != 0
                    want = np.stack([np.bincount(src[..., b][keep], minlength=levels) for b in sel])
                    hist = net.scene_bands_hist(v, sel, None if valid is None else torch.from_numpy(valid).cuda())
                    assert hist.dtype == torch.uint32 and tuple(hist.shape) == (3, levels)
                    got = hist.cpu().numpy().astype(np.int64)
                    np.testing.assert_array_equal(got, want, err_msg=f"{np_dtype.__name__} C {C} {kind} mask {valid is not None}")
                    assert (got.sum(axis=1) == int(keep.sum())).all()
                # a second call into the same buffer, which holds garbage: the call zeroes it itself
                buf = torch.full((3 * levels + 8,), 0x7F7F7F7F, dtype=torch.int32, device=dev)
                sel_c = (ctypes.c_int32 * 3)(*sel)
                want = np.stack([np.bincount(src[..., b].reshape(-1), minlength=levels) for b in sel]).reshape(-1)
                for _ in range(2):
                    rc = ctx.lib.srh_scene_bands_hist(ctx.handle, v.data_ptr(), 2 if np_dtype is np.uint8 else 5, H * W, C, sel_c, None,
                                                      buf.data_ptr() + 16, net._stream(dev))
                    assert rc == 0
                    b = buf.cpu().numpy()
                    np.testing.assert_array_equal(b[4:4 + 3 * levels], want)
                    assert (b[:4] == 0x7F7F7F7F).all() and (b[4 + 3 * levels:] == 0x7F7F7F7F).all()


def test_bad_arguments_are_refused():
    from sam_road_amd import _lib
    net = _net_for(P)
    dev = torch.device("cuda")
    ctx, _ = net._weights(dev)
    buf = torch.zeros(1 << 20, dtype=torch.uint8, device=dev)
    p, s, lib = buf.data_ptr(), net._stream(dev), ctx.lib
    src, lut, dst, hist = p, p + 4096, p + (1 << 18), p + (1 << 19)
    sel = (ctypes.c_int32 * 3)(0, 1, 2)
    assert lib.srh_scene_bands_apply(ctx.handle, src, 2, 64, 3, sel, lut, dst, s) == 0
    assert lib.srh_scene_bands_hist(ctx.handle, src, 2, 64, 3, sel, None, hist, s) == 0
    assert lib.srh_scene_bands_hist(ctx.handle, src, 2, 64, 3, sel, src, hist, s) == 0
    for dtype, n, C, select in ((0, 64, 3, (0, 1, 2)), (1, 64, 3, (0, 1, 2)), (3, 64, 3, (0, 1, 2)), (4, 64, 3, (0, 1, 2)), (6, 64, 3, (0, 1, 2)),
                                (2, 64, 0, (0, 0, 0)), (2, 64, 17, (0, 1, 2)), (5, 64, -1, (0, 1, 2)), (2, 64, 3, (0, 1, 3)), (2, 64, 3, (-1, 1, 2)),
                                (5, 64, 1, (0, 0, 1)), (2, 0, 3, (0, 1, 2)), (2, -5, 3, (0, 1, 2)), (5, 2 ** 31, 3, (0, 1, 2))):
        bad = (ctypes.c_int32 * 3)(*select)
        assert lib.srh_scene_bands_apply(ctx.handle, src, dtype, n, C, bad, lut, dst, s) == -1, (dtype, n, C, select)
        assert lib.srh_scene_bands_hist(ctx.handle, src, dtype, n, C, bad, None, hist, s) == -1, (dtype, n, C, select)
    assert lib.srh_scene_bands_apply(ctx.handle, src + 1, 5, 64, 3, sel, lut, dst, s) == -1          # a u16 source is 2-byte aligned
    assert lib.srh_scene_bands_hist(ctx.handle, src + 1, 5, 64, 3, sel, None, hist, s) == -1
    for args in ((None, 2, 64, 3, sel, lut, dst), (src, 2, 64, 3, None, lut, dst), (src, 2, 64, 3, sel, None, dst), (src, 2, 64, 3, sel, lut, None)):
        assert lib.srh_scene_bands_apply(ctx.handle, *args, s) == -1
    for args in ((None, 2, 64, 3, sel, None, hist), (src, 2, 64, 3, None, None, hist), (src, 2, 64, 3, sel, None, None)):
        assert lib.srh_scene_bands_hist(ctx.handle, *args, s) == -1
    with pytest.raises(_lib.SrhError):
        ctx.check(lib.srh_scene_bands_apply(ctx.handle, src, 2, 64, 17, sel, lut, dst, s), "srh_scene_bands_apply")
    with pytest.raises(_lib.SrhError):
        ctx.check(lib.srh_scene_bands_hist(ctx.handle, src, 7, 64, 3, sel, None, hist, s), "srh_scene_bands_hist")
    raw = torch.zeros((8, 8, 4), dtype=torch.uint16, device=dev)
    lut16 = torch.zeros((3, 65536), dtype=torch.uint8, device=dev)
    for bad_src in (raw.float(), raw[:, ::2], torch.zeros((8, 8, 17), dtype=torch.uint8, device=dev)):
        with pytest.raises(ValueError):
            net.scene_bands_apply(bad_src, [0, 1, 2], lut16)
        with pytest.raises(ValueError):
            net.scene_bands_hist(bad_src, [0, 1, 2])
    with pytest.raises(ValueError):
        net.scene_bands_apply(raw, [0, 1, 4], lut16)
    with pytest.raises(ValueError):
        net.scene_bands_apply(raw, [0, 1, 2], lut16[:, :256].contiguous())       # the u8 table for a u16 scene
    with pytest.raises(ValueError):
        net.scene_bands_hist(raw, [0, 1, 2], torch.ones((8, 7), dtype=torch.uint8, device=dev))
    torch.cuda.synchronize()


def test_abi_has_the_entries_and_stays_11():
    assert_abi_11([("srh_scene_bands_hist", 9), ("srh_scene_bands_apply", 9)])


# ---- 3. the contract: a run with the key == the existing pipeline on the numpy-converted scene ----------------------------------------------
H0, W0, PER_EDGE, SEED = 401, 523, 4, 43


def _contract(raw, key, valid=None, extra=None):
    """infer_one_img(raw, cfg + SCENE_BANDS) == infer_one_img(converted, cfg) bit for bit — nodes, edges, both masks — with converted =
    the tables of the definition (numpy) gathered with numpy.  The thresholds are percentiles of the converted run's own masks, so the
    graph is never empty: at least 30 nodes and 1 edge are asserted on the run WITHOUT the key."""
    from sam_road_amd import Config
    from sam_road_amd.inferencer import infer_one_img
    from sam_road_amd.radiometry import apply_luts
    net = _net_for(P)
    tables = expected_tables(raw, key, valid)
    converted = np.ascontiguousarray(apply_luts(raw, key["select"], tables))
    kw = {} if valid is None else dict(valid=valid)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        base = Config(dict(CFG, INFER_PATCHES_PER_EDGE=PER_EDGE, **(extra or {})))
        _, _, kp0, road0 = infer_one_img(net, converted, base, **kw)
        plain = Config(dict(base, **_thresholds(kp0, road0)))
        want = infer_one_img(net, converted, plain, **kw)
        raw_before = raw.copy()
        got = infer_one_img(net, raw, Config(dict(plain, SCENE_BANDS=key)), **kw)
    np.testing.assert_array_equal(raw, raw_before)
    print(key, extra, "nodes", want[0].shape[0], "edges", want[1].shape[0])
    assert want[0].shape[0] >= 30 and want[1].shape[0] >= 1
    for a, b in zip(got, want):
        _same(a, b)
    return got, converted, plain


def test_contract_fixed_full_range_is_the_stock_scene():
    u8 = rect_scene(H0, W0, SEED)
    _, converted, _ = _contract(raw_scene(u8), {"select": SELECT, "stretch": [0, 65535]})
    np.testing.assert_array_equal(converted, u8)                                  # 257 v -> v


def test_contract_fixed_narrow_range():
    u8 = rect_scene(H0, W0, SEED)
    _, converted, _ = _contract(raw_scene(u8), {"select": SELECT, "stretch": [[6000, 60000], [4000, 58000], [5000, 62000]], "gamma": 1.4})
    assert not np.array_equal(converted, u8)


def test_contract_percentile_and_the_kernels_that_run():
    from sam_road_amd import Config, _lib
    from sam_road_amd.inferencer import infer_one_img
    u8 = rect_scene(H0, W0, SEED)
    raw = raw_scene(u8)
    key = {"select": SELECT, "stretch": {"percentile": [2, 98]}}
    _, converted, plain = _contract(raw, key)
    assert not np.array_equal(converted, u8)
    net = _net_for(P)
    ctx = _lib.Context.get(torch.cuda.current_device())
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        with kernel_rows(ctx) as rows:
            infer_one_img(net, raw, Config(dict(plain, SCENE_BANDS=key)))
            rows_pct = rows()
            infer_one_img(net, raw, Config(dict(plain, SCENE_BANDS={"select": SELECT})))
            rows_fixed = rows()
            infer_one_img(net, converted, plain)
            rows_plain = rows()
    assert not {"scene_bands_hist", "scene_bands_apply"} & rows_plain
    assert rows_pct == rows_plain | {"scene_bands_hist", "scene_bands_apply"} and rows_fixed == rows_plain | {"scene_bands_apply"}


def test_contract_percentile_with_a_mask():
    """The invalid region holds 65535 in every band: a histogram that ignored the mask would give other tables."""
    u8 = rect_scene(H0, W0, SEED)
    valid = make_mask("hole", H0, W0)
    raw = raw_scene(u8)
    raw[~valid] = 65535
    key = {"select": SELECT, "stretch": {"percentile": [2, 99]}}
    assert not np.array_equal(expected_tables(raw, key, valid), expected_tables(raw, key))
    got, _, plain = _contract(raw, key, valid=valid)
    assert not got[2][~valid].any() and not got[3][~valid].any()
    # the software-pipelined loop fetches the histogram over its upload lane: the same tuples
    from sam_road_amd import Config
    from sam_road_amd.inferencer import infer_imgs
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for res in infer_imgs(_net_for(P), iter([raw, raw]), Config(dict(plain, SCENE_BANDS=key)), valids=iter([valid, valid])):
            for a, b in zip(res, got):
                _same(a, b)


def test_contract_composed_with_pad_window_and_tta():
    u8 = rect_scene(H0, W0, SEED)
    _contract(raw_scene(u8), {"select": SELECT, "stretch": {"percentile": [1, 99]}, "gamma": 1.2},
              extra=dict(SCENE_PAD={"border": 24, "mode": "reflect"}, FUSE_WINDOW="hann", TTA=["id", "rot90"]))


def test_contract_group_of_three_chips():
    """infer_imgs(group=3) on three raw chips of different sizes == the same grouped loop on the numpy-converted chips (the same tile
    batches on both sides, so bit for bit): one apply launch over the group's ragged buffer precedes the unchanged pack kernel."""
    from sam_road_amd import Config, _lib
    from sam_road_amd.inferencer import infer_imgs, infer_one_img
    from sam_road_amd.radiometry import apply_luts
    net = _net_for(P)
    key = {"select": SELECT, "stretch": [3000, 62000]}
    chips_u8 = [rect_scene(300, 340, 51), rect_scene(401, 523, 43), rect_scene(290, 411, 52)]
    raws = [raw_scene(c, seed=7 + i) for i, c in enumerate(chips_u8)]
    converted = [np.ascontiguousarray(apply_luts(r, SELECT, expected_tables(r, key))) for r in raws]
    ctx = _lib.Context.get(torch.cuda.current_device())
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        base = Config(dict(CFG, INFER_PATCHES_PER_EDGE=2))
        _, _, kp0, road0 = infer_one_img(net, converted[1], base)
        plain = Config(dict(base, **_thresholds(kp0, road0)))
        want = list(infer_imgs(net, iter(converted), plain, group=3))
        with kernel_rows(ctx) as rows:
            got = list(infer_imgs(net, iter(raws), Config(dict(plain, SCENE_BANDS=key)), group=3))
            names = rows()
    assert {"scene_bands_apply", "scene_group_pack"} <= names and "scene_bands_hist" not in names
    assert len(got) == len(want) == 3
    print("nodes / edges per chip:", [(w[0].shape[0], w[1].shape[0]) for w in want])
    assert want[1][0].shape[0] >= 30 and want[1][1].shape[0] >= 1
    for w, g in zip(want, got):
        for a, b in zip(g, w):
            _same(a, b)
