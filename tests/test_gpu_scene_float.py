"""SCENE_FLOAT (float32 scenes quantised exactly on the device) on the HIP path.  Run on an MI355X: pytest -m gpu.

Nothing here has a tolerance.  The valid kernel must equal rule 1 of sam_road_amd/float_scene.py byte for byte, the apply kernel
np.searchsorted on the ordered keys (0 on invalid pixels) byte for byte, both histogram passes np.bincount count for count; a run with the
key on a float scene must equal, bit for bit, embeddings included, the existing pipeline on float_scene_ref's uint8 scene and mask.
"""
import ctypes
import warnings

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from sam_road_amd import float_scene as fs

from scene_kit import CFG, assert_abi_11, kernel_rows, rect_scene
from scene_kit import net_for as _net_for
from scene_kit import same_bits as _same
from scene_kit import thresholds as _thresholds

P = CFG["PATCH_SIZE"]
SELECT = [2, 0, 3]
SHAPES = [(1, 1), (3, 6000), (37, 53), (401, 523)]
CS = (1, 3, 5, 16)
F32 = np.float32
INF32 = F32(np.inf)
NODATA = F32(-9999)
ROWS = {"scene_float_valid", "scene_float_hist", "scene_float_apply"}


def _selections(C):
    return [[C - 1, 0, C // 2], [0, 0, 0]]               # a permutation where C >= 3, and repeats


def _tables():
    """The threshold tables the op tests use: from float_thresholds (a wide range, one across zero with gamma, the collapsed one)."""
    lo = F32(0.75)
    key = fs.as_key({"stretch": [0, 1], "gamma": 2.2})
    return fs.float_thresholds([(F32(-3), F32(3)), (F32(-1e-38), F32(2e-38)), (lo, np.nextafter(lo, INF32))], key)


def _data(H, W, C, rng, T):
    """Random floats with NaN, +-inf, +-0, denormals, the nodata value, and every threshold of T with both of its neighbours planted."""
    x = (rng.normal(size=(H, W, C)) * 2).astype(F32)
    flat = x.reshape(-1)
    special = np.concatenate([F32([np.nan, -np.nan, np.inf, -np.inf, 0.0, -0.0, 1e-45, -1e-45, 5e-39, -5e-39, 1.1754942e-38, NODATA, 3.4028235e38]),
                              T.reshape(-1), np.nextafter(T.reshape(-1), -INF32), np.nextafter(T.reshape(-1), INF32)])
    n = min(flat.size, max(1, flat.size // 3))
    flat[rng.choice(flat.size, n, replace=False)] = rng.choice(special, n)
    return x


def _view_at(arr, off):
    """arr on the device as a view at byte offset `off` of a larger allocation filled with 0xA5: (the big u8 tensor, the view)."""
    big = torch.full((arr.nbytes + 32,), 0xA5, dtype=torch.uint8, device="cuda")
    v = big[off:off + arr.nbytes].view(torch.float32).view(arr.shape)
    v.view(torch.int32).copy_(torch.from_numpy(arr.view(np.int32)))               # bit patterns, NaN payloads included
    assert v.data_ptr() == big.data_ptr() + off
    return big, v


def _levels(src, sel, tk, valid):
    k = fs.float_keys(src)
    out = np.stack([np.searchsorted(tk[b, :255], k[..., sel[b]], side="right") for b in range(3)], -1).astype(np.uint8)
    out[valid == 0] = 0
    return out


# ---- 1. the valid and the apply kernel -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=[f"{h}x{w}" for h, w in SHAPES])
def test_valid_and_apply_equal_the_rule(shape):
    net = _net_for(P)
    dev = torch.device("cuda")
    ctx, _ = net._weights(dev)
    H, W = shape
    n = H * W
    rng = np.random.default_rng(H * 1000 + W)
    T = _tables()
    random_tk = np.sort(rng.integers(0, 2 ** 32, size=(3, 256), dtype=np.uint64).astype(np.uint32), axis=1)
    random_tk[:, 255] = 0xffffffff
    tables = [fs.threshold_keys(T), random_tk]
    caller = (rng.random((H, W)) < 0.7).astype(np.uint8) * 200
    caller_d = torch.from_numpy(caller).cuda()
    for C in CS:
        src = _data(H, W, C, rng, T)
        for k, sel in enumerate(_selections(C)):
            big, v = _view_at(src, (4, 12)[k])
            before = big.cpu().numpy().copy()
            key = fs.as_key({"select": sel, "stretch": [0.5, 1], "nodata": [float(NODATA), 0.0][:1 + k], "transfer": ("linear", "log")[k]})
            valid_in = None if k == 0 else caller
            want_valid = fs.float_valid_ref(src, key, valid_in)
            got_valid = net.scene_float_valid(v, sel, [int(x) for x in fs.nodata_keys(key)], key.log, None if valid_in is None else caller_d)
            assert got_valid.dtype == torch.uint8 and tuple(got_valid.shape) == (H, W)
            np.testing.assert_array_equal(got_valid.cpu().numpy(), want_valid, err_msg=f"valid C {C} select {sel}")
            tk = tables[k]
            tk_d = torch.from_numpy(tk).cuda()
            mask = want_valid if k == 0 else caller                               # the apply kernel takes any mask: non-zero = valid
            mask_d = torch.from_numpy(mask).cuda()
            want = _levels(src, sel, tk, mask)
            out = net.scene_float_apply(v, sel, mask_d, tk_d)
            assert out.dtype == torch.uint8 and tuple(out.shape) == (H, W, 3)
            np.testing.assert_array_equal(out.cpu().numpy(), want, err_msg=f"apply C {C} select {sel}")
            # the outputs at odd addresses inside guard bytes: the C entries themselves
            sel_c = (ctypes.c_int32 * 3)(*sel)
            nd = [int(x) for x in fs.nodata_keys(key)]
            nd_c = (ctypes.c_uint32 * len(nd))(*nd)
            for dst_off in (0, 5, 15):
                guard = torch.full((3 * n + 48,), 0x5A, dtype=torch.uint8, device=dev)
                assert ctx.lib.srh_scene_float_apply(ctx.handle, v.data_ptr(), n, C, sel_c, mask_d.data_ptr(), tk_d.data_ptr(), guard.data_ptr() + 16 + dst_off,
                                                     net._stream(dev)) == 0
                g = guard.cpu().numpy()
                np.testing.assert_array_equal(g[16 + dst_off:16 + dst_off + 3 * n], want.reshape(-1))
                assert (g[:16 + dst_off] == 0x5A).all() and (g[16 + dst_off + 3 * n:] == 0x5A).all()
            for out_off in (0, 3):
                guard = torch.full((n + 48,), 0x5A, dtype=torch.uint8, device=dev)
                assert ctx.lib.srh_scene_float_valid(ctx.handle, v.data_ptr(), n, C, sel_c, nd_c, len(nd), 1 if key.log else 0,
                                                     None if valid_in is None else caller_d.data_ptr(), guard.data_ptr() + 16 + out_off,
                                                     net._stream(dev)) == 0
                g = guard.cpu().numpy()
                np.testing.assert_array_equal(g[16 + out_off:16 + out_off + n], want_valid.reshape(-1))
                assert (g[:16 + out_off] == 0x5A).all() and (g[16 + out_off + n:] == 0x5A).all()
            np.testing.assert_array_equal(big.cpu().numpy(), before)              # the source (and the bytes around it) are untouched


def test_apply_at_and_around_every_threshold():
    """Every threshold of three tables and both float32 neighbours, in every band: the levels of float_thresholds' own searchsorted."""
    net = _net_for(P)
    for gamma, ranges, transfer in ((1, [(0, 1), (-25, 0), (100, 4000)], "linear"), (2.2, [(0.02, 0.35), (0, 1), (1e-3, 10)], "linear"),
                                    (0.5, [(0.02, 0.35), (1, 2), (1e-3, 10)], "log")):
        key = fs.as_key({"stretch": [list(q) for q in ranges], "gamma": gamma, "transfer": transfer})
        T = fs.float_thresholds(key.ranges, key)
        x = np.concatenate([T.reshape(-1), np.nextafter(T.reshape(-1), -INF32), np.nextafter(T.reshape(-1), INF32)])
        src = np.stack([x, x[::-1], np.roll(x, 7)], -1).reshape(1, -1, 3).copy()
        valid = np.ones(src.shape[:2], np.uint8)
        want = np.stack([np.searchsorted(T[b], src[..., b], side="right") for b in range(3)], -1).astype(np.uint8)
        out = net.scene_float_apply(torch.from_numpy(src).cuda(), [0, 1, 2], torch.from_numpy(valid).cuda(), torch.from_numpy(fs.threshold_keys(T)).cuda())
        np.testing.assert_array_equal(out.cpu().numpy(), want)


# ---- 2. the histograms ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=[f"{h}x{w}" for h, w in SHAPES])
def test_hist_pass_1_equals_bincount(shape):
    net = _net_for(P)
    H, W = shape
    rng = np.random.default_rng(H * 7 + W)
    T = _tables()
    mask = (rng.random((H, W)) < 0.6).astype(np.uint8) * 3
    for C in CS:
        src = _data(H, W, C, rng, T)
        for k, sel in enumerate(_selections(C)):
            _, v = _view_at(src, (4, 12)[k])
            for valid in (np.ones((H, W), np.uint8), mask):
                keys = fs.float_keys(src)[valid != 0]
                want = np.stack([np.bincount(keys[:, b] >> 16, minlength=65536) for b in sel])
                hist = net.scene_float_hist(v, sel, torch.from_numpy(valid).cuda())
                assert hist.dtype == torch.uint32 and tuple(hist.shape) == (3, 65536)
                got = hist.cpu().numpy().astype(np.int64)
                np.testing.assert_array_equal(got, want, err_msg=f"C {C} select {sel}")
                assert (got.sum(axis=1) == int((valid != 0).sum())).all()


def test_hist_pass_2_target_sets():
    net = _net_for(P)
    dev = torch.device("cuda")
    ctx, _ = net._weights(dev)
    rng = np.random.default_rng(3)
    H, W, C = 37, 53, 5
    src = (rng.normal(size=(H, W, C)) * 0.01 + 1.0).astype(F32)                   # few top-16-bit buckets, many low halves
    src[rng.random((H, W, C)) < 0.1] = np.nan                                     # counted all the same: the mask decides, not the value
    valid = (rng.random((H, W)) < 0.7).astype(np.uint8)
    keys = fs.float_keys(src)
    top = keys >> 16
    common = [int(v) for v in np.argsort(np.bincount(top.reshape(-1)))[::-1][:3]]
    absent = next(v for v in range(65536) if not (top == v).any())
    sets = {"one band, two prefixes": [(1, common[0]), (1, common[1])],
            "a prefix no pixel has": [(0, common[0]), (2, absent)],
            "six targets": [(0, common[0]), (0, common[1]), (3, common[0]), (4, common[2]), (4, common[0]), (2, common[1])],
            "one target": [(4, common[0])]}
    _, v = _view_at(src, 12)
    for name, targets in sets.items():
        want = np.stack([np.bincount(keys[..., b][(valid != 0) & (top[..., b] == pre)] & 0xffff, minlength=65536) for b, pre in targets])
        hist = net.scene_float_hist(v, [0, 1, 2], torch.from_numpy(valid).cuda(), targets)
        assert hist.dtype == torch.uint32 and tuple(hist.shape) == (len(targets), 65536)
        np.testing.assert_array_equal(hist.cpu().numpy().astype(np.int64), want, err_msg=name)
        if name == "a prefix no pixel has":
            assert not want[1].any() and want[0].any()
    # a second call into the same buffer, which holds garbage: the call zeroes its rows itself and nothing else
    targets = sets["one band, two prefixes"]
    want = np.stack([np.bincount(keys[..., b][(valid != 0) & (top[..., b] == pre)] & 0xffff, minlength=65536) for b, pre in targets]).reshape(-1)
    buf = torch.full((2 * 65536 + 8,), 0x7F7F7F7F, dtype=torch.int32, device=dev)
    tg = (ctypes.c_uint32 * 4)(*[x for t in targets for x in t])
    valid_d = torch.from_numpy(valid).cuda()
    for _ in range(2):
        assert ctx.lib.srh_scene_float_hist(ctx.handle, v.data_ptr(), H * W, C, (ctypes.c_int32 * 3)(0, 1, 2), valid_d.data_ptr(), tg, 2, buf.data_ptr() + 16,
                                            net._stream(dev)) == 0
        b = buf.cpu().numpy()
        np.testing.assert_array_equal(b[4:4 + 2 * 65536], want)
        assert (b[:4] == 0x7F7F7F7F).all() and (b[4 + 2 * 65536:] == 0x7F7F7F7F).all()
    # a constant scene at 3 x 6000: every add of a pass goes to one address per band
    const = np.full((3, 6000, 3), F32(0.3))
    ones = torch.ones((3, 6000), dtype=torch.uint8, device=dev)
    k0 = int(fs.float_keys(F32([0.3]))[0])
    h1 = net.scene_float_hist(torch.from_numpy(const).cuda(), [0, 1, 2], ones).cpu().numpy()
    assert (h1[:, k0 >> 16] == 18000).all() and h1.sum() == 3 * 18000
    h2 = net.scene_float_hist(torch.from_numpy(const).cuda(), [0, 1, 2], ones, [(0, k0 >> 16), (2, k0 >> 16), (1, (k0 >> 16) + 1)]).cpu().numpy()
    assert h2[0, k0 & 0xffff] == h2[1, k0 & 0xffff] == 18000 and h2.sum() == 2 * 18000
    # the whole radix select through the device's counts equals the sorted-index rule
    key = fs.as_key({"select": [1, 4, 1], "stretch": {"percentile": [2, 98]}})
    ok = fs.float_valid_ref(src, key, valid)
    ok_d = torch.from_numpy(ok).cuda()
    targets, picks = fs.float_hist_targets(net.scene_float_hist(v, key.select, ok_d).cpu().numpy(), key)
    got = fs.float_ranges_from_hists(targets, picks, net.scene_float_hist(v, key.select, ok_d, targets).cpu().numpy(), key)
    assert [(a.tobytes(), b.tobytes()) for a, b in got] == [(a.tobytes(), b.tobytes()) for a, b in fs.float_ranges_ref(src, key, valid)]


# ---- 3. refusals ---------------------------------------------------------------------------------------------------------------------------
def test_bad_arguments_are_refused_and_launch_nothing():
    from sam_road_amd import _lib
    net = _net_for(P)
    dev = torch.device("cuda")
    ctx, _ = net._weights(dev)
    buf = torch.zeros(1 << 22, dtype=torch.uint8, device=dev)                     # hist: six rows of 65536 counts behind the 2 MiB mark
    p, s, lib, h = buf.data_ptr(), net._stream(dev), ctx.lib, ctx.handle
    src, mask, thr, dst, vout, hist = p, p + 8192, p + 16384, p + (1 << 18), p + (1 << 19), p + (1 << 21)
    buf[16384:16384 + 3072].view(torch.int32).fill_(-1)
    sel = (ctypes.c_int32 * 3)(0, 1, 2)
    nd = (ctypes.c_uint32 * 4)(1, 2, 3, 4)
    tg = (ctypes.c_uint32 * 12)(0, 1, 1, 2, 2, 3, 0, 4, 1, 5, 2, 6)
    with kernel_rows(ctx) as rows:
        assert lib.srh_scene_float_valid(h, src, 64, 3, sel, nd, 4, 1, mask, vout, s) == 0
        assert lib.srh_scene_float_valid(h, src, 64, 3, sel, None, 0, 0, None, vout, s) == 0
        assert lib.srh_scene_float_hist(h, src, 64, 3, sel, mask, None, 0, hist, s) == 0
        assert lib.srh_scene_float_hist(h, src, 64, 3, sel, mask, tg, 6, hist, s) == 0
        assert lib.srh_scene_float_apply(h, src, 64, 3, sel, mask, thr, dst, s) == 0
        assert rows() >= ROWS
        for n, C, select in ((64, 0, (0, 0, 0)), (64, 17, (0, 1, 2)), (64, -1, (0, 1, 2)), (64, 3, (0, 1, 3)), (64, 3, (-1, 1, 2)), (64, 1, (0, 0, 1)),
                             (0, 3, (0, 1, 2)), (-5, 3, (0, 1, 2)), (2 ** 31, 3, (0, 1, 2))):
            bad = (ctypes.c_int32 * 3)(*select)
            assert lib.srh_scene_float_valid(h, src, n, C, bad, nd, 1, 0, None, vout, s) == -1, (n, C, select)
            assert lib.srh_scene_float_hist(h, src, n, C, bad, mask, None, 0, hist, s) == -1, (n, C, select)
            assert lib.srh_scene_float_apply(h, src, n, C, bad, mask, thr, dst, s) == -1, (n, C, select)
        for off in (1, 2, 3):                                                     # a source that is not 4-byte aligned
            assert lib.srh_scene_float_valid(h, src + off, 64, 3, sel, None, 0, 0, None, vout, s) == -1
            assert lib.srh_scene_float_hist(h, src + off, 64, 3, sel, mask, None, 0, hist, s) == -1
            assert lib.srh_scene_float_apply(h, src + off, 64, 3, sel, mask, thr, dst, s) == -1
        # null pointers, the optional ones excepted
        for args in ((None, 64, 3, sel, nd, 1, 0, None, vout), (src, 64, 3, None, nd, 1, 0, None, vout), (src, 64, 3, sel, None, 1, 0, None, vout),
                     (src, 64, 3, sel, nd, 1, 0, None, None)):
            assert lib.srh_scene_float_valid(h, *args, s) == -1
        for args in ((None, 64, 3, sel, mask, None, 0, hist), (src, 64, 3, None, mask, None, 0, hist), (src, 64, 3, sel, None, None, 0, hist),
                     (src, 64, 3, sel, mask, None, 0, None), (src, 64, 3, sel, mask, None, 2, hist), (src, 64, 3, sel, mask, tg, 0, hist)):
            assert lib.srh_scene_float_hist(h, *args, s) == -1
        for args in ((None, 64, 3, sel, mask, thr, dst), (src, 64, 3, None, mask, thr, dst), (src, 64, 3, sel, None, thr, dst), (src, 64, 3, sel, mask, None, dst),
                     (src, 64, 3, sel, mask, thr, None)):
            assert lib.srh_scene_float_apply(h, *args, s) == -1
        # more than 4 nodata keys, more than 6 targets, a target outside the bands or the prefixes, log outside 0 / 1, misaligned tables, overlaps
        assert lib.srh_scene_float_valid(h, src, 64, 3, sel, nd, 5, 0, None, vout, s) == -1
        assert lib.srh_scene_float_valid(h, src, 64, 3, sel, nd, -1, 0, None, vout, s) == -1
        assert lib.srh_scene_float_valid(h, src, 64, 3, sel, nd, 1, 2, None, vout, s) == -1
        assert lib.srh_scene_float_hist(h, src, 64, 3, sel, mask, tg, 7, hist, s) == -1
        assert lib.srh_scene_float_hist(h, src, 64, 3, sel, mask, (ctypes.c_uint32 * 2)(3, 0), 1, hist, s) == -1
        assert lib.srh_scene_float_hist(h, src, 64, 3, sel, mask, (ctypes.c_uint32 * 2)(0, 65536), 1, hist, s) == -1
        assert lib.srh_scene_float_hist(h, src, 64, 3, sel, mask, None, 0, hist + 2, s) == -1
        assert lib.srh_scene_float_apply(h, src, 64, 3, sel, mask, thr + 1, dst, s) == -1
        assert lib.srh_scene_float_apply(h, src, 64, 3, sel, mask, thr, src + 16, s) == -1
        assert lib.srh_scene_float_valid(h, src, 64, 3, sel, None, 0, 0, None, src + 700, s) == -1
        assert lib.srh_scene_float_valid(h, src, 64, 3, sel, None, 0, 0, mask, mask + 10, s) == -1
        assert lib.srh_scene_float_hist(h, src, 64, 3, sel, mask, None, 0, src + 256, s) == -1
        assert lib.srh_scene_float_hist(h, src, 64, 3, sel, mask, tg, 1, mask - 65536 * 4 + 8, s) == -1
        assert not rows() & ROWS                                                  # nothing of all that was launched
    with pytest.raises(_lib.SrhError):
        ctx.check(lib.srh_scene_float_apply(h, src, 64, 17, sel, mask, thr, dst, s), "srh_scene_float_apply")
    raw = torch.zeros((8, 8, 4), dtype=torch.float32, device=dev)
    ok = torch.ones((8, 8), dtype=torch.uint8, device=dev)
    thr_t = torch.from_numpy(np.full((3, 256), 0xffffffff, np.uint32)).cuda()
    for bad_src in (raw.double(), raw.half(), raw[:, ::2], torch.zeros((8, 8, 17), dtype=torch.float32, device=dev)):
        with pytest.raises(ValueError):
            net.scene_float_valid(bad_src, [0, 1, 2])
        with pytest.raises(ValueError):
            net.scene_float_hist(bad_src, [0, 1, 2], ok)
        with pytest.raises(ValueError):
            net.scene_float_apply(bad_src, [0, 1, 2], ok, thr_t)
    with pytest.raises(ValueError):
        net.scene_float_apply(raw, [0, 1, 4], ok, thr_t)
    with pytest.raises(ValueError):
        net.scene_float_apply(raw, [0, 1, 2], ok, torch.from_numpy(np.full((3, 255), 0xffffffff, np.uint32)).cuda())
    with pytest.raises(ValueError):
        net.scene_float_apply(raw, [0, 1, 2], ok[:, :7].contiguous(), thr_t)
    with pytest.raises(ValueError):
        net.scene_float_valid(raw, [0, 1, 2], [1, 2, 3, 4, 5])
    with pytest.raises(ValueError):
        net.scene_float_hist(raw, [0, 1, 2], ok, [(0, 1)] * 7)
    with pytest.raises(ValueError):
        net.scene_float_hist(raw, [0, 1, 2], ok, [(4, 1)])
    torch.cuda.synchronize()


def test_abi_has_the_entries_and_stays_11():
    assert_abi_11([("srh_scene_float_valid", 11), ("srh_scene_float_hist", 10), ("srh_scene_float_apply", 9)])


# ---- 4. the contract: a run with the key == the existing pipeline on float_scene_ref's outputs ------------------------------------------------
H0, W0, PER_EDGE, SEED = 401, 523, 4, 43


def reflectance(u8, select=SELECT, C=4, seed=1):
    """f32 [H,W,C]: band select[b] = channel b of the u8 scene / 255, noise elsewhere."""
    rng = np.random.default_rng(seed)
    raw = rng.normal(size=u8.shape[:2] + (C,)).astype(F32)
    for b, s in enumerate(select):
        raw[..., s] = u8[..., b].astype(F32) / F32(255)
    return raw


class _Embeddings:
    """Records what scene_pass1 returns: the embeddings are part of the contract."""

    def __init__(self, net):
        self.net, self.inner, self.seen = net, net.scene_pass1, []

    def __enter__(self):
        def pass1(*a, **kw):
            out = self.inner(*a, **kw)
            self.seen.append(out[2].detach().cpu().numpy().copy())
            return out
        self.net.scene_pass1 = pass1
        return self.seen

    def __exit__(self, *exc):
        del self.net.scene_pass1


def _contract(raw, key, valid=None, extra=None, aoi=None, least=30):
    """infer_one_img(raw, cfg + SCENE_FLOAT) == infer_one_img(float_scene_ref's scene, cfg, valid = float_scene_ref's mask) bit for bit —
    nodes, edges, both masks, the embeddings of pass 1.  The thresholds are percentiles of the converted run's own masks, so the graph is
    never empty."""
    from sam_road_amd import Config
    from sam_road_amd.aoi import aoi_ref, scene_aoi_key
    from sam_road_amd.inferencer import infer_one_img
    net = _net_for(P)
    area = valid if aoi is None else aoi_ref(raw.shape[:2], scene_aoi_key(Config(SCENE_AOI=aoi)), valid)
    u8, ok = fs.float_scene_ref(raw, key, area)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        base = Config(dict(CFG, INFER_PATCHES_PER_EDGE=PER_EDGE, **(extra or {})))
        _, _, kp0, road0 = infer_one_img(net, u8, base, valid=ok)
        plain = Config(dict(base, **_thresholds(kp0, road0)))
        with _Embeddings(net) as emb_want:
            want = infer_one_img(net, u8, plain, valid=ok)
        raw_before = raw.copy()
        keyed = Config(dict(plain, SCENE_FLOAT=key, **({} if aoi is None else dict(SCENE_AOI=aoi))))
        with _Embeddings(net) as emb_got:
            got = infer_one_img(net, raw, keyed, **({} if valid is None else dict(valid=valid)))
    assert np.array_equal(raw.view(np.uint32), raw_before.view(np.uint32))
    print(key, extra, "nodes", want[0].shape[0], "edges", want[1].shape[0], "valid", float(ok.mean()))
    assert want[0].shape[0] >= least and want[1].shape[0] >= 1
    for a, b in zip(got, want):
        _same(a, b)
    assert len(emb_got) == len(emb_want) == 1 and emb_want[0].size > 0
    _same(emb_got[0], emb_want[0])
    return got, u8, ok, plain, keyed


def test_contract_fixed_range_and_the_kernels_that_run():
    from sam_road_amd import Config, _lib
    from sam_road_amd.inferencer import infer_one_img
    u8 = rect_scene(H0, W0, SEED)
    raw = reflectance(u8)
    raw[350:, 400:, SELECT[2]] = np.nan
    got, conv, ok, plain, keyed = _contract(raw, {"select": SELECT, "stretch": [0, 1]})
    np.testing.assert_array_equal(conv[ok != 0], u8[ok != 0])                     # v / 255 under [0, 1] -> v
    assert not ok[350:, 400:].any() and ok[:350].all() and not got[3][350:, 400:].any()
    net = _net_for(P)
    ctx = _lib.Context.get(torch.cuda.current_device())
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        with kernel_rows(ctx) as rows:
            infer_one_img(net, raw, keyed)
            rows_fixed = rows()
            infer_one_img(net, raw, Config(dict(keyed, SCENE_FLOAT={"select": SELECT, "stretch": {"percentile": [2, 98]}})))
            rows_pct = rows()
            infer_one_img(net, conv, plain, valid=ok)
            rows_plain = rows()
            infer_one_img(net, conv, Config(dict(plain, SCENE_FLOAT=None)))
            infer_one_img(net, conv, Config(dict(plain, SCENE_FLOAT={})))
            rows_unmasked = rows()
    assert not ROWS & rows_plain and not ROWS & rows_unmasked                     # without the key no scene_float_* row appears
    assert rows_fixed == rows_plain | {"scene_float_valid", "scene_float_apply"} and rows_pct == rows_plain | ROWS


def test_contract_percentile_one_bucket_half_nan_and_constant():
    """Band 2: 1 + k 2^-23, all of it in ONE top-16-bit bucket (pass 2 does the whole selection); band 0: half NaN; band 3: constant (lo ==
    hi: the collapsed table)."""
    u8 = rect_scene(H0, W0, SEED)
    raw = reflectance(u8)
    raw[..., 2] = (F32(1.0).view(np.uint32) + u8[..., 0].astype(np.uint32) * np.uint32(16) + np.uint32(3)).view(F32)
    raw[:, W0 // 2:, 0] = np.nan
    raw[..., 3] = F32(0.3)
    key = {"select": SELECT, "stretch": {"percentile": [2, 98]}}
    assert len(np.unique(fs.float_keys(raw[..., 2]) >> 16)) == 1
    ranges = fs.float_ranges_ref(raw, key)
    assert ranges[2] == (F32(0.3), np.nextafter(F32(0.3), INF32)) and ranges[0][0] > 1 and ranges[0][1] < 1.001
    got, conv, ok, _, _ = _contract(raw, key, least=10)
    assert not ok[:, W0 // 2:].any() and ok[:, :W0 // 2].all() and not conv[..., 2].any() and len(np.unique(conv[..., 0])) > 20


def test_contract_with_scene_pad_scene_scale_tta_and_scene_aoi():
    u8 = rect_scene(H0, W0, SEED)
    raw = reflectance(u8)
    raw[100:130, 200:260] = NODATA
    aoi = {"include": [[[[20, 30], [380.5, 60], [390, 500.25], [40, 480]]]], "buffer": 2}
    _, _, ok, _, _ = _contract(raw, {"select": SELECT, "stretch": {"percentile": [2, 98]}, "gamma": 1.2, "nodata": float(NODATA)}, aoi=aoi, least=10,
                               extra=dict(SCENE_PAD=24, SCENE_SCALE=[3, 2], TTA=["id", "rot90"]))
    assert 0.3 < ok.mean() < 0.95 and not ok[100:130, 200:260].any()


def test_pipelined_loop_over_three_scenes():
    """infer_imgs fetches both histograms over its upload lane: the tuples of infer_one_img, for three scenes of different shapes and band
    counts, with a caller's mask on one of them."""
    from sam_road_amd import Config
    from sam_road_amd.inferencer import infer_imgs, infer_one_img
    net = _net_for(P)
    a = reflectance(rect_scene(H0, W0, SEED))
    b = reflectance(rect_scene(300, 340, 51), C=5, seed=2)
    c = reflectance(rect_scene(290, 411, 52), C=16, seed=3)
    b[:50] = np.inf
    valid_c = np.ones(c.shape[:2], np.uint8)
    valid_c[:, :100] = 0
    for key in ({"select": SELECT, "stretch": {"percentile": [2, 98]}, "nodata": 0}, {"select": SELECT, "stretch": [0.05, 0.9], "gamma": 0.8}):
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            base = Config(dict(CFG, INFER_PATCHES_PER_EDGE=2, SCENE_FLOAT=key))
            _, _, kp0, road0 = infer_one_img(net, a, base)
            cfg = Config(dict(base, **_thresholds(kp0, road0)))
            want = [infer_one_img(net, im, cfg, **kw) for im, kw in ((a, {}), (b, {}), (c, dict(valid=valid_c)))]
            got = list(infer_imgs(net, iter([a, b, c]), cfg, valids=iter([None, None, valid_c])))
        assert len(got) == 3 and want[0][0].shape[0] >= 10
        for w, g in zip(want, got):
            for x, y in zip(g, w):
                _same(x, y)
        assert not got[1][3][:50].any() and not got[2][3][:, :100].any()


def test_uint16_cast_to_float_equals_scene_bands():
    """A uint16 scene cast to float32 under SCENE_FLOAT {stretch: [0, 510]} equals the same scene under SCENE_BANDS {stretch: [0, 510]}, whole
    tuple: the thresholds are the odd integers, exact in every format.  (The float scene carries an all-valid mask, which changes nothing.)"""
    from sam_road_amd import Config
    from sam_road_amd.inferencer import infer_one_img
    net = _net_for(P)
    u8 = rect_scene(H0, W0, SEED)
    rng = np.random.default_rng(9)
    raw16 = rng.integers(0, 65536, size=u8.shape[:2] + (4,), dtype=np.uint16)
    for b, s in enumerate(SELECT):
        raw16[..., s] = u8[..., b].astype(np.uint16) * 2 + rng.integers(0, 2, size=u8.shape[:2], dtype=np.uint16)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        base = Config(dict(CFG, INFER_PATCHES_PER_EDGE=PER_EDGE, SCENE_BANDS={"select": SELECT, "stretch": [0, 510]}))
        _, _, kp0, road0 = infer_one_img(net, raw16, base)
        bands_cfg = Config(dict(base, **_thresholds(kp0, road0)))
        want = infer_one_img(net, raw16, bands_cfg)
        float_cfg = Config(dict(bands_cfg, SCENE_BANDS=None, SCENE_FLOAT={"select": SELECT, "stretch": [0, 510]}))
        got = infer_one_img(net, raw16.astype(F32), float_cfg)
    assert want[0].shape[0] >= 30 and want[1].shape[0] >= 1
    for a, b in zip(got, want):
        _same(a, b)
