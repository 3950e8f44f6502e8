"""SCENE_NODATA (the validity mask derived from a nodata value on the device) on the HIP path.  Run on an MI355X: pytest -m gpu.

The reference has no such step, so the behaviour is pinned by the rule and by COMPOSITION: the two kernels must equal numpy byte for
byte at every shape at which their addressing can go wrong, match -> mask_clean -> grow must equal nodata_ref, and a run with the key must
equal, bit for bit, the existing pipeline called with valid = nodata_ref(raw, key, valid).  There is no tolerance anywhere."""
import warnings

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import scene_nodata_kit as nk
from scene_kit import CFG, PARITY_SCENES, SCENES, check_scene_parity, oracle_scene, pair, rect_scene, thresholds  # noqa: F401
from scene_kit import net_for as _net_for
from scene_kit import same_bits as _same

from sam_road_amd.mask_clean import MaskRule, mask_clean_table
from sam_road_amd.nodata import nodata_ref, nodata_table, scene_nodata_check, scene_nodata_key

P = CFG["PATCH_SIZE"]
GUARD = 64


def _key(**kw):
    from sam_road_amd import Config
    return scene_nodata_key(Config(SCENE_NODATA=kw))


def _guarded(n, offset=0):
    """(buffer of 0xA5, its view of n bytes that starts GUARD + offset bytes in)."""
    buf = torch.full((n + 2 * GUARD + 16,), 0xA5, dtype=torch.uint8, device="cuda")
    return buf, buf[GUARD + offset:GUARD + offset + n]


def _guards_ok(buf, view_off, n):
    b = buf.cpu().numpy()
    return (b[:GUARD + view_off] == 0xA5).all() and (b[GUARD + view_off + n:] == 0xA5).all()


# ---- 1. the match kernel against numpy ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.uint8, np.uint16])
def test_match_equals_numpy(dtype):
    """n in {1, 3, 4, 17, 257 * 300}: less than an item, one whole item, a clipped last item, many workgroups; C in {1, 3, 4, 16}; all /
    any; t in {0, 3, levels - 1} around v = 0 and v = levels - 1 (the range clamps at both ends); the source a view at byte offsets 1 and
    3 (u8) / 2 (u16) of its allocation, so the 16-byte chunks straddle the items; the output at every alignment mod 4, between guards."""
    net = _net_for(P)
    levels = 256 if dtype == np.uint8 else 65536
    es = np.dtype(dtype).itemsize
    rng = np.random.default_rng(7)
    case = 0
    for n in (1, 3, 4, 17, 257 * 300):
        for C in (1, 3, 4, 16):
            for v in (0, levels - 1):
                for t in (0, 3, levels - 1):
                    case += 1
                    # values crowd within 5 levels of v, so that hits are common at t = 0 and t = 3
                    raw = (v + rng.integers(0, 6, size=(n, C)) * (1 if v == 0 else -1)).astype(dtype)
                    lo, hi = [max(0, v - t)] * C, [min(levels - 1, v + t)] * C
                    if C > 1:                             # one band with a range of its own
                        lo[C - 1], hi[C - 1] = (1, 4) if v == 0 else (levels - 5, levels - 2)
                    off = ((1, 3) if es == 1 else (2, 2))[case & 1]
                    store = torch.zeros(n * C * es + 16, dtype=torch.uint8, device="cuda")
                    src = store[off:off + n * C * es].view(torch.uint8 if es == 1 else torch.uint16).view(n, C)
                    src.copy_(torch.from_numpy(raw))
                    aw_np = (rng.integers(0, 3, size=n) * 100).astype(np.uint8)
                    per = (raw.astype(np.int64) >= np.asarray(lo)) & (raw.astype(np.int64) <= np.asarray(hi))
                    for match, hit in (("all", per.all(-1)), ("any", per.any(-1))):
                        for invert, with_and in ((False, False), (True, True), (True, False), (False, True)):
                            if n > 17 and (invert, with_and) in ((True, False), (False, True)):
                                continue
                            out_off = (case + invert + 2 * with_and) & 3
                            buf, out = _guarded(n, out_off)
                            aw = torch.from_numpy(aw_np).cuda() if with_and else None
                            got = net.scene_nodata_match(src, lo, hi, match, and_with=aw, invert=invert, out=out)
                            want = (~hit if invert else hit) & ((aw_np != 0) if with_and else True)
                            assert got.data_ptr() == out.data_ptr()
                            np.testing.assert_array_equal(out.cpu().numpy(), want.astype(np.uint8), err_msg=f"n {n} C {C} v {v} t {t} {match} {invert} {with_and}")
                            assert _guards_ok(buf, out_off, n)
                            if n == 257 * 300 and t == 3 and match == "all":
                                assert 0 < hit.sum() < n              # neither all nor nothing: a kernel that ignores the source cannot pass
                    np.testing.assert_array_equal(src.cpu().numpy(), raw)                   # the source was not written
    # without `out`: a new tensor of the scene's shape
    raw = rng.integers(0, 3, size=(37, 53, 3)).astype(dtype)
    got = net.scene_nodata_match(torch.from_numpy(raw).cuda(), [0] * 3, [1] * 3)
    assert tuple(got.shape) == (37, 53) and got.dtype == torch.uint8
    np.testing.assert_array_equal(got.cpu().numpy(), (raw <= 1).all(-1).astype(np.uint8))


# ---- 2. the grow kernel against the brute-force window maximum -------------------------------------------------------------------------------------
def _seeds(kind, H, W, rng):
    s = np.zeros((H, W), np.uint8)
    if kind == "corners":
        s[0, 0] = s[0, W - 1] = s[H - 1, 0] = s[H - 1, W - 1] = 255
    elif kind == "borders":                               # both sides of every workgroup-block boundary (64 x 64 outputs per workgroup)
        for y in range(63, H, 64):
            s[y, rng.integers(0, W)] = 1
            if y + 1 < H:
                s[y + 1, rng.integers(0, W)] = 2
        for x in range(63, W, 64):
            s[rng.integers(0, H), x] = 3
            if x + 1 < W:
                s[rng.integers(0, H), x + 1] = 4
        if H > 64 and W > 64:
            s[63, 63] = s[64, 64] = 5
    elif kind == "isolated":
        s[H // 2, W // 2] = 9
    elif kind == "all":
        s[...] = 1
    elif kind == "sparse":
        s[rng.random((H, W)) < 0.002] = 77
    return s                                              # "none": all zero


@pytest.mark.parametrize("r", [1, 2, 7, 16])
def test_grow_equals_the_window_maximum(r):
    """Images 1 x 1, 7 x 5, 64 x 64 (exactly one block), 65 x 130 (a second block row of one row; three block columns, the last 2 wide),
    257 x 300; r in {1, 2, 7, 16}: larger than the image at the small ones, the full staging window at 16."""
    net = _net_for(P)
    rng = np.random.default_rng(11)
    rule = MaskRule(1, 1, 0)
    for H, W in ((1, 1), (7, 5), (64, 64), (65, 130), (257, 300)):
        for kind in ("corners", "borders", "isolated", "all", "none", "sparse"):
            s = _seeds(kind, H, W, rng)
            want = nk.window_max(s, r)
            aw_np = (rng.integers(0, 4, size=(H, W)) != 0).astype(np.uint8) * 200
            table = mask_clean_table([(0, H, W, rule)])
            for invert, with_and in ((False, False), (True, True)):
                buf, out = _guarded(H * W, (H + r) & 3)
                aw = torch.from_numpy(aw_np).cuda().view(-1) if with_and else None
                src = torch.from_numpy(s).cuda().view(-1)
                got = net.scene_nodata_grow(src, table, r, and_with=aw, invert=invert, out=out)
                w = ((1 - want) if invert else want) & ((aw_np != 0) if with_and else 1)
                assert got.data_ptr() == out.data_ptr()
                np.testing.assert_array_equal(out.cpu().numpy().reshape(H, W), w, err_msg=f"{H}x{W} {kind} r {r} invert {invert}")
                assert _guards_ok(buf, (H + r) & 3, H * W)
                np.testing.assert_array_equal(src.cpu().numpy().reshape(H, W), s)
            if kind == "isolated" and H > 2 * r + 1 and W > 2 * r + 1:
                assert 0 < want.sum() < H * W
    # the library's own statement of the grow agrees with the brute force
    from sam_road_amd.nodata import grow_ref
    s = _seeds("sparse", 65, 130, rng)
    np.testing.assert_array_equal(grow_ref(s, r), nk.window_max(s, r))


def test_grow_three_images_in_one_call_at_odd_offsets():
    """Three images of different sizes in one buffer, at odd offsets, the table not in buffer order, gaps in front, between and behind; the
    gaps of the source are SET, so a grow that ignored the blocks' borders would spread them into the images; the gaps of the destination
    are guards."""
    net = _net_for(P)
    rng = np.random.default_rng(13)
    dims, offs = [(65, 67), (1, 1), (9, 131)], [3, 3 + 65 * 67 + 5, 3 + 65 * 67 + 5 + 1 + 1]
    total = offs[-1] + 9 * 131 + 2
    flat = np.full(total, 255, np.uint8)
    aw_np = (rng.integers(0, 3, size=total) != 0).astype(np.uint8)
    for (H, W), o in zip(dims, offs):
        flat[o:o + H * W] = (rng.random(H * W) < 0.004) * 9
    flat[offs[1]] = 0
    for order in ((0, 1, 2), (2, 0, 1)):
        for r in (2, 16):
            table = mask_clean_table([(offs[k], *dims[k], MaskRule(1, 1, 0)) for k in order])
            want = np.full(total, 0xA5, np.uint8)
            for (H, W), o in zip(dims, offs):
                want[o:o + H * W] = ((1 - nk.window_max(flat[o:o + H * W].reshape(H, W), r)) & aw_np[o:o + H * W].reshape(H, W)).reshape(-1)
            buf, out = _guarded(total, 1)
            net.scene_nodata_grow(torch.from_numpy(flat).cuda(), table, r, and_with=torch.from_numpy(aw_np).cuda(), invert=True,
                                  table_dev=torch.from_numpy(table).cuda(), out=out)
            np.testing.assert_array_equal(out.cpu().numpy(), want)                  # the gaps included: untouched
            assert _guards_ok(buf, 1, total) and 0 < want[offs[0]:offs[0] + 65 * 67].sum() < 65 * 67
    assert want[offs[1]] == aw_np[offs[1]]                                          # the 1 x 1 image is empty: nothing reaches it from outside


# ---- 3. match -> mask_clean -> grow against nodata_ref ------------------------------------------------------------------------------------------
KIT_H, KIT_W, PER_EDGE, SEED = SCENES["401x523"]
FULL = dict(value=0, tolerance=3, min_area=50, grow=2)       # the fringe hits, singles and blobs (<= 40 px) are not nodata, the collar grows


def test_three_steps_equal_the_reference_on_the_kit_scene():
    from sam_road_amd.inferencer import _scene_nodata_mask
    net = _net_for(P)
    img, painted = nk.collar_scene(KIT_H, KIT_W, SEED)
    caller = np.ones((KIT_H, KIT_W), np.uint8)
    caller[300:, 400:] = 0
    for kw in (FULL, dict(value=0), dict(value=[0, 0, 0], tolerance=3, match="any"), dict(value=0, tolerance=3, min_area=50, connectivity=4),
               dict(value=0, grow=16), dict(value=0, tolerance=2, min_area=13, grow=1)):
        key = _key(**kw)
        lo, hi = scene_nodata_check(img, key)
        table = nodata_table([(0, KIT_H, KIT_W)], key)
        for valid in (None, caller):
            want = nodata_ref(img, key, valid)
            got = _scene_nodata_mask(net, key, torch.from_numpy(img).cuda(), lo, hi, None if valid is None else torch.from_numpy(valid).cuda(), table, None)
            np.testing.assert_array_equal(got.cpu().numpy().reshape(KIT_H, KIT_W), want, err_msg=str(kw))
    # what the kit scene is for (on the reference): with the full key the interior specks stay valid and the collar and its fringe do not
    full = nodata_ref(img, _key(**FULL)).astype(bool)
    collar = nk.collar_of(KIT_H, KIT_W)
    assert not full[collar].any() and not full[nk.collar_of(KIT_H, KIT_W, shift=3) & ~collar].any() and full[painted & ~collar].all()
    bare = nodata_ref(img, _key(value=0)).astype(bool)
    assert not bare[painted].any() and bare[~painted].all()


# ---- 4. end to end: a run with the key == the existing pipeline with valid = nodata_ref(...) -------------------------------------------------------
ECFG = dict(CFG, INFER_PATCHES_PER_EDGE=PER_EDGE)


def _run(net, img, cfg, **kw):
    from sam_road_amd import Config
    from sam_road_amd.inferencer import infer_one_img
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return infer_one_img(net, img, Config(cfg), **kw)


def _same_result(got, want):
    for g, w in zip(got, want):
        _same(g, w)


def test_infer_one_img_equals_the_composition(pair):
    """The test that fails on code that ignores the key."""
    _, net = pair
    img, painted = nk.collar_scene(KIT_H, KIT_W, SEED)
    plain = _run(net, img, ECFG)
    for kw in (FULL, dict(value=0)):
        valid = nodata_ref(img, _key(**kw))
        want = _run(net, img, ECFG, valid=valid)
        got = _run(net, img, dict(ECFG, SCENE_NODATA=kw))
        _same_result(got, want)
        assert not got[2][valid == 0].any() and not got[3][valid == 0].any() and got[3].any() and (got[3] != plain[3]).any()
    # a caller's mask is ANDed in
    caller = np.ones((KIT_H, KIT_W), bool)
    caller[250:, 300:] = False
    want = _run(net, img, ECFG, valid=nodata_ref(img, _key(**FULL), caller))
    got = _run(net, img, dict(ECFG, SCENE_NODATA=FULL), valid=caller)
    _same_result(got, want)
    assert not got[3][250:, 300:].any() and got[3].any()
    # a bare int is {value: ...}
    _same_result(_run(net, img, dict(ECFG, SCENE_NODATA=0)), _run(net, img, ECFG, valid=nodata_ref(img, _key(value=0))))


def test_the_pipelined_loop_over_the_three_scene_kinds(pair):
    from sam_road_amd import Config
    from sam_road_amd.inferencer import _empty_result, infer_imgs
    _, net = pair
    collar, _ = nk.collar_scene(KIT_H, KIT_W, SEED)
    clean = nk.plain_scene(384, 640, 41)
    empty = np.zeros((300, 421, 3), np.uint8)
    key = _key(**FULL)
    cfg = dict(ECFG, SCENE_NODATA=FULL)
    assert nodata_ref(clean, key).all() and not nodata_ref(empty, key).any()
    imgs = [collar, clean, empty, collar]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        res = list(infer_imgs(net, iter(imgs), Config(cfg)))
    wants = [_run(net, im, ECFG, valid=nodata_ref(im, key)) for im in imgs]
    for got, want in zip(res, wants):
        _same_result(got, want)
    _same_result(res[1], _run(net, clean, ECFG))                                 # no hit pixel: the all-true-mask result = the unmasked one
    _same_result(res[2], _empty_result(300, 421))                                # all nodata


def test_group_of_three(pair):
    from sam_road_amd import Config
    from sam_road_amd.inferencer import infer_imgs
    _, net = pair
    shapes = [(288, 288), (300, 421), (401, 523)]
    imgs = [nk.collar_scene(h, w, 50 + i)[0] for i, (h, w) in enumerate(shapes)]
    imgs[1] = np.zeros((300, 421, 3), np.uint8)                                  # one scene of the group is all nodata
    key = _key(**FULL)
    gcfg = dict(CFG, INFER_PATCHES_PER_EDGE=2, SCENE_PAD=24)
    callers = [None, None, np.ones((401, 523), np.uint8)]
    callers[2][:, 450:] = 0
    for valids in (None, callers):
        vs = valids or [None] * 3
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            wants = list(infer_imgs(net, iter(imgs), Config(gcfg), group=3, valids=[nodata_ref(im, key, v) for im, v in zip(imgs, vs)]))
            res = list(infer_imgs(net, iter(imgs), Config(dict(gcfg, SCENE_NODATA=FULL)), group=3, **({} if valids is None else dict(valids=valids))))
        for got, want, hw in zip(res, wants, shapes):
            assert got[2].shape == hw
            _same_result(got, want)
        assert not res[1][3].any() and res[0][3].any() and res[2][3].any()


def test_u16_four_bands_with_a_percentile_stretch(pair):
    """The ranges of the stretch must be those of the derived-valid pixels: the collar holds 65535, which would move the upper percentile."""
    _, net = pair
    raw, painted = nk.raw16_scene(KIT_H, KIT_W, SEED)
    bands = dict(select=[2, 1, 0], stretch=dict(percentile=[2, 98]))
    kw = dict(value=65535, tolerance=3, min_area=50, grow=2)
    cfg = dict(ECFG, SCENE_BANDS=bands)
    valid = nodata_ref(raw, _key(**kw))
    want = _run(net, raw, cfg, valid=valid)
    got = _run(net, raw, dict(cfg, SCENE_NODATA=kw))
    _same_result(got, want)
    unmasked = _run(net, raw, cfg)
    assert (want[3] != unmasked[3])[valid != 0].any() and got[3].any()           # the stretch itself differs, not only the zeros on nodata
    # per-band values, and a list of the wrong length
    _same_result(_run(net, raw, dict(cfg, SCENE_NODATA=dict(kw, value=[65535] * 4))), want)
    with pytest.raises(ValueError):
        _run(net, raw, dict(cfg, SCENE_NODATA=dict(kw, value=[65535] * 3)))


def test_scene_scale_and_scene_pad(pair):
    _, net = pair
    key = _key(**FULL)
    big, _ = nk.collar_scene(2 * KIT_H, 2 * KIT_W, SEED)
    scaled = dict(ECFG, SCENE_SCALE=[1, 2])
    valid = nodata_ref(big, key)
    got = _run(net, big, dict(scaled, SCENE_NODATA=FULL))
    _same_result(got, _run(net, big, scaled, valid=valid))
    assert got[2].shape == (2 * KIT_H, 2 * KIT_W) and not got[3][valid == 0].any() and got[3].any()
    img, _ = nk.collar_scene(KIT_H, KIT_W, SEED)
    padded = dict(ECFG, SCENE_PAD=24)
    got = _run(net, img, dict(padded, SCENE_NODATA=FULL))
    _same_result(got, _run(net, img, padded, valid=nodata_ref(img, key)))
    assert got[3].any()


# ---- 5. the launch contract -----------------------------------------------------------------------------------------------------------------------
CLEAN_ROWS = ("mask_clean_init", "mask_clean_merge", "mask_clean_flatten", "mask_clean_stats", "mask_clean_apply")


def _launches(ctx, fn):
    ctx.profile_read()
    ctx.profile_enable(True)
    try:
        out = fn()
        torch.cuda.synchronize()
        return out, {r["name"]: r["launches"] for r in ctx.profile_read() if r["launches"]}
    finally:
        ctx.profile_enable(False)


def test_launch_contract(pair, monkeypatch):
    from sam_road_amd import Config, _lib
    from sam_road_amd import inferencer as inf
    _, net = pair
    img, _ = nk.collar_scene(KIT_H, KIT_W, SEED)
    ctx = _lib.Context.get(torch.cuda.current_device())
    uploads = []
    orig = inf._LaneIO.upload
    monkeypatch.setattr(inf._LaneIO, "upload", lambda self, name, arr: (uploads.append(name), orig(self, name, arr))[1])

    def loop(cfg, n=3, **kw):
        uploads.clear()
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            return list(inf.infer_imgs(net, iter([img] * n), Config(cfg), **kw))

    # key absent: neither new row, and None / a missing key are the same run
    _, base = _launches(ctx, lambda: loop(ECFG))
    assert "scene_nodata_match" not in base and "scene_nodata_grow" not in base and not any(r.startswith("mask_clean") for r in base)
    base_uploads = list(uploads)
    _, rows = _launches(ctx, lambda: loop(dict(ECFG, SCENE_NODATA=None)))
    assert rows == base and uploads == base_uploads
    # the same loop with the mask passed: what a keyed loop must look like behind the front
    valid = nodata_ref(img, _key(value=0))
    _, masked = _launches(ctx, lambda: loop(ECFG, valids=[valid] * 3))
    assert uploads.count("valid_mask") == 3
    # value-only key: exactly ONE launch per scene, no mask staged or uploaded, everything else as the masked loop
    _, rows = _launches(ctx, lambda: loop(dict(ECFG, SCENE_NODATA=dict(value=0))))
    assert rows == dict(masked, scene_nodata_match=3), (rows, masked)
    assert "valid_mask" not in uploads and "nodata_table" not in uploads
    # the full key: one match, the five mask_clean rows, one grow — per scene
    valid = nodata_ref(img, _key(**FULL))
    _, masked = _launches(ctx, lambda: loop(ECFG, valids=[valid] * 3))
    _, rows = _launches(ctx, lambda: loop(dict(ECFG, SCENE_NODATA=FULL)))
    assert rows == dict(masked, scene_nodata_match=3, scene_nodata_grow=3, **{r: 3 for r in CLEAN_ROWS}), (rows, masked)
    assert "valid_mask" not in uploads and uploads.count("nodata_table") == 3
    # a group of three: one of each for the whole group
    gcfg = dict(CFG, INFER_PATCHES_PER_EDGE=2)
    _, gmasked = _launches(ctx, lambda: loop(gcfg, group=3, valids=[valid] * 3))
    _, grows = _launches(ctx, lambda: loop(dict(gcfg, SCENE_NODATA=FULL), group=3))
    assert grows == dict(gmasked, scene_nodata_match=1, scene_nodata_grow=1, **{r: 1 for r in CLEAN_ROWS}), (grows, gmasked)


# ---- 6. both entries' rejections --------------------------------------------------------------------------------------------------------------------
def test_entries_reject_bad_arguments_and_launch_nothing():
    import ctypes
    from sam_road_amd import _lib
    net = _net_for(P)
    dev = torch.device("cuda")
    ctx, _ = net._weights(dev)
    lib, s = ctx.lib, net._stream(dev)
    src = torch.zeros(64, dtype=torch.uint8, device=dev)
    out = torch.full((64,), 0xA5, dtype=torch.uint8, device=dev)
    aw = torch.ones(64, dtype=torch.uint8, device=dev)
    i32 = lambda *v: (ctypes.c_int32 * len(v))(*v)

    def match(src_p=src.data_ptr(), dtype=_lib.SRH_U8, n=16, C=3, lo=i32(0, 0, 0), hi=i32(1, 1, 1), mode=0, aw_p=None, invert=0, out_p=out.data_ptr()):
        return lib.srh_scene_nodata_match(ctx.handle, src_p, dtype, n, C, lo, hi, mode, aw_p, invert, out_p, s)

    bad = (dict(src_p=None), dict(out_p=None), dict(lo=None), dict(hi=None), dict(dtype=_lib.SRH_F32), dict(dtype=_lib.SRH_I32), dict(C=0), dict(C=17),
           dict(n=0), dict(n=-5), dict(n=2 ** 31), dict(mode=2), dict(mode=-1), dict(invert=2), dict(lo=i32(-1, 0, 0)), dict(hi=i32(0, 65536, 0)),
           dict(dtype=_lib.SRH_U16, src_p=src.data_ptr() + 1), dict(out_p=src.data_ptr() + 40), dict(aw_p=out.data_ptr() + 8))
    for kw in bad:
        assert match(**kw) == -1, kw
    assert lib.srh_scene_nodata_match(None, src.data_ptr(), _lib.SRH_U8, 16, 3, i32(0, 0, 0), i32(1, 1, 1), 0, None, 0, out.data_ptr(), s) == -1

    table = mask_clean_table([(0, 4, 5, MaskRule(1, 1, 0)), (20, 3, 3, MaskRule(1, 1, 0))])     # 29 bytes

    def grow(src_p=src.data_ptr(), dst_p=out.data_ptr(), nbytes=29, t=table, n=2, r=2, aw_p=aw.data_ptr(), invert=1, tdev=True):
        th = torch.from_numpy(np.ascontiguousarray(t))
        td = th.cuda()
        return lib.srh_scene_nodata_grow(ctx.handle, src_p, dst_p, nbytes, th.data_ptr(), td.data_ptr() if tdev else None, n, r, aw_p, invert, s)

    def edit(i, j, v):
        t = table.copy()
        t[i, j] = v
        return t

    bad = (dict(src_p=None), dict(dst_p=None), dict(tdev=False), dict(r=0), dict(r=17), dict(r=-1), dict(invert=2), dict(n=0), dict(n=4097), dict(nbytes=28),
           dict(nbytes=0), dict(t=edit(1, 0, 19)), dict(t=edit(1, 0, 21)), dict(t=edit(1, 0, -1)), dict(t=edit(0, 1, 0)), dict(t=edit(0, 2, 0)),
           dict(dst_p=src.data_ptr() + 28), dict(dst_p=src.data_ptr()), dict(aw_p=out.data_ptr() + 1))
    for kw in bad:
        assert grow(**kw) == -1, kw
    huge = mask_clean_table([(0, 46341, 46341, MaskRule(1, 1, 0))])                  # more than 2^31 - 1 pixels
    assert grow(t=huge, n=1, nbytes=2 ** 40) == -1
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == 0xA5).all()                                         # nothing was launched
    assert match() == 0 and grow() == 0
    with pytest.raises(_lib.SrhError, match="r is 1 to 16"):
        ctx.check(grow(r=17), "srh_scene_nodata_grow")
    raw = torch.zeros((4, 5, 3), dtype=torch.uint8, device=dev)
    for kw in (dict(src=raw.float()), dict(lo=[0, 0]), dict(hi=[0, 0, 70000]), dict(match="most"), dict(and_with=aw[:7]), dict(src=raw[:, :, :2]),
               dict(out=out[:19])):
        kw = dict(dict(src=raw, lo=[0, 0, 0], hi=[1, 1, 1]), **kw)
        with pytest.raises(ValueError):
            net.scene_nodata_match(kw.pop("src"), kw.pop("lo"), kw.pop("hi"), **kw)
    for kw in (dict(src=src.view(8, 8)), dict(r=0), dict(r=17), dict(table=np.zeros((1, 7), np.int64)), dict(and_with=aw[:5])):
        kw = dict(dict(src=src[:29], table=table, r=2), **kw)
        with pytest.raises(ValueError):
            net.scene_nodata_grow(kw.pop("src"), kw.pop("table"), kw.pop("r"), **kw)
    torch.cuda.synchronize()


# ---- 7. against the oracle ----------------------------------------------------------------------------------------------------------------------------
ORACLE_SCENE = "523x701"


def test_parity_with_the_oracle_on_a_collar_scene(pair):
    """check_scene_parity with valid = nodata_ref(...), the kit's bounds and caps unchanged, on the 523 x 701 scene of PARITY_SCENES with
    the kit's collar (nk.COLLAR), fringe, singles and blobs painted in and the full key (value 0, tolerance 3, min_area 50, grow 2).
    Chosen WITH THE ORACLE ALONE on the CPU (points from the oracle's own masks), so that the symmetric-difference cap is a condition:
      valid share 0.904, 20 tiles kept, 499 points, 8216 voted edges, 598 oracle edges, 0.40 % within TOPO_SCORE of the threshold
    (384x640 with the same collar: 0.902, 15, 423, 7875, 515, 0.39 % — not used)."""
    from sam_road_amd import Config
    from sam_road_amd.inferencer import infer_one_img
    oracle, net = pair
    H, W, per_edge, seed = PARITY_SCENES[ORACLE_SCENE]
    img, _ = nk.collar_scene(H, W, seed)
    valid = nodata_ref(img, _key(**FULL)).astype(bool)
    ref = oracle_scene(oracle, img, per_edge, valid=valid)
    cfg = dict(CFG, INFER_PATCHES_PER_EDGE=per_edge, **thresholds(ref[2], ref[3]))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        got = infer_one_img(net, img, Config(dict(cfg, SCENE_NODATA=FULL)))
    check_scene_parity(f"nodata_{ORACLE_SCENE}", got, ref, cfg, oracle, valid=valid, min_oracle_edges=200)
