"""SCENE_AOI (the validity mask rasterised from polygons on the device) on the HIP path.  Run on an MI355X: pytest -m gpu.

The reference has no such step, so the behaviour is pinned by the rule and by COMPOSITION: the kernel must equal aoi_ref byte for byte at
every shape at which its addressing can go wrong, fill -> grow must equal aoi_ref with a buffer, and a run with the key must equal, bit for
bit, the existing pipeline called with valid = aoi_ref(shape, key, valid).  There is no tolerance anywhere."""
import warnings

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import scene_aoi_kit as ak
import scene_nodata_kit as nk
from scene_kit import CFG, PARITY_SCENES, SCENES, check_scene_parity, oracle_scene, pair, rect_scene, thresholds  # noqa: F401
from scene_kit import net_for as _net_for
from scene_kit import same_bits as _same

from sam_road_amd.aoi import aoi_edges, aoi_pack, aoi_ref, scene_aoi_key
from sam_road_amd.mask_clean import MaskRule, mask_clean_table
from sam_road_amd.nodata import nodata_ref, scene_nodata_key

P = CFG["PATCH_SIZE"]
GUARD = 64
SEG = 4096                                                # the kernel's column-segment width (AOI_SEG of csrc/scene_aoi_piece.hpp)


def _key(v):
    from sam_road_amd import Config
    return scene_aoi_key(Config(SCENE_AOI=v))


def _guarded(n, offset=0):
    """(buffer of 0xA5, its view of n bytes that starts GUARD + offset bytes in)."""
    buf = torch.full((n + 2 * GUARD + 16,), 0xA5, dtype=torch.uint8, device="cuda")
    return buf, buf[GUARD + offset:GUARD + offset + n]


def _guards_ok(buf, view_off, n):
    b = buf.cpu().numpy()
    return (b[:GUARD + view_off] == 0xA5).all() and (b[GUARD + view_off + n:] == 0xA5).all()


def _fill(net, shape, key, off=0, invert=False, and_with=None):
    """The kernel on a guarded output at alignment `off`: (u8 [H, W] from the device, the edge table was not written, the guards hold)."""
    H, W = shape
    tab = aoi_edges(key, H, W)
    packed = aoi_pack(*tab[:2])
    table_d = torch.from_numpy(packed).cuda()
    buf, out = _guarded(H * W, off)
    aw = None if and_with is None else torch.from_numpy(and_with).cuda()
    got = net.scene_aoi_fill((H, W), *tab, and_with=aw, invert=invert, table_dev=table_d, out=out)
    assert got.data_ptr() == out.data_ptr()
    np.testing.assert_array_equal(table_d.cpu().numpy(), packed)            # the edge table is not written
    assert _guards_ok(buf, off, H * W)
    return out.cpu().numpy().reshape(H, W)


# ---- 1. the kernel against aoi_ref -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(1, 1), (7, 5), (64, 64), (65, 130), (257, 300)])
def test_fill_equals_the_reference(shape):
    """The polygon menu of the CPU tests on every scene, the output at every alignment mod 4 between 0xA5 guards; and_with and invert in all
    four combinations on the small scenes (both on and both off on the others)."""
    net = _net_for(P)
    H, W = shape
    rng = np.random.default_rng(H * 1000 + W)
    aw = (rng.integers(0, 3, size=(H, W)) * 100).astype(np.uint8)
    small = H * W <= 64 * 64
    partial = 0
    for n, (name, value) in enumerate(ak.menu(H, W).items()):
        key = _key(value)
        want = aoi_ref((H, W), key)
        for invert, with_and in ((False, False), (True, True), (True, False), (False, True)) if small else ((False, False), (True, True)):
            got = _fill(net, (H, W), key, off=(n + invert + 2 * with_and) & 3, invert=invert, and_with=aw if with_and else None)
            w = ((1 - want) if invert else want) & ((aw != 0) if with_and else 1)
            np.testing.assert_array_equal(got, w, err_msg=f"{name} {H}x{W} invert {invert} and {with_and}")
        partial += 0 < want.sum() < H * W
    assert partial >= (8 if H > 1 else 0)                 # neither all nor nothing: a kernel that ignores the table cannot pass


def test_fill_many_edges_ties_and_the_limits():
    """A 1000-vertex circle (more edges than lanes, many per row), a vertex on a pixel centre, a diagonal through centres, the 64-polygon
    and the 16384-edge limit — on 65 x 130 and 257 x 300."""
    net = _net_for(P)
    for H, W in ((65, 130), (257, 300)):
        cases = {"circle": ak.circle(H / 2 + 0.25, W / 2, 0.45 * min(H, W)), "centre_vertex": ak.menu(H, W)["centre_vertex"], "diagonal": ak.menu(H, W)["diagonal"],
                 "polygons": ak.many_polygons(H, W, 64), "edges": ak.many_edges(H, W, 16384)}
        for n, (name, value) in enumerate(cases.items()):
            key = _key(value if isinstance(value, dict) else [value] if name == "circle" else value)
            want = aoi_ref((H, W), key)
            assert 0 < want.sum() < H * W, name
            np.testing.assert_array_equal(_fill(net, (H, W), key, off=n & 3), want, err_msg=f"{name} {H}x{W}")
        e, o, ni, ne = aoi_edges(_key(cases["edges"]), H, W)
        assert e.shape[0] == 16384 and (ni, ne) == (1, 0)
        e, o, ni, ne = aoi_edges(_key(cases["polygons"]), H, W)
        assert ni + ne == 64 and ne > 0
        assert aoi_edges(_key([cases["circle"]]), H, W)[0].shape[0] > (256 if H > 65 else 64)      # what is left of 1000 edges once the horizontal ones are dropped
    # a centre on the diagonal is on a right edge: outside; the pixel left of it inside
    d = _fill(net, (65, 130), _key(ak.menu(65, 130)["diagonal"]))
    assert d[30, 30] == 0 and d[30, 29] == 1 and d[31, 30] == 1


@pytest.mark.parametrize("W", [SEG, SEG + 1])
def test_fill_a_row_of_the_segment_width_and_one_pixel_wider(W):
    net = _net_for(P)
    H = 1
    ring = [[-1.0, 100.25], [2.0, 90.0], [2.0, W + 3.0], [-1.0, W + 5.0]]         # starts inside the first segment, ends right of the scene
    zig = [[-1.0 if i % 2 == 0 else 2.0, 40.0 + i * (W - 50.0) / 400] for i in range(400)] + [[5.0, float(W)], [5.0, 0.0]]
    for n, value in enumerate(([[ring]], [[zig]], {"exclude": [[ring]]}, {"include": [[[[-1, 4000.5], [2, 4000.5], [2, 5000], [-1, 5000]]]]})):
        key = _key(value)
        want = aoi_ref((H, W), key)
        assert 0 < want.sum() < W
        for off in range(4):
            np.testing.assert_array_equal(_fill(net, (H, W), key, off=off, invert=bool(n & 1)), (1 - want) if n & 1 else want, err_msg=f"case {n} off {off}")
    assert aoi_ref((H, W), _key([[ring]]))[0, W - 1] == 1                        # the wider row's last pixel, alone in its segment, is inside


# ---- 2. fill -> grow against aoi_ref with a buffer ------------------------------------------------------------------------------------------------------
KIT_H, KIT_W, PER_EDGE, SEED = SCENES["401x523"]
TRIANGLE = [[[[-10.0, -10.0], [330.5, -10.0], [-10.0, 420.25]]]]          # over the scene's origin corner: leaves tiles out
HOLED = {"include": [[[[20, 30], [380.5, 60], [390, 500.25], [40, 480]], [[150, 200], [160.5, 330], [260, 320.25], [250, 210]]]], "exclude": [[[[300, 100], [390, 120], [380, 220]]]]}


def test_fill_then_grow_equals_the_reference_on_the_kit_scene():
    from sam_road_amd.inferencer import _scene_aoi_mask
    net = _net_for(P)
    caller = np.ones((KIT_H, KIT_W), np.uint8)
    caller[300:, 400:] = 0
    grow = mask_clean_table([(0, KIT_H, KIT_W, MaskRule(1, 1, 0))])
    for b in (2, -2, 16, -16, 0):
        key = _key(dict(HOLED, buffer=b))
        tab = aoi_edges(key, KIT_H, KIT_W)
        for valid in (None, caller):
            want = aoi_ref((KIT_H, KIT_W), key, valid)
            got = _scene_aoi_mask(net, key, (KIT_H, KIT_W), None if valid is None else torch.from_numpy(valid).cuda(), tab, None, grow, None)
            np.testing.assert_array_equal(got.cpu().numpy().reshape(KIT_H, KIT_W), want, err_msg=f"buffer {b}")
            assert 0 < want.sum() < KIT_H * KIT_W
    assert aoi_ref((KIT_H, KIT_W), _key(dict(HOLED, buffer=2))).sum() > aoi_ref((KIT_H, KIT_W), _key(HOLED)).sum() > aoi_ref((KIT_H, KIT_W), _key(dict(HOLED, buffer=-2))).sum()


# ---- 3. end to end: a run with the key == the existing pipeline with valid = aoi_ref(...) -----------------------------------------------------------------
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
    from sam_road_amd import Config
    from sam_road_amd.inferencer import scene_tiles
    _, net = pair
    img = rect_scene(KIT_H, KIT_W, SEED)
    plain = _run(net, img, ECFG)
    valid = aoi_ref((KIT_H, KIT_W), _key(TRIANGLE))
    want = _run(net, img, ECFG, valid=valid)
    got = _run(net, img, dict(ECFG, SCENE_AOI=TRIANGLE))
    _same_result(got, want)
    # masks and nodes are empty off the area and non-empty on it
    assert not got[2][valid == 0].any() and not got[3][valid == 0].any() and got[2].any() and got[3].any() and (got[3] != plain[3]).any()
    assert got[0].shape[0] > 0 and valid[got[0][:, 0], got[0][:, 1]].all()
    # the triangle leaves tiles out, and scene_tiles shows it: the device plan, the host plan and the masked plan are one
    tiles = scene_tiles(img.shape, Config(dict(ECFG, SCENE_AOI=TRIANGLE)), net=net)
    assert 0 < len(tiles) < len(scene_tiles(img.shape, Config(ECFG)))
    assert list(tiles) == list(scene_tiles(img.shape, Config(dict(ECFG, SCENE_AOI=TRIANGLE)))) == list(scene_tiles(img.shape, Config(ECFG), valid=valid, net=net))
    # a caller's mask is ANDed in
    caller = np.ones((KIT_H, KIT_W), bool)
    caller[:150, :200] = False
    got = _run(net, img, dict(ECFG, SCENE_AOI=TRIANGLE), valid=caller)
    _same_result(got, _run(net, img, ECFG, valid=aoi_ref((KIT_H, KIT_W), _key(TRIANGLE), caller)))
    assert not got[3][:150, :200].any() and got[3].any()
    # aoi= takes the place of the key
    holed = dict(HOLED, buffer=-3)
    got = _run(net, img, dict(ECFG, SCENE_AOI=TRIANGLE), aoi=holed)
    _same_result(got, _run(net, img, ECFG, valid=aoi_ref((KIT_H, KIT_W), _key(holed))))
    _same_result(_run(net, img, ECFG, aoi=TRIANGLE), want)


def test_scene_nodata_scale_pad_and_bands(pair):
    _, net = pair
    # SCENE_NODATA + SCENE_AOI on the collar scene: each mask with its own grow, ANDed
    img, _ = nk.collar_scene(KIT_H, KIT_W, SEED)
    nd = dict(value=0, tolerance=3, min_area=50, grow=2)
    far = {"include": [[[[60, 80], [390.5, 100], [395, 510.25], [80, 500]]]], "buffer": -2}
    from sam_road_amd import Config
    both = nodata_ref(img, scene_nodata_key(Config(SCENE_NODATA=nd)), aoi_ref((KIT_H, KIT_W), _key(far)))
    got = _run(net, img, dict(ECFG, SCENE_NODATA=nd, SCENE_AOI=far))
    _same_result(got, _run(net, img, ECFG, valid=both))
    assert got[3].any() and (both != aoi_ref((KIT_H, KIT_W), _key(far))).any() and not got[3][both == 0].any()
    # SCENE_SCALE [1, 2]: the area is in scene pixels
    big = rect_scene(2 * KIT_H, 2 * KIT_W, SEED)
    doubled = {"include": [[[[2 * r, 2 * c] for r, c in ring] for ring in poly] for poly in HOLED["include"]], "buffer": 3}
    scaled = dict(ECFG, SCENE_SCALE=[1, 2])
    vbig = aoi_ref(big.shape, _key(doubled))
    got = _run(net, big, dict(scaled, SCENE_AOI=doubled))
    _same_result(got, _run(net, big, scaled, valid=vbig))
    assert got[2].shape == (2 * KIT_H, 2 * KIT_W) and not got[3][vbig == 0].any() and got[3].any()
    # SCENE_PAD 24: the area is in the real scene's frame
    plain = rect_scene(KIT_H, KIT_W, SEED)
    padded = dict(ECFG, SCENE_PAD=24)
    got = _run(net, plain, dict(padded, SCENE_AOI=HOLED))
    _same_result(got, _run(net, plain, padded, valid=aoi_ref((KIT_H, KIT_W), _key(HOLED))))
    assert got[3].any()
    # u16, four bands, a percentile stretch: the histogram counts the pixels of the area
    raw, _ = nk.raw16_scene(KIT_H, KIT_W, SEED)
    cfg = dict(ECFG, SCENE_BANDS=dict(select=[2, 1, 0], stretch=dict(percentile=[2, 98])))
    valid = aoi_ref((KIT_H, KIT_W), _key(far))
    want = _run(net, raw, cfg, valid=valid)
    _same_result(_run(net, raw, dict(cfg, SCENE_AOI=far)), want)
    assert (want[3] != _run(net, raw, cfg)[3])[valid != 0].any()                 # the stretch itself differs, not only the zeros off the area


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


def test_launch_contract(pair, monkeypatch):
    from sam_road_amd import Config, _lib
    from sam_road_amd import inferencer as inf
    _, net = pair
    img = rect_scene(KIT_H, KIT_W, SEED)
    ctx = _lib.Context.get(torch.cuda.current_device())
    uploads = []
    orig = inf._LaneIO.upload
    monkeypatch.setattr(inf._LaneIO, "upload", lambda self, name, arr: (uploads.append(name), orig(self, name, arr))[1])

    def loop(cfg, n=3, **kw):
        uploads.clear()
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            return list(inf.infer_imgs(net, iter([img] * n), Config(cfg), **kw))

    # key absent: no new row, and None / {} / a missing key / aois of None are the same run with the same uploads
    _, base = _launches(ctx, lambda: loop(ECFG))
    assert "scene_aoi_fill" not in base and "scene_nodata_grow" not in base
    base_uploads = list(uploads)
    for cfg, kw in ((dict(ECFG, SCENE_AOI=None), {}), (dict(ECFG, SCENE_AOI={}), {}), (ECFG, dict(aois=[None] * 3))):
        _, rows = _launches(ctx, lambda: loop(cfg, **kw))
        assert rows == base and uploads == base_uploads
    # the same loop with the mask passed: what a keyed loop must look like behind the front
    valid = aoi_ref((KIT_H, KIT_W), _key(TRIANGLE))
    res_m, masked = _launches(ctx, lambda: loop(ECFG, valids=[valid] * 3))
    assert uploads.count("valid_mask") == 3
    masked_uploads = [u for u in uploads if u != "valid_mask"]
    # keyed: exactly ONE launch per scene, no mask staged or uploaded, everything else as the masked loop
    res_k, rows = _launches(ctx, lambda: loop(dict(ECFG, SCENE_AOI=TRIANGLE)))
    assert rows == dict(masked, scene_aoi_fill=3), (rows, masked)
    assert "valid_mask" not in uploads and uploads.count("aoi_table") == 3 and [u for u in uploads if u != "aoi_table"] == masked_uploads
    for got, want in zip(res_k, res_m):
        _same_result(got, want)
    # with a buffer: one fill and one grow per scene
    _, rows = _launches(ctx, lambda: loop(dict(ECFG, SCENE_AOI={"include": TRIANGLE, "buffer": -2})))
    vb = aoi_ref((KIT_H, KIT_W), _key({"include": TRIANGLE, "buffer": -2}))
    _, masked_b = _launches(ctx, lambda: loop(ECFG, valids=[vb] * 3))
    assert rows == dict(masked_b, scene_aoi_fill=3, scene_nodata_grow=3), (rows, masked_b)
    # per-scene areas: only the scenes that bring one take the step
    _, rows = _launches(ctx, lambda: loop(ECFG, aois=[None, TRIANGLE, None]))
    assert rows.get("scene_aoi_fill") == 1


# ---- 5. the entry's rejections ------------------------------------------------------------------------------------------------------------------------------
def test_entry_rejects_bad_arguments_and_launches_nothing():
    import ctypes
    from sam_road_amd import _lib
    net = _net_for(P)
    dev = torch.device("cuda")
    ctx, _ = net._weights(dev)
    lib, s = ctx.lib, net._stream(dev)
    buf, out = _guarded(64, 1)
    aw = torch.ones(64, dtype=torch.uint8, device=dev)
    edges = np.array([[0, 0, 1024, 0], [0, 1500, 1024, 1500], [100, 300, 900, 300], [100, 700, 900, 800]], np.int32)
    polys = np.array([0, 2, 4], np.int32)

    def fill(e=edges, o=polys, ni=1, ne=1, H=8, W=8, aw_p=aw.data_ptr(), invert=0, out_p=out.data_ptr(), e_host=True, e_dev=True, o_host=True, o_dev=True, dev_off=0):
        eh, oh = torch.from_numpy(np.ascontiguousarray(e)), torch.from_numpy(np.ascontiguousarray(o))
        ed, od = eh.cuda(), oh.cuda()
        return lib.srh_scene_aoi_fill(ctx.handle, eh.data_ptr() if e_host else None, ed.data_ptr() + dev_off if e_dev else None, oh.data_ptr() if o_host else None,
                                      od.data_ptr() if o_dev else None, ni, ne, H, W, aw_p, invert, out_p, s)

    def edit(a, i, v):
        a = a.copy()
        a.reshape(-1)[i] = v
        return a

    bad = (dict(e_host=False), dict(e_dev=False), dict(o_host=False), dict(o_dev=False), dict(out_p=None), dict(H=0), dict(W=0), dict(H=-3), dict(H=65536, W=32768),
           dict(ni=-1, ne=3), dict(ni=1, ne=-1), dict(ni=40, ne=25, o=np.zeros(66, np.int32)), dict(o=edit(polys, 0, 1)), dict(o=edit(polys, 1, 5)),
           dict(o=edit(polys, 2, 1)), dict(o=np.array([0, 2, 16385], np.int32)), dict(e=edit(edges, 2, 0)), dict(e=edit(edges, 2, -5)), dict(e=edit(edges, 5, 2 ** 28 + 1)),
           dict(e=edit(edges, 4, -2 ** 28 - 1)), dict(invert=2), dict(invert=-1), dict(dev_off=4), dict(aw_p=out.data_ptr() + 8), dict(aw_p=out.data_ptr() - 60))
    for kw in bad:
        assert fill(**kw) == -1, kw
    assert lib.srh_scene_aoi_fill(None, None, None, None, None, 1, 1, 8, 8, None, 0, out.data_ptr(), s) == -1
    torch.cuda.synchronize()
    assert (buf.cpu().numpy() == 0xA5).all()                                      # nothing was launched: the guarded out is unchanged
    assert fill() == 0 and fill(aw_p=None, ni=0, ne=2) == 0
    torch.cuda.synchronize()
    assert _guards_ok(buf, 1, 64)
    with pytest.raises(_lib.SrhError, match="inconsistent table"):
        ctx.check(fill(e=edit(edges, 2, 0)), "srh_scene_aoi_fill")
    for kw in (dict(shape=(0, 5)), dict(polys=polys[:2]), dict(n_include=2), dict(and_with=aw[:7]), dict(out=out[:19]), dict(table_dev=torch.zeros(3, dtype=torch.int32, device=dev))):
        kw = dict(dict(shape=(8, 8), edges=edges, polys=polys, n_include=1, n_exclude=1), **kw)
        with pytest.raises(ValueError):
            net.scene_aoi_fill(kw.pop("shape"), kw.pop("edges"), kw.pop("polys"), kw.pop("n_include"), kw.pop("n_exclude"), **kw)
    torch.cuda.synchronize()


# ---- 6. against the oracle --------------------------------------------------------------------------------------------------------------------------------------
ORACLE_SCENE = "523x701"
ORACLE_AOI = [[[(-20, 60.25), (90.5, 690), (300, 740), (540, 610.5), (500.75, 40), (250, -10)], [(200, 300), (215.5, 420), (330, 405.25), (310, 290)]]]


def test_parity_with_the_oracle_inside_an_area_with_a_hole(pair):
    """check_scene_parity with valid = aoi_ref(...), the kit's bounds and caps unchanged, on the 523 x 701 scene of PARITY_SCENES under one
    include polygon of two rings in (row, col): the outer ring cuts all four borders of the scene, the hole lies inside.
    Chosen WITH THE ORACLE ALONE on the CPU (points from the oracle's own masks), so that the caps are conditions:
      valid share 0.8405, 20 tiles, 502 points (none off the area), 8352 voted edges, 744 oracle edges, the firm filter leaves out 0.49 %."""
    from sam_road_amd import Config
    from sam_road_amd.inferencer import infer_one_img
    oracle, net = pair
    H, W, per_edge, seed = PARITY_SCENES[ORACLE_SCENE]
    img = rect_scene(H, W, seed)
    aoi = [[[list(p) for p in ring] for ring in poly] for poly in ORACLE_AOI]
    valid = aoi_ref((H, W), _key(aoi)).astype(bool)
    ref = oracle_scene(oracle, img, per_edge, valid=valid)
    cfg = dict(CFG, INFER_PATCHES_PER_EDGE=per_edge, **thresholds(ref[2], ref[3]))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        got = infer_one_img(net, img, Config(dict(cfg, SCENE_AOI=aoi)))
    check_scene_parity(f"aoi_{ORACLE_SCENE}", got, ref, cfg, oracle, valid=valid, min_oracle_edges=200)
