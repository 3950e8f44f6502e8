"""SCENE_PAD (scenes padded at their borders on the device) on the HIP path.  Run on an MI355X: pytest -m gpu.

The reference has no such step, so the behaviour is pinned by COMPOSITION of what is already pinned: the kernel must equal numpy.pad
byte for byte, and a run with the key must equal, bit for bit, the existing pipeline on the numpy-padded scene (and mask), cropped — with
the graph built by hand from those cropped masks, that run's embeddings and the tiles moved into the real scene's frame (no tolerance).
The parity test against the CPU oracle does the same with oracle.scene's pieces and reuses the bounds of
test_rect_scene_parity_with_oracle (tests/tolerances.py).
"""
import warnings

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from scene_kit import CFG, FILL, check_scene_parity, kernel_rows, make_mask, np_pad, oracle_scene, pair, rect_grid, rect_scene  # noqa: F401
from scene_kit import crop_pads as _crop
from scene_kit import net_for as _net_for
from scene_kit import same_bits as _same
from scene_kit import shift_infos as _shift
from scene_kit import thresholds as _thresholds
from scene_kit import xy_of as _xy

MODES = ("reflect", "edge", "constant")
P, MARGIN, BS = CFG["PATCH_SIZE"], CFG["SAMPLE_MARGIN"], CFG["INFER_BATCH_SIZE"]


# ---- 1. the kernel ---------------------------------------------------------------------------------------------------------------------
# (H, W), (top, bottom, left, right): no pad at all, small pads, pads several times the axis (multiple reflections), axes of length 1,
# the odd row pitch of the scene tests, and a row of more than 16 KiB (two workgroups per row)
KERNEL_CASES = [((37, 53), (0, 0, 0, 0)), ((37, 53), (5, 9, 3, 1)), ((37, 53), (80, 3, 120, 0)), ((1, 64), (2, 3, 70, 9)), ((64, 1), (70, 9, 2, 3)),
                ((401, 523), (24, 24, 24, 24)), ((3, 6000), (1, 1, 5, 6))]


@pytest.mark.parametrize("shape,pads", KERNEL_CASES, ids=[f"{h}x{w}-{'_'.join(map(str, p))}" for (h, w), p in KERNEL_CASES])
def test_scene_pad_equals_numpy_pad(shape, pads):
    net = _net_for(P)
    H, W = shape
    rng = np.random.default_rng(H * 1000 + W)
    img = rng.integers(0, 256, size=(H, W, 3), dtype=np.uint8)
    mask = (rng.random((H, W)) < 0.5)
    for mode in MODES:
        for fill in (FILL, (0, 255, 7)):
            for src in (img, mask.astype(np.uint8) * 200, mask):
                t = torch.from_numpy(src).cuda()
                f = fill if src.ndim == 3 else (0 if src.dtype == bool else fill[0],) * 3      # a mask takes the first value
                out = net.scene_pad(t, pads, mode, f)
                want = np_pad(src, pads, mode, f)
                assert out.dtype == t.dtype and tuple(out.shape) == want.shape and out.data_ptr() != t.data_ptr()
                np.testing.assert_array_equal(out.cpu().numpy(), want, err_msg=f"{mode} {fill} {src.dtype} {src.shape}")
                np.testing.assert_array_equal(t.cpu().numpy(), src)              # the source is untouched
            if mode != "constant":
                break                                                            # the fill colour enters constant padding only
    # a source view at byte offsets 1 and 3 of a larger allocation: no address is 4-byte aligned against the destination's
    for off in (1, 3):
        for src in (img, mask.astype(np.uint8) * 255):
            big = torch.full((src.size + 16,), 0xA5, dtype=torch.uint8, device="cuda")
            v = big[off:off + src.size].view(src.shape)
            v.copy_(torch.from_numpy(src))
            before = big.cpu().numpy().copy()
            for mode in MODES:
                out = net.scene_pad(v, pads, mode, FILL)
                np.testing.assert_array_equal(out.cpu().numpy(), np_pad(src, pads, mode, FILL if src.ndim == 3 else (FILL[0],) * 3))
            np.testing.assert_array_equal(big.cpu().numpy(), before)


def test_scene_pad_rejects_bad_arguments():
    from sam_road_amd import _lib
    net = _net_for(P)
    dev = torch.device("cuda")
    ctx, _ = net._weights(dev)
    buf = torch.zeros(4096, dtype=torch.uint8, device=dev)
    p, s, lib = buf.data_ptr(), net._stream(dev), ctx.lib
    import ctypes
    rgb = (ctypes.c_int32 * 3)(1, 2, 3)
    ok = (8, 8, 3, 1, 1, 1, 1, 0)
    assert lib.srh_scene_pad(ctx.handle, p, *ok, rgb, p + 2048, s) == 0
    for bad in ((8, 8, 2, 1, 1, 1, 1, 0), (8, 8, 4, 1, 1, 1, 1, 0), (8, 8, 3, -1, 1, 1, 1, 0), (8, 8, 3, 1, 1, 1, -2, 0), (8, 8, 3, 1, 1, 1, 1, 3),
                (8, 8, 3, 1, 1, 1, 1, -1), (0, 8, 3, 1, 1, 1, 1, 0), (8, -8, 3, 1, 1, 1, 1, 0), (46341, 46341, 1, 0, 0, 0, 0, 0),
                (8, 8, 1, 2 ** 30, 2 ** 30, 0, 0, 0), (40000, 40000, 1, 3200, 3200, 3200, 3200, 0), (8, 8, 3, 2 ** 31 - 1, 2 ** 31 - 1, 0, 0, 0)):
        assert lib.srh_scene_pad(ctx.handle, p, *bad, rgb, p + 2048, s) == -1, bad
    for fill in ((256, 0, 0), (0, -1, 0), (0, 0, 1000)):
        assert lib.srh_scene_pad(ctx.handle, p, *ok, (ctypes.c_int32 * 3)(*fill), p + 2048, s) == -1, fill
    assert lib.srh_scene_pad(ctx.handle, None, *ok, rgb, p + 2048, s) == -1
    assert lib.srh_scene_pad(ctx.handle, p, *ok, rgb, None, s) == -1
    assert lib.srh_scene_pad(ctx.handle, p, *ok[:7], 2, None, p + 2048, s) == -1           # constant needs the colour
    assert lib.srh_scene_pad(ctx.handle, p, *ok, None, p + 2048, s) == 0                   # the others do not
    with pytest.raises(_lib.SrhError):
        ctx.check(lib.srh_scene_pad(ctx.handle, p, 8, 8, 2, 1, 1, 1, 1, 0, rgb, p + 2048, s), "srh_scene_pad")
    for bad in (torch.zeros((8, 8, 3), dtype=torch.float32, device=dev), torch.zeros((8, 8, 4), dtype=torch.uint8, device=dev),
                torch.zeros((8, 16, 3), dtype=torch.uint8, device=dev)[:, ::2]):
        with pytest.raises(ValueError):
            net.scene_pad(bad, (1, 1, 1, 1))
    with pytest.raises(ValueError):
        net.scene_pad(buf[:192].view(8, 8, 3), (1, 1, 1, 1), "wrap")
    with pytest.raises(ValueError):
        net.scene_pad(buf[:192].view(8, 8, 3), (1, -1, 1, 1))
    torch.cuda.synchronize()


# ---- 2. / 3. a run with the key == the existing pipeline on the numpy-padded scene, cropped ------------------------------------------------
def _check_against_composition(net, img, per_edge, key, pads, mode="reflect", least=20):
    """Both equalities of the issue for an unmasked scene; returns the run's tuple."""
    from sam_road_amd import Config
    from sam_road_amd.graph_points import extract_graph_points
    from sam_road_amd.inferencer import edge_votes, infer_one_img, scene_pad_plan, scene_tiles, votes_to_edges
    H, W = img.shape[:2]
    padded = np_pad(img, pads, mode)
    Hv, Wv = padded.shape[:2]
    infos = rect_grid(Hv, Wv, MARGIN, P, per_edge)
    xy = _xy(infos)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        kp_c, road_c, emb = net.scene_pass1(torch.from_numpy(padded).cuda(), xy, BS)
        kp_u8, road_u8 = net.scene_normalise(kp_c, road_c, xy)
        kp_m, road_m = _crop(kp_u8.cpu().numpy(), pads, (H, W)), _crop(road_u8.cpu().numpy(), pads, (H, W))
        thr = _thresholds(kp_m, road_m)
        plain = Config(dict(CFG, INFER_PATCHES_PER_EDGE=per_edge, **thr))
        cfg = Config(dict(plain, SCENE_PAD=key))
        assert scene_pad_plan(img.shape, cfg)[:4] == tuple(pads)
        tiles = scene_tiles(img.shape, cfg)
        assert list(tiles) == _shift(infos, pads) and tiles.pads == tuple(pads)
        whole = infer_one_img(net, padded, plain)                                # the existing pipeline on the host-padded scene
        img_before = img.copy()
        nodes, edges, kp_o, road_o = infer_one_img(net, img, cfg)
    np.testing.assert_array_equal(img, img_before)
    assert kp_o.shape == road_o.shape == (H, W) and kp_o.dtype == road_o.dtype == np.uint8
    _same(kp_o, _crop(whole[2], pads, (H, W)))
    _same(road_o, _crop(whole[3], pads, (H, W)))
    _same(kp_o, kp_m)
    _same(road_o, road_m)
    pts = extract_graph_points(kp_m, road_m, plain)
    _same(nodes, pts[:, ::-1])
    assert pts.shape[0] > least
    assert nodes[:, 0].max() < H and nodes[:, 1].max() < W and nodes.min() >= 0  # no node in the padding
    votes = edge_votes(net, emb, pts, _shift(infos, pads), 0, len(infos), plain, torch.device("cuda"))
    _same(edges, votes_to_edges(*votes, pts.shape[0], plain.TOPO_THRESHOLD))
    print(f"{H}x{W} pads {pads} {mode}: {len(infos)} tiles, {pts.shape[0]} points, {edges.shape[0]} edges")
    assert edges.shape[0] > least
    return (nodes, edges, kp_o, road_o), cfg, plain


def test_scene_smaller_than_a_tile(pair):
    """200 x 300 at PATCH_SIZE 256, margin 16: the height lacks 88 px, so 44 rows are mirrored on at the top and at the bottom."""
    from sam_road_amd import Config
    from sam_road_amd.inferencer import infer_one_img
    _, net = pair
    img = rect_scene(200, 300, 45)
    with pytest.raises(ValueError, match="smaller than"):
        infer_one_img(net, img, Config(dict(CFG, INFER_PATCHES_PER_EDGE=[1, 2])))
    (nodes, edges, kp, road), _, _ = _check_against_composition(net, img, [1, 2], {"border": 0}, (44, 44, 0, 0), least=5)   # 60 k pixels: a small graph
    assert kp.shape == (200, 300)
    assert road[:MARGIN].any() and road[-MARGIN:].any() and not road[:, :MARGIN].any()   # rows reach the border now, the columns' margin stays 0


def test_border_on_the_odd_pitch_scene(pair):
    from sam_road_amd import Config, _lib
    from sam_road_amd.inferencer import infer_one_img
    _, net = pair
    img = rect_scene(401, 523, 43)
    got, cfg, plain = _check_against_composition(net, img, 4, 24, (24, 24, 24, 24))
    # the unpadded run leaves the 16-px frame at 0; the padded one predicts there
    bare = infer_one_img(net, img, plain)
    assert not bare[3][:MARGIN].any() and not bare[3][:, -MARGIN:].any() and got[3][:MARGIN].any() and got[3][:, -MARGIN:].any()
    # border 0 on a scene that is large enough: the bytes of a run without the key, and the pad kernel is not launched
    ctx = _lib.Context.get(torch.cuda.current_device())
    with kernel_rows(ctx) as rows:
        zero = infer_one_img(net, img, Config(dict(plain, SCENE_PAD={"border": 0, "mode": "edge"})))
        rows_zero = rows()
        infer_one_img(net, img, cfg)
        rows_pad = rows()
        infer_one_img(net, img, plain)
        rows_plain = rows()
    for a, b in zip(zero, bare):
        _same(a, b)
    assert "scene_pad" not in rows_zero and rows_zero == rows_plain and rows_pad == rows_plain | {"scene_pad"}


# ---- 4. everything at once ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["edge", "constant"])
def test_pad_with_mask_window_and_tta(pair, mode):
    """384 x 640, border [8, 40], the band mask, FUSE_WINDOW hann, TTA [id, rot90]: equals the existing pipeline on the host-padded scene
    and the host-padded mask.  edge replicates the mask's validity; constant padding is nodata."""
    from sam_road_amd import Config
    from sam_road_amd.graph_points import extract_graph_points
    from sam_road_amd.inferencer import edge_votes, infer_one_img, scene_tiles, votes_to_edges
    _, net = pair
    H, W, per_edge, pads = 384, 640, [3, 5], (8, 8, 40, 40)
    img, valid = rect_scene(H, W, 41), make_mask("band", H, W)
    extra = dict(FUSE_WINDOW="hann", TTA=["id", "rot90"])
    padded, valid_p = np_pad(img, pads, mode), np_pad(valid, pads, mode, (0, 0, 0))
    assert valid_p.dtype == bool and valid_p.shape == (400, 720)
    if mode == "constant":
        assert not valid_p[:8].any() and not valid_p[:, :40].any() and not valid_p[:, -40:].any()
    base = Config(dict(CFG, INFER_PATCHES_PER_EDGE=per_edge, **extra))
    _, _, kp0, road0 = infer_one_img(net, padded, base, valid=valid_p)
    plain = Config(dict(base, **_thresholds(_crop(kp0, pads, (H, W)), _crop(road0, pads, (H, W)))))
    cfg = Config(dict(plain, SCENE_PAD={"border": [8, 40], "mode": mode}))
    whole = infer_one_img(net, padded, plain, valid=valid_p)
    nodes, edges, kp, road = infer_one_img(net, img, cfg, valid=valid)
    kp_m, road_m = _crop(whole[2], pads, (H, W)), _crop(whole[3], pads, (H, W))
    _same(kp, kp_m)
    _same(road, road_m)
    assert not kp[~valid].any() and not road[~valid].any() and road[valid].any()
    # the kept tiles are those numpy selects on the padded mask, in the real scene's frame
    infos_v = rect_grid(400, 720, MARGIN, P, per_edge)
    kept_v = [t for t in infos_v if valid_p[t[1][1]:t[2][1], t[1][0]:t[2][0]].any()]
    kept = scene_tiles(img.shape, cfg, valid=valid, net=net)
    assert list(kept) == _shift(kept_v, pads) and kept.pads == pads and kept.orientations == ["id", "rot90"]
    assert list(scene_tiles(padded.shape, plain, valid=valid_p, net=net)) == kept_v
    print(f"{mode}: {len(kept_v)} of {len(infos_v)} tiles kept")
    # the graph: points from the cropped masks; edges from the embeddings of orientation id (those of a run without TTA, bit for bit) of the
    # kept tiles on the filled padded scene, with the tiles moved to the real scene's frame
    pts = extract_graph_points(kp_m, road_m, plain)
    _same(nodes, pts[:, ::-1])
    assert pts.shape[0] > 20 and valid[nodes[:, 0], nodes[:, 1]].all()
    filled = np.ascontiguousarray(np.where(valid_p[..., None], padded, np.array(FILL, np.uint8)))
    _, _, emb = net.scene_pass1(torch.from_numpy(filled).cuda(), _xy(kept_v), BS)
    votes = edge_votes(net, emb, pts, _shift(kept_v, pads), 0, len(kept_v), plain, torch.device("cuda"))
    _same(edges, votes_to_edges(*votes, pts.shape[0], plain.TOPO_THRESHOLD))
    assert edges.shape[0] > 20


def test_constant_padding_is_nodata_tiles_wholly_in_it_are_dropped(pair):
    """A 200 x 300 scene under 300 rows of constant padding above and below, every real pixel valid: of the four tile rows of the 800-row
    virtual scene, the first and the last lie wholly in the padding and are dropped; reflect / edge padding keeps all four."""
    from sam_road_amd import Config
    from sam_road_amd.inferencer import infer_one_img, scene_tiles
    _, net = pair
    img, valid = rect_scene(200, 300, 46), np.ones((200, 300), bool)
    cfg = dict(CFG, INFER_PATCHES_PER_EDGE=[4, 1])
    ys = [16, 187, 357, 528]
    assert [t[1][1] for t in rect_grid(800, 300, MARGIN, P, [4, 1])] == ys
    for mode, want in (("constant", ys[1:3]), ("reflect", ys), ("edge", ys)):
        c = Config(dict(cfg, SCENE_PAD={"border": [300, 0], "mode": mode}))
        tiles = scene_tiles(img.shape, c, valid=valid, net=net)
        assert [t[1][1] for t in tiles] == [y - 300 for y in want] and tiles.pads == (300, 300, 0, 0), mode
    c = Config(dict(cfg, SCENE_PAD={"border": [300, 0], "mode": "constant"}))
    padded, valid_p = np_pad(img, (300, 300, 0, 0), "constant"), np_pad(valid, (300, 300, 0, 0), "constant", (0, 0, 0))
    whole = infer_one_img(net, padded, Config(cfg), valid=valid_p)
    got = infer_one_img(net, img, c, valid=valid)
    _same(got[2], _crop(whole[2], (300, 300, 0, 0), (200, 300)))
    _same(got[3], _crop(whole[3], (300, 300, 0, 0), (200, 300)))
    assert got[3].any()


# ---- 5. the loops ------------------------------------------------------------------------------------------------------------------------
def test_infer_imgs_pipelined_equals_infer_one_img(pair):
    """[small scene, 401 x 523, small scene] through the software-pipelined loop — the third scene reuses the first one's page-locked staging,
    the second has another virtual size — and once more with a mask on the middle scene (its count kernel runs on the upload lane, after
    the pad of the compute stream): infer_one_img's tuples, in order."""
    from sam_road_amd import Config
    from sam_road_amd.inferencer import infer_imgs, infer_one_img
    _, net = pair
    imgs = [rect_scene(200, 300, 45), rect_scene(401, 523, 43), rect_scene(200, 300, 47)]
    base = Config(dict(CFG, SCENE_PAD=24))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        _, _, kp0, road0 = infer_one_img(net, imgs[1], base)
        cfg = Config(dict(base, **_thresholds(kp0, road0)))
        want = [infer_one_img(net, im, cfg) for im in imgs]
        print("points / edges per scene:", [(w[0].shape[0], w[1].shape[0]) for w in want])
        assert [w[2].shape for w in want] == [(200, 300), (401, 523), (200, 300)]
        assert want[1][0].shape[0] > 20 and want[1][1].shape[0] > 20 and all(w[0].shape[0] > 5 and w[1].shape[0] > 5 for w in want)
        for _ in range(2):
            got = list(infer_imgs(net, iter(imgs), cfg))
            assert len(got) == 3
            for w, g in zip(want, got):
                for a, b in zip(w, g):
                    _same(a, b)
        valids = [None, make_mask("band", 401, 523), np.ones((200, 300), bool)]
        want_v = [infer_one_img(net, im, cfg, valid=v) for im, v in zip(imgs, valids)]
        assert not want_v[1][3][~valids[1]].any() and want_v[1][0].shape[0] > 5
        for w, g in zip(want_v, infer_imgs(net, iter(imgs), cfg, valids=iter(valids))):
            for a, b in zip(w, g):
                _same(a, b)
        for a, b in zip(want_v[2], want[2]):                                      # an all-true mask is no mask
            _same(a, b)


# ---- 6. against the oracle ------------------------------------------------------------------------------------------------------------------
def test_padded_scene_parity_with_oracle(pair):
    """The checks and bounds of test_rect_scene_parity_with_oracle (tests/tolerances.py) on the 523 x 701 scene with a reflected border of
    24 px: the oracle runs oracle.scene's pieces on the numpy-padded scene, its masks are cropped, its pass 2 takes the shifted tiles."""
    from sam_road_amd import Config
    from sam_road_amd.inferencer import infer_one_img
    oracle, net = pair
    H, W, per_edge, seed, pads = 523, 701, [4, 5], 44, (24, 24, 24, 24)
    img = rect_scene(H, W, seed)
    ref = oracle_scene(oracle, img, per_edge, pads=pads)
    assert ref[2].shape == ref[3].shape == (H, W) and ref[0] == _shift(rect_grid(H + 48, W + 48, MARGIN, P, per_edge), pads)
    cfg = dict(CFG, INFER_PATCHES_PER_EDGE=per_edge, SCENE_PAD=24, **_thresholds(ref[2], ref[3]))
    got = infer_one_img(net, img, Config(cfg))
    check_scene_parity(f"pad24_{H}x{W}", got, ref, cfg, oracle)
    for mask in got[2:]:
        # the border of 24 px closes the 16-px frame no tile covered: every pixel of the real scene is covered now
        assert (mask[:MARGIN] > 0).any() and (mask[-MARGIN:] > 0).any() and (mask[:, :MARGIN] > 0).any() and (mask[:, -MARGIN:] > 0).any()
