"""TTA (test-time augmentation over the 8 tile orientations) on the HIP path.  Run on an MI355X: pytest -m gpu.

The reference has no TTA, so the behaviour is pinned exactly, by what is already pinned:
  * the oriented crop + im2col must give, bit for bit, the A matrix the unchanged kernel writes for a tile that was oriented on the
    host, and the score un-orient must be the permutation `unorient_tile` (bit patterns compared as uint32);
  * the scene-level call must equal, bit for bit, the COMPOSITION of pieces that exist without this feature: host-oriented u8 tiles
    through infer_masks_and_img_features, un-oriented in numpy, added by the existing add, normalised with the k-fold tile list;
  * against the CPU oracle, with the checks and bounds of test_rect_scene_parity_with_oracle, unchanged.
No statement about the quality of the roads is made: there are no trained weights here.
State: written and checked on the CPU (index maps, oracle conditions); not yet run on a device.
"""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import scene as oscene
from oracle.samroad import AttrDict

from scene_kit import (CFG, FILL, NAMES, PARITY_SCENES, SCENES, check_scene_parity, kernel_rows, make_mask, np_kept, oracle_scene, pair,  # noqa: F401
                       rect_grid, rect_scene)
from scene_kit import dev as _dev
from scene_kit import net_for as _net_for
from scene_kit import same_bits as _same
from scene_kit import thresholds as _thresholds
from scene_kit import xy_of as _xy


def _helpers():
    from sam_road_amd.inferencer import orient_tile, unorient_tile
    return orient_tile, unorient_tile


# ---- 1. oriented crop + normalise + im2col, bit for bit ------------------------------------------------------------------------------
def _f16_ordinal(a):
    """f16 bit patterns as integers that are monotone in the value: the difference of two is their distance in ulps."""
    i = np.ascontiguousarray(a).view(np.int16).astype(np.int32)
    return np.where(i < 0, -(i & 0x7FFF), i)


@pytest.mark.parametrize("P", [128, 208, 512])
def test_oriented_im2col_equals_the_plain_kernel_on_host_oriented_tiles(P):
    orient_tile, _ = _helpers()
    net = _net_for(P)
    H, W = 2 * P + 17, 2 * P + P // 4 + 1
    assert W % 2 == 1 and (W * 3) % 4 != 0                                      # rows are not 4-byte aligned against each other
    rng = np.random.default_rng(P)
    scene = rng.integers(0, 256, size=(H, W, 3), dtype=np.uint8)
    # the four corners, an x0 with x0 % 4 == 3, origins not divisible by 4 or 16, one tile twice
    xy = np.array([[0, 0], [W - P, 0], [0, H - P], [W - P, H - P], [7, 5], [P // 2 + 1, 13], [19, H - P - 3], [7, 5]], dtype=np.int32)
    assert xy[4, 0] % 4 == 3 and xy[:, 0].max() + P <= W and xy[:, 1].max() + P <= H
    n, S = len(xy), P // 16
    scene_d, xy_d = _dev(scene), _dev(xy)
    side_xy = _dev(np.array([[i * P, 0] for i in range(n)], dtype=np.int32))
    crops = [scene[y0:y0 + P, x0:x0 + P] for x0, y0 in xy.tolist()]
    got_id = net.op_patch_im2col(scene_d, xy_d, orient=0).cpu().numpy()
    assert got_id.dtype == np.float16 and got_id.shape == (n * S * S, 768)
    # id against the f32 formula rounded to f16: within 1 f16 ulp (the kernel multiplies by the f32 reciprocal of std)
    mean = np.array([123.675, 116.28, 103.53], np.float32)
    std = np.array([58.395, 57.12, 57.375], np.float32)
    ref = np.stack([((c.astype(np.float32) - mean) / std).reshape(S, 16, S, 16, 3).transpose(0, 2, 1, 3, 4).reshape(S * S, 768) for c in crops])
    ulp = np.abs(_f16_ordinal(got_id) - _f16_ordinal(ref.reshape(-1, 768).astype(np.float16)))
    print(f"[tta] im2col id vs f32 formula, P={P}: max {ulp.max()} f16 ulp, differing {np.count_nonzero(ulp)} of {ulp.size}")
    assert ulp.max() <= 1
    seen = set()
    for code, name in enumerate(NAMES):
        side = np.ascontiguousarray(np.concatenate([orient_tile(c, name) for c in crops], axis=1))      # [P, n P, 3]
        want = net.op_patch_im2col(_dev(side), side_xy, orient=0).cpu().numpy()
        got = net.op_patch_im2col(scene_d, xy_d, orient=code).cpu().numpy()
        np.testing.assert_array_equal(got.view(np.uint16), want.view(np.uint16), err_msg=f"P={P} {name}")
        seen.add(got.tobytes())
    assert len(seen) == 8                                                       # the 8 orientations give 8 different matrices
    # a scene whose base address is off the 4-byte grid: a view into a larger allocation, filled to its last byte
    big = torch.zeros(H * W * 3 + 8, dtype=torch.uint8, device="cuda")
    for off in (1, 3):
        v = big[off:off + H * W * 3].view(H, W, 3)
        v.copy_(scene_d)
        for code in (5, 6):
            want = net.op_patch_im2col(scene_d, xy_d, orient=code)
            assert torch.equal(net.op_patch_im2col(v, xy_d, orient=code).view(torch.int16), want.view(torch.int16)), (off, code)


# ---- 2. the score un-orient is a permutation of bit patterns --------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 5])
@pytest.mark.parametrize("P", [128, 208, 512])
def test_scores_unorient_is_the_permutation(P, n):
    _, unorient_tile = _helpers()
    net = _net_for(P)
    rng = np.random.default_rng(P * 10 + n)
    scores = rng.standard_normal((n, P, P, 2)).astype(np.float32)
    bits = scores.view(np.uint32)
    bits[:, ::7, 3::5, 0] = 0x80000000                                          # negative zero
    bits[:, 1::9, ::4, 1] = 0x7FC12345                                          # NaN payloads: nothing may compute with the values
    bits[:, 2::11, 1::6, 0] = 0xFFA00001
    src = _dev(scores)
    for code, name in enumerate(NAMES):
        got = net.op_scores_unorient(src, code).cpu().numpy().view(np.uint32)
        want = np.stack([np.ascontiguousarray(unorient_tile(t, name)) for t in bits])
        np.testing.assert_array_equal(got, want, err_msg=f"P={P} n={n} {name}")
    np.testing.assert_array_equal(src.cpu().numpy().view(np.uint32), bits)      # the input is left alone


# ---- 3. the scene call is the composition of the pieces, bit for bit -------------------------------------------------------------------
def _compose(net, filled, infos, names, w_d, bs):
    """Pass 1 with TTA from pieces that exist without it: (canvas_kp, canvas_road, id embeddings)."""
    orient_tile, unorient_tile = _helpers()
    H, W = filled.shape[:2]
    xy = _xy(infos)
    kp_f, road_f = torch.zeros((H, W), device="cuda"), torch.zeros((H, W), device="cuda")
    embs = []
    for name in names:
        for off in range(0, len(infos), bs):
            tiles = np.stack([orient_tile(filled[y0:y1, x0:x1], name) for _, (x0, y0), (x1, y1) in infos[off:off + bs]])
            scores, e = net.infer_masks_and_img_features(_dev(tiles))
            back = np.stack([unorient_tile(t, name) for t in scores.cpu().numpy()])
            net.op_scene_fuse_window(_dev(back), xy[off:off + bs].contiguous(), w_d, kp_f, road_f)
            if name == "id":
                embs.append(e)
    return kp_f, road_f, torch.cat(embs)


COMPOSITION_CASES = [(list(NAMES), None, None), (["id", "rot90", "flip_v"], "hann", None), (["id", "transpose"], None, "band")]


@pytest.mark.parametrize("names,window,kind", COMPOSITION_CASES)
def test_tta_run_equals_composition_bit_for_bit(pair, names, window, kind):
    from sam_road_amd import Config
    from sam_road_amd.graph_points import extract_graph_points
    from sam_road_amd.inferencer import edge_votes, fuse_window, infer_one_img, scene_tiles, tta_plan, votes_to_edges
    _, net = pair
    H, W, per_edge, seed = SCENES["401x523"]
    P, bs = CFG["PATCH_SIZE"], CFG["INFER_BATCH_SIZE"]
    img = rect_scene(H, W, seed)
    infos = rect_grid(H, W, CFG["SAMPLE_MARGIN"], P, per_edge)
    valid, filled = None, img
    if kind is not None:
        valid = make_mask(kind, H, W)
        kept = np_kept(valid, infos, P)
        assert 0 < len(kept) <= len(infos)
        infos = [infos[i] for i in kept]
        filled = np.ascontiguousarray(np.where(valid[..., None], img, np.array(FILL, np.uint8)))
    base = dict(CFG, INFER_PATCHES_PER_EDGE=per_edge, TTA=names, **({} if window is None else dict(FUSE_WINDOW=window)))
    codes = tta_plan(Config(base))[1]
    assert codes == [NAMES.index(n) for n in names]
    k = len(names)
    w1 = fuse_window(Config(base))
    wkw = {} if w1 is None else dict(window=_dev(w1))
    ones = torch.ones(P, device="cuda")                                         # the header: an all-ones profile gives the bytes of the unweighted add
    xy, scene_d = _xy(infos), _dev(filled)
    valid_d = None if valid is None else _dev(valid)
    kp_f, road_f, emb_f = _compose(net, filled, infos, names, wkw.get("window", ones), bs)
    kp_c, road_c, emb = net.scene_pass1(scene_d, xy, bs, tta=codes, **wkw)
    _same(kp_c.cpu().numpy(), kp_f.cpu().numpy())
    _same(road_c.cpu().numpy(), road_f.cpu().numpy())
    kp0, road0, emb0 = net.scene_pass1(scene_d, xy, bs, **wkw)                  # a plain run: the same embeddings, other canvases
    _same(emb.cpu().numpy(), emb0.cpu().numpy())
    _same(emb.cpu().numpy(), emb_f.cpu().numpy())
    assert not np.array_equal(kp_c.cpu().numpy(), kp0.cpu().numpy())
    # normalise = the existing entry with the k-fold list
    vkw = {} if valid is None else dict(valid=valid_d)
    kp_u8, road_u8 = net.scene_normalise(kp_c, road_c, xy.repeat(k, 1), **wkw, **vkw)
    kp_m, road_m = kp_u8.cpu().numpy(), road_u8.cpu().numpy()
    plain = net.scene_normalise(kp0, road0, xy, **wkw, **vkw)
    assert not np.array_equal(kp_m, plain[0].cpu().numpy())                     # TTA changes the masks
    # the whole call
    cfg = Config(dict(base, **_thresholds(kp_m, road_m)))
    plan = scene_tiles((H, W), cfg, **({} if valid is None else dict(valid=valid, net=net)))
    assert plan == infos and plan.orientations == names
    nodes, edges, kp_o, road_o = infer_one_img(net, img, cfg, valid=valid)
    _same(kp_o, kp_m)
    _same(road_o, road_m)
    pts = extract_graph_points(kp_m, road_m, cfg)
    _same(nodes, pts[:, ::-1])
    assert pts.shape[0] > 20
    votes = edge_votes(net, emb, pts, infos, 0, len(infos), cfg, torch.device("cuda"))      # pass 2 sees the id embeddings only
    _same(edges, votes_to_edges(*votes, pts.shape[0], cfg.TOPO_THRESHOLD))
    assert edges.shape[0] > 20
    if valid is not None:
        assert not kp_o[~valid].any() and not road_o[~valid].any() and valid[nodes[:, 0], nodes[:, 1]].all()


# ---- 4. identities --------------------------------------------------------------------------------------------------------------------
def test_id_alone_is_the_key_absent_and_the_batch_size_changes_no_byte(pair):
    from sam_road_amd import Config
    from sam_road_amd.inferencer import infer_one_img
    _, net = pair
    H, W, per_edge, seed = SCENES["401x523"]
    img = rect_scene(H, W, seed)
    base = dict(CFG, INFER_PATCHES_PER_EDGE=per_edge)
    _, _, kp0, road0 = infer_one_img(net, img, Config(base))
    base.update(_thresholds(kp0, road0))
    want = infer_one_img(net, img, Config(base))
    assert want[0].shape[0] > 20 and want[1].shape[0] > 20
    for v in (["id"], None, "id"):
        for a, b in zip(infer_one_img(net, img, Config(dict(base, TTA=v))), want):
            _same(a, b)
    # the summation order is (orientation, tile): cutting the list into other batches changes no byte of the canvases
    xy = _xy(rect_grid(H, W, CFG["SAMPLE_MARGIN"], CFG["PATCH_SIZE"], per_edge))
    scene_d = _dev(img)
    a = net.scene_pass1(scene_d, xy, 5, tta=[0, 6, 1])
    b = net.scene_pass1(scene_d, xy, 2, tta=[0, 6, 1])
    for name, x, y in zip(("kp", "road"), a[:2], b[:2]):
        x, y = x.cpu().numpy(), y.cpu().numpy()
        d = np.abs(x - y)
        print(f"[tta] canvas {name}, INFER_BATCH_SIZE 5 vs 2: {np.count_nonzero(x.view(np.uint32) != y.view(np.uint32))} of {x.size} values differ, max abs {d.max():.3e}")
    _same(a[0].cpu().numpy(), b[0].cpu().numpy())
    _same(a[1].cpu().numpy(), b[1].cpu().numpy())


def test_infer_imgs_with_tta_equals_serial(pair):
    from sam_road_amd import Config
    from sam_road_amd.inferencer import infer_imgs, infer_one_img
    _, net = pair
    shapes = [(384, 640), (401, 523)]
    imgs = [rect_scene(h, w, 50 + i) for i, (h, w) in enumerate(shapes)]
    names = ["id", "anti_transpose", "flip_h"]
    _, _, kp0, road0 = infer_one_img(net, imgs[0], Config(dict(CFG, TTA=names)))
    cfg = Config(dict(CFG, TTA=names, **_thresholds(kp0, road0)))
    want = [infer_one_img(net, im, cfg) for im in imgs]
    print("points / edges per scene:", [(w[0].shape[0], w[1].shape[0]) for w in want])
    assert all(w[0].shape[0] > 20 and w[1].shape[0] > 20 for w in want)
    got = list(infer_imgs(net, iter(imgs), cfg))
    assert len(got) == len(want)
    for w, g in zip(want, got):
        for a, b in zip(w, g):
            _same(a, b)


# ---- 5. profile rows ------------------------------------------------------------------------------------------------------------------
def test_profile_rows_and_abi_rejections(pair):
    from sam_road_amd import Config, _lib
    from sam_road_amd.inferencer import infer_one_img
    _, net = pair
    dev = torch.device("cuda")
    H, W, per_edge, seed = SCENES["384x640"]
    img = rect_scene(H, W, seed)
    base = dict(CFG, INFER_PATCHES_PER_EDGE=per_edge)
    ctx = _lib.Context.get(torch.cuda.current_device())
    new = {"patch_im2col_oriented", "scores_unorient"}
    with kernel_rows(ctx) as rows:
        infer_one_img(net, img, Config(base))
        infer_one_img(net, img, Config(dict(base, TTA=["id"])))
        plain = rows()
        infer_one_img(net, img, Config(dict(base, TTA=["id", "flip_v", "rot270"])))
        tta = rows()
        print("kernel classes, plain:", sorted(plain), "| TTA:", sorted(tta))
        assert not (new & plain) and {"patch_im2col", "scene_add", "scene_count", "scene_normalise"} <= plain
        assert new <= tta and plain <= tta                                      # id's batches take today's path
        # ---- 6. the entry rejects a bad orientation list and launches nothing
        _, wh = net._weights(dev)
        scene = torch.zeros((384, 640, 3), dtype=torch.uint8, device=dev)
        xy = torch.zeros((1, 2), dtype=torch.int32, device=dev)
        kp, road = torch.zeros((384, 640), device=dev), torch.zeros((384, 640), device=dev)
        emb = torch.zeros((1, 16, 16, 256), device=dev)
        s, lib = net._stream(dev), ctx.lib

        def call(codes, k=None, orients="given"):
            arr = (ctypes.c_uint8 * max(1, len(codes)))(*codes)
            return lib.srh_scene_pass1_tta_hw(ctx.handle, wh, scene.data_ptr(), 384, 640, xy.data_ptr(), 1, 5, arr if orients == "given" else None,
                                              len(codes) if k is None else k, None, kp.data_ptr(), road.data_ptr(), emb.data_ptr(), s)
        for codes, k in (([1, 0], None), ([5], None), ([0, 8], None), ([0, 3, 3], None), ([0, 0], None), ([0], 0), (list(range(8)) + [0], 9), ([0], -1)):
            assert call(codes, k) == -1, (codes, k)
        assert call([0], orients=None) == -1
        assert not rows() and not kp.any() and not road.any()               # SRH_ERR_BAD_ARG before anything is launched
        assert call([0, 5]) == 0                                                # the same arguments with a good list run
        assert new <= rows() and kp.any()
        with pytest.raises(ValueError, match="tta"):
            net.scene_pass1(scene, xy, 5, tta=[])


# ---- 7. against the oracle ------------------------------------------------------------------------------------------------------------
ORACLE_TTA = ["id", "rot90", "flip_h"]        # three orientations keep the CPU oracle within seconds
# The scene was chosen WITH THE ORACLE ALONE on the CPU (points from the oracle's own masks):
#   (tiles, points, voted edges, oracle edges, share within TOPO_SCORE of the threshold)
#   384x640: 15, 468, 8670, 650, 0.52 %      401x523: 16, 230, 3567, 428, 0.62 %      523x701: 20, 515, 8360, 748, 0.47 %
ORACLE_SCENE = "384x640"


def test_tta_scene_parity_with_oracle(pair):
    """The assertions and bounds of test_rect_scene_parity_with_oracle (tests/tolerances.py) on a TTA-fused scene: the oracle's per-tile
    scores on oriented tiles, un-oriented and fused by oscene.fuse_masks over the k-fold info list."""
    from sam_road_amd import Config
    from sam_road_amd.inferencer import infer_one_img
    oracle, net = pair
    H, W, per_edge, seed = PARITY_SCENES[ORACLE_SCENE]
    img = rect_scene(H, W, seed)
    ref = oracle_scene(oracle, img, per_edge, orientations=ORACLE_TTA)
    cfg = dict(CFG, INFER_PATCHES_PER_EDGE=per_edge, TTA=ORACLE_TTA, **_thresholds(ref[2], ref[3]))
    assert oscene.extract_graph_points(ref[2], ref[3], AttrDict(cfg)).shape[0] > 20      # and on the oracle's own masks
    check_scene_parity(f"tta_{ORACLE_SCENE}", infer_one_img(net, img, Config(cfg)), ref, cfg, oracle)
