"""Rectangular scenes (H x W, H != W) through the whole scene pipeline on the HIP path.  Run on an MI355X: pytest -m gpu.

There is no reference behaviour for H != W (the reference reads img.shape[0] for both axes), so the main check needs no tolerance: a
rectangular scene embedded in the top-left corner of a zero square scene, run through the SQUARE C entry points (srh_scene_pass1 /
srh_scene_normalise, one `int S`) with the rectangle's tile origins, reads identical pixels through identical kernels — the
rectangular entry points must give the same bits.  The parity tests against the CPU oracle reuse the bounds tests/test_gpu_scene.py
applies to this very configuration; the oracle's tile list is built in tests/scene_kit.py, independently of sam_road_amd/tiling.py.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import scene as oscene
from oracle.synth import synth_scene

from scene_kit import CFG, check_scene_parity, oracle_scene, pair, rect_grid, rect_scene, thresholds  # noqa: F401  (pair is a fixture)
from scene_kit import same_bits as _same_bits
from scene_kit import xy_of as _xy

# (H, W, INFER_PATCHES_PER_EDGE, scene seed): H < W with a ragged last batch (15 tiles, batch 5 ... 3 x 5), H > W, and an odd
# pitch whose rows are not 4-byte aligned.  Seeds and the percentile thresholds below were chosen WITH THE ORACLE ALONE on the CPU:
#   384x640 seed 41: 453 points, 8419 voted edges, 0.38 % of them within TOPO_SCORE of the threshold
#   640x384 seed 42: 489 points, 9302 voted edges, 0.22 %
#   401x523 seed 43: 260 points, 4183 voted edges, 0.77 %
SCENES = [(384, 640, [3, 5], 41), (640, 384, [5, 3], 42), (401, 523, 4, 43)]


def _abi_pass1(net, entry, scene, dims, xy, bs):
    """One of the two C entries, called directly: entry "srh_scene_pass1" with dims (S,), "srh_scene_pass1_hw" with (H, W)."""
    dev = scene.device
    ctx, wh = net._weights(dev)
    H, W = scene.shape[:2]
    n, h = xy.shape[0], net.image_size // 16
    kp = torch.zeros((H, W), dtype=torch.float32, device=dev)
    road = torch.zeros((H, W), dtype=torch.float32, device=dev)
    emb = torch.empty((n, h, h, 256), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        ctx.check(getattr(ctx.lib, entry)(ctx.handle, wh, scene.data_ptr(), *dims, xy.data_ptr(), n, int(bs), kp.data_ptr(),
                                          road.data_ptr(), emb.data_ptr(), net._stream(dev)), entry)
    return kp, road, emb


def _abi_normalise(net, entry, kp_c, road_c, dims, xy):
    dev = kp_c.device
    ctx, _ = net._weights(dev)
    kp = torch.empty(kp_c.shape, dtype=torch.uint8, device=dev)
    road = torch.empty(kp_c.shape, dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        ctx.check(getattr(ctx.lib, entry)(ctx.handle, kp_c.data_ptr(), road_c.data_ptr(), *dims, xy.data_ptr(), xy.shape[0],
                                          net.image_size, kp.data_ptr(), road.data_ptr(), net._stream(dev)), entry)
    return kp, road


@pytest.mark.parametrize("H,W,per_edge,seed", SCENES)
def test_rect_equals_square_path_bit_for_bit(pair, H, W, per_edge, seed):
    """The rectangle against the parent's square entry on the zero-padded max(H, W) square with the same tile origins: embeddings,
    both f32 canvases, both u8 masks bitwise; infer_one_img(rect) == the product's own stages on the square path's results."""
    from sam_road_amd import Config
    from sam_road_amd.graph_points import extract_graph_points
    from sam_road_amd.inferencer import edge_votes, infer_one_img, votes_to_edges
    _, net = pair
    img = rect_scene(H, W, seed)
    S, P, bs = max(H, W), CFG["PATCH_SIZE"], CFG["INFER_BATCH_SIZE"]
    padded = np.zeros((S, S, 3), np.uint8)
    padded[:H, :W] = img
    infos = rect_grid(H, W, CFG["SAMPLE_MARGIN"], P, per_edge)
    xy = _xy(infos)
    # the square side: the single-`int S` C entries
    kp_sq, road_sq, emb_sq = _abi_pass1(net, "srh_scene_pass1", torch.as_tensor(padded).cuda(), (S,), xy, bs)
    kpu_sq, roadu_sq = _abi_normalise(net, "srh_scene_normalise", kp_sq, road_sq, (S,), xy)
    # the rectangular side: the public Python surface
    kp_c, road_c, emb = net.scene_pass1(torch.as_tensor(img).cuda(), xy, bs)
    kpu, roadu = net.scene_normalise(kp_c, road_c, xy)
    assert kp_c.shape == road_c.shape == kpu.shape == roadu.shape == (H, W) and emb.shape == (len(infos), 256, P // 16, P // 16)
    _same_bits(emb, emb_sq.permute(0, 3, 1, 2))
    _same_bits(kp_c, kp_sq[:H, :W])
    _same_bits(road_c, road_sq[:H, :W])
    _same_bits(kpu, kpu_sq[:H, :W])
    _same_bits(roadu, roadu_sq[:H, :W])
    assert float(kp_sq[H:].abs().sum() + kp_sq[:, W:].abs().sum()) == 0.0          # no tile reached into the padding
    assert int(kpu.max()) > 0 and int(roadu.max()) > 0
    # whole pipeline: infer_one_img on the rectangle == the product's stages on the cropped square-path masks and embeddings
    kp_m = np.ascontiguousarray(kpu_sq[:H, :W].cpu().numpy())
    road_m = np.ascontiguousarray(roadu_sq[:H, :W].cpu().numpy())
    cfg = Config(dict(CFG, INFER_PATCHES_PER_EDGE=per_edge, **thresholds(kp_m, road_m)))
    pts = extract_graph_points(kp_m, road_m, cfg)
    assert pts.shape[0] > 20
    votes = edge_votes(net, emb_sq.permute(0, 3, 1, 2), pts, infos, 0, len(infos), cfg, torch.device("cuda"))
    want_edges = votes_to_edges(*votes, pts.shape[0], cfg.TOPO_THRESHOLD)
    nodes, edges, kp_o, road_o = infer_one_img(net, img, cfg)
    assert want_edges.shape[0] > 20
    for got, want in ((nodes, pts[:, ::-1]), (edges, want_edges), (kp_o, kp_m), (road_o, road_m)):
        got, want = np.asarray(got), np.asarray(want)
        assert got.dtype == want.dtype
        np.testing.assert_array_equal(got, want)
    # (row, col): rows below H, columns below W — a swapped axis shows when H != W
    assert nodes[:, 0].max() < H and nodes[:, 1].max() < W
    assert nodes[:, 1].max() >= H if W > H else nodes[:, 0].max() >= W


@pytest.mark.parametrize("H,W,per_edge,seed", SCENES)
def test_rect_scene_parity_with_oracle(pair, H, W, per_edge, seed):
    """Pass-1 u8 masks against the oracle's fuse_masks with the bounds of test_scene_pass1_masks; pass 2 on identical points with
    the bounds of test_infer_one_img_end_to_end.  The three conditions on the scene (points, voted edges, share of edges the "firm"
    filter leaves out) are asserted on the oracle's numbers."""
    from sam_road_amd import Config
    from sam_road_amd.inferencer import infer_one_img
    oracle, net = pair
    img = rect_scene(H, W, seed)
    m = CFG["SAMPLE_MARGIN"]
    ref = oracle_scene(oracle, img, per_edge)
    assert ref[2].shape == ref[3].shape == (H, W)
    cfg = dict(CFG, INFER_PATCHES_PER_EDGE=per_edge, **thresholds(ref[2], ref[3]))
    got = infer_one_img(net, img, Config(cfg))
    check_scene_parity(f"rect_{H}x{W}", got, ref, cfg, oracle)
    for mask in got[2:]:
        # the margin no tile covers is 0 on all four sides
        assert (mask[:m] == 0).all() and (mask[-m:] == 0).all() and (mask[:, :m] == 0).all() and (mask[:, -m:] == 0).all()
        assert (mask[m:-m, m:-m] > 0).any()


def test_square_stays_square(pair):
    """H = W = 448 through srh_scene_pass1_hw / srh_scene_normalise_hw and through the single-S entries: bitwise equal canvases,
    embeddings and masks; INFER_PATCHES_PER_EDGE = 4 and = [4, 4] give identical tuples."""
    from sam_road_amd import Config
    from sam_road_amd.inferencer import infer_one_img
    _, net = pair
    S, bs = 448, CFG["INFER_BATCH_SIZE"]
    img = synth_scene(S, seed=5)
    infos = oscene.get_patch_info_one_img(0, S, CFG["SAMPLE_MARGIN"], CFG["PATCH_SIZE"], 4)
    assert infos == rect_grid(S, S, CFG["SAMPLE_MARGIN"], CFG["PATCH_SIZE"], 4)
    xy, scene = _xy(infos), torch.as_tensor(img).cuda()
    a = _abi_pass1(net, "srh_scene_pass1", scene, (S,), xy, bs)
    b = _abi_pass1(net, "srh_scene_pass1_hw", scene, (S, S), xy, bs)
    for x, y in zip(a, b):
        _same_bits(x, y)
    na = _abi_normalise(net, "srh_scene_normalise", a[0], a[1], (S,), xy)
    nb = _abi_normalise(net, "srh_scene_normalise_hw", a[0], a[1], (S, S), xy)
    for x, y in zip(na, nb):
        _same_bits(x, y)
    assert int(na[0].max()) > 0 and int(na[1].max()) > 0
    kp0 = na[0].cpu().numpy()
    road0 = na[1].cpu().numpy()
    thr = thresholds(kp0, road0)
    one = infer_one_img(net, img, Config(dict(CFG, INFER_PATCHES_PER_EDGE=4, **thr)))
    two = infer_one_img(net, img, Config(dict(CFG, INFER_PATCHES_PER_EDGE=[4, 4], **thr)))
    assert one[0].shape[0] > 20 and one[1].shape[0] > 20
    for x, y in zip(one, two):
        assert np.asarray(x).dtype == np.asarray(y).dtype
        np.testing.assert_array_equal(np.asarray(x), np.asarray(y))
    np.testing.assert_array_equal(one[2], kp0)


def test_abi_rejects_bad_scene_sizes(pair):
    """Host-side validation of the _hw entries: an axis below PATCH_SIZE and more than 2^31 - 1 pixels are SRH_ERR_BAD_ARG before
    anything is launched (the pointers are small valid buffers that are never touched)."""
    from sam_road_amd import _lib
    _, net = pair
    dev = torch.device("cuda")
    ctx, wh = net._weights(dev)
    buf = torch.zeros(1024, dtype=torch.float32, device=dev)
    xy = torch.zeros((1, 2), dtype=torch.int32, device=dev)
    p = buf.data_ptr()
    for H, W in ((255, 640), (640, 255), (46341, 46341), (0, 640)):
        rc = ctx.lib.srh_scene_pass1_hw(ctx.handle, wh, p, H, W, xy.data_ptr(), 1, 1, p, p, p, net._stream(dev))
        assert rc == -1, (H, W, rc)
    for H, W in ((46341, 46341), (0, 640), (640, -1)):
        rc = ctx.lib.srh_scene_normalise_hw(ctx.handle, p, p, H, W, xy.data_ptr(), 1, 256, p, p, net._stream(dev))
        assert rc == -1, (H, W, rc)
    with pytest.raises(_lib.SrhError):
        ctx.check(ctx.lib.srh_scene_pass1_hw(ctx.handle, wh, p, 255, 640, xy.data_ptr(), 1, 1, p, p, p, net._stream(dev)), "srh_scene_pass1_hw")
    with pytest.raises(ValueError):
        net.scene_pass1(torch.zeros((640, 200, 3), dtype=torch.uint8, device=dev), xy, 1)


def test_infer_imgs_pipeline_rect_scenes_equal_serial(pair):
    """The software-pipelined loop over scenes of different SHAPES — among them a 640 x 384 scene right after a 384 x 640 one: the
    same byte count in the reused page-locked staging buffers, a different pitch — equals infer_one_img scene by scene, array for
    array, on two consecutive runs."""
    from sam_road_amd import Config
    from sam_road_amd.inferencer import infer_imgs, infer_one_img
    _, net = pair
    shapes = [(384, 640), (640, 384), (448, 448), (640, 384), (401, 523)]
    imgs = [rect_scene(h, w, 50 + i) for i, (h, w) in enumerate(shapes)]
    assert [im.shape[:2] for im in imgs] == shapes and imgs[0].nbytes == imgs[1].nbytes
    _, _, kp0, road0 = infer_one_img(net, imgs[0], Config(dict(CFG)))
    cfg = Config(dict(CFG, **thresholds(kp0, road0)))      # 4 tiles per axis for every shape
    want = [infer_one_img(net, im, cfg) for im in imgs]
    print("points / edges per scene:", [(w[0].shape[0], w[1].shape[0]) for w in want])
    assert min(w[0].shape[0] for w in want) > 20 and min(w[1].shape[0] for w in want) > 20
    assert [w[2].shape for w in want] == shapes and [w[3].shape for w in want] == shapes
    for _ in range(2):
        got = list(infer_imgs(net, iter(imgs), cfg))
        assert len(got) == len(want)
        for w, g in zip(want, got):
            for a, b in zip(w, g):
                assert np.asarray(a).dtype == np.asarray(b).dtype
                np.testing.assert_array_equal(np.asarray(a), np.asarray(b))
