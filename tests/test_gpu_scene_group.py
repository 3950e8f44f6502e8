"""SCENE_GROUP (the tiles of several small scenes batched into one pass 1) on the HIP path.  Run on an MI355X: pytest -m gpu.

The reference has no such step, so the behaviour is pinned by COMPOSITION of what is already pinned: the pack kernel must equal the stack
built with numpy.pad byte for byte, the crop kernel numpy slicing, and a grouped run must equal, bit for bit, the existing pipeline (today's
scene_pass1 / scene_tile_valid / scene_fill_invalid / scene_normalise) on that host-built stack, cut apart, with every graph built by hand
from the crops and that run's embeddings.  Against scene-by-scene runs the tile batches are composed differently (12 tiles in batches of
5 / 5 / 2 cross the scene borders), so there the masks agree within the kit's +-1-level bounds; the oracle parity uses the kit's check."""
import ctypes
import warnings

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import tolerances
from scene_kit import CFG, FILL, check_scene_parity, make_mask, np_pad, oracle_scene, pair, rect_grid, rect_scene  # noqa: F401
from scene_kit import dev as _dev
from scene_kit import net_for as _net_for
from scene_kit import same_bits as _same
from scene_kit import shift_infos as _shift
from scene_kit import thresholds as _thresholds

MODES = ("reflect", "edge", "constant")
P, MARGIN, BS = CFG["PATCH_SIZE"], CFG["SAMPLE_MARGIN"], CFG["INFER_BATCH_SIZE"]
GCFG = dict(CFG, INFER_PATCHES_PER_EDGE=2)               # three scenes: 12 tiles, batches of 5 / 5 / 2 that cross the scene borders


# ---- 1. the kernels ------------------------------------------------------------------------------------------------------------------
# (H, W), (top, bottom, left, right): mixed pads, axes of length 1, the odd row pitch of the scene tests; gap columns beside all but the widest
KERNEL_SCENES = [((1, 1), (3, 4, 5, 2)), ((7, 5), (0, 0, 0, 0)), ((200, 300), (44, 44, 0, 7)), ((401, 523), (24, 24, 24, 24))]


def _tables(scenes, C):
    """(pack table for C bytes per pixel, crop table, Ha, Wa) of [(shape, pads)], restated from DESIGN.md §6h."""
    rows, row0, px = [], 0, 0
    for (H, W), (top, bottom, left, right) in scenes:
        rows.append([px, H, W, top, left, H + top + bottom, W + left + right, row0])
        row0 += H + top + bottom
        px += H * W
    crop = np.array(rows, dtype=np.int64)
    pack = crop.copy()
    pack[:, 0] *= C
    return pack, crop, row0, int(crop[:, 6].max())


def _np_stack(blocks, scenes, mode, fill, Ha, Wa):
    out = np.zeros((Ha, Wa) + blocks[0].shape[2:], dtype=blocks[0].dtype)
    row0 = 0
    for b, (_, pads) in zip(blocks, scenes):
        p = np_pad(b, pads, mode, fill)
        out[row0:row0 + p.shape[0], :p.shape[1]] = p
        row0 += p.shape[0]
    return out


def test_group_pack_equals_the_numpy_stack():
    net = _net_for(P)
    rng = np.random.default_rng(11)
    imgs = [rng.integers(0, 256, size=s + (3,), dtype=np.uint8) for s, _ in KERNEL_SCENES]
    masks = [rng.random(s) < 0.5 for s, _ in KERNEL_SCENES]
    for blocks, C in ((imgs, 3), ([m.astype(np.uint8) * 200 for m in masks], 1), (masks, 1)):
        pack, _, Ha, Wa = _tables(KERNEL_SCENES, C)
        flat = np.concatenate([b.reshape(-1) for b in blocks])
        for mode in MODES:
            fill = FILL if C == 3 else ((0, 0, 0) if blocks[0].dtype == bool else (FILL[0],) * 3)
            want = _np_stack(blocks, KERNEL_SCENES, mode, fill, Ha, Wa)
            t = torch.from_numpy(flat).cuda()
            out = net.scene_group_pack(t, torch.from_numpy(pack), C, Ha, Wa, mode, fill)
            assert out.dtype == t.dtype and tuple(out.shape) == want.shape
            np.testing.assert_array_equal(out.cpu().numpy(), want, err_msg=f"{mode} C {C} {flat.dtype}")
            np.testing.assert_array_equal(t.cpu().numpy(), flat)                 # the source is untouched
            # a source view at byte offsets 1 and 3 of a larger allocation, and the table already on the device
            for off in (1, 3):
                big = torch.full((flat.size + 16,), 0xA5, dtype=torch.uint8, device="cuda")
                v = big[off:off + flat.size]
                v.copy_(torch.from_numpy(flat.view(np.uint8)))
                out = net.scene_group_pack(v, torch.from_numpy(pack), C, Ha, Wa, mode, fill, table_dev=torch.from_numpy(pack).cuda())
                np.testing.assert_array_equal(out.cpu().numpy(), want.view(np.uint8))
    # guard bytes around dst stay untouched: the C entry writes Ha * Wa * 3 bytes at an odd address inside a larger buffer
    pack, _, Ha, Wa = _tables(KERNEL_SCENES, 3)
    flat = np.concatenate([b.reshape(-1) for b in imgs])
    ctx, _ = net._weights(torch.device("cuda"))
    n = Ha * Wa * 3
    for lead in (5, 16):
        big = torch.full((lead + n + 37,), 0xA5, dtype=torch.uint8, device="cuda")
        src, tab = torch.from_numpy(flat).cuda(), torch.from_numpy(pack)
        rc = ctx.lib.srh_scene_group_pack(ctx.handle, src.data_ptr(), src.numel(), tab.data_ptr(), tab.cuda().data_ptr(), len(KERNEL_SCENES), 3, Ha, Wa,
                                          0, None, big.data_ptr() + lead, net._stream(torch.device("cuda")))
        assert rc == 0
        got = big.cpu().numpy()
        assert (got[:lead] == 0xA5).all() and (got[lead + n:] == 0xA5).all()
        np.testing.assert_array_equal(got[lead:lead + n].reshape(Ha, Wa, 3), _np_stack(imgs, KERNEL_SCENES, "reflect", FILL, Ha, Wa))


def test_group_crop_equals_numpy_slicing():
    net = _net_for(P)
    rng = np.random.default_rng(12)
    _, crop, Ha, Wa = _tables(KERNEL_SCENES, 1)
    total = int((crop[:, 1] * crop[:, 2]).sum())
    for extra in (0, 3):                                                         # a stack wider than its widest scene as well
        kp, road = (rng.integers(0, 256, size=(Ha, Wa + extra), dtype=np.uint8) for _ in range(2))
        out = net.scene_group_crop(_dev(kp), _dev(road), torch.from_numpy(crop))
        assert out.dtype == torch.uint8 and tuple(out.shape) == (2, total)
        got = out.cpu().numpy()
        for off, H, W, top, left, _, _, row0 in crop.tolist():
            for j, m in enumerate((kp, road)):
                np.testing.assert_array_equal(got[j, off:off + H * W].reshape(H, W), m[row0 + top:row0 + top + H, left:left + W])


def test_group_entries_reject_bad_arguments():
    from sam_road_amd import _lib
    net = _net_for(P)
    dev = torch.device("cuda")
    ctx, _ = net._weights(dev)
    lib, s = ctx.lib, net._stream(dev)
    buf = torch.zeros(8192, dtype=torch.uint8, device=dev)
    p = buf.data_ptr()
    good = np.array([[0, 4, 5, 1, 2, 6, 8, 0], [60, 3, 3, 0, 0, 3, 3, 6]], dtype=np.int64)       # Ha 9, Wa 8, C 3: 87 source bytes
    rgb = (ctypes.c_int32 * 3)(1, 2, 3)

    def pack(table=good, src=p, src_bytes=87, n=2, C=3, Ha=9, Wa=8, mode=0, fill=rgb, dst=p + 4096, tdev=True):
        t = torch.from_numpy(np.ascontiguousarray(table))
        td = t.cuda()
        return lib.srh_scene_group_pack(ctx.handle, src, src_bytes, t.data_ptr(), td.data_ptr() if tdev else None, n, C, Ha, Wa, mode, fill, dst, s)

    def crop(table, out_bytes, Ha=9, Wa=8, n=2, kp=p, out=p + 4096, tdev=True):
        t = torch.from_numpy(np.ascontiguousarray(table))
        td = t.cuda()
        return lib.srh_scene_group_crop(ctx.handle, kp, p + 1024, Ha, Wa, t.data_ptr(), td.data_ptr() if tdev else None, n, out,
                                        None if out is None else out + 1024, out_bytes, s)

    def edit(i, j, v, base=good):
        t = base.copy()
        t[i, j] = v
        return t

    assert pack() == 0 and pack(fill=None) == 0
    for kw in (dict(src=None), dict(dst=None), dict(tdev=False), dict(n=0), dict(C=2), dict(C=4), dict(mode=3), dict(mode=-1), dict(mode=2, fill=None),
               dict(fill=(ctypes.c_int32 * 3)(256, 0, 0)), dict(src_bytes=86), dict(Ha=10), dict(Ha=8), dict(Wa=7), dict(Ha=0), dict(n=1),
               dict(table=edit(0, 1, 0)), dict(table=edit(0, 3, -1)), dict(table=edit(0, 4, -1)), dict(table=edit(0, 5, 4)), dict(table=edit(0, 6, 6)),
               dict(table=edit(1, 7, 5)), dict(table=edit(1, 0, 61)), dict(table=edit(1, 0, -1)), dict(table=edit(1, 5, 4))):
        assert pack(**kw) == -1, kw
    assert pack(table=edit(1, 0, 0)) == 0                                        # source blocks may repeat
    cgood = good.copy()
    cgood[1, 0] = 20                                                             # the crop's blocks tile its outputs: 4 * 5, then 3 * 3
    assert crop(cgood, 29) == 0
    for kw in (dict(kp=None), dict(out=None), dict(tdev=False), dict(n=0), dict(out_bytes=28), dict(out_bytes=30), dict(Ha=10), dict(Wa=7),
               dict(table=edit(1, 0, 19, cgood)), dict(table=edit(0, 0, 1, cgood)), dict(table=edit(0, 5, 5, cgood)), dict(table=edit(1, 2, 0, cgood))):
        kw = dict(dict(table=cgood, out_bytes=29), **kw)
        assert crop(**kw) == -1, kw
    # a stack past 2^31 - 1 pixels
    huge = np.array([[0, 1, 1, 0, 0, 46341, 46341, 0]], dtype=np.int64)
    assert pack(table=huge, n=1, Ha=46341, Wa=46341, src_bytes=3) == -1 and crop(huge, 1, Ha=46341, Wa=46341, n=1) == -1
    with pytest.raises(_lib.SrhError):
        ctx.check(pack(C=2), "srh_scene_group_pack")
    for bad in (dict(table=torch.zeros((2, 7), dtype=torch.int64)), dict(table=torch.zeros((2, 8), dtype=torch.int32)), dict(C=2), dict(mode="wrap"),
                dict(ragged=torch.zeros((8, 8), dtype=torch.uint8, device=dev)), dict(ragged=torch.zeros(87, dtype=torch.float32, device=dev))):
        kw = dict(dict(ragged=buf[:87], table=torch.from_numpy(good), C=3, Ha=9, Wa=8, mode="reflect"), **bad)
        with pytest.raises(ValueError):
            net.scene_group_pack(kw.pop("ragged"), kw.pop("table"), **kw)
    with pytest.raises(ValueError):
        net.scene_group_crop(buf[:72].view(9, 8), buf[:72].view(8, 9), torch.from_numpy(cgood))
    torch.cuda.synchronize()


# ---- 2. a grouped run == the existing pipeline on the host-built stack, cut apart --------------------------------------------------------
def _host_stack(imgs, valids, cfg):
    """(stack u8, mask stack bool or None, [(row0, pads, virtual size)], union tile list as infos on the stack, first tile per scene) from
    numpy.pad and the restated tile rule."""
    from sam_road_amd import Config
    from sam_road_amd.inferencer import scene_pad_plan
    plans = [scene_pad_plan(im.shape, Config(cfg)) for im in imgs]
    pads = [tuple(p[:4]) if p is not None else (0, 0, 0, 0) for p in plans]
    mode = plans[0][4] if plans[0] is not None else "reflect"
    padded = [np_pad(im, p, mode) for im, p in zip(imgs, pads)]
    Ha, Wa = sum(p.shape[0] for p in padded), max(p.shape[1] for p in padded)
    stack = np.zeros((Ha, Wa, 3), np.uint8)
    mask = np.zeros((Ha, Wa), bool) if any(v is not None for v in valids) else None
    geo, infos, first, row0 = [], [], [0], 0
    for im, v, p, pd in zip(imgs, valids, padded, pads):
        Hv, Wv = p.shape[:2]
        stack[row0:row0 + Hv, :Wv] = p
        if mask is not None:
            mask[row0:row0 + Hv, :Wv] = True if v is None else np_pad(v, pd, mode, (0, 0, 0))
        infos += [(0, (x0, y0 + row0), (x1, y1 + row0)) for _, (x0, y0), (x1, y1) in rect_grid(Hv, Wv, MARGIN, P, cfg["INFER_PATCHES_PER_EDGE"])]
        first.append(len(infos))
        geo.append((row0, pd, (Hv, Wv)))
        row0 += Hv
    return stack, mask, geo, infos, first


def _existing_pipeline(net, stack, mask, infos, cfg):
    """Today's entries on the stack, by hand: [count, select, fill,] pass 1 [window, TTA], normalise [valid, window].  Returns (kp u8,
    road u8, embeddings, kept indices)."""
    from sam_road_amd import Config
    from sam_road_amd.inferencer import fuse_window, select_tiles, tta_plan
    window, codes = fuse_window(Config(cfg)), tta_plan(Config(cfg))[1]
    xy = torch.tensor([[t[1][0], t[1][1]] for t in infos], dtype=torch.int32).cuda()
    scene, kept = _dev(stack), np.arange(len(infos))
    norm_kw = {} if window is None else dict(window=_dev(window))
    pass1_kw = dict(norm_kw, **({} if len(codes) == 1 else dict(tta=list(codes))))
    if mask is not None:
        valid_d = _dev(mask.view(np.uint8))
        kept = select_tiles(net.scene_tile_valid(valid_d, xy).cpu().numpy(), P, 0.0)
        xy = xy[torch.from_numpy(kept).cuda()].contiguous()
        scene = net.scene_fill_invalid(scene, valid_d, FILL)
        norm_kw = dict(valid=valid_d, **norm_kw)
    kp_c, road_c, emb = net.scene_pass1(scene, xy, BS, **pass1_kw)
    kp, road = net.scene_normalise(kp_c, road_c, xy.repeat(len(codes), 1) if len(codes) > 1 else xy, **norm_kw)
    return kp.cpu().numpy(), road.cpu().numpy(), emb, kept


def _check_group_against_stack(net, imgs, valids, cfg, least=20):
    from sam_road_amd import Config
    from sam_road_amd.graph_points import extract_graph_points
    from sam_road_amd.inferencer import _BlockingIO, _SceneSetup, _pass1_front, _plan_group_scene, edge_votes, infer_imgs, votes_to_edges
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        stack, mask, geo, infos, first = _host_stack(imgs, valids, cfg)
        kp_s, road_s, emb_s, kept = _existing_pipeline(net, stack, mask, infos, cfg)
        crops = [tuple(np.ascontiguousarray(m[r0 + pd[0]:r0 + pd[0] + im.shape[0], pd[2]:pd[2] + im.shape[1]]) for m in (kp_s, road_s))
                 for im, (r0, pd, _) in zip(imgs, geo)]
        big = max(range(len(imgs)), key=lambda k: imgs[k].size)
        cfg = dict(cfg, **_thresholds(*crops[big]))
        # the front end alone: the embeddings are the slices, the masks are the crops
        ctx = _SceneSetup(net, Config(cfg), None, sharded=False)
        group = [_plan_group_scene(im, v, Config(cfg)) for im, v in zip(imgs, valids)]
        job = _pass1_front(ctx, _BlockingIO(ctx.device), None, None, group)
        _same(job.emb, emb_s)
        both, cut = job.kp_u8.cpu().numpy(), np.searchsorted(kept, first)
        for k, (c, im) in enumerate(zip(job.group, imgs)):
            n = im.shape[0] * im.shape[1]
            assert (c.lo, c.hi, c.mask_off) == (cut[k], cut[k + 1], sum(i.shape[0] * i.shape[1] for i in imgs[:k]))
            _same(both[0, c.mask_off:c.mask_off + n].reshape(im.shape[:2]), crops[k][0])
            _same(both[1, c.mask_off:c.mask_off + n].reshape(im.shape[:2]), crops[k][1])
        # the loop: every graph from the crops, that run's embeddings and the scene's own tiles in its own real frame
        got = list(infer_imgs(net, iter(imgs), Config(cfg), group=len(imgs), valids=iter(valids)))
        assert len(got) == len(imgs)
        for k, ((nodes, edges, kp, road), im) in enumerate(zip(got, imgs)):
            r0, pd, _ = geo[k]
            _same(kp, crops[k][0])
            _same(road, crops[k][1])
            if valids[k] is not None:
                assert not kp[~valids[k]].any() and not road[~valids[k]].any() and road[valids[k]].any()
            pts = extract_graph_points(*crops[k], Config(cfg))
            _same(nodes, pts[:, ::-1])
            mine = kept[cut[k]:cut[k + 1]]
            own = _shift([(0, (x0, y0 - r0), (x1, y1 - r0)) for _, (x0, y0), (x1, y1) in (infos[i] for i in mine)], pd)
            votes = edge_votes(net, emb_s[cut[k]:cut[k + 1]], pts, own, 0, len(own), Config(cfg), torch.device("cuda"))
            _same(edges, votes_to_edges(*votes, pts.shape[0], cfg["TOPO_THRESHOLD"]))
            print(f"scene {k} {im.shape[:2]} pads {pd}: {len(mine)} tiles, {pts.shape[0]} points, {edges.shape[0]} edges")
            assert nodes.shape[0] == 0 or (nodes[:, 0].max() < im.shape[0] and nodes[:, 1].max() < im.shape[1] and nodes.min() >= 0)
        assert got[big][0].shape[0] > least and got[big][1].shape[0] > least
    return got, cfg, (emb_s, kept, first, crops, infos, geo)


SHAPES3 = [(288, 288), (300, 421), (401, 523)]


@pytest.fixture(scope="module")
def plain_group(pair):
    _, net = pair
    imgs = [rect_scene(h, w, 50 + i) for i, (h, w) in enumerate(SHAPES3)]
    return (imgs,) + _check_group_against_stack(net, imgs, [None] * 3, GCFG)


def test_group_equals_the_existing_pipeline_on_the_stack(plain_group):
    imgs, got, _, (emb, kept, first, _, infos, _) = plain_group
    assert len(infos) == 12 and list(first) == [0, 4, 8, 12] and len(kept) == 12 and emb.shape[0] == 12      # batches 5 / 5 / 2
    assert [g[2].shape for g in got] == SHAPES3


def test_group_with_mask_window_and_tta(pair):
    _, net = pair
    imgs = [rect_scene(h, w, 50 + i) for i, (h, w) in enumerate(SHAPES3)]
    valids = [None, make_mask("band", *SHAPES3[1]), None]
    _check_group_against_stack(net, imgs, valids, dict(GCFG, FUSE_WINDOW="hann", TTA=["id", "rot90"]))


def test_group_with_scene_pad_and_a_scene_smaller_than_a_tile(pair):
    _, net = pair
    shapes = SHAPES3 + [(200, 300)]
    imgs = [rect_scene(h, w, 50 + i) for i, (h, w) in enumerate(shapes)]
    got, _, (_, _, first, _, _, geo) = _check_group_against_stack(net, imgs, [None] * 4, dict(GCFG, SCENE_PAD=24))
    assert [g[1] for g in geo] == [(24, 24, 24, 24)] * 3 + [(44, 44, 24, 24)] and geo[3][2] == (288, 348) and list(first) == [0, 4, 8, 12, 16]
    assert got[3][2].shape == (200, 300) and got[3][3].any()


def _pass2_children(plain_group):
    """The stack's job and one child per scene with its points and flat queries, from the crops of the plain group."""
    from sam_road_amd import Config
    from sam_road_amd.graph_points import extract_graph_points
    from sam_road_amd.inferencer import _SceneJob, build_all_patch_queries
    _, _, cfg, (emb, kept, first, crops, infos, geo) = plain_group
    cfg_o = Config(cfg)
    kids = []
    for k, (kp, road) in enumerate(crops):
        r0, pd, _ = geo[k]
        own = _shift([(0, (x0, y0 - r0), (x1, y1 - r0)) for _, (x0, y0), (x1, y1) in infos[first[k]:first[k + 1]]], pd)
        c = _SceneJob(kp.shape, own, None, pd, lo=first[k], hi=first[k + 1])
        c.graph_points = extract_graph_points(kp, road, cfg_o)
        c.fq = build_all_patch_queries(c.graph_points, own, 0, len(own), cfg_o, flat=True)
        assert c.fq is not None and c.fq.offsets[-1] > 0
        kids.append(c)
    return _SceneJob((0, 0), [], None, emb=emb), kids


def test_one_pass2_launch_sequence_equals_per_scene_launches(pair, plain_group):
    """The rows of TopoNet are independent: the scores of the group's ONE ragged launch sequence, read per scene, are those of a launch
    sequence per scene on the same embeddings, bit for bit."""
    from sam_road_amd.inferencer import _BlockingIO, _concat_queries, _queue_pass2
    _, net = pair
    job, kids = _pass2_children(plain_group)
    device, K = torch.device("cuda"), CFG["MAX_NEIGHBOR_QUERIES"]
    fq = _concat_queries(job, kids)
    plan, scores = _queue_pass2(net, job.emb, fq, BS, K, True, _BlockingIO(device))
    assert plan == "ragged" and len(scores) == 1 and scores[0].shape[0] == fq.offsets[-1]
    rows = 0
    for c in kids:
        plan_c, sc = _queue_pass2(net, job.emb[c.lo:c.hi], c.fq, BS, K, True, _BlockingIO(device))
        R = int(c.fq.offsets[-1])
        assert plan_c == "ragged" and sc[0].shape[0] == R and c.row0 == rows
        _same(scores[0][c.row0:c.row0 + R], sc[0])
        rows += R
    assert rows == scores[0].shape[0] > 100


# ---- 3. grouped against scene by scene ---------------------------------------------------------------------------------------------------
def test_grouped_masks_within_one_level_of_per_scene_runs(pair, plain_group):
    """Other batch compositions select other GEMM kernels (tests/tolerances.py: BATCH_INDEP_SCORE), so the masks agree within the kit's
    bounds — one level on U8_WITHIN1 of the pixels, two anywhere — and not bit for bit."""
    from sam_road_amd import Config
    from sam_road_amd.inferencer import infer_one_img
    _, net = pair
    imgs, got, cfg, _ = plain_group
    for k, (im, g) in enumerate(zip(imgs, got)):
        alone = infer_one_img(net, im, Config(cfg))
        for name, a, b in (("kp", g[2], alone[2]), ("road", g[3], alone[3])):
            d = np.abs(a.astype(int) - b.astype(int))
            print(f"[parity] group_vs_alone_{k}_{name}: max diff {d.max()} levels, identical {(d == 0).mean():.6f}")
            tolerances.check(f"group_vs_alone_{k}_{name}_u8_within1", (d <= 1).mean(), tolerances.U8_WITHIN1, at_least=True)
            tolerances.check(f"group_vs_alone_{k}_{name}_u8_max_diff", d.max(), 3)                # integers: < 3 is <= 2 levels


# ---- 4. against the oracle ---------------------------------------------------------------------------------------------------------------
PARITY = [(401, 523, 43), (523, 701, 44)]                # (H, W, seed) of the kit's PARITY_SCENES
PARITY_PER_EDGE = [2, 3]                                 # 6 tiles each: 12 tiles in batches of 5 / 5 / 2


def test_group_parity_with_oracle(pair):
    from sam_road_amd import Config
    from sam_road_amd.inferencer import infer_imgs
    oracle, net = pair
    imgs = [rect_scene(h, w, s) for h, w, s in PARITY]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        refs = [oracle_scene(oracle, im, PARITY_PER_EDGE) for im in imgs]
        thr = _thresholds(np.concatenate([r[2].ravel() for r in refs]), np.concatenate([r[3].ravel() for r in refs]))
        cfg = dict(CFG, INFER_PATCHES_PER_EDGE=PARITY_PER_EDGE, **thr)
        got = list(infer_imgs(net, iter(imgs), Config(cfg), group=2))
    for (h, w, _), g, ref in zip(PARITY, got, refs):
        check_scene_parity(f"group2_{h}x{w}", g, ref, cfg, oracle)


# ---- 5. the launch contract ---------------------------------------------------------------------------------------------------------------
def _launches(ctx, fn):
    ctx.profile_read()
    ctx.profile_enable(True)
    try:
        out = fn()
        torch.cuda.synchronize()
        return out, {r["name"]: r["launches"] for r in ctx.profile_read() if r["launches"]}
    finally:
        ctx.profile_enable(False)


def test_launch_contract(pair, plain_group):
    from sam_road_amd import Config, _lib
    from sam_road_amd.inferencer import infer_imgs, infer_one_img
    _, net = pair
    imgs, got, cfg, _ = plain_group
    ctx = _lib.Context.get(torch.cuda.current_device())
    alone = [infer_one_img(net, im, Config(cfg)) for im in imgs]
    # key absent, None or 1: neither kernel, and the bytes of the loop as it was (infer_one_img's, scene by scene)
    for kw, c in ((dict(), cfg), (dict(group=1), cfg), (dict(), dict(cfg, SCENE_GROUP=1)), (dict(group=1), dict(cfg, SCENE_GROUP=3))):
        res, rows = _launches(ctx, lambda: list(infer_imgs(net, iter(imgs), Config(c), **kw)))
        assert "scene_group_pack" not in rows and "scene_group_crop" not in rows and "scene_pad" not in rows
        for a, b in zip(res, alone):
            for x, y in zip(a, b):
                _same(x, y)
    _, base = _launches(ctx, lambda: infer_one_img(net, imgs[0], Config(cfg)))
    # group = 3 over seven scenes: groups of 3, 3 and 1 — one pack and one crop per group, the group of one takes the old path
    seven = imgs + imgs + imgs[:1]
    res, rows = _launches(ctx, lambda: list(infer_imgs(net, iter(seven), Config(cfg), group=3)))
    assert rows["scene_group_pack"] == 2 and rows["scene_group_crop"] == 2
    assert set(rows) == set(base) | {"scene_group_pack", "scene_group_crop"}
    for a, b in zip(res, got + got + alone[:1]):
        for x, y in zip(a, b):
            _same(x, y)
    # with a mask in the group: a second pack, for the mask stack
    valids = [None, make_mask("band", *SHAPES3[1]), None]
    _, rows = _launches(ctx, lambda: list(infer_imgs(net, iter(imgs), Config(cfg), group=3, valids=iter(valids))))
    assert rows["scene_group_pack"] == 2 and rows["scene_group_crop"] == 1
    # the key in the config groups too
    _, rows = _launches(ctx, lambda: list(infer_imgs(net, iter(imgs), Config(dict(cfg, SCENE_GROUP=3)))))
    assert rows["scene_group_pack"] == 1 and rows["scene_group_crop"] == 1
