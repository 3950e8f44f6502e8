"""MASK_CLEAN (small mask components dropped on the device) on the HIP path.  Run on an MI355X: pytest -m gpu.

The reference has no such step, so the behaviour is pinned by the rule and by COMPOSITION: the kernels must equal mask_clean_ref byte for
byte on every shape and pattern at which the union-find can go wrong, and a run with the key must equal, bit for bit, the existing
pipeline with its two masks replaced by mask_clean_ref of them before the point extraction (tests/mask_clean_kit.py)."""
import warnings

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import mask_clean_kit as kit
from scene_kit import CFG, SCENES, pair, rect_scene, thresholds  # noqa: F401
from scene_kit import net_for as _net_for
from scene_kit import same_bits as _same

from sam_road_amd.mask_clean import MaskCleanPlan, MaskRule, level_above, mask_clean_ref, mask_clean_stats, mask_clean_table

P = CFG["PATCH_SIZE"]
# A segment is 64 columns of a row and a workgroup four consecutive segments of the image (kit.SEGMENT, kit.WORKGROUP).  257 x 300: five
# segments per row, the last 44 wide, so every row crosses four segment borders, a workgroup border falls at another column in every row
# (segment 4 j of the image) and runs over from one row to the next; 3 x 6000: 94 segments per row, 71 workgroups; 64 x 1 and 1 x 1:
# one-pixel segments; 1 x 64: exactly one full segment; 37 x 53: one partial segment per row.
SHAPES = [(1, 1), (1, 64), (64, 1), (37, 53), (257, 300), (3, 6000)]
RANDOM = ("r30", "r41", "r50", "r60")                    # both percolation thresholds lie inside: 0.407 (8-connectivity) and 0.593 (4)


def _clean(net, m, rule, conn):
    t = torch.from_numpy(m).cuda()
    out = net.mask_clean(t.view(-1), mask_clean_table([(0, m.shape[0], m.shape[1], rule)]), connectivity=conn)
    assert out.data_ptr() == t.data_ptr()                 # in place
    return t.cpu().numpy()


def _dropped_kept(m, rule, conn):
    areas, peaks = mask_clean_stats(m, rule.t_on, conn)
    keep = (areas >= rule.min_area) & (peaks >= rule.t_peak)
    return int((~keep).sum()), int(keep.sum())


# ---- 1. the kernels against the rule ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("conn", [8, 4])
def test_every_shape_and_pattern_equals_the_reference(conn):
    net = _net_for(P)
    cases = [(kind, H, W) for H, W in SHAPES for kind in kit.PATTERNS] + [("spiral", 63, 63), ("comb", 63, 63), ("u", 130, 257)]
    for k, (kind, H, W) in enumerate(cases):
        m = kit.levels(kit.pattern(kind, H, W, k), 128, k)
        for rule in (MaskRule(128, 5, 0), MaskRule(128, 5, 230), MaskRule(128, 1, 200)):
            want = mask_clean_ref(m, *rule, conn)
            if kind in RANDOM and (H, W) == (257, 300) and rule == MaskRule(128, 5, 0):
                dropped, kept = _dropped_kept(m, rule, conn)
                print(f"{kind} {H}x{W} conn {conn}: the reference drops {dropped} components and keeps {kept}")
                assert dropped >= 1 and kept >= 1         # a kernel that drops nothing, or everything, cannot pass
            np.testing.assert_array_equal(_clean(net, m, rule, conn), want, err_msg=f"{kind} {H}x{W} conn {conn} {rule}")
    # the patterns are what their names say (on the reference): one component of H W pixels; one under 8 and singletons under 4; one chain
    assert mask_clean_stats(kit.levels(kit.pattern("all", 257, 300), 128), 128, conn)[0].tolist() == [257 * 300]
    checker = mask_clean_stats(kit.levels(kit.pattern("checker", 257, 300), 128), 128, conn)[0]
    assert checker.tolist() == [257 * 300 // 2] if conn == 8 else (checker == 1).all()
    assert mask_clean_stats(kit.levels(kit.pattern("spiral", 63, 63), 128), 128, conn)[0].tolist() == [2047]
    assert mask_clean_stats(kit.levels(kit.pattern("u", 130, 257), 128), 128, conn)[0].tolist() == [2 * 130 + 257 - 2]


def test_thresholds_at_their_ends_and_an_all_zero_mask():
    net = _net_for(P)
    m = kit.levels(kit.pattern("r41", 37, 53, 3), 100, 3)
    for rule in (MaskRule(256, 1000, 256), MaskRule(0, 37 * 53, 0), MaskRule(0, 37 * 53 + 1, 0), MaskRule(1, 1, 256), MaskRule(100, 1, 0),
                 MaskRule(100, 2 ** 40, 0), MaskRule(255, 1, 255)):
        np.testing.assert_array_equal(_clean(net, m, rule, 8), mask_clean_ref(m, *rule, 8), err_msg=str(rule))
    zero = np.zeros((257, 300), np.uint8)
    assert not _clean(net, zero, MaskRule(128, 5, 200), 4).any()


def test_two_large_masks_in_one_call():
    """The scale of a scene: two 1024 x 2048 masks in one call, 65 536 segments over every compute unit, blobs of a coarse random field
    with speckle around them, so that components of hundreds of pixels carry one- and two-pixel appendices across segment borders.  At
    this scale a lost link of the union-find showed that no small shape reached."""
    net = _net_for(P)
    rng = np.random.default_rng(21)
    H, W = 1024, 2048
    masks = []
    for _ in range(2):
        blobs = np.kron(rng.random((H // 8, W // 8)) < 0.12, np.ones((8, 8), bool))
        masks.append(kit.levels(blobs | (rng.random((H, W)) < 0.03), 93, len(masks)))
    plan = MaskCleanPlan(MaskRule(93, 20, 128), MaskRule(93, 200, 154), 8)
    for rep in range(3):
        a, b = net.mask_clean_pair(*torch.from_numpy(np.stack(masks)).cuda(), plan)
        for got, m, rule in ((a, masks[0], plan.keypoint), (b, masks[1], plan.road)):
            if rep == 0:
                dropped, kept = _dropped_kept(m, rule, 8)
                assert dropped > 1000 and kept > 100, (dropped, kept)
            np.testing.assert_array_equal(got.cpu().numpy(), mask_clean_ref(m, *rule, 8))


def test_ragged_call_nothing_connects_across_blocks():
    """Four images of different sizes and parameters in one buffer, with a gap between two of them and the table not in buffer order;
    every block begins and ends with a row of foreground, so a filter that ignored the blocks' borders would join them."""
    net = _net_for(P)
    rng = np.random.default_rng(5)
    dims = [(5, 70), (9, 64), (1, 130), (66, 3)]
    rules = [MaskRule(100 + 20 * k, 2 + 40 * k, 0 if k == 2 else 180) for k in range(4)]
    offs, off = [], 3
    for k, (H, W) in enumerate(dims):
        offs.append(off)
        off += H * W + (7 if k == 1 else 0)
    flat = rng.integers(0, 256, size=off + 5, dtype=np.uint8)
    for (H, W), o, r in zip(dims, offs, rules):
        flat[o:o + W] = flat[o + (H - 1) * W:o + H * W] = r.t_on + 3
    for order in ((0, 1, 2, 3), (2, 0, 3, 1)):
        for conn in (8, 4):
            want = flat.copy()
            for k in order:
                (H, W), o = dims[k], offs[k]
                want[o:o + H * W] = mask_clean_ref(flat[o:o + H * W].reshape(H, W), *rules[k], conn).reshape(-1)
            table = mask_clean_table([(offs[k], *dims[k], rules[k]) for k in order])
            buf = torch.from_numpy(flat).cuda()
            net.mask_clean(buf, table, table_dev=torch.from_numpy(table).cuda(), connectivity=conn)
            np.testing.assert_array_equal(buf.cpu().numpy(), want)                   # the gap and the bytes around the blocks included
            assert (want != flat).any()
    # the pair convenience: two separate masks, and two rows of one tensor
    kp, road = (kit.levels(kit.pattern(kind, 37, 53, 9), 128, 9) for kind in ("r41", "r50"))
    plan = MaskCleanPlan(MaskRule(128, 4, 0), MaskRule(128, 1, 240), 8)
    for tensors in ((torch.from_numpy(kp).cuda(), torch.from_numpy(road).cuda()), tuple(torch.from_numpy(np.stack([kp, road])).cuda())):
        a, b = net.mask_clean_pair(*tensors, plan)
        np.testing.assert_array_equal(a.cpu().numpy(), mask_clean_ref(kp, *plan.keypoint, 8))
        np.testing.assert_array_equal(b.cpu().numpy(), mask_clean_ref(road, *plan.road, 8))


def test_entry_rejects_bad_arguments_and_leaves_the_buffer_alone():
    from sam_road_amd import _lib
    net = _net_for(P)
    dev = torch.device("cuda")
    ctx, _ = net._weights(dev)
    lib, s = ctx.lib, net._stream(dev)
    rule = MaskRule(100, 3, 0)
    good = mask_clean_table([(0, 4, 5, rule), (20, 3, 3, rule)])                    # 29 bytes, 29 workspace pixels
    src = np.random.default_rng(1).integers(0, 256, size=64, dtype=np.uint8)
    buf = torch.from_numpy(src).cuda()
    ws = torch.zeros((3, 64), dtype=torch.int32, device=dev)

    def call(table=good, b=buf.data_ptr(), nbytes=29, n=2, conn=8, parent=ws[0].data_ptr(), area=ws[1].data_ptr(), peak=ws[2].data_ptr(), px=29, tdev=True):
        t = torch.from_numpy(np.ascontiguousarray(table))
        td = t.cuda()
        return lib.srh_mask_clean(ctx.handle, b, nbytes, t.data_ptr(), td.data_ptr() if tdev else None, n, conn, parent, area, peak, px, s)

    def edit(i, j, v):
        t = good.copy()
        t[i, j] = v
        return t

    bad = (dict(b=None), dict(tdev=False), dict(parent=None), dict(area=None), dict(peak=None), dict(n=0), dict(n=-1), dict(conn=6), dict(conn=0),
           dict(nbytes=28), dict(px=28), dict(parent=ws[0].data_ptr() + 2), dict(table=edit(1, 0, 19)), dict(table=edit(1, 0, 21)),
           dict(table=edit(1, 0, -1)), dict(table=edit(0, 1, 0)), dict(table=edit(0, 2, 0)), dict(table=edit(0, 3, 257)), dict(table=edit(0, 3, -1)),
           dict(table=edit(0, 4, 0)), dict(table=edit(0, 5, 257)), dict(table=edit(1, 6, 19)), dict(table=edit(1, 7, 5)), dict(table=edit(0, 6, 1)))
    for kw in bad:
        assert call(**kw) == -1, kw
    huge = mask_clean_table([(0, 46341, 46341, rule)])                              # more than 2^31 - 1 pixels
    assert call(table=huge, n=1, nbytes=2 ** 40, px=2 ** 40) == -1
    two = mask_clean_table([(0, 40000, 40000, rule), (1600000000, 40000, 40000, rule)])      # each fits, their sum does not
    assert call(table=two, nbytes=2 ** 40, px=2 ** 40) == -1
    torch.cuda.synchronize()
    np.testing.assert_array_equal(buf.cpu().numpy(), src)                           # nothing was launched
    assert call() == 0
    with pytest.raises(_lib.SrhError, match="connectivity"):
        ctx.check(call(conn=6), "srh_mask_clean")
    for kw in (dict(buf=buf.view(8, 8)), dict(buf=buf.float()), dict(connectivity=6), dict(table=np.zeros((1, 7), np.int64)),
               dict(table=np.zeros((1, 8), np.int32))):
        kw = dict(dict(buf=buf, table=good, connectivity=8), **kw)
        with pytest.raises(ValueError):
            net.mask_clean(kw.pop("buf"), kw.pop("table"), **kw)
    torch.cuda.synchronize()


# ---- 2. end to end: a run with the key == the existing pipeline with its masks cleaned before the point extraction ------------------------------
H, W, PER_EDGE, SEED = SCENES["401x523"]
ECFG = dict(CFG, INFER_PATCHES_PER_EDGE=PER_EDGE)


def _median_key(kp, road, cfg, conn=8):
    """min_area the median component area and min_peak the level just below the median component peak, per mask; asserts on the
    reference that in each mask at least one component goes and at least one stays."""
    from sam_road_amd import Config
    from sam_road_amd.inferencer import mask_clean_plan
    key = {"connectivity": conn}
    for name, m, thr in (("keypoint", kp, cfg["ITSC_THRESHOLD"]), ("road", road, cfg["ROAD_THRESHOLD"])):
        areas, peaks = mask_clean_stats(m, level_above(thr), conn)
        key[name] = {"min_area": int(np.median(areas)), "min_peak": (int(np.median(peaks)) - 0.5) / 255.0}
    plan = mask_clean_plan(Config(dict(cfg, MASK_CLEAN=key)))
    for name, m, rule in (("keypoint", kp, plan.keypoint), ("road", road, plan.road)):
        dropped, kept = _dropped_kept(m, rule, conn)
        print(f"{name}: {rule}, the reference drops {dropped} components and keeps {kept}")
        assert dropped >= 1 and kept >= 1
    return key, plan


@pytest.fixture(scope="module")
def scene_run(pair):
    from sam_road_amd import Config
    from sam_road_amd.inferencer import infer_one_img
    _, net = pair
    img = rect_scene(H, W, SEED)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        plain = infer_one_img(net, img, Config(ECFG))
        cfg = ECFG
        few = min(mask_clean_stats(m, level_above(0.5))[0].size for m in plain[2:])
        if few < 4:                                       # the kit's thresholds leave too few components: its percentile thresholds
            cfg = dict(ECFG, **thresholds(plain[2], plain[3]))
            plain = infer_one_img(net, img, Config(cfg))
        key, plan = _median_key(plain[2], plain[3], cfg)
        want = kit.composed(plan, lambda: [infer_one_img(net, img, Config(cfg))])[0]
    return img, cfg, plain, key, plan, want


def test_infer_one_img_equals_the_composition(pair, scene_run):
    """The test that fails on code that ignores the key."""
    from sam_road_amd import Config
    from sam_road_amd.inferencer import infer_one_img
    _, net = pair
    img, cfg, plain, key, plan, want = scene_run
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        got = infer_one_img(net, img, Config(dict(cfg, MASK_CLEAN=key)))
    print("nodes", plain[0].shape[0], "->", got[0].shape[0], "edges", plain[1].shape[0], "->", got[1].shape[0])
    assert (want[2] != plain[2]).any() and (want[3] != plain[3]).any() and want[2].any() and want[3].any()
    for g, w in zip(got, want):
        _same(g, w)
    assert got[2].flags.c_contiguous and got[3].flags.c_contiguous and got[0].shape[0] < plain[0].shape[0]


def test_the_other_paths_equal_the_composition(pair, scene_run):
    from sam_road_amd import Config
    from sam_road_amd.inferencer import infer_imgs, infer_one_img
    from sam_road_amd.resample import resample_ref
    _, net = pair
    img, cfg, plain, key, plan, want = scene_run
    keyed = dict(cfg, MASK_CLEAN=key)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        # the pipelined loop
        other = rect_scene(384, 640, 41)
        want_other = kit.composed(plan, lambda: [infer_one_img(net, other, Config(cfg))])[0]
        res = list(infer_imgs(net, iter([img, other, img]), Config(keyed)))
        for got, w in zip(res, (want, want_other, want)):
            for g, x in zip(got, w):
                _same(g, x)
        # a group of three scenes of different sizes under SCENE_PAD: every scene filtered as if it ran alone
        shapes = [(288, 288), (300, 421), (401, 523)]
        imgs = [rect_scene(h, w, 50 + i) for i, (h, w) in enumerate(shapes)]
        gcfg = dict(cfg, INFER_PATCHES_PER_EDGE=2, SCENE_PAD=24)
        wants = kit.composed(plan, lambda: list(infer_imgs(net, iter(imgs), Config(gcfg), group=3)))
        res = list(infer_imgs(net, iter(imgs), Config(dict(gcfg, MASK_CLEAN=key)), group=3))
        changed = 0
        for got, w, hw in zip(res, wants, shapes):
            assert got[2].shape == hw
            for g, x in zip(got, w):
                _same(g, x)
        plain_group = list(infer_imgs(net, iter(imgs), Config(gcfg), group=3))
        changed = sum(int((w[3] != p[3]).any()) for w, p in zip(wants, plain_group))
        assert changed >= 2 and all(w[3].any() for w in wants)
        # SCENE_SCALE [1, 2]: the filter runs in the model frame; the caller's masks are resampled from the cleaned ones
        big = rect_scene(2 * H, 2 * W, SEED)
        scaled = dict(cfg, SCENE_SCALE=[1, 2])
        seen = []
        with kit.cleaned_before_extraction(plan, seen):
            nodes, edges, _, _ = infer_one_img(net, big, Config(scaled))
        assert len(seen) == 1 and seen[0][0].shape == (H, W)
        got = infer_one_img(net, big, Config(dict(scaled, MASK_CLEAN=key)))
        for g, x in zip(got, (nodes, edges) + tuple(resample_ref(m, 2, 1, out_shape=(2 * H, 2 * W)) for m in seen[0])):
            _same(g, x)
        model_plain = infer_one_img(net, big, Config(scaled))
        assert (got[3] != model_plain[3]).any() and got[3].any()


# ---- 3. the launch contract -----------------------------------------------------------------------------------------------------------------
ROWS = ("mask_clean_init", "mask_clean_merge", "mask_clean_flatten", "mask_clean_stats", "mask_clean_apply")


def _launches(ctx, fn):
    ctx.profile_read()
    ctx.profile_enable(True)
    try:
        out = fn()
        torch.cuda.synchronize()
        return out, {r["name"]: r["launches"] for r in ctx.profile_read() if r["launches"]}
    finally:
        ctx.profile_enable(False)


def test_launch_contract(pair, scene_run):
    """A fixed number of launches per call, whatever the masks hold: five, for an all-zero mask as for the random mask at 0.5, for a
    group of three as for one scene; without the key none, and every other row as without the key."""
    from sam_road_amd import Config, _lib
    from sam_road_amd.inferencer import infer_imgs, infer_one_img
    _, net = pair
    img, cfg, plain, key, plan, want = scene_run
    ctx = _lib.Context.get(torch.cuda.current_device())
    five = {name: 1 for name in ROWS}
    rule = MaskRule(128, 5, 200)
    for m in (np.zeros((257, 300), np.uint8), kit.levels(kit.pattern("r50", 257, 300, 1), 128, 1), kit.levels(kit.pattern("all", 257, 300), 128)):
        _, rows = _launches(ctx, lambda: _clean(net, m, rule, 8))
        assert rows == five, rows
    keyed = dict(cfg, MASK_CLEAN=key)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        _, base = _launches(ctx, lambda: infer_one_img(net, img, Config(cfg)))
        assert not any(name.startswith("mask_clean") for name in base)
        for idle in (None, {}, {"road": {"min_area": 1}}):
            res, rows = _launches(ctx, lambda: infer_one_img(net, img, Config(dict(cfg, MASK_CLEAN=idle))))
            assert rows == base
            for g, x in zip(res, plain):
                _same(g, x)
        _, rows = _launches(ctx, lambda: infer_one_img(net, img, Config(keyed)))
        assert rows == dict(base, **five), (rows, base)
        # a group of three: still five launches, and the group's own rows as without the key
        imgs = [rect_scene(h, w, 50 + i) for i, (h, w) in enumerate([(288, 288), (300, 421), (401, 523)])]
        gcfg = dict(cfg, INFER_PATCHES_PER_EDGE=2)
        _, gbase = _launches(ctx, lambda: list(infer_imgs(net, iter(imgs), Config(gcfg), group=3)))
        _, grows = _launches(ctx, lambda: list(infer_imgs(net, iter(imgs), Config(dict(gcfg, MASK_CLEAN=key)), group=3)))
        assert not any(name.startswith("mask_clean") for name in gbase) and grows == dict(gbase, **five), (grows, gbase)
        # three scenes one by one in the pipelined loop: five per scene
        _, rows = _launches(ctx, lambda: list(infer_imgs(net, iter([img] * 3), Config(keyed))))
        assert {name: rows[name] for name in ROWS} == {name: 3 for name in ROWS}
