"""CPU self-test of tests/scene_kit.py, on HOST_CFG's 128-px tiles and one 384 x 640 scene: the stand-in's feature gate, the oracle's
pass 1 without options against the composition written out here, and the parity check — it passes on the oracle against itself and
fails on a mask pixel three levels off, on a moved node and on a firm edge left out."""
import numpy as np
import pytest
import torch

import scene_kit as K
import tolerances
from oracle import scene as oscene
from oracle.samroad import AttrDict

H, W = 384, 640
CFG = dict(K.HOST_CFG, SAMPLE_MARGIN=0, INFER_PATCHES_PER_EDGE=[3, 5])           # 3 x 5 disjoint tiles


@pytest.fixture(scope="module")
def img():
    return K.rect_scene(H, W, 60)


def test_standin_without_features_has_no_feature_method_and_refuses_the_keywords(img):
    net = K.SceneStandIn(CFG)
    assert not any(hasattr(net, m) for m in ("scene_tile_valid", "scene_fill_invalid", "scene_pad"))
    full = K.SceneStandIn(CFG, K.SceneStandIn.FEATURES)
    assert all(hasattr(full, m) for m in ("scene_tile_valid", "scene_fill_invalid", "scene_pad"))
    scene, xy, canvas = torch.from_numpy(img), torch.tensor([[0, 0]], dtype=torch.int32), torch.zeros((H, W))
    for kw in (dict(window=torch.ones(128)), dict(tta=[0, 1])):
        with pytest.raises(TypeError):
            net.scene_pass1(scene, xy, 1, **kw)
    for kw in (dict(valid=torch.ones((H, W), dtype=torch.bool)), dict(window=torch.ones(128)), dict(tta=[0, 1])):
        with pytest.raises(TypeError):
            net.scene_normalise(canvas, canvas, xy, **kw)
    with pytest.raises(TypeError):                            # one feature on does not let another one's keyword through
        K.SceneStandIn(CFG, ("valid",)).scene_normalise(canvas, canvas, xy, window=torch.ones(128))
    assert net.calls == []                                    # refused before anything ran


def test_every_feature_on_and_every_option_off_is_the_featureless_standin(img):
    from sam_road_amd import Config
    from sam_road_amd.inferencer import infer_one_img
    plain = infer_one_img(K.SceneStandIn(CFG), img, Config(CFG), device="cpu")
    full = K.SceneStandIn(CFG, K.SceneStandIn.FEATURES)
    got = infer_one_img(full, img, Config(CFG), device="cpu")
    assert full.calls == [("pass1", 15), ("normalise", 15)]
    assert plain[0].shape[0] > 30 and plain[1].shape[0] > 100
    for a, b in zip(got, plain):
        K.same_bits(a, b)


@pytest.fixture(scope="module")
def oracle_run(img):
    """The oracle's pass 1, its points and its pass 2, at the percentile thresholds of the GPU tests (the greedy NMS stays at a second):
    (oracle, oracle_scene's result, cfg, the oracle's own (nodes, edges, kp, road), sums, counts)."""
    oracle, _ = K.build_oracle(CFG)
    ref = K.oracle_scene(oracle, img, CFG["INFER_PATCHES_PER_EDGE"], cfg=CFG)
    infos, feats, kp, road = ref
    cfg = dict(CFG, **K.thresholds(kp, road))
    pts = oscene.extract_graph_points(kp, road, AttrDict(cfg))
    edges, sums, cnts = oscene.infer_pass2(oracle, feats, pts, infos, AttrDict(cfg))
    return oracle, ref, cfg, (pts[:, ::-1], edges, kp, road), sums, cnts


def test_oracle_scene_without_options_is_the_fuse_masks_composition(img, oracle_run):
    oracle, (infos, feats, kp, road), _, _, _, _ = oracle_run
    want_infos = [(0, (x, y), (x + 128, y + 128)) for x in (0, 128, 256, 384, 512) for y in (0, 128, 256)]
    assert infos == want_infos
    scores, want_feats = [], []
    for i in range(0, 15, CFG["INFER_BATCH_SIZE"]):
        s, f = oracle.infer_masks_and_img_features(oscene.get_batch_img_patches(img, want_infos[i:i + CFG["INFER_BATCH_SIZE"]]))
        scores.append(s)
        want_feats.append(f)
    want_kp, want_road = oscene.fuse_masks((H, W), want_infos, scores)
    K.same_bits(kp, want_kp)
    K.same_bits(road, want_road)
    assert len(feats) == len(want_feats) == 5
    for a, b in zip(feats, want_feats):
        K.same_bits(a, b)


def test_parity_check_passes_on_the_oracle_against_itself(oracle_run, monkeypatch):
    recorded = {}                                             # the record of GPU measurements is not this test's to write
    monkeypatch.setattr(tolerances, "check", lambda name, value, bound, at_least=False: recorded.update({name: (float(value), at_least)}))
    oracle, ref, cfg, own, _, _ = oracle_run
    pts = K.check_scene_parity("kit_self", own, ref, cfg, oracle)
    np.testing.assert_array_equal(pts[:, ::-1], own[0])
    assert recorded == {"kit_self_kp_u8_within1": (1.0, True), "kit_self_kp_u8_max_diff": (0.0, False), "kit_self_road_u8_within1": (1.0, True),
                        "kit_self_road_u8_max_diff": (0.0, False), "kit_self_edge_symdiff": (0.0, False)}
    K.check_scene_parity(None, own, ref, cfg, oracle, valid=np.ones((H, W), bool), min_oracle_edges=100)


def _broken(case, own, sums, cnts):
    nodes, edges, kp, road = own
    if case == "mask pixel 3 levels up":
        kp = kp.copy()
        y, x = np.argwhere(kp < 250)[0]
        kp[y, x] += 3
    elif case == "one node moved":
        nodes = nodes.copy()
        nodes[0, 1] += 1
    elif case == "one firm edge removed":
        firm = [i for i, (a, b) in enumerate(edges.tolist()) if abs(sums[(a, b)] / cnts[(a, b)] - CFG["TOPO_THRESHOLD"]) > tolerances.TOPO_SCORE]
        edges = np.delete(edges, firm[0], axis=0)
    return nodes, edges, kp, road


@pytest.mark.parametrize("case", ["mask pixel 3 levels up", "one node moved", "one firm edge removed"])
def test_parity_check_fails_on(case, oracle_run):
    oracle, ref, cfg, own, sums, cnts = oracle_run
    broken = _broken(case, own, sums, cnts)
    assert sum(not np.array_equal(a, b) for a, b in zip(broken, own)) == 1
    with pytest.raises(AssertionError):
        K.check_scene_parity(None, broken, ref, cfg, oracle)
