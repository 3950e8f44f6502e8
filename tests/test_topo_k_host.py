"""Host side of MAX_NEIGHBOR_QUERIES (K) != 16: pass-2 query building, packing and vote sums at other K, the tile-sharded merge at
K = 8, and the inferencer's up-front check of K (1..64, ABI 10).  CPU only."""
import numpy as np
import pytest

from sam_road_amd import Config
from sam_road_amd import inferencer as inf
from sam_road_amd.tiling import get_patch_info_one_img


def _points(seed, n=900, size=400):
    rng = np.random.default_rng(seed)
    pts = np.unique(rng.integers(0, size // 4, size=(n, 2)) * 4, axis=0).astype(np.int64)      # a 4-px lattice: many equidistant neighbours
    return pts


@pytest.mark.parametrize("K", [1, 4, 8, 24, 64])
def test_pass2_fill_vs_scipy_at_k(K):
    """srh_pass2_fill (the library's kNN(K+1) per tile) == scipy.spatial.KDTree.query(k=K+1, distance_upper_bound=R) per tile, on a
    lattice where the K-th and (K+1)-th neighbours are often equidistant."""
    pts = _points(K)
    cfg = Config(NEIGHBOR_RADIUS=48, MAX_NEIGHBOR_QUERIES=K)
    infos = get_patch_info_one_img(0, 400, 0, 160, 4)
    fq = inf.build_all_patch_queries(pts, infos, 0, len(infos), cfg, flat=True)
    assert fq is not None and fq.knn.shape[1] == K
    rows = n_tied = 0
    for t, (_, (x0, y0), (x1, y1)) in enumerate(infos):
        ids, local, pairs, valid = fq.tile(t)
        ids_r, local_r, pairs_r, valid_r = inf.build_patch_queries(pts, x0, y0, x1, y1, cfg)
        np.testing.assert_array_equal(ids, ids_r)
        np.testing.assert_array_equal(local, local_r)
        np.testing.assert_array_equal(valid, valid_r)
        np.testing.assert_array_equal(pairs[..., 0], pairs_r[..., 0])
        # rows with a tie at the cut-off (K-th and (K+1)-th equidistant) follow scipy's kd-tree element for element; elsewhere the
        # same neighbours, ordered by (distance, index) inside a group of equidistant ones where scipy's order is heap-internal
        a = int(fq.offsets[t])
        tied = fq.tied[a:a + len(ids)].astype(bool)
        np.testing.assert_array_equal(pairs[tied], pairs_r[tied])
        np.testing.assert_array_equal(np.sort(pairs[..., 1], -1), np.sort(pairs_r[..., 1], -1))
        rows += len(ids)
        n_tied += int(tied.sum())
    assert rows > 200 and (n_tied > 0 or K in (1, 64))         # K = 64: hardly a row has 65 neighbours within the radius


@pytest.mark.parametrize("K", [3, 8, 24])
def test_pack_ragged_and_vote_sums_at_k(K):
    """srh_pass2_pack_ragged rows == the per-tile queries concatenated; srh_pass2_vote_sums == the numpy restatement of
    inferencer.py:179-228 (votes of every valid pair, in the reference's order) at K != 16."""
    pts = _points(30 + K)
    cfg = Config(NEIGHBOR_RADIUS=40, MAX_NEIGHBOR_QUERIES=K)
    infos = get_patch_info_one_img(0, 400, 0, 128, 4)
    fq = inf.build_all_patch_queries(pts, infos, 0, len(infos), cfg, flat=True)
    R, p_h, t_h, q_h, v_h = inf._pack_pass2_ragged(fq, K)
    assert q_h.shape[1:] == (K, 2) and v_h.shape[1:] == (K,)
    for t in range(len(infos)):
        a, b = int(fq.offsets[t]), int(fq.offsets[t + 1])
        _, local, pairs, valid = fq.tile(t)
        np.testing.assert_array_equal(t_h[a:b], t)
        np.testing.assert_array_equal(p_h[a:b], local.astype(np.float32))
        np.testing.assert_array_equal(q_h[a:b], pairs + a)
        np.testing.assert_array_equal(v_h[a:b].astype(bool), valid)
    rng = np.random.default_rng(K)
    n_max = int(np.diff(fq.offsets).max())
    sc = rng.random((len(infos), n_max, K)).astype(np.float32)
    batches = [(0, len(infos), sc)]
    want = inf._accumulate_votes(*inf._votes_from_scores(fq, 0, batches, pts.shape[0], K))
    got = inf._vote_sums(fq, 0, batches, pts.shape[0], K)
    assert len(want[0]) > 50
    for g, w in zip(got, want):
        np.testing.assert_array_equal(g, w)


def test_tile_sharded_merge_at_k8():
    """infer_one_img split over 2 gloo ranks (CPU oracle stand-in for the model) == one process, at MAX_NEIGHBOR_QUERIES = 8, on
    disjoint tiles (every canvas pixel has one addend, so the results are identical)."""
    from scene_kit import run_worlds
    overrides = dict(SAMPLE_MARGIN=0, INFER_PATCHES_PER_EDGE=2, MAX_NEIGHBOR_QUERIES=8)
    res = run_worlds((1, 2), dict(base="e2e", overrides=overrides, shapes=[(512, 512)], seeds=[6], mode="serial"))
    results = {1: res[1][0], 2: res[2][0]}
    assert results[1][0].shape[0] > 30 and results[1][1].shape[0] > 50
    for a, b in zip(results[1], results[2]):
        np.testing.assert_array_equal(a, b)


class _NoDevice:
    """A stand-in model that fails the test if the inferencer touches it."""

    def parameters(self):
        raise AssertionError("the model was touched before MAX_NEIGHBOR_QUERIES was checked")

    def __getattr__(self, name):
        raise AssertionError(f"the model was touched ({name}) before MAX_NEIGHBOR_QUERIES was checked")


@pytest.mark.parametrize("k", [0, 65, 2.5, -1, True, "8"])
def test_inferencer_rejects_k_before_any_gpu_work(k):
    from oracle.synth import synth_scene
    cfg = Config(dict(PATCH_SIZE=256, SAMPLE_MARGIN=16, INFER_PATCHES_PER_EDGE=4, INFER_BATCH_SIZE=4, MAX_NEIGHBOR_QUERIES=k,
                      NEIGHBOR_RADIUS=64))
    img = synth_scene(448, seed=1)
    with pytest.raises(ValueError, match="MAX_NEIGHBOR_QUERIES must be an int from 1 to 64"):
        inf.infer_one_img(_NoDevice(), img, cfg, device="cpu")
    with pytest.raises(ValueError, match="from 1 to 64"):
        next(iter(inf.infer_imgs(_NoDevice(), iter([img]), cfg, device="cpu", tile_sharded=False)))
    with pytest.raises(ValueError, match="from 1 to 64"):
        inf._scene_plan(img, cfg)


@pytest.mark.parametrize("k", [1, 8, 16, 64, np.int64(32)])
def test_inferencer_accepts_k_in_range(k):
    assert inf.neighbor_queries(Config(dict(MAX_NEIGHBOR_QUERIES=k))) == int(k)
