"""Scene-level tiled inference (reference inferencer.py:61-234) on the HIP path.

    infer_one_img(net, img, config) -> (pred_nodes[N,2] (row, col), pred_edges[E,2],
                                        keypoint_mask u8[H,W], road_mask u8[H,W])

Pass 1 (tile batcher, model, mask fusion, normalise) runs entirely on the GPU behind
SAMRoad.scene_pass1 / scene_normalise: the u8 scene is uploaded ONCE (the reference ships 4x the
bytes as f32 tiles, inferencer.py:56,94) and tiles are cropped on the device.  The step between the
passes (mask -> points) and the pass-2 query builder / edge vote stay on the host as in the
reference (SURVEY.md §8f "next" rows), with the python triple loop replaced by numpy.

With torch.distributed initialised (one process per GPU) the tile list is split into contiguous
chunks per rank; canvases are summed on rank 0, points broadcast, edge votes gathered
(sam_road_amd/distributed.py).  Only rank 0 returns the graph; other ranks return None.
"""
import ctypes as C
import dataclasses
import functools
import os
import time
import warnings

import numpy as np
import scipy.spatial
import torch

from . import _lib
from . import distributed as D
from .aoi import aoi_edges, aoi_key_of, aoi_pack, aoi_ref, scene_aoi_key
from .geotiff import TiffScene
from .graph_points import extract_graph_points
from .hostcpu import fill_threads, worker_threads
from .mask_clean import MaskRule, idle as _rule_idle, mask_clean_key, mask_clean_table
from .nodata import nodata_table, scene_nodata_check, scene_nodata_key
from .resample import map_nodes, model_shape, scene_scale_key
from .float_scene import (float_hist_targets, float_ranges_from_hists, float_thresholds, nodata_keys as float_nodata_keys, scene_float_check,
                          scene_float_key, threshold_keys)
from .radiometry import band_luts, fixed_ranges, scene_bands_check, scene_bands_key, stretch_from_hist
from .tiling import get_patch_info_hw, get_patch_info_one_img, patches_per_axis, shard_tiles


def _vp(a):
    return a.ctypes.data_as(C.c_void_p)


class _Laps:
    """The tuning aid of SRH_PROFILE_HOST=1: `[tag] label: ms` since the previous lap, printed as each section ends.  `sync`: a device to
    synchronise before the clock is read (infer_one_img's stages); None: host wall time only.  Off (tag None, or the variable not set) a
    lap costs one test."""

    def __init__(self, tag=None, sync=None):
        self.on = tag is not None and os.environ.get("SRH_PROFILE_HOST") == "1"
        self.tag, self.sync, self.t = tag, sync, time.perf_counter()

    def __call__(self, label):
        if self.on and label:
            if self.sync is not None:
                torch.cuda.synchronize(self.sync)
            t = time.perf_counter()
            print(f"[{self.tag}] {label}: {(t - self.t) * 1e3:.1f} ms", flush=True)
            self.t = t


def build_patch_queries(graph_points, x0, y0, x1, y1, config):
    """inferencer.py:148-176 for one tile: closed-box point query (rtree.intersection semantics for
    degenerate boxes), kNN(k+1) within NEIGHBOR_RADIUS, self removed, missing neighbour -> source."""
    gx, gy = graph_points[:, 0], graph_points[:, 1]
    ids = np.nonzero((gx >= x0) & (gx <= x1) & (gy >= y0) & (gy <= y1))[0]
    n, k = len(ids), int(config.MAX_NEIGHBOR_QUERIES)
    pts = graph_points[ids, :] - np.array([[x0, y0]], dtype=graph_points.dtype)
    if n == 0:
        return ids, pts.reshape(0, 2), np.zeros((0, k, 2), np.int64), np.zeros((0, k), bool)
    tree = scipy.spatial.KDTree(pts)          # the reference's class (inferencer.py:156): leafsize 10, which decides ties
    _, knn = tree.query(pts, k=k + 1, distance_upper_bound=config.NEIGHBOR_RADIUS)
    knn = knn[:, 1:]
    src = np.tile(np.arange(n)[:, None], (1, k))
    valid = knn < n
    tgt = np.where(valid, knn, src)
    return ids, pts, np.stack([src, tgt], -1), valid


class _FlatQueries:
    """Pass-2 queries of tiles [lo, hi) as flat arrays (the library's layout): offsets [n_tiles+1] rows per tile, ids [total]
    global point index of every row, local [total,2] tile-local (x, y), knn [total,K] int32 tile-local target or -1."""

    def __init__(self, offsets, ids, local, knn, tied=None):
        self.offsets, self.ids, self.local, self.knn = offsets, ids, local, knn
        self.tied = tied          # u8 [total]: rows decided by the kd-tree restatement (tie at the cut-off / coincident point)
        self.n_tiles = offsets.shape[0] - 1

    def tile(self, t):
        """(ids, points, pairs[n,K,2], valid[n,K]) of tile t in the reference's per-tile form (inferencer.py:148-176)."""
        a, b = int(self.offsets[t]), int(self.offsets[t + 1])
        knn = self.knn[a:b]
        valid = knn >= 0
        src = np.arange(b - a, dtype=np.int64)[:, None]
        pairs = np.stack([np.broadcast_to(src, knn.shape), np.where(valid, knn, src)], axis=-1)
        return self.ids[a:b], self.local[a:b], pairs, valid


_KDTREE_OK = [None]      # None: not checked yet; True / False: the library's kd-tree restatement agrees with the installed scipy


def _kdtree_selfcheck():
    """csrc/kdtree_emul.hpp restates how scipy's kd-tree (validated against scipy 1.15) breaks ties at the k-th neighbour.  Another
    scipy build could break them differently with no signal, so the first call compares the two on a small lattice where almost
    every row is tied (one tile, 13 x 11 points 8 px apart plus duplicates); on a mismatch the per-tile scipy path answers from
    then on — the reference's own call, slower — and a warning names the installed version."""
    if _KDTREE_OK[0] is not None:
        return _KDTREE_OK[0]
    _KDTREE_OK[0] = True                                        # re-entrancy guard: the check itself goes through the library path
    xs, ys = np.meshgrid(np.arange(13) * 8 + 3, np.arange(11) * 8 + 5)
    pts = np.stack([xs.ravel(), ys.ravel()], 1).astype(np.int64)
    pts = np.concatenate([pts, pts[[5, 5, 40, 77]]], 0)         # coincident points as well
    cfg = type("C", (), dict(MAX_NEIGHBOR_QUERIES=16, NEIGHBOR_RADIUS=64))()
    infos = [(0, (0, 0), (127, 127))]
    try:
        want = build_patch_queries(pts, 0, 0, 127, 127, cfg)
        got = build_all_patch_queries(pts, infos, 0, 1, cfg)[0]
        # the SET of neighbours of every source point must be scipy's (which points fall on the kept side of a tie); the order inside a
        # group of equidistant neighbours is heap-internal in scipy and (distance, index) in the library — the edge vote does not see it
        nbr = lambda q: np.sort(np.where(q[3], q[2][..., 1], -1), axis=1)
        ok = np.array_equal(want[0], got[0]) and np.array_equal(want[1], got[1]) and np.array_equal(nbr(want), nbr(got))
    except Exception:
        ok = False
    if not ok:
        warnings.warn(f"the kd-tree tie-breaking restated in libsamroad_hip (validated against scipy 1.15) differs from the installed scipy "
                      f"{scipy.__version__}: pass-2 queries fall back to the per-tile scipy path", RuntimeWarning)
    _KDTREE_OK[0] = ok
    return ok


def build_all_patch_queries(graph_points, infos, lo, hi, config, flat=False, n_threads=None):
    """build_patch_queries for tiles [lo, hi) in ONE call into the library's host code (srh_pass2_count / srh_pass2_fill,
    csrc/host_geom.hip: closed-box filter + exact integer kNN per tile, worker threads).  Source points whose scipy result is
    not determined by distances alone (tie at the k-th neighbour, coincident points) are answered by the library's restatement
    of scipy's kd-tree on their tile's points (ids ascending; csrc/kdtree_emul.hpp), so those rows equal the reference's call
    element for element; elsewhere the order inside a group of equidistant neighbours is (distance, index) where scipy's is
    heap-internal.  Returns a list of per-tile tuples, or the flat form.  n_threads: worker threads of the fill (None: fill_threads());
    the result does not depend on it."""
    k, r = int(config.MAX_NEIGHBOR_QUERIES), config.NEIGHBOR_RADIUS
    n_tiles = hi - lo
    if n_tiles <= 0:
        return None if flat else []
    if float(r) != int(r) or not np.issubdtype(graph_points.dtype, np.integer) or not _kdtree_selfcheck():
        if flat:
            return None
        return [build_patch_queries(graph_points, *infos[t][1], *infos[t][2], config) for t in range(lo, hi)]
    lap = _Laps("queries")
    lib = _lib.load()
    pts = np.ascontiguousarray(graph_points, dtype=np.int64)
    boxes = np.ascontiguousarray([[*infos[t][1], *infos[t][2]] for t in range(lo, hi)], dtype=np.int32)
    counts = np.zeros(n_tiles, dtype=np.int64)
    if lib.srh_pass2_count(_vp(pts), pts.shape[0], _vp(boxes), n_tiles, _vp(counts)) != 0:
        raise _lib.SrhError("srh_pass2_count failed")
    offsets = np.zeros(n_tiles + 1, dtype=np.int64)
    np.cumsum(counts, out=offsets[1:])
    total = int(offsets[-1])
    ids = np.empty(total, dtype=np.int64)                     # srh_pass2_fill writes every element of the four arrays
    knn = np.empty((total, k), dtype=np.int32)
    amb = np.empty(total, dtype=np.uint8)
    local = np.empty((total, 2), dtype=np.int64)
    if lib.srh_pass2_fill(_vp(pts), pts.shape[0], _vp(boxes), n_tiles, k, int(r), _vp(offsets), _vp(ids), _vp(knn), _vp(amb), _vp(local),
                          fill_threads() if n_threads is None else max(1, int(n_threads))) != 0:
        raise _lib.SrhError("srh_pass2_fill failed")
    lap("count + fill (library)")
    # (source points whose answer is not determined by distances alone — a tie at the K-th neighbour, a coincident point — were
    # decided inside the library the way the reference's scipy kd-tree decides them, csrc/kdtree_emul.hpp; round 2 re-queried
    # scipy per tile here: 11.5 ms per CityScale scene)
    fq = _FlatQueries(offsets, ids, local, knn, amb)
    if flat:
        return fq
    return [fq.tile(t) for t in range(n_tiles)]


def _collate(xs):
    """Zero-pad along axis 0 to the longest item and stack (graph_collate_fn-style padding, inferencer.py:179-185)."""
    length = max(x.shape[0] for x in xs)
    out = np.zeros((len(xs), length) + xs[0].shape[1:], dtype=xs[0].dtype)
    for i, x in enumerate(xs):
        out[i, :x.shape[0]] = x
    return out


PASS2_SORT_TILES = True       # False: batches of consecutive tiles, as the reference forms them (tools / tests set it; no environment switch)


def _pass2_plan(fq, bs, sort_tiles=None):
    """Which tiles share a TopoNet batch: [(tiles int64 [nb] — indices into fq —, n_max, base_row)]; a batch is padded to its longest
    tile (graph_collate_fn-style, inferencer.py:179-185) and owns rows [base, base + nb * n_max) of the staging buffers.
    The reference batches consecutive tiles, so one dense tile makes 63 others carry its padding: a CityScale-like scene has 48 k
    query rows and 121 k padded ones.  TopoNet treats every row on its own (the sampler reads the row's tile, the transformer runs
    over the row's K neighbours), so WHICH tiles share a launch cannot change a score: tiles are grouped by ascending row count
    instead — 68 k padded rows, a little over half the device time and half the upload / download bytes of pass 2 — and the votes
    are still read in tile order (the reference's visiting order).  Empty tiles join no batch."""
    counts = np.diff(fq.offsets)
    if PASS2_SORT_TILES if sort_tiles is None else sort_tiles:
        idx = np.flatnonzero(counts > 0)
        idx = idx[np.argsort(counts[idx], kind="stable")]
        groups = [idx[i:i + bs] for i in range(0, len(idx), bs)]
    else:
        groups = [np.arange(i, min(i + bs, fq.n_tiles)) for i in range(0, fq.n_tiles, bs)]
    plan, rows_total = [], 0
    for tiles in groups:
        n_max = int(counts[tiles].max()) if len(tiles) else 0
        if n_max:
            plan.append((tiles.astype(np.int64), n_max, rows_total))
            rows_total += len(tiles) * n_max
    return plan, rows_total


def _contiguous(tiles):
    return len(tiles) > 0 and int(tiles[-1]) - int(tiles[0]) == len(tiles) - 1 and bool((np.diff(tiles) == 1).all())


def _pack_pass2_batches(fq, lo, hi, bs, K, alloc=None, sort_tiles=None):
    """Padded collate (inferencer.py:179-185) of every batch of _pass2_plan into ONE host buffer per kind: returns
    (plan, points f32 [rows,2], pairs i32 [rows,K,2], valid u8 [rows,K]).  Indices travel as int32 and the integer pixel coordinates
    as float32 (exact; srh_toponet accepts both, model.py:47's division promotes anyway).  `alloc(name, shape, dtype)` supplies the
    arrays (page-locked ones in the pipelined path).  (lo, hi: the tile range fq was built for; fq indexes tiles from 0.)"""
    if alloc is None:
        alloc = lambda name, shape, dtype: np.zeros(shape, dtype)
    plan, rows_total = _pass2_plan(fq, bs, sort_tiles)
    pts_h = alloc("points", (max(rows_total, 1), 2), np.float32)
    pairs_h = alloc("pairs", (max(rows_total, 1), K, 2), np.int32)
    valid_h = alloc("valid", (max(rows_total, 1), K), np.uint8)
    lib = _lib.load()
    local = np.ascontiguousarray(fq.local, dtype=np.int64)
    offsets = np.ascontiguousarray(fq.offsets, dtype=np.int64)
    knn = np.ascontiguousarray(fq.knn, dtype=np.int32)
    a_off, a_loc, a_knn = offsets.ctypes.data, local.ctypes.data, knn.ctypes.data
    a_pts, a_pairs, a_valid = pts_h.ctypes.data, pairs_h.ctypes.data, valid_h.ctypes.data
    for tiles, n_max, base in plan:
        # library host code (srh_pass2_pack): the numpy scatter of ~90k rows x 16 slots took 4 ms per CityScale scene.  One call per
        # run of consecutive tiles (raw addresses: a ctypes cast per argument would cost more than a tile's packing)
        runs = [(0, len(tiles))] if _contiguous(tiles) else [(j, j + 1) for j in range(len(tiles))]
        for j0, j1 in runs:
            row = base + j0 * n_max
            if lib.srh_pass2_pack(a_off + int(tiles[j0]) * 8, a_loc, a_knn, j1 - j0, n_max, K, a_pts + row * 8, a_pairs + row * K * 8,
                                  a_valid + row * K) != 0:
                raise _lib.SrhError("srh_pass2_pack failed")
    return plan, pts_h, pairs_h, valid_h


def _launch_pass2_batches(net, emb, plan, pts_d, pairs_d, valid_d, K, lo=0):
    """Sampler + TopoNet (inferencer.py:187-207) for every planned batch; nothing is fetched.  Returns [(tiles, scores)] with scores
    [nb, n_max, K] on the device (NaN -> -100 as the reference does before its range check); emb[t] = embeddings of fq's tile t."""
    out = []
    for tiles, n_max, base in plan:
        nb, sl = len(tiles), slice(base, base + len(tiles) * n_max)
        if _contiguous(tiles):
            e = emb[int(tiles[0]):int(tiles[-1]) + 1]
        else:
            # emb is an NCHW view of channels-last memory ([B,h,w,256] is what the library wrote and what srh_toponet reads): gather in
            # the STORAGE layout — index_select on the view would write an NCHW-contiguous copy that _topo then copies back
            e = emb.permute(0, 2, 3, 1).index_select(0, torch.as_tensor(tiles, device=emb.device)).permute(0, 3, 1, 2)
        scores = net.infer_toponet(e, pts_d[sl].view(nb, n_max, 2), pairs_d[sl].view(nb, n_max, K, 2), valid_d[sl].view(nb, n_max, K))
        out.append((tiles, torch.where(torch.isnan(scores), -100.0, scores).squeeze(-1)))
    return out


def _cfg_switch(v, default):
    """One parser for the boolean switches a YAML / override may spell several ways (PASS2_RAGGED, TILE_SHARD_PIPELINE): a missing key
    (the Config object's empty node) or None is the default; 'false' / 'no' / 'off' / '0' / '' are False; anything else bool(v)."""
    if v is None or (not isinstance(v, (bool, int, float, str)) and not v):     # absent key: addict-style empty node
        return default
    if isinstance(v, str):
        return v.strip().lower() not in ("false", "no", "off", "0", "")
    return bool(v)


def _poll_finite(net, device):
    """The library's non-finite sentinel (SAMRoad.check_finite, no synchronisation): an fp16 overflow in the encoder raises here instead
    of producing silently wrong masks.  The CPU stand-in models of the gloo tests have no such method."""
    chk = getattr(net, "check_finite", None)
    if chk is not None:
        chk(device, synchronize=False)


def _ragged_pass2(net, config):
    """Pass 2 without padding (srh_toponet_ragged: one launch for all query rows of the scene's tiles) unless the config switches it
    off (PASS2_RAGGED: False) or the model object has no such entry point (the CPU stand-in of the gloo tests)."""
    return _cfg_switch(config.PASS2_RAGGED, True) and hasattr(net, "infer_toponet_ragged")


def _pack_pass2_ragged(fq, K, alloc=None):
    """Unpadded collate of ALL query rows of fq's tiles (srh_pass2_pack_ragged): (points f32 [R,2], point_tile i32 [R], pairs i32
    [R,K,2], valid u8 [R,K]); rows keep their position in the flat query arrays, so tile t's scores are rows offsets[t] .. offsets[t+1]."""
    if alloc is None:
        alloc = lambda name, shape, dtype: np.zeros(shape, dtype)
    lib = _lib.load()
    offsets = np.ascontiguousarray(fq.offsets, dtype=np.int64)
    R = int(offsets[-1] - offsets[0])
    pts_h = alloc("points", (max(R, 1), 2), np.float32)
    tile_h = alloc("point_tile", (max(R, 1),), np.int32)
    pairs_h = alloc("pairs", (max(R, 1), K, 2), np.int32)
    valid_h = alloc("valid", (max(R, 1), K), np.uint8)
    local = np.ascontiguousarray(fq.local, dtype=np.int64)
    knn = np.ascontiguousarray(fq.knn, dtype=np.int32)
    if lib.srh_pass2_pack_ragged(offsets.ctypes.data, local.ctypes.data, knn.ctypes.data, fq.n_tiles, K, pts_h.ctypes.data,
                                 pairs_h.ctypes.data, valid_h.ctypes.data, tile_h.ctypes.data) != 0:
        raise _lib.SrhError("srh_pass2_pack_ragged failed")
    return R, pts_h, tile_h, pairs_h, valid_h


def _ragged_offsets(fq):
    """Row offsets of fq's tiles counted from 0 (int64 [n_tiles + 1]): what srh_toponet_ragged chunks the scene by."""
    return np.ascontiguousarray(np.asarray(fq.offsets, dtype=np.int64) - int(fq.offsets[0]))


def _ragged_batches(fq, scores_flat):
    """The per-tile view _tile_slots / _vote_sums take, of one flat score array [R, K]: tile t = rows offsets[t] .. offsets[t+1]."""
    off = np.asarray(fq.offsets, dtype=np.int64) - int(fq.offsets[0])
    sc = np.ascontiguousarray(scores_flat, dtype=np.float32)
    return [(np.array([t], dtype=np.int64), sc[off[t]:off[t + 1]][None]) for t in range(fq.n_tiles) if off[t + 1] > off[t]]


def _tile_slots(fq, lo, batches, K):
    """Per-tile view of the score batches: [(tile, address of its f32 [n_max, K] block, n_max)] in ascending tile order, plus the
    arrays that keep the memory alive.  batches = [(tiles, scores [nb,n_max,K])] or, for consecutive tiles, [(off, end, scores)]
    with absolute tile numbers (off - lo indexes fq)."""
    keep, slots = [], []
    for b in batches:
        if len(b) == 3:
            tiles, sc = np.arange(b[0] - lo, b[1] - lo, dtype=np.int64), b[2]
        else:
            tiles, sc = b
        sc = np.ascontiguousarray(sc, dtype=np.float32)
        if sc.ndim != 3 or sc.shape[0] != len(tiles) or sc.shape[2] != K:
            raise ValueError("score batch of the wrong shape")
        keep.append(sc)
        stride = sc.shape[1] * K * 4
        slots.extend((int(t), sc.ctypes.data + j * stride, sc.shape[1]) for j, t in enumerate(tiles))
    slots.sort(key=lambda x: x[0])
    return slots, keep


def _votes_from_scores(fq, lo, batches, n_pts, K):
    """inferencer.py:209-221's visiting order (tile, source point, neighbour slot) as flat (key, score) vote arrays; batches as in
    _tile_slots, on the host (srh_pass2_votes, csrc/host_geom.hip; it also enforces the reference's 0 <= score <= 1 assertion)."""
    lib = _lib.load()
    slots, keep = _tile_slots(fq, lo, batches, K)
    cap = int((fq.knn >= 0).sum())
    k = np.empty(cap, np.int64)
    s = np.empty(cap, np.float64)
    cnt_c = C.c_int64(0)
    offsets = np.ascontiguousarray(fq.offsets, dtype=np.int64)
    a_off = offsets.ctypes.data
    # runs of consecutive tiles that sit one after the other in one score array go through one call
    i = 0
    while i < len(slots):
        t, addr, n_max = slots[i]
        j = i + 1
        while j < len(slots) and slots[j][0] == slots[j - 1][0] + 1 and slots[j][2] == n_max and slots[j][1] == slots[j - 1][1] + n_max * K * 4:
            j += 1
        rc = lib.srh_pass2_votes(addr, j - i, n_max, K, a_off + t * 8, _vp(fq.ids), _vp(fq.knn), n_pts, _vp(k), _vp(s), cap, C.byref(cnt_c))
        if rc != 0:
            raise AssertionError("edge score outside [0, 1] (reference inferencer.py:219) or inconsistent query arrays")
        i = j
    del keep
    return k[:cnt_c.value], s[:cnt_c.value]


def _vote_sums(fq, lo, batches, n_pts, K, n_threads=None):
    """_votes_from_scores + _accumulate_votes without the ~700k intermediate votes of a CityScale scene: the library groups the
    query rows by source point and adds every point's votes into a table of its few dozen targets (srh_pass2_vote_sums,
    csrc/host_geom.hip; visiting order per key kept, so the float64 sums, counts and first-vote positions are the same, bit for
    bit — tests/test_host_logic.py).  batches as in _tile_slots (every tile is handed over as a "batch" of one: where its scores
    lie does not matter)."""
    lib = _lib.load()
    slots, keep = _tile_slots(fq, lo, batches, K)
    nb = len(slots)
    ptrs = (C.c_void_p * max(nb, 1))(*[a for _, a, _ in slots])
    tile0 = np.array([t for t, _, _ in slots], dtype=np.int32)
    cnt = np.ones(nb, dtype=np.int32)
    n_max = np.array([m for _, _, m in slots], dtype=np.int64)
    cap = int(fq.knn.size)                     # >= the number of distinct edges; the pages beyond them are never touched
    uk, sums, cnts, first = np.empty(cap, np.int64), np.empty(cap, np.float64), np.empty(cap, np.float64), np.empty(cap, np.int64)
    nu = C.c_int64(0)
    rc = lib.srh_pass2_vote_sums(ptrs, _vp(tile0), _vp(cnt), _vp(n_max), nb, K, _vp(fq.offsets), fq.n_tiles, _vp(fq.ids), _vp(fq.knn),
                                 n_pts, _vp(uk), _vp(sums), _vp(cnts), _vp(first), cap, C.byref(nu),
                                 worker_threads() if n_threads is None else max(1, int(n_threads)))
    del keep
    if rc != 0:
        raise AssertionError("edge score outside [0, 1] (reference inferencer.py:219) or inconsistent query arrays")
    return uk[:nu.value], sums[:nu.value], cnts[:nu.value], first[:nu.value]


def _accumulate_votes(k, s):
    """The reference's dict accumulation (float64 sums in visiting order) as a stable radix sort by key + one sequential pass
    in the library's host code (np.unique + np.bincount did the same in 11 ms per CityScale scene)."""
    if k.shape[0] == 0:
        return np.zeros(0, np.int64), np.zeros(0), np.zeros(0), np.zeros(0, np.int64)
    uk, sums, cnts, first = np.empty_like(k), np.empty_like(s), np.empty_like(s), np.empty_like(k)
    nu = C.c_int64(0)
    if _lib.load().srh_edge_vote_accumulate_mt(_vp(k), _vp(s), k.shape[0], _vp(uk), _vp(sums), _vp(cnts), _vp(first), C.byref(nu),
                                               worker_threads()) != 0:
        raise _lib.SrhError("srh_edge_vote_accumulate failed")
    return uk[:nu.value], sums[:nu.value], cnts[:nu.value], first[:nu.value]


def _queue_pass2(net, emb, fq, bs, K, ragged, io):
    """Pass 2 of fq's tiles (embeddings emb[t]) on its way: collate into `io`'s staging arrays, upload, launch the sampler + TopoNet, NaN
    -> -100 (as the reference does before its range check); nothing is fetched.  Every array of a kind is ONE host buffer and one copy:
    per-batch non_blocking uploads of pageable numpy memory went through torch's pinned-staging allocator and stalled 30-40 ms in some
    scenes (profiles/r02_scene_stages.txt).  ragged: every query row in ONE unpadded launch (srh_toponet_ragged: 68 k padded rows -> 48 k
    real ones on a CityScale scene); else the padded batches of _pass2_plan.  Returns (plan, score tensors on the device) for
    _collect_pass2; plan is empty when there is no query row (nothing was launched)."""
    if ragged:
        R, *host = _pack_pass2_ragged(fq, K, io.alloc)
        if R == 0:
            return [], []
        dev = [io.upload_packed(name, x[:R]) for name, x in zip(("points", "point_tile", "pairs", "valid"), host)]
        io.step("pass 2 uploaded")
        scores = net.infer_toponet_ragged(emb, *dev, tile_offsets=_ragged_offsets(fq))
        plan, scores = "ragged", [torch.where(torch.isnan(scores), -100.0, scores)]
    else:
        plan, *host = _pack_pass2_batches(fq, 0, fq.n_tiles, bs, K, io.alloc)
        if not plan:
            return [], []
        dev = [io.upload_packed(name, x) for name, x in zip(("points", "pairs", "valid"), host)]
        io.step("pass 2 uploaded")
        scores = [sc for _, sc in _launch_pass2_batches(net, emb, plan, *dev, K)]
    io.step("pass 2 launched")
    return plan, scores


def _collect_pass2(fq, plan, scores, n_pts, K, raw=False, n_threads=None):
    """The votes of a pass 2 that _queue_pass2 launched, from its scores on the host (numpy, in the order returned): the unique keys with
    their sums, counts and first-vote positions (_vote_sums), or for raw=True the votes themselves in visiting order."""
    batches = _ragged_batches(fq, scores[0]) if plan == "ragged" else [(tiles, sc) for (tiles, _, _), sc in zip(plan, scores)]
    if raw:
        return _votes_from_scores(fq, 0, batches, n_pts, K)
    return _vote_sums(fq, 0, batches, n_pts, K, n_threads)


def edge_votes(net, emb, graph_points, infos, lo, hi, config, device, raw=False):
    """Pass 2 over tiles [lo, hi) whose embeddings are emb[0 : hi-lo] (inferencer.py:135-221): returns the
    unique directed edge keys (src * n_points + tgt) with their score sums, counts and first-vote positions.  The sums are
    accumulated in float64 in the reference's order (tile, point, neighbour slot), so they are bit-identical to its dict loop
    for the tiles of THIS call (a multi-rank merge of such results: see distributed.gather_edge_votes).  raw=True returns the
    votes themselves, (keys int64, scores float64) in visiting order, for an exact merge on one rank."""
    lap = _Laps("edge_votes")                             # tuning aid: the wall time of each section
    bs = int(config.INFER_BATCH_SIZE)
    n_pts = graph_points.shape[0]
    K = int(config.MAX_NEIGHBOR_QUERIES)
    empty = (np.zeros(0, np.int64), np.zeros(0)) if raw else (np.zeros(0, np.int64), np.zeros(0), np.zeros(0), np.zeros(0, np.int64))
    fq = build_all_patch_queries(graph_points, infos, lo, hi, config, flat=True)
    lap("build_all_patch_queries")
    if fq is not None:
        # the library path: queue everything, then fetch with blocking copies (infer_imgs does the same two steps through its lane)
        ragged = _ragged_pass2(net, config)
        plan, scores = _queue_pass2(net, emb, fq, bs, K, ragged, _BlockingIO(device))
        lap("collate + H2D + launch (ragged)" if ragged else "collate + H2D + launch")
        if not plan:
            return empty
        out = _collect_pass2(fq, plan, [sc.cpu().numpy() for sc in scores], n_pts, K, raw)
        lap("score fetch + keys" if raw else "score fetch + vote sums")
        return out
    # non-integer coordinates / radius: the reference's per-tile scipy path, every batch launched before any scores are fetched, votes
    # gathered in numpy
    if hi - lo <= 0:
        return empty
    all_q = [build_patch_queries(graph_points, *infos[t][1], *infos[t][2], config) for t in range(lo, hi)]
    launched = []
    for off in range(lo, hi, bs):
        end = min(off + bs, hi)
        qs = all_q[off - lo:end - lo]
        if max(q[1].shape[0] for q in qs) == 0:
            continue
        pts = _collate([q[1].astype(np.float32) for q in qs])
        pairs = _collate([q[2].astype(np.int32) for q in qs])
        valid = _collate([q[3] for q in qs])
        scores = net.infer_toponet(emb[off - lo:end - lo], torch.as_tensor(pts).to(device), torch.as_tensor(pairs).to(device),
                                   torch.as_tensor(valid).to(device))
        launched.append((qs, torch.where(torch.isnan(scores), -100.0, scores).squeeze(-1)))
    lap("collate + H2D + launch")
    keys_l, score_l = [], []
    for qs, scores_dev in launched:
        scores = scores_dev.cpu().numpy()
        for b, (ids, _, prs, vld) in enumerate(qs):
            n = len(ids)
            if n == 0:
                continue
            sc = scores[b, :n][vld]
            assert ((sc >= 0.0) & (sc <= 1.0)).all()
            keys_l.append(ids[prs[:, :, 0]][vld].astype(np.int64) * n_pts + ids[prs[:, :, 1]][vld].astype(np.int64))
            score_l.append(sc.astype(np.float64))
    if not keys_l:
        return empty
    k = np.ascontiguousarray(np.concatenate(keys_l), dtype=np.int64)
    s = np.ascontiguousarray(np.concatenate(score_l), dtype=np.float64)
    lap("score fetch + keys")
    if raw:
        return k, s
    if k.shape[0] == 0:
        return empty
    out = _accumulate_votes(k, s)
    lap("accumulate")
    return out


def votes_to_edges(uk, sums, cnts, first, n_pts, threshold):
    """inferencer.py:224-228: mean directed score > TOPO_THRESHOLD, as an [E,2] array in the INSERTION order of the
    reference's dict (= order of each key's first vote; `first` from edge_votes / gather_edge_votes).  That order follows the
    per-tile point order, which in the reference is whatever rtree.intersection yields; here tiles list their points by
    ascending global index (the edge SET does not depend on it — pinned by tests/test_refrun_golden.py).  Among EQUIDISTANT
    neighbours of one source point the slot order is scipy-heap-internal in the reference and distance-then-index here."""
    n = int(uk.shape[0])
    arrs = [np.ascontiguousarray(a, dtype=d) for a, d in ((uk, np.int64), (sums, np.float64), (cnts, np.float64), (first, np.int64))]
    if n == 0 or n_pts <= 0 or any(a.shape != (n,) for a in arrs):
        keep = (sums / np.maximum(cnts, 1.0)) > threshold
        k = uk[keep][np.argsort(first[keep], kind="stable")]
        return np.stack([k // n_pts, k % n_pts], axis=1).reshape(-1, 2)
    out = np.empty((n, 2), dtype=np.int64)
    ne = C.c_int64(0)
    # library host code (srh_votes_to_edges): the kept edges dropped into a table indexed by first-vote position, read back in order
    rc = _lib.load().srh_votes_to_edges(*(_vp(a) for a in arrs), n, int(n_pts), float(threshold), _vp(out), C.byref(ne))
    if rc != 0:
        raise _lib.SrhError(f"srh_votes_to_edges failed ({rc})")
    return out[:ne.value].copy()


def _numpy_hugepages(enabled):
    """numpy's switch for madvise(MADV_HUGEPAGE) on array allocations of 4 MiB and more (NUMPY_MADVISE_HUGEPAGE); returns the
    previous state, None if this numpy has no such switch."""
    try:
        from numpy._core.multiarray import _set_madvise_hugepage
    except ImportError:
        try:
            from numpy.core.multiarray import _set_madvise_hugepage
        except ImportError:
            return None
    return bool(_set_madvise_hugepage(bool(enabled)))


def _host_quiet():
    """Context manager around the host stages of a scene.  Two process-wide settings are switched off inside and restored after:
    * the cyclic garbage collector — cheap insurance against a generation-2 sweep landing inside a scene; reference counting still
      frees every array as it goes.  (It was introduced for +20-30 ms scenes that turned out to be the second item.)
    * numpy's transparent-huge-page madvise for large arrays.  Every first touch / split of such a 2 MiB mapping raises an MMU
      notifier, and the amdgpu driver answers by taking the process's GPU queues off the hardware for 20-30 ms: with the host
      stages running beside pass 1 (infer_imgs) ONE kernel per scene was frozen for that long during the first ~30 scenes of a
      process — pass 1 took 105 instead of 75 ms on the device — until the heap had warmed up (profiles/r02_scene_pipeline.txt,
      rocprofv3 kernel trace); with plain 4 KiB pages the stalls are gone from the first scene on."""
    import contextlib
    import gc

    @contextlib.contextmanager
    def cm():
        was_gc = gc.isenabled()
        gc.disable()
        was_huge = _numpy_hugepages(False)
        try:
            yield
        finally:
            if was_huge:
                _numpy_hugepages(True)
            if was_gc:
                gc.enable()
    return cm()


def infer_one_img(net, img, config, device=None, valid=None, aoi=None):
    """reference inferencer.py:61-234: (pred_nodes (row, col), pred_edges, keypoint_mask u8, road_mask u8) of one scene (with the
    garbage collector and numpy's huge-page madvise paused for the duration of the call, see _host_quiet).
    valid (extension; bool or uint8 [H,W], non-zero = valid pixel; None = every pixel): only tiles that hold enough valid pixels are
    run (config.MIN_VALID_FRACTION), nodata pixels are replaced by config.NODATA_FILL on the device copy of the scene, and both masks
    are 0 on nodata, so no graph point lies there.  An all-true mask gives the result of valid=None bit for bit.
    config.SCENE_SCALE (extension): img (and valid) are at another ground resolution than the model's; both passes run on
    the scene resampled on the device, and the masks [H,W] and the nodes (row, col) come back in the scene's own pixels.
    aoi (extension): this scene's area of interest, a SCENE_AOI value (aoi.py) that takes the place of the config's key; None =
    the config's key.  The polygons are rasterised on the device and the result is a validity mask like `valid`, ANDed with it."""
    with _host_quiet():
        return _infer_one_img(net, img, config, device, valid, aoi)


MAX_NEIGHBOR_QUERIES_RANGE = (1, 64)


def neighbor_queries(config):
    """config.MAX_NEIGHBOR_QUERIES (K: candidate edges per graph point, inferencer.py:160-166), checked against what the fused TopoNet
    trunk supports.  Raises ValueError for anything but an int in 1..64 — before pass 1, not after a whole encoder pass."""
    k = config.MAX_NEIGHBOR_QUERIES
    lo, hi = MAX_NEIGHBOR_QUERIES_RANGE
    if isinstance(k, (bool, np.bool_)) or not isinstance(k, (int, np.integer)) or not lo <= k <= hi:
        raise ValueError(f"MAX_NEIGHBOR_QUERIES must be an int from {lo} to {hi}, got {k!r}")
    return int(k)


def _scene_plan(img, config):
    """Validated scene + its tile list (inferencer.py:63-76): (img u8 [H,W,3], infos, tile origins int32 [n,2] (x0, y0)) — under
    SCENE_PAD infos and origins are those of the padded scene (scene_pad_plan(img.shape, config) says how it is padded); under
    SCENE_BANDS img is the raw scene, u8 / u16 [H,W,C], checked against the key; under SCENE_SCALE the pads and the tiles are
    those of the MODEL frame, ceil(H p / q) x ceil(W p / q), and its size is what the limits apply to (the scene itself stays within 2^31 - 1
    pixels).
    H and W are independent; the reference's tile rule is applied per axis (tiling.get_patch_info_hw), and
    INFER_PATCHES_PER_EDGE may be an int or [n_y, n_x].  Everything that can be refused is refused here, before the device is
    touched."""
    neighbor_queries(config)
    img = img if isinstance(img, TiffScene) else np.asarray(img)      # a GeoTIFF scene (GEOTIFF) is checked by its header and decoded on the device
    # the reference uses img.shape[0] for both axes (inferencer.py:63,67) and casts whatever it gets to f32: it would mis-stride a
    # non-square scene and silently convert a non-u8 one.  Here H and W are separate all the way down; non-u8 is refused
    bands = scene_bands_key(config)
    flt = scene_float_plan(config)
    if flt is not None:                                    # SCENE_FLOAT: a raw float32 scene of 1 to 16 bands
        scene_float_check(img, flt)
    elif bands is not None:                                # SCENE_BANDS: a raw u8 / u16 scene of 1 to 16 bands
        scene_bands_check(img, bands)
    elif img.ndim != 3 or img.shape[2] != 3 or img.dtype != np.uint8:
        raise ValueError(f"infer_one_img expects an HxWx3 uint8 scene, got {img.dtype} {tuple(img.shape)}")
    if img.shape[0] < 1 or img.shape[1] < 1:
        raise ValueError(f"infer_one_img expects a scene of at least 1 x 1 pixels, got {tuple(img.shape)}")
    nodata = scene_nodata_key(config)
    if nodata is not None:                                 # SCENE_NODATA: the value(s) against THIS scene's dtype and bands
        scene_nodata_check(img, nodata)
    scene_aoi_key(config)                                  # SCENE_AOI: a key that cannot be used is refused here
    Hm, Wm = _model_frame(img.shape, scene_scale_key(config))
    pad = scene_pad_plan((Hm, Wm), config)
    top, bottom, left, right = pad[:4] if pad is not None else (0, 0, 0, 0)
    # SCENE_PAD: the tiles are planned on the virtual (padded) scene; infos / origins are in ITS frame
    infos, all_xy = _tile_plan(Hm + top + bottom, Wm + left + right, config, padded=pad is not None)
    return img, infos, all_xy


def scene_float_plan(config):
    """config.SCENE_FLOAT parsed: a float_scene.SceneFloat, or None when the key is missing, None or empty — no scene takes a
    step of it then.  ValueError, before the device is touched, for a key that cannot be used and for one that meets SCENE_BANDS (the key
    of integer scenes) or SCENE_NODATA (its values are integer levels; SCENE_FLOAT.nodata is the float form)."""
    flt = scene_float_key(config)
    if flt is not None and scene_bands_key(config) is not None:
        raise ValueError("SCENE_FLOAT does not combine with SCENE_BANDS (a scene is float32 or uint8 / uint16, not both): drop one of them")
    if flt is not None and scene_nodata_key(config) is not None:
        raise ValueError("SCENE_FLOAT does not combine with SCENE_NODATA (its values are integer levels): give the float values as nodata of SCENE_FLOAT")
    return flt


def _model_frame(shape, scale):
    """(H, W) of the frame pass 1 runs in: the scene's own without SCENE_SCALE, else ceil(H p / q) x ceil(W p / q) — and the scene itself
    must stay within the 2^31 - 1 pixels the resample entry takes."""
    H, W = int(shape[0]), int(shape[1])
    if scale is not None and H * W > 2 ** 31 - 1:
        raise ValueError(f"scene {H} x {W} has more than 2^31 - 1 pixels")
    return model_shape((H, W), scale)


def _tile_plan(H, W, config, stacklevel=3, padded=False):
    """The candidate tiles of an H x W scene: (infos, tile origins int32 [n,2] (x0, y0)), or ValueError.  A stride warning is attributed to
    the caller of this function's caller (stacklevel): whoever called _scene_plan or scene_tiles.  padded: H x W is the virtual size of a
    scene under SCENE_PAD (only the wording of the size limit differs: such a scene is never too small)."""
    P, m = int(config.PATCH_SIZE), int(config.SAMPLE_MARGIN or 0)
    for axis, size in (("height", H), ("width", W)):
        if size < P + 2 * m:
            raise ValueError(f"scene {axis} {size} px is smaller than PATCH_SIZE + 2 * SAMPLE_MARGIN = {P + 2 * m} (the config key SCENE_PAD "
                             f"pads such a scene at its borders)")
    if H * W > 2 ** 31 - 1:
        raise ValueError(f"scene {H} x {W}{' (padded by SCENE_PAD)' if padded else ''} has more than 2^31 - 1 pixels")
    n_y, n_x = patches_per_axis(config.INFER_PATCHES_PER_EDGE)
    for axis, size, n in (("height", H, n_y), ("width", W, n_x)):
        span = size - P - 2 * m                        # first to last tile origin
        if span > (n - 1) * P:                         # stride > PATCH_SIZE (one tile: any span at all)
            need = -(-span // P) + 1
            warnings.warn(f"INFER_PATCHES_PER_EDGE = {n} along the {axis} ({size} px) leaves pixels between the {P}-px tiles that no "
                          f"tile covers (they come out as 0); {need} tiles close the gap", stacklevel=stacklevel)
    infos = get_patch_info_hw(0, H, W, config.SAMPLE_MARGIN, config.PATCH_SIZE, (n_y, n_x))
    all_xy = np.array([[p[1][0], p[1][1]] for p in infos], dtype=np.int32)
    assert all_xy.min() >= 0 and all_xy[:, 0].max() + P <= W and all_xy[:, 1].max() + P <= H
    return infos, all_xy


# ---- scenes with a per-pixel validity mask (nodata) ---------------------------------------------------------------------------------
NODATA_FILL_DEFAULT = (124, 116, 104)     # the pixel mean (123.675, 116.28, 103.53) rounded: ~0 after normalisation


def _absent(v):
    """A config key that is not there: None, or the empty node a Config returns for a missing key."""
    return v is None or (isinstance(v, dict) and not v)


def _is_int(v):
    return isinstance(v, (int, np.integer)) and not isinstance(v, (bool, np.bool_))


def _valid_plan(valid, shape_hw, config):
    """Validated mask arguments, before the device is touched: (valid u8 [H,W] C-contiguous (a bool mask reinterpreted, not copied),
    MIN_VALID_FRACTION as a float in [0, 1] (missing key: 0), NODATA_FILL as three ints 0..255 (missing key: the rounded pixel
    mean)).  ValueError for a mask of another shape or dtype and for keys outside their range."""
    valid = np.asarray(valid)
    if valid.dtype not in (np.dtype(bool), np.dtype(np.uint8)):
        raise ValueError(f"valid must be a bool or uint8 mask, got dtype {valid.dtype}")
    if tuple(valid.shape) != tuple(shape_hw):
        raise ValueError(f"valid must have the scene's shape {tuple(shape_hw)}, got {tuple(valid.shape)}")
    return (np.ascontiguousarray(valid).view(np.uint8), *_mask_keys(config))


def _mask_keys(config):
    """(MIN_VALID_FRACTION as a float in [0, 1] (missing key: 0), NODATA_FILL as three ints 0..255): what a masked scene reads from the
    config, whether its mask was passed or derived (SCENE_NODATA).  ValueError for keys outside their range."""
    frac = 0.0 if _absent(config.MIN_VALID_FRACTION) else config.MIN_VALID_FRACTION
    if not (_is_int(frac) or isinstance(frac, (float, np.floating))) or not 0.0 <= float(frac) <= 1.0:        # NaN fails the range
        raise ValueError(f"MIN_VALID_FRACTION must be a number in [0, 1], got {frac!r}")
    return float(frac), _nodata_fill(config)


def _nodata_fill(config):
    """config.NODATA_FILL as three ints 0..255 (missing key: the rounded pixel mean), or ValueError."""
    fill = NODATA_FILL_DEFAULT if _absent(config.NODATA_FILL) else config.NODATA_FILL
    if not isinstance(fill, (list, tuple, np.ndarray)) or len(fill) != 3 or not all(_is_int(v) and 0 <= v <= 255 for v in fill):
        raise ValueError(f"NODATA_FILL must be three ints in 0..255, got {fill!r}")
    return tuple(int(v) for v in fill)


# ---- scenes padded at their borders (SCENE_PAD) --------------------------------------------------------------------------------------
SCENE_PAD_MODES = ("reflect", "edge", "constant")


def scene_pad_key(config):
    """config.SCENE_PAD (extension key) as (b_y, b_x, mode), or None for a missing key / None: nothing changes anywhere.
    An int b >= 0 means {border: b}; otherwise a mapping with `border` (an int or [b_y, b_x], values >= 0, default 0) and `mode` (one of
    SCENE_PAD_MODES, default 'reflect').  ValueError — before the device is touched — for anything else, unknown mapping keys included."""
    v = config.SCENE_PAD
    if _absent(v):                                       # None, or the empty node of a missing key (an empty mapping written out counts as that)
        return None
    if _is_int(v):
        v = {"border": v}
    if not isinstance(v, dict):
        raise ValueError(f"SCENE_PAD must be an int >= 0 or a mapping with border / mode, got {v!r}")
    unknown = sorted(set(v) - {"border", "mode"}, key=str)
    if unknown:
        raise ValueError(f"SCENE_PAD: unknown key {unknown[0]!r} (border, mode)")
    b = v.get("border", 0)
    if _is_int(b):
        b = [b, b]
    if not isinstance(b, (list, tuple)) or len(b) != 2 or not all(_is_int(x) and 0 <= x <= 2 ** 31 - 1 for x in b):
        raise ValueError(f"SCENE_PAD: border must be an int >= 0 or [b_y, b_x] of two such ints, got {v.get('border')!r}")
    mode = v.get("mode", "reflect")
    name = mode.strip().lower() if isinstance(mode, str) else mode
    if not isinstance(name, str) or name not in SCENE_PAD_MODES:
        raise ValueError(f"SCENE_PAD: mode must be one of {SCENE_PAD_MODES}, got {mode!r}")
    return int(b[0]), int(b[1]), name


def scene_pad_plan(shape, config):
    """How a scene of `shape` = (H, W[, 3]) is padded under config.SCENE_PAD: (top, bottom, left, right, mode, fill), or None when the key
    is absent (scene_pad_key).  Per axis the border b is added on both sides, and what the scene still lacks to hold one tile, short =
    max(0, PATCH_SIZE + 2 SAMPLE_MARGIN - (n + 2 b)), is split short // 2 before and the rest after.  fill: config.NODATA_FILL (the
    colour of `constant` padding), checked here.  The virtual scene is (H + top + bottom) x (W + left + right); its size limit is
    checked where the tiles are planned.  All four pads 0: the run is that of a scene without the key."""
    key = scene_pad_key(config)
    if key is None:
        return None
    b_y, b_x, mode = key
    need = int(config.PATCH_SIZE) + 2 * int(config.SAMPLE_MARGIN or 0)
    out = []
    for n, b in ((int(shape[0]), b_y), (int(shape[1]), b_x)):
        if n < 1:
            raise ValueError(f"a scene has at least 1 x 1 pixels, got shape {tuple(shape)}")
        short = max(0, need - (n + 2 * b))
        out += [b + short // 2, b + short - short // 2]
    return (*out, mode, _nodata_fill(config))


def scene_pad_override(config, border=None, mode=None):
    """The SCENE_PAD mapping of the command line's --scene-pad B / --scene-pad-mode MODE laid over the config's key: a flag that is given
    replaces that field, the other field stays as the config has it (defaults: border 0, reflect)."""
    key = scene_pad_key(config)
    b_y, b_x, m = key if key is not None else (0, 0, "reflect")
    return {"border": [b_y, b_x] if border is None else border, "mode": m if mode is None else mode}


def select_tiles(counts, patch_size, min_valid_fraction):
    """Indices (ascending: the kept tiles keep their relative order) of the tiles to run, from their valid-pixel counts: a tile is
    kept iff count > 0 and count >= MIN_VALID_FRACTION * PATCH_SIZE^2."""
    counts = np.asarray(counts, dtype=np.int64)
    if (counts < 0).any():
        raise ValueError("a tile lies outside the scene")
    return np.flatnonzero((counts > 0) & (counts >= float(min_valid_fraction) * int(patch_size) * int(patch_size)))


def scene_tiles(shape, config, valid=None, net=None, img=None, aoi=None):
    """The tiles infer_one_img runs for a scene of `shape` = (H, W[, 3]): the list of (0, (x0, y0), (x1, y1)) in the reference's
    x-outer / y-inner order.  With `valid` (see infer_one_img) only the kept tiles, selected exactly as infer_one_img selects them: the
    counts come from `net.scene_tile_valid` on the model's device, so `net` is required then (there is no host fallback).  The list is
    a TilePlan: its `orientations` are the names of config.TTA (['id'] without the key) — every tile of the list runs once per name.
    Under config.SCENE_PAD the tiles are those of the padded scene in the frame of the REAL one — origin (x0 - left, y0 - top), so a tile
    may start below 0 or overhang — and `pads` holds (top, bottom, left, right); the mask is padded like the scene before it is counted.
    Under config.SCENE_SCALE the plan is that of the MODEL frame: `scale` holds (p, q) ((1, 1) without the key), `model_shape` the frame's
    (H, W), the tiles, the pads and the size limits refer to it, and the mask is resampled by the validity rule before it is counted.
    Under config.SCENE_NODATA the plan depends on the pixels: `img`, the raw scene of that shape, is required (and `net`),
    and the mask is derived from it on the device exactly as infer_one_img derives it, ANDed with `valid` where one is given.
    Under config.SCENE_AOI (`aoi`: a scene's own value in its place, see infer_one_img) the polygons become a mask as in
    infer_one_img: on the device when `net` is given, and — the plan depends on no pixel — from aoi.aoi_ref on the host, counted by numpy,
    when it is not (and no SCENE_NODATA asks for the device)."""
    neighbor_queries(config)
    aoi = aoi_key_of(aoi) if aoi is not None else scene_aoi_key(config)
    nodata = scene_nodata_key(config)
    if nodata is not None:
        if img is None:
            raise ValueError("scene_tiles: with SCENE_NODATA the plan depends on the pixels of the scene: pass the raw scene as img=")
        img = np.asarray(img)
        lo, hi = scene_nodata_check(img, nodata)
        if tuple(img.shape[:2]) != tuple(int(v) for v in shape[:2]):
            raise ValueError(f"img must have the shape {tuple(shape[:2])}, got {tuple(img.shape[:2])}")
        shape = tuple(shape[:2])
    if len(shape) not in (2, 3) or (len(shape) == 3 and shape[2] != 3):
        raise ValueError(f"shape must be (H, W) or (H, W, 3), got {tuple(shape)}")
    H, W = int(shape[0]), int(shape[1])
    orientations = tta_plan(config)[0]
    if H < 1 or W < 1:
        raise ValueError(f"a scene has at least 1 x 1 pixels, got shape {tuple(shape)}")
    scale = scene_scale_key(config)
    Hm, Wm = _model_frame((H, W), scale)
    pad = scene_pad_plan((Hm, Wm), config)
    pads = pad[:4] if pad is not None else (0, 0, 0, 0)
    infos, all_xy = _tile_plan(Hm + pads[0] + pads[1], Wm + pads[2] + pads[3], config, padded=pad is not None)
    if valid is None and nodata is None and aoi is None:
        return TilePlan(_shift_infos(infos, pads), orientations, pads, scale, (Hm, Wm))
    v8, frac = (None, _mask_keys(config)[0]) if valid is None else _valid_plan(valid, (H, W), config)[:2]
    if net is None and aoi is not None and nodata is None:      # the host statement of the same plan
        from .resample import resample_ref
        v = aoi_ref((H, W), aoi, v8)
        if scale is not None:
            v = resample_ref(v, *scale, None, True, None)
        if any(pads):
            width = ((pads[0], pads[1]), (pads[2], pads[3]))
            v = np.pad(v, width, mode="constant") if pad[4] == "constant" else np.pad(v, width, mode=pad[4])
        P = int(config.PATCH_SIZE)
        counts = np.array([int(np.count_nonzero(v[y0:y0 + P, x0:x0 + P])) for x0, y0 in np.asarray(all_xy).tolist()], dtype=np.int64)
        return TilePlan(_shift_infos([infos[i] for i in select_tiles(counts, P, frac)], pads), orientations, pads, scale, (Hm, Wm))
    if net is None:
        raise ValueError("scene_tiles needs the model (net=) to count valid pixels on the device")
    device = next(net.parameters()).device
    valid_d = None if v8 is None else torch.from_numpy(v8).to(device)
    if aoi is not None:
        tab = aoi_edges(aoi, H, W)
        grow = mask_clean_table([(0, H, W, MaskRule(1, 1, 0))]) if aoi.buffer else None
        valid_d = _scene_aoi_mask(net, aoi, (H, W), valid_d, tab, None, grow, None).view(H, W)
    if nodata is not None:
        table = nodata_table([(0, H, W)], nodata)
        valid_d = _scene_nodata_mask(net, nodata, torch.from_numpy(np.ascontiguousarray(img)).to(device), lo, hi, valid_d, table, None).view(H, W)
    if scale is not None:
        valid_d = net.scene_resample(valid_d, *scale, valid_rule=True)
    if any(pads):
        valid_d = net.scene_pad(valid_d, pads, pad[4], (0, 0, 0))
    counts = net.scene_tile_valid(valid_d, torch.as_tensor(all_xy).to(device)).cpu().numpy()
    return TilePlan(_shift_infos([infos[i] for i in select_tiles(counts, config.PATCH_SIZE, frac)], pads), orientations, pads, scale, (Hm, Wm))


def _shift_infos(infos, pads):
    """Tiles of the padded scene in the frame of the real one: every corner moved by (-left, -top)."""
    top, _, left, _ = pads
    if not top and not left:
        return infos
    return [(k, (x0 - left, y0 - top), (x1 - left, y1 - top)) for k, (x0, y0), (x1, y1) in infos]


# ---- window-weighted fusion of overlapping tiles (FUSE_WINDOW) ----------------------------------------------------------------------
FUSE_WINDOW_RANGE = (2.0 ** -20, 2.0 ** 20)      # products of two values and sums over tiles stay normal f32 numbers
FUSE_WINDOW_NAMES = ("uniform", "hann", "triangle")


def fuse_window(config):
    """config.FUSE_WINDOW (extension key) as the 1-D profile w1, float32 [PATCH_SIZE] (numpy), or None for the uniform
    mean of the reference (key absent, None or 'uniform': nothing changes).  'hann': sin^2(pi (i + 0.5) / P); 'triangle':
    min(i + 0.5, P - i - 0.5) * 2 / P; a sequence of exactly P numbers: taken as given.  Computed in float64, rounded once to f32.
    A tile's weight at a pixel is w1[x - x0] * w1[y - y0].  ValueError — before the device is touched — for an unknown name, a wrong
    length, and a value that is not finite or not inside [2^-20, 2^20] (so zero and negative values too)."""
    v = config.FUSE_WINDOW
    if _absent(v):
        return None
    P = int(config.PATCH_SIZE)
    if isinstance(v, str):
        name = v.strip().lower()
        if name == "uniform":
            return None
        i = np.arange(P, dtype=np.float64)
        if name == "hann":
            w = np.sin(np.pi * (i + 0.5) / P) ** 2
        elif name == "triangle":
            w = np.minimum(i + 0.5, P - i - 0.5) * 2.0 / P
        else:
            raise ValueError(f"FUSE_WINDOW must be one of {FUSE_WINDOW_NAMES} or a sequence of PATCH_SIZE = {P} numbers, got {v!r}")
    else:
        if not isinstance(v, (list, tuple, np.ndarray)):
            raise ValueError(f"FUSE_WINDOW must be one of {FUSE_WINDOW_NAMES} or a sequence of PATCH_SIZE = {P} numbers, got {v!r}")
        try:
            w = np.asarray(v)
            numeric = w.dtype.kind in "iuf"
            w = w.astype(np.float64) if numeric else None
        except (TypeError, ValueError):
            w = None
        if w is None:
            raise ValueError("FUSE_WINDOW: a profile must hold plain numbers")
        if w.shape != (P,):
            raise ValueError(f"FUSE_WINDOW: a profile must have exactly PATCH_SIZE = {P} values, got shape {tuple(w.shape)}")
    lo, hi = FUSE_WINDOW_RANGE
    with np.errstate(over="ignore"):
        w32 = w.astype(np.float32)
    if not (np.isfinite(w).all() and np.isfinite(w32).all() and (w32 >= lo).all() and (w32 <= hi).all()):
        bad = int(np.flatnonzero(~(np.isfinite(w32) & (w32 >= lo) & (w32 <= hi)))[0])
        raise ValueError(f"FUSE_WINDOW: every value must be finite and inside [2^-20, 2^20]; value {bad} is {w[bad]!r}")
    return np.ascontiguousarray(w32)


# ---- test-time augmentation over the 8 orientations of a tile (TTA) ------------------------------------------------------------------
TTA_NAMES = ("id", "flip_h", "flip_v", "rot180", "transpose", "rot90", "rot270", "anti_transpose")      # the index is the code
_TTA_INVERSE = {"rot90": "rot270", "rot270": "rot90"}                                                   # every other one is its own inverse


def orient_tile(arr, name):
    """A square tile arr[row, col, ...] in orientation `name`, as a view: the table of DESIGN.md §6f, which IS the definition."""
    T = np.asarray(arr)
    if T.ndim < 2 or T.shape[0] != T.shape[1]:
        raise ValueError(f"a tile must be square in its first two axes, got shape {tuple(T.shape)}")
    if name == "id":
        return T
    if name == "flip_h":
        return T[:, ::-1]
    if name == "flip_v":
        return T[::-1, :]
    if name == "rot180":
        return T[::-1, ::-1]
    if name == "transpose":
        return T.swapaxes(0, 1)
    if name == "rot90":
        return np.rot90(T, 1, axes=(0, 1))
    if name == "rot270":
        return np.rot90(T, 3, axes=(0, 1))
    if name == "anti_transpose":
        return T[::-1, ::-1].swapaxes(0, 1)
    raise ValueError(f"an orientation must be one of {TTA_NAMES}, got {name!r}")


def unorient_tile(arr, name):
    """The inverse of orient_tile: unorient_tile(orient_tile(T, name), name) == T."""
    return orient_tile(arr, _TTA_INVERSE.get(name, name))


def tta_plan(config):
    """config.TTA (extension key) as (names, codes): the orientations every tile is run in, in config order, and their
    codes 0..7 (the index in TTA_NAMES).  Key absent or None: (['id'], [0]) — nothing changes.  A sequence of names, or one string of
    names separated by commas (the CLI's form).  ValueError — before the device is touched — for an unknown name, a name listed twice, a
    first entry that is not 'id' (its embeddings feed pass 2), an empty list and more than 8 entries."""
    v = config.TTA
    if _absent(v):
        return ["id"], [0]
    if isinstance(v, str):
        v = [t for t in v.split(",")]
    if not isinstance(v, (list, tuple)):
        raise ValueError(f"TTA must be a sequence of orientation names out of {TTA_NAMES}, got {v!r}")
    if not 1 <= len(v) <= 8:
        raise ValueError(f"TTA must list 1 to 8 orientations, got {len(v)}")
    names = []
    for t in v:
        name = t.strip().lower() if isinstance(t, str) else t
        if not isinstance(name, str) or name not in TTA_NAMES:
            raise ValueError(f"TTA: an orientation must be one of {TTA_NAMES}, got {t!r}")
        if name in names:
            raise ValueError(f"TTA: orientation {name!r} is listed twice")
        names.append(name)
    if names[0] != "id":
        raise ValueError(f"TTA: the first orientation must be 'id' (its embeddings feed pass 2), got {names[0]!r}")
    return names, [TTA_NAMES.index(n) for n in names]


# ---- several small scenes as one pass 1 (SCENE_GROUP) --------------------------------------------------------------------------------
def scene_group_key(config, group=None):
    """config.SCENE_GROUP (extension key), or `group` where it is given (infer_imgs' argument), as the number of
    consecutive scenes that run as one: 1 for a missing key, None or 1 — nothing changes anywhere.  ValueError — before the device is
    touched — for anything but None and an int >= 1."""
    v = config.SCENE_GROUP if group is None else group
    if _absent(v):
        return 1
    if not _is_int(v) or v < 1:
        raise ValueError(f"SCENE_GROUP must be an int >= 1 (the number of consecutive scenes that run as one), got {v!r}")
    return int(v)


@dataclasses.dataclass
class _GroupScene:
    """One scene of a group, planned: everything _pass1_front fixes for a scene before the device is touched."""
    img: np.ndarray                   # u8 [H,W,3]; under SCENE_BANDS the raw scene, u8 / u16 [H,W,C]
    valid: np.ndarray                 # u8 [H,W], or None
    shape: tuple                      # (H, W)
    pads: tuple                       # (top, bottom, left, right): zeros without SCENE_PAD
    infos: list                       # the candidate tiles and their origins in the scene's VIRTUAL frame
    all_xy: np.ndarray
    row0: int = 0                     # the stack row the virtual scene starts at

    @property
    def virtual(self):
        return self.shape[0] + self.pads[0] + self.pads[1], self.shape[1] + self.pads[2] + self.pads[3]


def _plan_group_scene(img, valid, config):
    """_pass1_front's planning step for one scene of a group: the same checks in the same order, so a scene that would raise alone
    raises the same error here."""
    if isinstance(img, TiffScene):
        raise ValueError(f"{img.path}: a GeoTIFF scene (GEOTIFF) does not combine with SCENE_GROUP (a group's scenes are packed from host arrays): "
                         "drop one of them")
    img, infos, all_xy = _scene_plan(img, config)
    pad = scene_pad_plan(img.shape, config)
    shape = tuple(int(v) for v in img.shape[:2])
    if valid is not None:
        valid = _valid_plan(valid, shape, config)[0]
    return _GroupScene(np.ascontiguousarray(img), valid, shape, tuple(pad[:4]) if pad is not None else (0, 0, 0, 0), infos, all_xy)


def group_fits(sizes, n_max):
    """Whether scenes of the virtual sizes `sizes` = [(H', W'), ...] may share one stack: at most n_max of them, and the stack (sum H') x
    (max W') within the 2^31 - 1 pixels a scene may have.  (The existing entries have no tile limit of their own below that of an int.)"""
    return len(sizes) <= n_max and sum(h for h, _ in sizes) * max(w for _, w in sizes) <= 2 ** 31 - 1


def _scene_groups(imgs, valids, config, n):
    """The scenes of a stream as planned groups, lazily: lists of up to n consecutive _GroupScene.  A group closes at n scenes and before
    a scene that would take the stack past group_fits or, under SCENE_BANDS, whose dtype or band count differs (one apply launch serves the
    group's ragged buffer); `valids` is read in step with `imgs`.  Every scene is planned (and refused) as it is read."""
    group = []
    for img in imgs:
        sc = _plan_group_scene(img, next(valids), config)
        if group and (not group_fits([g.virtual for g in group] + [sc.virtual], n) or (sc.img.dtype, sc.img.shape[2]) != (group[0].img.dtype, group[0].img.shape[2])):
            yield group
            group = []
        group.append(sc)
        if len(group) == n:
            yield group
            group = []
    if group:
        yield group


def group_geometry(scenes, any_mask=None, all_masked=False):
    """The stack of a group: (Ha, Wa, tables int64 [T,n,8], tile origins int32 [N,2] on the stack, first tile of every
    scene [n+1]); sets every scene's row0.  Table rows are {byte offset, H, W, top, left, H', W', row0} (include/samroad_hip.h).  tables[0]
    packs the scenes (offsets into the ragged u8 [sum H W 3] buffer), tables[1] crops the masks (offsets into the ragged [sum H W]
    outputs) and, if any scene has a mask, tables[2] packs the masks: a masked scene's block is its H x W mask, an unmasked scene's is H' x
    W' ones with no pads — its whole rectangle is valid, whatever the pad mode.  all_masked (SCENE_NODATA: the device derives an H x W mask
    for every scene): every row of tables[2] takes the masked-scene form, at the offsets of tables[1]."""
    if any_mask is None:
        any_mask = any(sc.valid is not None for sc in scenes)
    any_mask = any_mask or all_masked
    n = len(scenes)
    tables = np.zeros((3 if any_mask else 2, n, 8), dtype=np.int64)
    row0 = off = moff = 0
    xy, first = [], [0]
    for k, sc in enumerate(scenes):
        (H, W), (Hv, Wv), (top, _, left, _) = sc.shape, sc.virtual, sc.pads
        sc.row0 = row0
        tables[0, k] = (3 * off, H, W, top, left, Hv, Wv, row0)
        tables[1, k] = (off, H, W, top, left, Hv, Wv, row0)
        if any_mask:
            own = all_masked or sc.valid is not None
            tables[2, k] = (moff, H, W, top, left, Hv, Wv, row0) if own else (moff, Hv, Wv, 0, 0, Hv, Wv, row0)
            moff += H * W if own else Hv * Wv
        xy.append(sc.all_xy + np.array([[0, row0]], dtype=np.int32))
        first.append(first[-1] + len(sc.infos))
        off += H * W
        row0 += Hv
    Wa = max(sc.virtual[1] for sc in scenes)
    return row0, Wa, tables, np.ascontiguousarray(np.concatenate(xy), dtype=np.int32), np.array(first, dtype=np.int64)


def _group_stack(ctx, io, scenes):
    """The device side of a group's front end up to where a single scene stands after its pad step: one staged ragged upload of the real
    scenes (and one of the masks, if any scene has one), the tables, the pack launches.  Returns (stack u8 [Ha,Wa,3], mask stack u8
    [Ha,Wa] or None, tile origins on the stack, first tile per scene, crop table (host), crop table (device))."""
    net, config = ctx.net, ctx.config
    pad = scene_pad_plan(scenes[0].shape, config)
    mode, fill = (pad[4], pad[5]) if pad is not None else ("reflect", (0, 0, 0))
    any_mask, nodata = any(sc.valid is not None for sc in scenes), ctx.nodata
    Ha, Wa, tables, all_xy, first = group_geometry(scenes, any_mask, all_masked=nodata is not None)

    def stage(name, n):
        return io.alloc(name, (n,), np.uint8) if io.alloc is not None else np.empty(n, np.uint8)

    n_px, raw = int(tables[1, -1, 0] + tables[1, -1, 1] * tables[1, -1, 2]), scenes[0].img
    if ctx.bands is None:
        src = stage("group_scene", n_px * 3)
        for sc, off in zip(scenes, tables[0, :, 0]):
            src[off:off + sc.img.size] = sc.img.reshape(-1)
    else:                                              # SCENE_BANDS: the ragged buffer holds the raw pixels, n_px x C elements of one dtype
        src = stage("group_scene", n_px * raw.shape[2] * raw.itemsize)
        elems = src.view(raw.dtype)
        for sc, off in zip(scenes, tables[1, :, 0] * raw.shape[2]):
            elems[off:off + sc.img.size] = sc.img.reshape(-1)
    ragged = io.upload_packed("group_scene", src)
    tables_d = io.upload("group_tables", tables)
    if nodata is not None and (nodata.min_area > 1 or nodata.grow > 0):      # the scenes' H x W blocks of the derived mask, at tables[1]'s offsets
        nd_table = nodata_table([(int(off), int(h), int(w)) for off, h, w in tables[1, :, :3]], nodata)
        nd_table_d = io.upload("nodata_table", nd_table)
    else:
        nd_table = nd_table_d = None
    if any_mask:
        msrc = stage("group_mask", int(tables[2, -1, 0] + tables[2, -1, 1] * tables[2, -1, 2]))
        for sc, (off, h, w) in zip(scenes, tables[2, :, :3]):
            msrc[off:off + h * w] = 1 if sc.valid is None else sc.valid.reshape(-1)
        mragged = io.upload_packed("group_mask", msrc)
    io.step("upload")
    host = torch.from_numpy(tables)
    if nodata is not None:                             # SCENE_NODATA: the ragged raw buffer is matched in one launch (it knows nothing of rows);
        lo, hi = scene_nodata_check(raw, nodata)       # the grow and the area rule run table-driven over the scenes' blocks
        pixels = ragged.view(torch.from_numpy(raw[:0, :0].reshape(0)).dtype).view(n_px, raw.shape[2])
        mragged = _scene_nodata_mask(net, nodata, pixels, lo, hi, mragged if any_mask else None, nd_table, nd_table_d)
        any_mask = True
        io.step("nodata")
    if ctx.bands is not None:                          # one apply launch over the ragged buffer, then the unchanged pack kernel
        ragged = _scene_bands_front(ctx, io, ragged.view(torch.from_numpy(raw[:0, :0].reshape(0)).dtype).view(n_px, raw.shape[2])).view(-1)
    scene = net.scene_group_pack(ragged, host[0], 3, Ha, Wa, mode, fill, table_dev=tables_d[0])
    valid_d = net.scene_group_pack(mragged, host[2], 1, Ha, Wa, mode, (0, 0, 0), table_dev=tables_d[2]) if any_mask else None
    io.step("pack")
    return scene, valid_d, all_xy, first, host[1], tables_d[1]


class TilePlan(list):
    """What scene_tiles returns: the list of tiles, in `orientations` the names every one of them is run in, in `pads` the (top, bottom,
    left, right) of SCENE_PAD (zeros without it), in `scale` the (p, q) of SCENE_SCALE ((1, 1) without it) and in `model_shape` the (H, W)
    of the frame the tiles lie in (None: the scene's own)."""

    def __init__(self, infos, orientations, pads=(0, 0, 0, 0), scale=None, model_shape=None):
        super().__init__(infos)
        self.orientations = list(orientations)
        self.pads = tuple(int(v) for v in pads)
        self.scale = (1, 1) if scale is None else (int(scale[0]), int(scale[1]))
        self.model_shape = None if model_shape is None else (int(model_shape[0]), int(model_shape[1]))


def _empty_result(H, W):
    """What a scene without a kept tile returns: no nodes, no edges, zero masks."""
    return np.zeros((0, 2), dtype=np.int64), np.zeros((0, 2), dtype=np.int32), np.zeros((H, W), np.uint8), np.zeros((H, W), np.uint8)


class _StagingPool:
    """Page-locked host staging buffers of one in-flight scene, grown on demand and reused (a hipHostMalloc costs
    milliseconds).  On a CPU device (the gloo / stand-in tests) plain tensors take their place."""

    def __init__(self, device):
        self._pin = device.type == "cuda"
        self._t = {}

    def get(self, name, shape, dtype):
        n = int(np.prod(shape))
        t = self._t.get(name)
        if t is None or t.dtype != dtype or t.numel() < n:
            t = torch.empty(max(n + n // 4, 1), dtype=dtype, pin_memory=self._pin)
            self._t[name] = t
        return t[:n].view(tuple(shape))


class _Lane:
    """Stream plumbing of infer_imgs: uploads go through page-locked staging on a side stream, the compute stream waits on an
    event, downloads are asynchronous copies into page-locked buffers followed by an event — no call blocks the host until the
    results are actually needed.  (A pageable-memory hipMemcpyAsync is stream-ordered AND host-blocking: issued behind a scene's
    pass 1 it would park the host for the whole pass.)  Degenerates to synchronous copies on a CPU device."""

    times = None       # tools set a list here (tools/scene_bench.py; no environment switch): every unit of infer_imgs that ran a pass 2 then
                       # appends (scenes in the unit, device ms of pass 1, device ms of pass 2), from the events of the profile

    def __init__(self, device):
        self.device = device
        self.cuda = device.type == "cuda"
        self.copy_stream = torch.cuda.Stream(device) if self.cuda else None

    def upload(self, pool, name, arr):
        """numpy array -> device tensor, stream-ordered before everything launched on the compute stream afterwards."""
        t_dtype = torch.from_numpy(arr[:0].reshape(0)).dtype
        stage = pool.get("up_" + name, arr.shape, t_dtype)
        stage.numpy()[...] = arr
        return self.upload_staged(stage)

    def upload_staged(self, stage):
        if not self.cuda:
            return stage.clone()
        main = torch.cuda.current_stream(self.device)
        dst = torch.empty(stage.shape, dtype=stage.dtype, device=self.device)
        self.copy_stream.wait_stream(main)           # dst may be a recycled block still in use by queued compute work
        with torch.cuda.stream(self.copy_stream):
            dst.copy_(stage, non_blocking=True)
        dst.record_stream(self.copy_stream)
        main.wait_stream(self.copy_stream)
        return dst

    def on_copy_stream(self, pool, name, fn):
        """fn() -> a small device tensor, launched on the copy stream (behind the uploads queued so far, which themselves wait for the
        compute work queued when they were issued) and fetched: returns it as a numpy array after ONE host wait on that stream's event.
        For work that touches nothing the compute stream owns."""
        if not self.cuda:
            return fn().numpy().copy()
        with torch.cuda.stream(self.copy_stream):
            t = fn()
            h = pool.get("down_" + name, t.shape, t.dtype)
            h.copy_(t, non_blocking=True)
            ev = torch.cuda.Event()
            ev.record(self.copy_stream)
        t.record_stream(self.copy_stream)
        ev.synchronize()
        return h.numpy().copy()

    def download(self, pool, name, tensors):
        """Device tensors -> page-locked host tensors (asynchronous) + the event that says they have landed."""
        outs = []
        for i, t in enumerate(tensors):
            h = pool.get(f"down_{name}{i}", t.shape, t.dtype)
            h.copy_(t, non_blocking=self.cuda)
            outs.append(h)
        ev = None
        if self.cuda:
            ev = torch.cuda.Event()
            ev.record(torch.cuda.current_stream(self.device))
        return outs, ev


class _BlockingIO:
    """How infer_one_img and the tile-sharded loops move a scene's arrays: one blocking copy each way, pageable memory.  The other
    implementation of the same four operations is _LaneIO.  `lap` (a _Laps) names the steps of pass 1 for the profile."""
    STEPS = {"upload": "scene upload", "tiff": "GeoTIFF assemble", "aoi": "area of interest mask", "nodata": "nodata mask", "bands": "band select + stretch", "float": "float scene -> u8 + mask", "scale": "scene resample", "pad": "scene pad", "pack": "group pack", "select": "tile selection (count kernel + counts D2H)", "fill": "nodata fill",
             "pass 1": "pass 1 (GPU)"}
    alloc = None                                       # the pass-2 collate fills plain numpy arrays

    def __init__(self, device, lap=None, async_scene=False):
        self.device, self.lap, self.async_scene = device, lap, async_scene

    def upload(self, name, arr):
        """numpy array -> device tensor.  On a CPU device the tensor shares the array's memory."""
        return torch.from_numpy(np.ascontiguousarray(arr)).to(self.device, non_blocking=self.async_scene and name == "scene")

    upload_packed = upload                             # an array that `alloc` supplied and the collate filled

    def counts(self, fn, after_compute=False, name="counts"):
        """fn() -> the valid-pixel counts on the device; returns them on the host (int32 [n]) after one wait.  (SCENE_BANDS fetches its
        histogram the same way, under a name of its own.)"""
        return fn().cpu().numpy()

    def step(self, name):
        if self.lap is not None:
            self.lap(self.STEPS.get(name))


class _LaneIO:
    """The operations of _BlockingIO on infer_imgs' lane, for ONE scene in flight (`pool`: its page-locked staging): uploads are staged
    and stream-ordered, the counts come back over the copy stream, the pass-2 collate writes straight into the staging buffers.  With the
    profile on, five device events time the scene's pass 1, pass 2 and score download."""
    STEPS = {"upload": "stage + queue scene upload", "tiff": "queue GeoTIFF assemble", "aoi": "queue area of interest mask", "nodata": "queue nodata mask", "bands": "band select + stretch (upload lane)", "float": "float scene -> u8 + mask (upload lane)", "scale": "queue scene resample", "pad": "queue scene pad", "pack": "queue group pack", "select": "tile selection (upload lane)", "pass 1": "queue pass 1"}
    EVENTS = {"launch pass 1": 0, "normalised": 1, "pass 2 uploaded": 2, "pass 2 launched": 3, "pass 2 on its way back": 4}

    def __init__(self, lane, pool, lap):
        self.lane, self.pool, self.lap, self.stage = lane, pool, lap, {}
        self.t = [torch.cuda.Event(enable_timing=True) for _ in self.EVENTS] if (lap.on or lane.times is not None) and lane.cuda else None

    def upload(self, name, arr):
        return self.lane.upload(self.pool, name, arr)

    def alloc(self, name, shape, dtype):
        self.stage[name] = self.pool.get("up_" + name, shape, torch.from_numpy(np.zeros(0, dtype)).dtype)
        return self.stage[name].numpy()                # srh_pass2_pack writes every row, padding included

    def upload_packed(self, name, arr):
        return self.lane.upload_staged(self.stage[name][:arr.shape[0]])

    def counts(self, fn, after_compute=False, name="counts"):
        # after_compute: fn reads what the compute stream produced (the padded mask of SCENE_PAD), so the upload lane waits for it first
        if after_compute and self.lane.cuda:
            self.lane.copy_stream.wait_stream(torch.cuda.current_stream(self.lane.device))
        # on the upload lane: the count kernel uses no workspace of the library context, so it and the n int32 on their way back are
        # queued on the copy stream.  Like every upload of this lane they start after what the compute stream holds at this moment (the
        # previous scene's TopoNet work, about a millisecond), and the host waits for the counts
        return self.lane.on_copy_stream(self.pool, name, fn)

    def step(self, name):
        if self.t is not None and name in self.EVENTS:
            self.t[self.EVENTS[name]].record()
        self.lap(self.STEPS.get(name))


MASK_CLEAN_MAX_IMAGES = 4096             # = MC_MAX_IMAGES of csrc/mask_clean_piece.hpp: the images of one srh_mask_clean call


def mask_clean_plan(config):
    """config.MASK_CLEAN parsed: a mask_clean.MaskCleanPlan — per mask (t_on, min_area, t_peak), and the connectivity —
    or None when the key is missing, None, empty or names nothing that could drop a component: no scene takes a step of it then.
    ValueError for anything else (mask_clean.mask_clean_key), before the device is touched."""
    return mask_clean_key(config)


def _mask_clean_images(plan, blocks, total):
    """The images of one srh_mask_clean call over a uint8 [2, total] buffer (row 0 keypoint masks, row 1 road masks) that holds the H x W
    blocks `blocks` = [(offset in a row, H, W), ...]: the table (host, int64 [n,8]), or None when no mask has a rule that can drop."""
    images = [(row * total + off, H, W, rule) for row, rule in enumerate((plan.keypoint, plan.road)) if not _rule_idle(rule) for off, H, W in blocks]
    return mask_clean_table(images) if images else None


class _SceneSetup:
    """What one infer_one_img / infer_imgs / _infer_imgs_tile_sharded call fixes for all of its scenes.  sharded: the scenes' tiles are
    split over the ranks of torch.distributed (world 1 without it); False: this process runs whole scenes and issues no collective."""

    def __init__(self, net, config, device, sharded):
        self.net, self.config, self.sharded = net, config, sharded
        self.device = torch.device(device) if device is not None else next(net.parameters()).device
        self.K = neighbor_queries(config)
        self.bs = int(config.INFER_BATCH_SIZE)
        dist = sharded and D.is_distributed()
        self.world = torch.distributed.get_world_size() if dist else 1
        self.rank = torch.distributed.get_rank() if dist else 0
        self.bands = scene_bands_key(config)             # SCENE_BANDS, or None: no scene takes a step of it
        self.bands_luts = {}                             # levels -> the tables of a fixed range on the device, built once per call
        self.float = scene_float_plan(config)            # SCENE_FLOAT as a SceneFloat, or None: no scene takes a step of it
        self.float_thr = None                            # the threshold keys of a fixed range on the device, built once per call
        self.scale = scene_scale_key(config)             # SCENE_SCALE as (p, q), or None: no scene takes a step of it
        self.clean = mask_clean_plan(config)             # MASK_CLEAN as a MaskCleanPlan, or None: no scene takes a step of it
        self.nodata = scene_nodata_key(config)           # SCENE_NODATA as a SceneNodata, or None: no scene takes a step of it
        self.aoi = scene_aoi_key(config)                 # SCENE_AOI as a SceneAoi, or None: no scene takes a step of it (unless it brings its own)
        self.aoi_tables = {}                             # (H, W) -> the host tables of the CONFIG's key, built once per scene size

    @functools.cached_property
    def features(self):
        """(keywords FUSE_WINDOW and TTA add to scene_pass1, keywords FUSE_WINDOW adds to scene_normalise, number of orientations) — no
        keyword at all for a feature that is off, so that those calls get exactly the arguments they always got.  Checked (FUSE_WINDOW,
        then TTA) and the window uploaded at the first scene, once its shape and mask have passed: bad input is refused in that order,
        before the device is touched."""
        window, codes = fuse_window(self.config), tta_plan(self.config)[1]
        wkw = {} if window is None else dict(window=torch.from_numpy(window).to(self.device))
        return {**wkw, **({} if len(codes) == 1 else dict(tta=list(codes)))}, wkw, len(codes)


@dataclasses.dataclass
class _SceneJob:
    """One scene from pass 1 to its result."""
    shape: tuple                      # (H, W) of the real scene: what the masks and the nodes the caller gets refer to
    infos: list                       # the tiles that run (the kept ones under a mask), in the frame of the real scene (SCENE_PAD: shifted;
                                      # SCENE_SCALE: of the model frame, in which pass 2 runs)
    all_xy: np.ndarray                # their origins int32 [n,2] (x0, y0) on the canvases (SCENE_PAD: the virtual scene)
    pads: tuple = (0, 0, 0, 0)        # SCENE_PAD's (top, bottom, left, right): the canvases are shape + pads
    empty: bool = False               # a mask kept no tile: nothing was launched and the fields below stay as they are
    lo: int = 0                       # this rank's chunk of the tiles; emb holds their embeddings
    hi: int = 0
    emb: torch.Tensor = None
    bands: list = None                # the column bands of the canvas reduce (world > 1)
    kp_u8: torch.Tensor = None        # the two masks on the device (rank 0)
    road_u8: torch.Tensor = None
    # what infer_imgs' pipeline adds as the scene moves through it
    io: _LaneIO = None
    masks: list = None                # the masks on their way to the host, and the event that says they have landed
    e1: object = None
    kp_mask: np.ndarray = None
    road_mask: np.ndarray = None
    graph_points: np.ndarray = None
    fq: _FlatQueries = None
    plan: object = ()                 # _queue_pass2's plan, its scores on their way to the host and their event
    scores: list = None
    e2: object = None
    votes: tuple = None
    # a scene group (SCENE_GROUP): this job is the stack — shape (Ha, Wa), infos / all_xy the kept tiles on the stack, emb all of them,
    # kp_u8 the u8 [2, sum H W] tensor of every scene's cropped masks — and `group` holds one child job per scene: its tiles in its
    # own real frame, [lo, hi) its rows of the stack's emb (empty: it kept no tile), mask_off the byte offset of its masks
    group: list = None
    mask_off: int = 0
    row0: int = 0                     # first query row of a child in the group's one ragged pass 2
    # SCENE_SCALE: the scene carries two frames.  kp_u8 / road_u8 above are the masks of the scene frame (`shape`), the
    # ones the caller gets; the model-frame masks travel too, for the unchanged point extraction, and the nodes are mapped at the end
    scale: tuple = None               # (p, q), or None: one frame, nothing below is used
    model_shape: tuple = None         # (H, W) of the model frame (None: `shape`)
    model_kp_u8: torch.Tensor = None  # the model-frame masks on the device (rank 0), then on their way to the host
    model_road_u8: torch.Tensor = None
    model_masks: list = None


def _upload_scene(net, io, img):
    """THE scene upload of every loop.  An array goes as it always went.  A TiffScene (GEOTIFF) goes as the decompressed
    segments of its file, predictor, byte order, planes and tiles as the file has them, and one launch assembles the raster [H, W, C] on
    the device (step "tiff"): the decoded, interleaved scene never exists on the host, and everything behind this sees the device raster
    it always saw.  A file that IS the raster (little-endian, uncompressed, predictor 1, chunky strips) is uploaded and used as it is."""
    if not isinstance(img, TiffScene):
        return io.upload("scene", img)
    flat, table = img.loaded(fill_threads())
    if img.is_raster:
        return io.upload("scene", flat.view(img.dtype).reshape(img.shape))
    flat_d, table_d = io.upload("scene", flat), io.upload("tiff_table", table)
    scene = net.tiff_assemble(img, flat_d, table, table_d)
    io.step("tiff")
    return scene


def _pass1_front(ctx, io, img, valid=None, group=None, aoi=None):
    """Pass 1 of one scene, queued (GPU): plan, upload, [band step,] [resample,] [border padding,] [tile selection, nodata fill,] crop ->
    encoder -> decoder -> fused canvases, [canvas reduce,] normalise[, masks cropped back][, small components dropped][, masks resampled
    back].  `io` decides how arrays travel and when the host waits
    (_BlockingIO / _LaneIO); everything else is the same for every loop.  Returns the _SceneJob: embeddings resident, the u8 masks on the
    device of rank 0 — fetching them is the caller's.  SCENE_PAD lives here and nowhere else: the real scene (and mask)
    is uploaded and padded on the device, everything up to the normalise runs on that virtual scene through the same calls, the u8 masks
    are cropped to the real scene before they travel, and the job carries the tiles in the real scene's frame for pass 2.
    SCENE_BANDS: the raw u8 / u16 [H,W,C] scene is uploaded and converted to the u8 [H,W,3] scene right behind the upload
    (_scene_bands_front), before the pad and the fill; nothing after that step knows of it.
    SCENE_SCALE lives here and nowhere else: right behind the band step the scene is resampled to the model frame by p/q
    (the mask by the validity rule), everything up to the crop runs in that frame through the same calls, and at the end both masks are
    resampled back to the scene's own size by q/p, 0 wherever the scene's mask is.  The job carries both pairs of masks (the model-frame
    ones feed the unchanged point extraction and pass 2) and the tiles in the model frame; the nodes are mapped where the result is formed.
    MASK_CLEAN lives here and nowhere else: on rank 0, behind the normalise and the crop to the real scene and in front of
    the way back and the download, the connected components of each thresholded mask that are too small or too faint are set to 0 in
    place (net.mask_clean: five queued launches, nothing read back); its table travels with the scene's other uploads.
    SCENE_NODATA lives here and nowhere else: right behind the upload and in front of SCENE_BANDS the validity mask that the
    device derives from the raw pixels (_scene_nodata_mask: one launch for value / tolerance / match, plus srh_mask_clean and the grow for
    min_area / grow), ANDed with the caller's mask if there is one, takes the place of the uploaded mask; behind that point the scene "has
    a mask" (masked) and nothing knows of the key.  The counts follow those kernels (after_compute); no mask is staged or uploaded unless the
    caller gave one.
    SCENE_AOI lives here and nowhere else: right behind the upload, in front of SCENE_NODATA and SCENE_BANDS, the mask the
    device rasterises from the polygons (_scene_aoi_mask: one launch, plus the grow for a buffer; `aoi`, a scene's own SCENE_AOI value, takes
    the place of the config's key), ANDed with the caller's mask, takes the place of the uploaded one; SCENE_NODATA then ANDs its own into it.
    The edge table travels with the scene's other uploads; no mask is staged or uploaded unless the caller gave one.
    SCENE_FLOAT lives here and nowhere else: where SCENE_BANDS sits, behind SCENE_AOI and in front of SCENE_SCALE, the raw
    f32 [H,W,C] scene becomes the u8 [H,W,3] scene AND its validity mask (_scene_float_front); a float scene is always a masked scene, and
    nothing after that step knows of the key.
    group (SCENE_GROUP; img and valid are None then): a planned group, a list of _GroupScene, takes the place of the one
    scene — one ragged upload and one pack launch build the vertical stack of the scenes (each padded by its own pads) and of their masks,
    then the stack IS the scene of the code below, and one crop launch cuts every scene's window out of the stack's masks; the job
    is the stack's, its `group` the scenes' (see _SceneJob).  Without a group none of its branches is taken."""
    net, config = ctx.net, ctx.config
    if group is not None:
        with_mask = [sc for sc in group if sc.valid is not None]
        masked = bool(with_mask) or ctx.nodata is not None
        if with_mask:
            min_frac, fill = _valid_plan(with_mask[0].valid, with_mask[0].shape, config)[1:]
        elif masked:
            min_frac, fill = _mask_keys(config)
        pass1_kw, norm_kw, n_orient = ctx.features
        scene, valid_d, all_xy, first, crop_table, crop_table_d = _group_stack(ctx, io, group)
        infos = list(range(all_xy.shape[0]))           # on the stack a tile is known by its index alone
        xy_dev = io.upload("xy", all_xy)
        shape, pads, job_pads = tuple(int(v) for v in scene.shape[:2]), None, (0, 0, 0, 0)
        scene_shape, aoi = shape, None                 # SCENE_AOI does not combine with a group (refused by infer_imgs)
        if ctx.clean is not None:                      # MASK_CLEAN: one image per mask and scene, at its place in scene_group_crop's output
            n_px = sum(sc.shape[0] * sc.shape[1] for sc in group)
            clean_table = _mask_clean_images(ctx.clean, [(int(off), *sc.shape) for sc, off in zip(group, crop_table[:, 0])], n_px)
    else:
        img, infos, all_xy = _scene_plan(img, config)
        aoi = aoi_key_of(aoi) if aoi is not None else ctx.aoi
        scene_shape = tuple(int(v) for v in img.shape[:2])
        shape = model_shape(scene_shape, ctx.scale)        # the frame of everything between the two resample steps (no key: the scene's)
        pad = scene_pad_plan(shape, config)
        pads = pad[:4] if pad is not None and any(pad[:4]) else None     # all four 0: the launches of a run without the key
        masked, valid_d = valid is not None or ctx.nodata is not None or aoi is not None or ctx.float is not None, None
        if valid is not None:
            valid, min_frac, fill = _valid_plan(valid, scene_shape, config)
        elif masked:
            min_frac, fill = _mask_keys(config)
        pass1_kw, norm_kw, n_orient = ctx.features
        scene = _upload_scene(net, io, img)                # the u8 scene, ONCE; tiles are cropped on the device
        xy_dev = io.upload("xy", all_xy)
        if ctx.clean is not None:                          # MASK_CLEAN: the two masks of the real scene (model frame), one above the other
            clean_table = _mask_clean_images(ctx.clean, [(0, *shape)], shape[0] * shape[1])
        if valid is not None:
            valid_d = io.upload("valid_mask", valid)       # a key of its own: "valid" stages pass 2's pair flags
        if ctx.nodata is not None and (ctx.nodata.min_area > 1 or ctx.nodata.grow > 0):
            nd_table = nodata_table([(0, *scene_shape)], ctx.nodata)
            nd_table_d = io.upload("nodata_table", nd_table)
        if aoi is not None:
            aoi_tab = ctx.aoi_tables.get(scene_shape) if aoi is ctx.aoi else None
            if aoi_tab is None:
                aoi_tab = aoi_edges(aoi, *scene_shape)
                if aoi is ctx.aoi:
                    ctx.aoi_tables[scene_shape] = aoi_tab
            aoi_tab_d = io.upload("aoi_table", aoi_pack(*aoi_tab[:2]))
            aoi_grow = mask_clean_table([(0, *scene_shape, MaskRule(1, 1, 0))]) if aoi.buffer else None
            aoi_grow_d = io.upload("aoi_grow_table", aoi_grow) if aoi.buffer else None
        io.step("upload")
        if aoi is not None:
            # SCENE_AOI lives here and nowhere else: the mask rasterised from the polygons, ANDed with the caller's, takes
            # the place of the uploaded one; SCENE_NODATA below ANDs its own into it
            valid_d = _scene_aoi_mask(net, aoi, scene_shape, valid_d, aoi_tab, aoi_tab_d, aoi_grow, aoi_grow_d).view(scene_shape)
            io.step("aoi")
        if ctx.nodata is not None:
            # SCENE_NODATA lives here and nowhere else: right behind the upload and in front of SCENE_BANDS the mask the
            # device derives from the raw pixels (ANDed with the caller's, if any) takes the place of the uploaded one.  From here on
            # "this scene has a mask" (masked) is all anything knows
            lo, hi = scene_nodata_check(img, ctx.nodata)
            key2 = ctx.nodata.min_area > 1 or ctx.nodata.grow > 0
            valid_d = _scene_nodata_mask(net, ctx.nodata, scene, lo, hi, valid_d, nd_table if key2 else None, nd_table_d if key2 else None).view(scene_shape)
            io.step("nodata")
        if ctx.bands is not None:                          # the raw scene -> the u8 [H,W,3] scene of every line below; the raw one is dropped
            scene = _scene_bands_front(ctx, io, scene, valid_d, after_compute=ctx.nodata is not None or aoi is not None)
        if ctx.float is not None:                          # the raw f32 scene -> the u8 [H,W,3] scene and ITS mask; the raw one is dropped
            scene, valid_d = _scene_float_front(ctx, io, scene, valid_d)
        if ctx.scale is not None:                          # the scene -> the model frame; the mask by the validity rule, and the scene-frame
            scene = net.scene_resample(scene, *ctx.scale)  # one is kept for the way back
            if masked:
                valid_scene, valid_d = valid_d, net.scene_resample(valid_d, *ctx.scale, valid_rule=True)
            io.step("scale")
        if pads is not None:
            scene = net.scene_pad(scene, pads, pad[4], pad[5])
            if masked:                                     # the mask by the same rule: reflect / edge mirror its validity, constant padding is nodata
                valid_d = net.scene_pad(valid_d, pads, pad[4], (0, 0, 0))
            io.step("pad")
        job_pads = pads or (0, 0, 0, 0)
    if ctx.clean is not None and clean_table is not None and ctx.rank == 0:
        clean_table_d = io.upload("clean_table", clean_table)     # travels with the scene: the filter below adds no host wait
    if masked:
        # every rank holds the scene and the mask, computes the same integer counts and therefore the same kept list: from here
        # on infos / all_xy / xy_dev ARE the kept tiles (a subsequence of an x-outer list is x-outer, so the banded reduce stays valid)
        kept = select_tiles(io.counts(lambda: net.scene_tile_valid(valid_d, xy_dev), after_compute=pads is not None or group is not None or ctx.scale is not None or ctx.nodata is not None or aoi is not None or ctx.float is not None),
                            config.PATCH_SIZE, min_frac)
        io.step("select")
        infos, all_xy = [infos[i] for i in kept], np.ascontiguousarray(all_xy[kept])
        if len(kept) == 0:                             # nothing to run: the encoder is not launched and no exchange step is entered
            job = _SceneJob(scene_shape, _shift_infos(infos, job_pads), all_xy, job_pads, empty=True)
            if group is not None:
                job.group = _group_children(group, first, infos)
            return job
        xy_dev = io.upload("xy_kept", all_xy)
        if scene.device.type != "cuda":                # a CPU tensor (the stand-in models of the gloo tests) may share the caller's memory
            scene = scene.clone()
        scene = net.scene_fill_invalid(scene, valid_d, fill)
        io.step("fill")
        norm_kw = dict(valid=valid_d, **norm_kw)
    job = _SceneJob(scene_shape, _shift_infos(infos, job_pads), all_xy, job_pads)
    if group is None and ctx.scale is not None:
        job.scale, job.model_shape = ctx.scale, shape
    job.lo, job.hi = shard_tiles(len(infos), ctx.world, ctx.rank)
    io.step("launch pass 1")
    # FUSE_WINDOW: every rank weights its own chunk of the kept list.  TTA: every orientation runs that chunk (selection and fill happened
    # once, above).  An empty shard (world > n_tiles) returns zero canvases
    kp_c, road_c, job.emb = net.scene_pass1(scene, xy_dev[job.lo:job.hi], ctx.bs, **pass1_kw)
    io.step("pass 1")
    if ctx.sharded:
        job.bands = D.tile_bands(all_xy, int(config.PATCH_SIZE), ctx.world) if ctx.world > 1 else None
        D.reduce_canvases(kp_c, road_c, dst=0, bands=job.bands)
    if ctx.rank == 0:
        # the full kept list, repeated once per orientation (the coverage count becomes k * count, the weight sum runs over k * n terms
        # in list order: DESIGN.md §6f) — count and weight sum follow from the list alone, so there is no collective for them
        xy_norm = xy_dev if n_orient == 1 else xy_dev.repeat(n_orient, 1)
        job.kp_u8, job.road_u8 = net.scene_normalise(kp_c, road_c, xy_norm, **norm_kw)
        if pads is not None:                           # the real scene's window of the virtual masks, cut out on the device: H * W bytes travel
            (top, _, left, _), (H, W) = pads, shape
            job.kp_u8, job.road_u8 = (m[top:top + H, left:left + W].contiguous() for m in (job.kp_u8, job.road_u8))
        if group is None and ctx.clean is not None and clean_table is not None:
            # MASK_CLEAN lives here and nowhere else: the components of the masks of the REAL scene — cropped, before they
            # are resampled back or travel — in place in one [2,H,W] tensor, so that one call serves both masks; queued, nothing read back
            both = torch.stack((job.kp_u8, job.road_u8))
            net.mask_clean(both.view(-1), clean_table, table_dev=clean_table_d, connectivity=ctx.clean.connectivity)
            job.kp_u8, job.road_u8 = both[0], both[1]
        if job.scale is not None:                      # the way back: both masks to the scene's own size by q/p, 0 on the scene's nodata
            (p, q), job.model_kp_u8, job.model_road_u8 = job.scale, job.kp_u8, job.road_u8
            job.kp_u8, job.road_u8 = (net.scene_resample(m, q, p, out_shape=scene_shape, zero_where=valid_scene if masked else None)
                                      for m in (job.model_kp_u8, job.model_road_u8))
        if group is not None:                          # every scene's window of the stack's masks, one launch, one allocation
            job.group = _group_children(group, first, infos)
            job.kp_u8, job.road_u8 = net.scene_group_crop(job.kp_u8, job.road_u8, crop_table, table_dev=crop_table_d), None
            if ctx.clean is not None and clean_table is not None:      # every mask of every scene is an image of its own: one call
                net.mask_clean(job.kp_u8.view(-1), clean_table, table_dev=clean_table_d, connectivity=ctx.clean.connectivity)
    io.step("normalised")
    return job


def _scene_bands_front(ctx, io, raw, valid_d=None, after_compute=False):
    """SCENE_BANDS lives here and nowhere else: the raw scene on the device (u8 / u16 [..., C]; a group's ragged buffer
    [n, C]) -> the u8 [..., 3] scene.  A percentile stretch counts the exact histogram of the selected bands over the valid pixels (before
    any padding or nodata fill), fetches it the way the tile selection fetches its counts, and reads the ranges off it on the host; the
    tables are built on the host in float64 (radiometry.py) — once per call for a fixed range — and the device only gathers from them.
    Every rank of a tile-sharded run holds the scene and the mask, counts the same integers and builds the same tables: no collective."""
    net, bands = ctx.net, ctx.bands
    levels = 256 if raw.dtype == torch.uint8 else 65536
    lut_d = ctx.bands_luts.get(levels)
    if bands.percentile is not None:
        # after_compute: valid_d is what the compute stream derived (SCENE_NODATA), so the upload lane waits for it first
        hist = io.counts(lambda: net.scene_bands_hist(raw, bands.select, valid_d), name="bands_hist", **(dict(after_compute=True) if after_compute else {}))
        lut_d = io.upload("bands_lut", band_luts(stretch_from_hist(hist, *bands.percentile), bands.gamma, levels))
    elif lut_d is None:
        lut_d = ctx.bands_luts[levels] = io.upload("bands_lut", band_luts(fixed_ranges(bands, levels), bands.gamma, levels))
    scene = net.scene_bands_apply(raw, bands.select, lut_d)
    io.step("bands")
    return scene


def _scene_float_front(ctx, io, raw, valid_d=None):
    """SCENE_FLOAT lives here and nowhere else: the raw scene on the device (f32 [H,W,C]) and the mask so far (the caller's,
    ANDed with SCENE_AOI's, or None) -> (the u8 [H,W,3] scene, the validity mask u8 [H,W] by rule 1 of float_scene.py).  Behind this point
    the scene is an ordinary masked scene.  A percentile stretch counts the ordered keys of the selected bands over the valid pixels in two
    exact 65536-bin passes, each fetched the way the tile selection fetches its counts, with the rank arithmetic on the host between and
    after them (float_scene.py); the thresholds are built on the host in float64 — once per call for a fixed range — and the device only
    compares integers against them.  Every rank of a tile-sharded run holds the scene and the mask, counts the same integers and builds
    the same thresholds: no collective."""
    net, key = ctx.net, ctx.float
    valid_d = net.scene_float_valid(raw, key.select, [int(k) for k in float_nodata_keys(key)], key.log, valid_d)
    thr_d = ctx.float_thr
    if key.percentile is not None:
        # after_compute: valid_d is what the compute stream just derived, so the upload lane waits for it first
        hist1 = io.counts(lambda: net.scene_float_hist(raw, key.select, valid_d), name="float_hist", after_compute=True)
        targets, picks = float_hist_targets(hist1, key)
        hist2 = io.counts(lambda: net.scene_float_hist(raw, key.select, valid_d, targets), name="float_hist_low", after_compute=True) if targets else None
        thr_d = io.upload("float_thr", threshold_keys(float_thresholds(float_ranges_from_hists(targets, picks, hist2, key), key)))
    elif thr_d is None:
        thr_d = ctx.float_thr = io.upload("float_thr", threshold_keys(float_thresholds(key.ranges, key)))
    scene = net.scene_float_apply(raw, key.select, valid_d, thr_d)
    io.step("float")
    return scene, valid_d


def _scene_nodata_mask(net, key, raw, lo, hi, and_with, table, table_d):
    """SCENE_NODATA's device steps: the raw pixels on the device (u8 / u16 [..., C]; a group's ragged buffer [n, C]) -> the
    flat u8 validity mask, one byte per pixel, that nodata.nodata_ref states: not nodata, ANDed with and_with (the caller's mask, laid out
    like the result, or None).  With value / tolerance / match alone it is ONE launch.  Otherwise the match writes `hit`, srh_mask_clean —
    as it is — clears its small components in place (min_area > 1), and the grow (or, without one, a second match on `hit` itself)
    writes the finished mask; table / table_d describe the scenes' H x W blocks (nodata.nodata_table).  All queued, nothing read back."""
    match = "any" if key.any else "all"
    if and_with is not None:
        and_with = and_with.view(-1)
    if key.min_area <= 1 and key.grow == 0:
        return net.scene_nodata_match(raw, lo, hi, match, and_with=and_with, invert=True).view(-1)
    hit = net.scene_nodata_match(raw, lo, hi, match).view(-1)
    if key.min_area > 1:
        net.mask_clean(hit, table, table_dev=table_d, connectivity=key.connectivity)
    if key.grow > 0:
        return net.scene_nodata_grow(hit, table, key.grow, and_with=and_with, invert=True, table_dev=table_d)
    return net.scene_nodata_match(hit.view(-1, 1), [0], [0], and_with=and_with).view(-1)          # not hit: the level of `hit` is 0


def _scene_aoi_mask(net, key, shape, and_with, tables, table_d, grow_table, grow_table_d):
    """SCENE_AOI's device steps: the u8 [H, W] validity mask that aoi.aoi_ref states, ANDed with and_with (the caller's mask
    [H, W], or None).  Without a buffer it is ONE launch.  With one the fill writes the area (inverted for a negative buffer), and
    srh_scene_nodata_grow — as it is — grows it by |buffer|, its invert flag turning the grown complement back, and takes and_with.
    tables: aoi.aoi_edges' tuple; table_d: aoi.aoi_pack of it on the device; grow_table / grow_table_d: the one H x W block of the grow.
    All queued, nothing read back."""
    edges, polys, n_include, n_exclude = tables
    if key.buffer == 0:
        return net.scene_aoi_fill(shape, edges, polys, n_include, n_exclude, and_with=and_with, table_dev=table_d)
    shrink = key.buffer < 0
    area = net.scene_aoi_fill(shape, edges, polys, n_include, n_exclude, invert=shrink, table_dev=table_d)
    return net.scene_nodata_grow(area.view(-1), grow_table, abs(key.buffer), and_with=None if and_with is None else and_with.view(-1), invert=shrink,
                                 table_dev=grow_table_d)


def _group_children(group, first, kept):
    """One child job per scene of a group: `kept`, ascending indices into the group's candidate tile list (scene k's candidates are
    first[k] .. first[k + 1]), mapped back to the scenes.  A child's tiles are its own, in its own real frame; [lo, hi) are its rows of
    the stack's embeddings; a scene that kept no tile is empty."""
    kept = np.asarray(kept, dtype=np.int64)
    cut = np.searchsorted(kept, first)
    children, off = [], 0
    for k, sc in enumerate(group):
        mine = kept[cut[k]:cut[k + 1]] - first[k]
        child = _SceneJob(sc.shape, _shift_infos([sc.infos[i] for i in mine], sc.pads), np.ascontiguousarray(sc.all_xy[mine]), sc.pads,
                          empty=len(mine) == 0, lo=int(cut[k]), hi=int(cut[k + 1]), mask_off=off)
        children.append(child)
        off += sc.shape[0] * sc.shape[1]
    return children


def _pass2_sharded(ctx, job, kp_mask, road_mask, stats=None, lap=None, scene_masks=None):
    """From a scene's masks on the host (rank 0; None elsewhere) to its result tuple on rank 0, None on the other ranks: graph points
    (host, rank 0) -> broadcast -> per-tile queries (host) -> sampler + TopoNet (GPU) -> directed edge votes of this rank's tiles ->
    gather -> edges.  The two exchange steps run in the same order on every rank.  `stats` collects wall times and exchanged bytes.
    scene_masks (SCENE_SCALE, rank 0): kp_mask / road_mask are the model-frame masks, everything above runs in that frame, and the result
    carries these scene-frame masks and the nodes mapped to the scene frame (_scene_frame)."""
    import collections
    net, config, device, world, rank = ctx.net, ctx.config, ctx.device, ctx.world, ctx.rank
    stats = stats if stats is not None else collections.defaultdict(float)
    lap = lap or _Laps()
    if job.empty:
        return _empty_result(*job.shape) if rank == 0 else None
    t0 = time.perf_counter()
    graph_points = None
    if rank == 0:
        graph_points = extract_graph_points(kp_mask, road_mask, config)
        lap("extract_graph_points")
    t1 = time.perf_counter()
    stats["points_host_ms"] += 1e3 * (t1 - t0)
    graph_points = D.broadcast_points(graph_points, src=0, device=device if world > 1 else None)
    stats["points_bytes"] += 16 * graph_points.shape[0] * ((world - 1) if rank == 0 else 1)     # rank 0: sent to every peer; others: received
    if graph_points.shape[0] == 0:
        return None if rank != 0 else _scene_frame(job, (graph_points, np.zeros((0, 2), dtype=np.int32), kp_mask, road_mask), scene_masks)
    n_pts = graph_points.shape[0]
    if world > 1 and config.EXACT_VOTE_MERGE:
        # exact multi-rank merge (extension key, default off): every raw vote goes to rank 0 in the one-process visiting order
        k_raw, s_raw = edge_votes(net, job.emb, graph_points, job.infos, job.lo, job.hi, config, device, raw=True)
        t2 = time.perf_counter()
        stats["votes_bytes"] += 16 * k_raw.shape[0]
        k_raw, s_raw = D.gather_raw_votes(k_raw, s_raw, dst=0, device=device)
        if rank != 0:
            stats["pass2_ms"] += 1e3 * (t2 - t1)
            return None
        uk, sums, cnts, first = _accumulate_votes(k_raw, s_raw)
    else:
        uk, sums, cnts, first = edge_votes(net, job.emb, graph_points, job.infos, job.lo, job.hi, config, device)
        lap("edge_votes")
        t2 = time.perf_counter()
        stats["votes_bytes"] += 32 * uk.shape[0]
        uk, sums, cnts, first = D.gather_edge_votes(uk, sums, cnts, n_pts, dst=0, device=device if world > 1 else None, first=first)
    stats["pass2_ms"] += 1e3 * (t2 - t1)
    job.emb = None
    if rank != 0:
        return None
    t3 = time.perf_counter()
    pred_edges = votes_to_edges(uk, sums, cnts, first, n_pts, config.TOPO_THRESHOLD)
    stats["merge_host_ms"] += 1e3 * (time.perf_counter() - t3)
    lap("threshold + edge list")
    return _scene_frame(job, (graph_points[:, ::-1], pred_edges, kp_mask, road_mask), scene_masks)      # nodes as (row, col)


def _scene_frame(job, result, scene_masks):
    """A result tuple formed in the model frame as the caller gets it under SCENE_SCALE: the nodes (row, col) mapped by the node rule
    (resample.map_nodes), the scene-frame masks in place of the model-frame ones; the edges are indices and stay.  No key: untouched."""
    if job.scale is None:
        return result
    nodes, edges, _, _ = result
    return map_nodes(nodes, job.shape, *job.scale), edges, scene_masks[0], scene_masks[1]


def _infer_one_img(net, img, config, device=None, valid=None, aoi=None):
    ctx = _SceneSetup(net, config, device, sharded=True)
    lap = _Laps("infer_one_img", sync=ctx.device)      # tuning aid: wall time of each stage (synchronises the device)
    job = _pass1_front(ctx, _BlockingIO(ctx.device, lap), img, valid, aoi=aoi)
    kp_mask = road_mask = scene_masks = None
    if job.kp_u8 is not None:                          # rank 0 of a scene that ran
        kp_mask, road_mask = job.kp_u8.cpu().numpy(), job.road_u8.cpu().numpy()
        if job.scale is not None:                      # those are the caller's; the points come from the model-frame masks
            scene_masks, (kp_mask, road_mask) = (kp_mask, road_mask), (job.model_kp_u8.cpu().numpy(), job.model_road_u8.cpu().numpy())
        _poll_finite(net, ctx.device)                  # the masks are on the host, so every LayerNorm pass of pass 1 has reported
        lap("normalise + mask D2H")
    return _pass2_sharded(ctx, job, kp_mask, road_mask, lap=lap, scene_masks=scene_masks)


def _valid_iter(valids):
    """The masks parallel to a scene sequence, one next() per scene: `valids` (any iterable, entries may be None), or None for ever."""
    import itertools
    return itertools.repeat(None) if valids is None else itertools.chain(iter(valids), itertools.repeat(None))


def infer_imgs(net, imgs, config, device=None, tile_sharded=None, pipelined=None, valids=None, group=None, aois=None):
    """infer_one_img over a sequence of scenes, as a generator of the same tuples in the same order — software-pipelined on
    one GPU: while the device runs pass 1 of scene i+1, the host does scene i's mask -> points -> pass-2 queries; scene i's
    TopoNet batches are queued behind that pass 1 and its edge vote runs while scene i+2 is on the device.  One compute stream
    (the library context is single-stream), one copy stream, events instead of device-wide synchronisation; every scene's
    canvases / embeddings are its own tensors, so nothing of the context is double-buffered.  The results are those of
    infer_one_img bit for bit (same kernels in the same order per scene).  The reference's loop (inferencer.py:289-349) is
    strictly serial; this is what the CLI uses.  tile_sharded (default: torch.distributed is initialised) selects the other
    multi-GPU mode instead — every scene's tiles split over the ranks; with tile_sharded=False each rank runs its own scenes through
    the pipeline and no collective is issued.  The tile-sharded mode has two loops: the SERIAL one (default) — infer_one_img scene by
    scene, its three exchange steps strictly in sequence — and the PIPELINED one (_infer_imgs_tile_sharded; `pipelined=True`, config
    key TILE_SHARD_PIPELINE, CLI `--shard tiles-pipelined`), which interleaves the band reduce of scene i+1 with the point broadcast
    and vote gather of scene i.  The pipelined loop has only ever run on gloo / CPU (no multi-GPU box was available to the builder:
    DESIGN.md §6), so it stays opt-in until an RCCL run exists; both give the same results (tests/test_distributed_cpu.py).
    valids: validity masks parallel to imgs (a list or any iterable, read in step with imgs; entries may be None), see infer_one_img.
    A masked scene's tile selection — mask upload, count kernel, n int32 back, one host wait — is issued on the upload lane; like every
    upload there it starts after the work the compute stream holds at that moment (the previous scene's pass 2).
    group (None: config.SCENE_GROUP): an int n >= 2 runs up to n consecutive scenes as ONE unit of this pipeline — one
    upload, one pass 1 over all their tiles in full batches, one normalise, one mask download, one ragged TopoNet launch sequence; the
    host stages run one scene per worker thread.  The tuples and their order do not change; a group's results are yielded once the group
    is finished, the last, shorter group when the input ends, and a group of one scene takes the single-scene path.  The tile batches
    are composed differently from a scene's own, so on the GPU the masks agree with infer_one_img's within a level (tests/tolerances.py,
    BATCH_INDEP_SCORE), not bit for bit.  Only this one-process loop groups: with a tile-sharded mode the key is a ValueError.
    aois: areas of interest parallel to imgs, as valids is: an entry is a SCENE_AOI value that takes the place of the config's
    key for that scene, None the config's key.  SCENE_AOI does not combine with a group: one pixel-frame area for a stream of chips has no
    meaning."""
    neighbor_queries(config)                          # fail before any scene touches the device
    fuse_window(config)
    tta_plan(config)
    scene_pad_key(config)
    bands = scene_bands_key(config)
    flt = scene_float_plan(config)
    clean = mask_clean_plan(config)
    n_group = scene_group_key(config, group)
    if flt is not None and n_group > 1:
        raise ValueError(f"SCENE_FLOAT does not combine with SCENE_GROUP = {n_group} (float scenes run one by one): drop one of them")
    if clean is not None and 2 * n_group > MASK_CLEAN_MAX_IMAGES:
        raise ValueError(f"MASK_CLEAN filters the two masks of every scene of a group in one call of at most {MASK_CLEAN_MAX_IMAGES} images: "
                         f"SCENE_GROUP = {n_group} is too large, use at most {MASK_CLEAN_MAX_IMAGES // 2}")
    nodata = scene_nodata_key(config)
    if nodata is not None and nodata.min_area > 1 and n_group > MASK_CLEAN_MAX_IMAGES:
        raise ValueError(f"SCENE_NODATA: min_area filters the derived mask of every scene of a group in one call of at most {MASK_CLEAN_MAX_IMAGES} "
                         f"images: SCENE_GROUP = {n_group} is too large")
    if scene_scale_key(config) is not None and n_group > 1:
        raise ValueError(f"SCENE_SCALE does not combine with SCENE_GROUP = {n_group} (a group's stack holds scenes of one frame): drop one of them")
    if n_group > 1 and (scene_aoi_key(config) is not None or aois is not None):
        raise ValueError(f"SCENE_AOI does not combine with SCENE_GROUP = {n_group} (the polygons are in the pixel frame of ONE scene): drop one of them")
    valids, aois = _valid_iter(valids), _valid_iter(aois)
    if D.is_distributed() if tile_sharded is None else tile_sharded:
        if n_group > 1:
            raise ValueError(f"SCENE_GROUP = {n_group} applies to the one-process scene loop (tile_sharded=False, CLI --shard scenes); a "
                             f"tile-sharded mode runs its scenes one by one: drop the key or the mode")
        if pipelined is None:
            pipelined = _cfg_switch(config.TILE_SHARD_PIPELINE, False)
        if pipelined:
            yield from _infer_imgs_tile_sharded(net, imgs, config, device, valids=valids, aois=aois)
        else:
            for img in imgs:
                yield infer_one_img(net, img, config, device=device, valid=next(valids), aoi=next(aois))
        return
    if n_group > 1 and bands is not None and bands.percentile is not None:
        raise ValueError("SCENE_BANDS: a percentile stretch needs every scene's own tables and a host round trip in the middle of a group; "
                         "with SCENE_GROUP use a fixed stretch range (or run the scenes one by one)")
    ctx = _SceneSetup(net, config, device, sharded=False)
    device, K = ctx.device, ctx.K
    lane = _Lane(device)
    pools = [_StagingPool(device), _StagingPool(device)]
    lap = _Laps("infer_imgs")                          # tuning aid: host wall time of each step (no device synchronisation)

    def launch_pass1(img, pool, valid=None, group=None, aoi=None):           # G1: upload, pass 1, normalise, masks on their way to the host
        io = _LaneIO(lane, pool, lap)
        job = _pass1_front(ctx, io, img, valid, group, aoi=aoi)
        job.io = io
        if job.empty:                                  # zero masks, no nodes (a group: every child is empty)
            job.masks = [torch.zeros(job.shape, dtype=torch.uint8) for _ in range(2)] if group is None else None
            return job
        job.masks, job.e1 = lane.download(pool, "mask", [job.kp_u8, job.road_u8] if group is None else [job.kp_u8])
        if job.scale is not None:                      # the second staged download: the model-frame masks; its event covers both
            job.model_masks, job.e1 = lane.download(pool, "model_mask", [job.model_kp_u8, job.model_road_u8])
        lap("queue normalise + mask download")
        return job

    def points_and_pass2(job):                         # H1 + G2: points, queries, TopoNet launches, scores on their way back
        if job.e1 is not None:
            job.e1.synchronize()
        job.kp_mask, job.road_mask = (m.numpy().copy() for m in job.masks)
        # SCENE_SCALE: the points come from the model-frame masks (read where they were staged: the pool is this scene's until it is done)
        job.graph_points = extract_graph_points(*((job.kp_mask, job.road_mask) if job.model_masks is None else (m.numpy() for m in job.model_masks)), config)
        lap("extract_graph_points")
        if job.graph_points.shape[0] == 0:
            return
        job.fq = build_all_patch_queries(job.graph_points, job.infos, 0, len(job.infos), config, flat=True)
        lap("build_all_patch_queries")
        if job.fq is None:                             # non-integer radius: the serial per-tile path
            job.votes = edge_votes(net, job.emb, job.graph_points, job.infos, 0, len(job.infos), config, device)
            return
        ragged = _ragged_pass2(net, config)
        job.plan, scores = _queue_pass2(net, job.emb, job.fq, ctx.bs, K, ragged, job.io)
        if not job.plan:
            return
        job.scores, job.e2 = lane.download(job.io.pool, "score", scores)
        job.io.step("pass 2 on its way back")
        job.emb = None
        lap("pack + queue pass 2 (ragged)" if ragged else "pack + queue pass 2")

    def finish(job):                                   # H2: votes -> edges
        nodes = job.graph_points[:, ::-1]              # (row, col)
        if job.scale is not None:
            nodes = map_nodes(nodes, job.shape, *job.scale)
        no_edges = np.zeros((0, 2), dtype=np.int32)
        if job.graph_points.shape[0] == 0:
            return job.graph_points, no_edges, job.kp_mask, job.road_mask
        n_pts = job.graph_points.shape[0]
        if job.votes is None:
            if not job.plan:
                return nodes, no_edges.astype(np.int64), job.kp_mask, job.road_mask
            if job.e2 is not None:
                job.e2.synchronize()
            lap("wait for pass-2 scores")
            if job.io.t is not None:
                t = job.io.t
                if lap.on:
                    print(f"[infer_imgs] device: pass 1 {t[0].elapsed_time(t[1]):.1f} ms, mask download -> pass 2 start {t[1].elapsed_time(t[2]):.1f} ms, "
                          f"pass 2 {t[2].elapsed_time(t[3]):.1f} ms, score download {t[3].elapsed_time(t[4]):.1f} ms", flush=True)
                if lane.times is not None:
                    lane.times.append((1, t[0].elapsed_time(t[1]), t[2].elapsed_time(t[3])))
            job.votes = _collect_pass2(job.fq, job.plan, [sc.numpy() for sc in job.scores], n_pts, K)
        edges = votes_to_edges(*job.votes, n_pts, config.TOPO_THRESHOLD)
        lap("votes -> edges")
        return nodes, edges, job.kp_mask, job.road_mask

    if n_group > 1:
        yield from _infer_imgs_grouped(ctx, lane, pools, lap, imgs, valids, n_group, launch_pass1, points_and_pass2, finish)
        return
    it = iter(imgs)
    img = next(it, None)
    if img is None:
        return
    with _host_quiet():
        cur = launch_pass1(img, pools[0], next(valids), aoi=next(aois))
    prev, i = None, 0
    while cur is not None:
        with _host_quiet():
            lap("(consumer)")
            if cur.e1 is not None:
                cur.e1.synchronize()                   # scene i's masks are on the host: the device is free for scene i+1
                _poll_finite(net, device)
            lap("wait for pass-1 masks")
            img = next(it, None)
            nxt = launch_pass1(img, pools[(i + 1) % 2], next(valids), aoi=next(aois)) if img is not None else None
            res = finish(prev) if prev is not None else None
        if prev is not None:
            yield res
        with _host_quiet():
            points_and_pass2(cur)
        prev, cur, i = cur, nxt, i + 1
    with _host_quiet():
        res = finish(prev)
    yield res


class _ChildIO:
    """A group's _LaneIO / _BlockingIO for ONE of its scenes in the padded pass 2 (PASS2_RAGGED off): the scenes' collates must not share
    staging buffers, since an upload is still on its way when the next scene is collated."""

    def __init__(self, io, k):
        self.io, self.k = io, k
        self.alloc = None if io.alloc is None else (lambda name, shape, dtype: io.alloc(f"{name}#{k}", shape, dtype))

    def upload_packed(self, name, arr):
        return self.io.upload_packed(f"{name}#{self.k}", arr)

    def step(self, name):
        pass


def _group_pool_threads(n):
    """Threads of the pool that runs a group's host stages, one scene per thread with ONE thread inside each call."""
    return max(1, min(int(n), worker_threads()))


def _concat_queries(job, live):
    """The flat queries of a group's scenes as ONE _FlatQueries over the tiles of the group's embedding tensor: a scene's tile t is tile lo
    + t there, its rows keep their order, and child.row0 is set to its first row.  (ids stay per scene: the votes read them there.)"""
    counts = np.zeros(int(job.emb.shape[0]), dtype=np.int64)
    for c in live:
        counts[c.lo:c.hi] = np.diff(c.fq.offsets)
    offsets = np.zeros(counts.shape[0] + 1, dtype=np.int64)
    np.cumsum(counts, out=offsets[1:])
    for c in live:
        c.row0 = int(offsets[c.lo])
    cat = lambda name: np.ascontiguousarray(np.concatenate([getattr(c.fq, name) for c in live], axis=0))
    return _FlatQueries(offsets, cat("ids"), cat("local"), cat("knn"))


def _infer_imgs_grouped(ctx, lane, pools, lap, imgs, valids, n_group, launch_pass1, points_and_pass2, finish):
    """infer_imgs' pipeline with a GROUP of scenes as its unit (SCENE_GROUP): while the device runs pass 1 of group i+1,
    the host does group i's points and queries, scene-parallel; group i's ONE ragged TopoNet launch sequence is queued behind that pass 1
    and its votes are read while group i+2 is on the device.  A group of one scene is a unit of the single-scene functions, untouched."""
    from concurrent.futures import ThreadPoolExecutor
    net, config, device, K = ctx.net, ctx.config, ctx.device, ctx.K
    no_edges = np.zeros((0, 2), dtype=np.int32)
    host_pool = ThreadPoolExecutor(_group_pool_threads(n_group), thread_name_prefix="srh-group")

    def launch(unit, pool):
        return launch_pass1(unit[0].img, pool, unit[0].valid) if len(unit) == 1 else launch_pass1(None, pool, None, unit)

    def group_points_and_pass2(job):                   # H1 + G2 of every scene: points and queries side by side, ONE pass 2
        if job.empty:
            return
        if job.e1 is not None:
            job.e1.synchronize()
        both = job.masks[0].numpy()                    # u8 [2, sum H W]: every scene's keypoint masks, then every scene's road masks
        _kdtree_selfcheck()                            # once, before the threads need its answer

        def one(c):
            (H, W), a = c.shape, c.mask_off
            c.kp_mask, c.road_mask = (both[j, a:a + H * W].reshape(H, W).copy() for j in (0, 1))
            c.graph_points = extract_graph_points(c.kp_mask, c.road_mask, config, n_threads=1)
            if c.graph_points.shape[0]:
                c.fq = build_all_patch_queries(c.graph_points, c.infos, 0, len(c.infos), config, flat=True, n_threads=1)

        list(host_pool.map(one, [c for c in job.group if not c.empty]))
        lap("group: points + queries")
        live = [c for c in job.group if not c.empty and c.graph_points.shape[0]]
        if not live:
            return
        if any(c.fq is None for c in live):            # non-integer radius: the serial per-tile path, scene by scene
            for c in live:
                c.votes = edge_votes(net, job.emb[c.lo:c.hi], c.graph_points, c.infos, 0, len(c.infos), config, device)
        elif _ragged_pass2(net, config):               # the rows of all scenes in ONE launch sequence: tile indices count through the group
            job.plan, scores = _queue_pass2(net, job.emb, _concat_queries(job, live), ctx.bs, K, True, job.io)
            if job.plan:
                job.scores, job.e2 = lane.download(job.io.pool, "score", scores)
                job.io.step("pass 2 on its way back")
        else:                                          # padded batches never mix scenes: per scene, as alone
            for k, c in enumerate(live):
                c.plan, scores = _queue_pass2(net, job.emb[c.lo:c.hi], c.fq, ctx.bs, K, False, _ChildIO(job.io, k))
                if c.plan:
                    c.scores, c.e2 = lane.download(job.io.pool, f"score#{k}_", scores)
        job.emb = None
        lap("group: pack + queue pass 2")

    def group_finish(job):                             # H2 of every scene, side by side
        rows = None
        if job.plan:
            if job.e2 is not None:
                job.e2.synchronize()
            rows = job.scores[0].numpy()
            if job.io.t is not None and lane.times is not None:
                t = job.io.t
                lane.times.append((len(job.group), t[0].elapsed_time(t[1]), t[2].elapsed_time(t[3])))
        for c in job.group:
            if c.e2 is not None:
                c.e2.synchronize()
        lap("group: wait for pass-2 scores")

        def one(c):
            if c.empty:
                return _empty_result(*c.shape)
            if c.graph_points.shape[0] == 0:
                return c.graph_points, no_edges, c.kp_mask, c.road_mask
            nodes, n_pts = c.graph_points[:, ::-1], c.graph_points.shape[0]
            if c.votes is None:
                R = int(c.fq.offsets[-1] - c.fq.offsets[0])
                if rows is not None and R:
                    c.votes = _collect_pass2(c.fq, "ragged", [rows[c.row0:c.row0 + R]], n_pts, K, n_threads=1)
                elif c.plan:
                    c.votes = _collect_pass2(c.fq, c.plan, [sc.numpy() for sc in c.scores], n_pts, K, n_threads=1)
                else:
                    return nodes, no_edges.astype(np.int64), c.kp_mask, c.road_mask
            return nodes, votes_to_edges(*c.votes, n_pts, config.TOPO_THRESHOLD), c.kp_mask, c.road_mask

        res = list(host_pool.map(one, job.group))
        lap("group: votes -> edges")
        return res

    try:
        units = _scene_groups(iter(imgs), valids, config, n_group)
        unit = next(units, None)
        if unit is None:
            return
        with _host_quiet():
            cur = launch(unit, pools[0])
        prev, i = None, 0
        while cur is not None:
            with _host_quiet():
                lap("(consumer)")
                if cur.e1 is not None:
                    cur.e1.synchronize()               # group i's masks are on the host: the device is free for group i+1
                    _poll_finite(net, device)
                lap("wait for pass-1 masks")
                unit = next(units, None)
                nxt = launch(unit, pools[(i + 1) % 2]) if unit is not None else None
                res = None if prev is None else [finish(prev)] if prev.group is None else group_finish(prev)
            if prev is not None:
                yield from res
            with _host_quiet():
                (points_and_pass2 if cur.group is None else group_points_and_pass2)(cur)
            prev, cur, i = cur, nxt, i + 1
        with _host_quiet():
            res = [finish(prev)] if prev.group is None else group_finish(prev)
        yield from res
    finally:
        host_pool.shutdown(wait=False)


def _infer_imgs_tile_sharded(net, imgs, config, device=None, stats=None, valids=None, aois=None):
    """Tile-sharded scenes (BASELINE configs[3]: ONE scene's tiles over the ranks of a node), software-pipelined like infer_imgs:
    every rank queues pass 1 of scene i+1 on its GPU BEFORE the host stages of scene i, so that rank 0's serial section (mask ->
    graph points, reference graph_extraction.py:130-139 / graph_utils.py:572-591, and the final vote merge) runs while all GPUs —
    its own included — are busy with the next scene's pass 1.  Per scene and rank the device then sees pass 1 / world + pass 2 /
    world back to back; the exchange steps are the three of infer_one_img (banded canvas reduce, point broadcast, vote gather) in
    the same order on every rank:   stage1(i+1): reduce_canvases(i+1)   |   stage2(i): broadcast_points(i), gather_*_votes(i).
    Results per scene are those of infer_one_img under the same world size (same kernels, same summation orders); rank 0 yields
    the tuples, the other ranks yield None.  `stats` (a dict) collects per-stage wall times and the bytes of every exchange."""
    ctx = _SceneSetup(net, config, device, sharded=True)
    device, rank = ctx.device, ctx.rank
    cuda = device.type == "cuda"
    io = _BlockingIO(device, async_scene=cuda)
    stats = stats if stats is not None else {}
    for k in ("pass1_queue_ms", "points_host_ms", "pass2_ms", "merge_host_ms", "canvas_bytes", "points_bytes", "votes_bytes", "scenes"):
        stats.setdefault(k, 0.0)

    valids, aois = _valid_iter(valids), _valid_iter(aois)

    def stage1(img, valid=None, aoi=None):
        t0 = time.perf_counter()
        job = _pass1_front(ctx, io, img, valid, aoi=aoi)
        if job.bands is not None:
            # this rank's own share: the band it ships to rank 0 (rank 0: what it receives), so that per-rank statistics are per rank
            x0, x1 = job.bands[rank]
            rows = (job.model_shape or job.shape)[0] + job.pads[0] + job.pads[1]      # a band is a strip of columns of the full canvas HEIGHT
            stats["canvas_bytes"] += D.canvas_bytes(job.bands, rows) if rank == 0 else 2 * 4 * rows * max(0, x1 - x0)
        if job.kp_u8 is not None:
            both = [job.kp_u8, job.road_u8] + ([job.model_kp_u8, job.model_road_u8] if job.scale is not None else [])
            if cuda:       # asynchronous download behind the scene's own kernels: the host does not wait here
                job.masks = [torch.empty(t.shape, dtype=t.dtype, pin_memory=True) for t in both]
                for h, t in zip(job.masks, both):
                    h.copy_(t, non_blocking=True)
                job.e1 = torch.cuda.Event()
                job.e1.record(torch.cuda.current_stream(device))
            else:
                job.masks = both
        stats["pass1_queue_ms"] += 1e3 * (time.perf_counter() - t0)
        return job

    def stage2(job):
        t0 = time.perf_counter()
        kp_mask = road_mask = scene_masks = None
        if job.masks is not None:
            if job.e1 is not None:
                job.e1.synchronize()
            kp_mask, road_mask, *model = (np.array(m.numpy()) for m in job.masks)
            if model:                                  # SCENE_SCALE: the scene-frame masks are the caller's, the points come from the model frame's
                scene_masks, (kp_mask, road_mask) = (kp_mask, road_mask), model
            stats["points_host_ms"] += 1e3 * (time.perf_counter() - t0)      # the wait for the masks counts as host time of the points
        return _pass2_sharded(ctx, job, kp_mask, road_mask, stats, scene_masks=scene_masks)

    it = iter(imgs)
    img = next(it, None)
    if img is None:
        return
    with _host_quiet():
        cur = stage1(img, next(valids), next(aois))
    while cur is not None:
        with _host_quiet():
            img = next(it, None)
            nxt = stage1(img, next(valids), next(aois)) if img is not None else None        # the next scene's pass 1 is on the device before this scene's host work
            res = stage2(cur)
        stats["scenes"] += 1
        yield res
        cur = nxt


def read_rgb_img(path):
    """dataset.py:16-19 (cv2.imread + BGR->RGB): [H,W,3] uint8 RGB.  PIL decodes the same 8-bit PNGs."""
    from PIL import Image
    return np.ascontiguousarray(np.array(Image.open(path).convert("RGB")))


def has_alpha(path):
    """Whether an image file has an alpha channel (reads the header only); False for .npy scenes."""
    from PIL import Image
    if str(path).endswith(".npy"):
        return False
    with Image.open(path) as im:
        return im.mode in ("RGBA", "LA", "PA") or "transparency" in im.info       # a palette / grey PNG with a tRNS chunk as well


def read_alpha_valid(path):
    """The validity mask an image file carries itself: alpha > 0 of a file with an alpha channel or a transparency (tRNS) entry as
    bool [H,W]; None for a file without one (read_rgb_img drops alpha)."""
    from PIL import Image
    if not has_alpha(path):
        return None
    return np.ascontiguousarray(np.array(Image.open(path).convert("RGBA").getchannel("A")) > 0)


def read_valid_mask(path):
    """A validity mask file: .npy (bool or uint8 [H,W]) as it is, or an image whose non-zero pixels are valid (read as 8-bit grey)."""
    from PIL import Image
    if str(path).endswith(".npy"):
        return np.load(path)
    return np.ascontiguousarray(np.array(Image.open(path).convert("L")) > 0)


def cityscale_data_partition():
    """dataset.py:21-38: (train, validation, test) region indices of the 180 CityScale regions."""
    train = [x for x in range(180) if x % 10 < 8]
    test = [x for x in range(180) if x % 10 == 9 or x % 20 == 8]
    val = [x for x in range(180) if x % 20 == 18]
    return train, val, test


def spacenet_data_partition():
    """dataset.py:41-53: reads ./spacenet/data_split.json relative to the working directory, as the reference does."""
    import json
    with open("./spacenet/data_split.json", "r") as jf:
        d = json.load(jf)
    return d["train"], d["validation"], d["test"]


def main(argv=None):
    """The command line lives in sam_road_amd/cli.py, which imports this module: see cli.main."""
    from . import cli
    return cli.main(argv)


if __name__ == "__main__":
    main()
