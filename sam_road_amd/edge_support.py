"""EDGE_SUPPORT: the one statement of how the road mask under every edge of a predicted graph is counted, how edges are
kept or dropped by those counts, and how the result is exported — on the host, in integers.  numpy (and the stdlib json) only; the device
(csrc/edge_support.hip) must equal edge_support_ref exactly.  The reference has no such step: its graph leaves as the votes produced it.

    EDGE_SUPPORT: {width: t,            # int 1 .. 255, default 1: the 8-connected centre line
                   on: T,               # float 0 .. 1, default ROAD_THRESHOLD; on_level = floor(T * 255)
                   min_mean: m,         # optional, float 0 .. 1
                   min_on: f,           # optional, float 0 .. 1
                   max_invalid: k,      # optional, int >= 0
                   drop_isolated: bool} # default false
    absent / None / {}: nothing is computed, nothing is launched.

THE COVERED SET.  C_e, the covered set of edge e = (a, b), holds the pixels of [0, H) x [0, W) that GRAPH_RASTER's rule
(sam_road_amd/graph_raster.py) covers for this edge alone at width t: exactly graph_raster_ref(nodes, [e], shape, t) == 1.  The graph is
checked by graph_raster.check_graph as it is: an edge spans at most 16383 pixels per axis, coordinates lie within +-2^28.

THE STATISTICS.  With M a uint8 [H, W] mask (the road mask) and V an optional uint8 / bool [H, W] validity mask, an edge has four int32:
    n         = |C_e|
    s         = sum of M[x] over x in C_e
    n_on      = #{x in C_e : M[x] > on_level}
    n_invalid = #{x in C_e : V[x] == 0}, 0 without V

THE 32-BIT BOUND.  C_e is the set of lattice points within t / 2 of a segment: the lattice points of a convex stadium of length
l <= MAX_SPAN sqrt(2) = 16383 sqrt(2) < 23170 and width t <= MAX_WIDTH = 255, of area A = l t + pi t^2 / 4 and perimeter P = 2 l + pi t.
A convex region of the plane holds at most A + P / 2 + 1 lattice points, so
    n <= 23170 * 255 + 51071 + (23170 + 401) + 1 = 5 982 993 < 6.0e6     (MAX_COVERED)
and s <= 255 n <= 1 525 663 215 < 2^31 = 2 147 483 648: the four statistics fit int32, and a lane's partial sums fit 32 bits in any order.

THE KEEP RULE (edge_keep), on the integers alone — the device never sees a float.  An edge is kept iff every condition the key states holds:
    min_mean m:     n > 0 and s > m * 255 * n           (the mean of M over C_e, in units of 255, above m)
    min_on f:       n > 0 and n_on >= f * n
    max_invalid k:  n_invalid <= k
With n = 0 the edge lies wholly outside the image and there is no evidence: min_mean and min_on fail, max_invalid passes.  A key that
states none of the three yields attributes and filters nothing.

THE KEPT GRAPH (filter_graph).  The kept edges stay in their order.  The nodes are untouched, unless drop_isolated removes the nodes of
degree 0 AFTER the filter; the remaining nodes keep their order and the edge indices are renumbered.

THE ATTRIBUTES (edge_attrs), per edge: n, mean = s / n (None when n = 0), on_frac = n_on / n (None when n = 0), n_invalid and length_px,
the Euclidean length of a -> b in float64.

THE EXPORT (graph_geojson).  A FeatureCollection of one LineString per edge whose properties are the attributes.  Coordinates are
[x, y] = [col + 1/2, row + 1/2]: a node is the centre of its pixel in the pixel-corner frame that sam_road_amd/aoi.py states.  With a
geotransform [g0 .. g5] they go through X = g0 + x g1 + y g2, Y = g3 + x g4 + y g5, the forward of SCENE_AOI's formula, so an exported
graph and an area of interest given in the same map frame line up.

Masks and nodes of a result are already in the real scene's frame under SCENE_SCALE and SCENE_PAD: nothing is resampled."""
import collections
import json

import numpy as np

from .graph_raster import MAX_WIDTH, _check_shape, check_graph

MAX_COVERED = 5982993                                     # |C_e| at most, from the bound above
assert 255 * MAX_COVERED < 2 ** 31
STATS = ("n", "s", "n_on", "n_invalid")
_KEYS = ("width", "on", "min_mean", "min_on", "max_invalid", "drop_isolated")

# width: int; on_level: int 0 .. 255; min_mean / min_on: float or None; max_invalid: int or None; drop_isolated: bool
EdgeSupport = collections.namedtuple("EdgeSupport", "width on_level min_mean min_on max_invalid drop_isolated")


def _is_int(v):
    return isinstance(v, (int, np.integer)) and not isinstance(v, (bool, np.bool_))


def _is_num(v):
    return isinstance(v, (int, float, np.integer, np.floating)) and not isinstance(v, (bool, np.bool_))


def _unit(name, v):
    if not _is_num(v) or not np.isfinite(v) or not 0 <= v <= 1:
        raise ValueError(f"EDGE_SUPPORT: {name} must be a number 0 .. 1, got {v!r}")
    return float(v)


def on_level_of(threshold):
    """floor(T * 255) for a threshold T in 0 .. 1: M > on_level iff M / 255 > T for a uint8 M whenever T * 255 is not a whole number."""
    return int(np.floor(_unit("on", threshold) * 255))


def check_width(width):
    if not _is_int(width) or not 1 <= width <= MAX_WIDTH:
        raise ValueError(f"EDGE_SUPPORT: width must be an int 1 .. {MAX_WIDTH}, got {width!r}")
    return int(width)


def check_on_level(on_level):
    if not _is_int(on_level) or not 0 <= on_level <= 255:
        raise ValueError(f"EDGE_SUPPORT: on_level must be an int 0 .. 255, got {on_level!r}")
    return int(on_level)


def edge_support_key_of(v, road_threshold=0.5, attributes_only=False):
    """An EDGE_SUPPORT value (the mapping of the module's docstring) as an EdgeSupport tuple; None for None / {}.  road_threshold: the
    default of `on`.  ValueError for anything else: unknown keys, bools used as numbers, values outside their range, and a key that states
    none of min_mean / min_on / max_invalid (it would filter nothing) unless the caller uses it for attributes only."""
    if v is None or (isinstance(v, dict) and not v):
        return None
    if isinstance(v, EdgeSupport):
        return v
    if not isinstance(v, dict):
        raise ValueError(f"EDGE_SUPPORT must be a mapping with {', '.join(_KEYS)}, got {v!r}")
    unknown = sorted(set(v) - set(_KEYS), key=str)
    if unknown:
        raise ValueError(f"EDGE_SUPPORT: unknown key {unknown[0]!r} ({', '.join(_KEYS)})")
    width = check_width(v.get("width", 1))
    on = v.get("on")
    level = on_level_of(road_threshold if on is None else on)
    min_mean = None if v.get("min_mean") is None else _unit("min_mean", v["min_mean"])
    min_on = None if v.get("min_on") is None else _unit("min_on", v["min_on"])
    k = v.get("max_invalid")
    if k is not None and (not _is_int(k) or k < 0):
        raise ValueError(f"EDGE_SUPPORT: max_invalid must be an int >= 0, got {k!r}")
    drop = v.get("drop_isolated", False)
    if not isinstance(drop, (bool, np.bool_)):
        raise ValueError(f"EDGE_SUPPORT: drop_isolated must be true or false, got {drop!r}")
    key = EdgeSupport(width, level, min_mean, min_on, None if k is None else int(k), bool(drop))
    if not attributes_only and not filters(key):
        raise ValueError("EDGE_SUPPORT: the key states none of min_mean, min_on, max_invalid: it would filter nothing (it serves attributes only, "
                         "as with --graph-geojson)")
    return key


def edge_support_key(config, attributes_only=False):
    """config.EDGE_SUPPORT as an EdgeSupport tuple, None without the key; ValueError before any device is touched.  A key that states none
    of min_mean / min_on / max_invalid filters nothing: it is a ValueError unless the caller uses it for attributes only."""
    v = config.get("EDGE_SUPPORT")
    thr = config.get("ROAD_THRESHOLD", 0.5)
    return edge_support_key_of(v, 0.5 if thr is None else thr, attributes_only)


def filters(key):
    """Does the key state a condition?"""
    return key is not None and (key.min_mean is not None or key.min_on is not None or key.max_invalid is not None)


def edge_support_override(config, width=None, on=None, min_mean=None, min_on=None, max_invalid=None, drop_isolated=None, attributes_only=False):
    """The EDGE_SUPPORT mapping with the CLI's flags laid over the config's key: a flag that is given replaces that field, the others stay
    as the config has them.  The result is validated."""
    base = config.get("EDGE_SUPPORT")
    thr = config.get("ROAD_THRESHOLD", 0.5)
    thr = 0.5 if thr is None else thr
    edge_support_key_of(base, thr, True)
    out = dict(base) if isinstance(base, dict) else {}
    for field, val in (("width", width), ("on", on), ("min_mean", min_mean), ("min_on", min_on), ("max_invalid", max_invalid)):
        if val is not None:
            out[field] = val
    if drop_isolated:
        out["drop_isolated"] = True
    edge_support_key_of(out, thr, attributes_only)
    return out


# ---- the rule --------------------------------------------------------------------------------------------------------------------------------
def _masks(mask, valid, H, W):
    mask = np.asarray(mask)
    if mask.dtype != np.uint8 or mask.shape != (H, W):
        raise ValueError(f"EDGE_SUPPORT: the mask must be uint8 [{H}, {W}], got {mask.dtype} {mask.shape}")
    if valid is not None:
        valid = np.asarray(valid)
        if valid.dtype not in (np.uint8, np.bool_) or valid.shape != (H, W):
            raise ValueError(f"EDGE_SUPPORT: valid must be uint8 / bool [{H}, {W}], got {valid.dtype} {valid.shape}")
    return mask, valid


def edge_support_ref(nodes, edges, mask, width, on_level, valid=None):
    """THE STATISTICS of the module's docstring on the host: int32 [E, 4], rows {n, s, n_on, n_invalid}."""
    mask = np.asarray(mask)
    H, W = _check_shape(mask.shape[:2] if mask.ndim == 2 else (0, 0))
    mask, valid = _masks(mask, valid, H, W)
    n, e = check_graph(nodes, edges)
    t, level = check_width(width), check_on_level(on_level)
    out = np.zeros((e.shape[0], 4), np.int32)
    for k, box, cov in covered_sets(n, e, H, W, t):
        m = mask[box][cov]
        out[k, 0], out[k, 1], out[k, 2] = m.size, int(m.sum(dtype=np.int64)), int((m > level).sum())
        if valid is not None:
            out[k, 3] = int((valid[box][cov] == 0).sum())
    return out


def covered_sets(nodes, edges, H, W, t):
    """THE COVERED SET of every edge that has pixels in the image, for the statistics that are taken over it (here and in road_width.py):
    yields (edge index, (row slice, column slice) of the edge's box grown by ceil(t / 2) and clipped to the image, bool mask of C_e
    inside that box).  nodes / edges: as check_graph returns them; t: a checked width.  An edge whose box is empty is not yielded."""
    n = nodes.astype(np.int64)
    g, tt = (t + 1) // 2, t * t
    for k, (ia, ib) in enumerate(edges.tolist()):
        (ar, ac), (br, bc) = n[ia].tolist(), n[ib].tolist()
        y0, y1 = max(min(ar, br) - g, 0), min(max(ar, br) + g, H - 1)
        x0, x1 = max(min(ac, bc) - g, 0), min(max(ac, bc) + g, W - 1)
        if y0 > y1 or x0 > x1:
            continue
        pr = (np.arange(y0, y1 + 1, dtype=np.int64) - ar)[:, None]
        pc = (np.arange(x0, x1 + 1, dtype=np.int64) - ac)[None, :]
        dr, dc = br - ar, bc - ac
        L = dr * dr + dc * dc
        cov = 4 * (pr * pr + pc * pc) <= tt
        if L:
            u = pr * dr + pc * dc
            at_b = 4 * ((pr - dr) ** 2 + (pc - dc) ** 2) <= tt
            cross = pr * dc - pc * dr
            cov = np.where(u <= 0, cov, np.where(u >= L, at_b, 4 * cross * cross <= tt * L))
        yield k, (slice(y0, y1 + 1), slice(x0, x1 + 1)), cov


def _stats(stats):
    s = np.asarray(stats)
    if s.size == 0:
        s = np.zeros((0, 4), np.int32)
    if s.ndim != 2 or s.shape[1] != 4 or s.dtype.kind not in "iu":
        raise ValueError(f"EDGE_SUPPORT: the statistics must be an integer [E, 4] array, got {s.dtype} {s.shape}")
    return s.astype(np.int64)


def edge_keep(stats, key):
    """THE KEEP RULE: bool [E].  Exact: the thresholds are taken as the rationals their floats are, the comparisons are in integers."""
    from fractions import Fraction
    s = _stats(stats)
    key = edge_support_key_of(key, attributes_only=True)
    keep = np.ones(s.shape[0], bool)
    if key is None:
        return keep
    n, tot, n_on, n_inv = (s[:, k] for k in range(4))
    n, tot, n_on, n_inv = (c.astype(object) for c in (n, tot, n_on, n_inv))          # Python ints: a float's denominator may exceed 64 bits
    if key.min_mean is not None:                           # s > m 255 n  <=>  s q > p 255 n  with m = p / q
        m = Fraction(key.min_mean)
        keep &= ((n > 0) & (tot * m.denominator > m.numerator * 255 * n)).astype(bool)
    if key.min_on is not None:                             # n_on >= f n  <=>  n_on q >= p n  with f = p / q
        f = Fraction(key.min_on)
        keep &= ((n > 0) & (n_on * f.denominator >= f.numerator * n)).astype(bool)
    if key.max_invalid is not None:
        keep &= n_inv <= key.max_invalid
    return keep


def filter_graph(nodes, edges, keep, drop_isolated=False):
    """THE KEPT GRAPH: (nodes, edges, node index of every kept node in the old array).  The arrays keep their dtypes."""
    nodes, edges = np.asarray(nodes), np.asarray(edges)
    nodes = nodes.reshape(-1, 2) if nodes.size == 0 else nodes
    edges = edges.reshape(-1, 2) if edges.size == 0 else edges
    keep = np.asarray(keep, bool)
    if keep.shape != (edges.shape[0],):
        raise ValueError(f"EDGE_SUPPORT: keep must be bool [{edges.shape[0]}], got {keep.shape}")
    edges = edges[keep]
    index = np.arange(nodes.shape[0])
    if drop_isolated:
        used = np.zeros(nodes.shape[0], bool)
        used[edges.reshape(-1).astype(np.int64)] = True
        index = np.flatnonzero(used)
        new = np.cumsum(used) - 1
        edges = new[edges.astype(np.int64)].astype(edges.dtype).reshape(-1, 2)
        nodes = nodes[index]
    return nodes, edges, index


def edge_attrs(nodes, edges, stats):
    """THE ATTRIBUTES: a list of {n, mean, on_frac, n_invalid, length_px}, one per edge."""
    n, e = check_graph(nodes, edges)
    s = _stats(stats)
    if s.shape[0] != e.shape[0]:
        raise ValueError(f"EDGE_SUPPORT: {s.shape[0]} rows of statistics for {e.shape[0]} edges")
    d = (n[e[:, 1]].astype(np.float64) - n[e[:, 0]].astype(np.float64)).reshape(-1, 2)
    length = np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1])
    return [dict(n=int(c), mean=None if c == 0 else int(t) / int(c), on_frac=None if c == 0 else int(o) / int(c), n_invalid=int(i), length_px=float(ln))
            for (c, t, o, i), ln in zip(s.tolist(), length.tolist())]


# ---- the export ------------------------------------------------------------------------------------------------------------------------------
def _geotransform(gt):
    if gt is None:
        return None
    if not isinstance(gt, (list, tuple, np.ndarray)) or len(gt) != 6 or not all(_is_num(g) and np.isfinite(g) for g in gt):
        raise ValueError(f"EDGE_SUPPORT: geotransform must be six finite numbers [g0 .. g5], got {gt!r}")
    return [float(g) for g in gt]


def graph_geojson(nodes, edges, attrs=None, geotransform=None):
    """THE EXPORT: a FeatureCollection dict, one LineString per edge in the edges' order, properties = the edge's attributes (plus its index
    `edge`).  json.dump writes it."""
    n, e = check_graph(nodes, edges)
    g = _geotransform(geotransform)
    if attrs is not None and len(attrs) != e.shape[0]:
        raise ValueError(f"EDGE_SUPPORT: {len(attrs)} attribute rows for {e.shape[0]} edges")

    def point(i):
        x, y = float(n[i, 1]) + 0.5, float(n[i, 0]) + 0.5
        return [x, y] if g is None else [g[0] + x * g[1] + y * g[2], g[3] + x * g[4] + y * g[5]]

    feats = [{"type": "Feature", "geometry": {"type": "LineString", "coordinates": [point(a), point(b)]},
              "properties": dict({"edge": k}, **({} if attrs is None else attrs[k]))} for k, (a, b) in enumerate(e.tolist())]
    return {"type": "FeatureCollection", "features": feats}


def write_geojson(path, nodes, edges, attrs=None, geotransform=None):
    with open(path, "w") as f:
        json.dump(graph_geojson(nodes, edges, attrs, geotransform), f)


# ---- the device ------------------------------------------------------------------------------------------------------------------------------
def _ops(device, net):
    if net is not None:
        return net
    from .model import DeviceGraphOps
    return DeviceGraphOps("cuda" if device is None else device)


def edge_stats(nodes, edges, mask, width=1, on_level=127, valid=None, device=None, net=None):
    """THE STATISTICS on the device (srh_graph_edge_stats): an int32 [E, 4] HOST array equal to edge_support_ref.  mask / valid: numpy
    arrays or tensors on the device.  net: the model whose device is used; without one the device `device` (default cuda).  Runs on
    torch's current stream and waits for that stream alone."""
    out = _ops(device, net).graph_edge_stats(nodes, edges, mask, width=width, on_level=on_level, valid=valid)
    return out.cpu().numpy()


def apply(key, result, valid=None, net=None, device=None):
    """The key applied to `result`, the 4-tuple (nodes, edges, kp_mask, road_mask) of infer_one_img:
    ((nodes, edges, kp_mask, road_mask), attrs) with the filtered graph and the attributes of its edges.  key None returns the result
    object itself (and no attributes) and calls nothing.  valid: the scene's validity mask, uint8 / bool [H, W], or None."""
    if key is None:
        return result, None
    nodes, edges, kp_mask, road_mask = result
    road = np.asarray(road_mask)
    if valid is not None:
        _masks(road, valid, *road.shape[:2])
    n, e = check_graph(nodes, edges)
    stats = edge_stats(n, e, road, key.width, key.on_level, valid=valid, device=device, net=net) if e.shape[0] else np.zeros((0, 4), np.int32)
    keep = edge_keep(stats, key)
    new_nodes, new_edges, _ = filter_graph(nodes, edges, keep, key.drop_isolated)
    return (new_nodes, new_edges, kp_mask, road_mask), edge_attrs(new_nodes, new_edges, stats[keep])


def apply_ref(key, result, valid=None):
    """apply() on the host statement alone."""
    if key is None:
        return result, None
    nodes, edges, kp_mask, road_mask = result
    stats = edge_support_ref(nodes, edges, np.asarray(road_mask), key.width, key.on_level, valid)
    keep = edge_keep(stats, key)
    new_nodes, new_edges, _ = filter_graph(nodes, edges, keep, key.drop_isolated)
    return (new_nodes, new_edges, kp_mask, road_mask), edge_attrs(new_nodes, new_edges, stats[keep])
