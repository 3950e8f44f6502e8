"""ROAD_WIDTH: the one statement of how wide the road under every edge of a predicted graph is — an exact, capped distance
map of the thresholded road mask, six integers per edge taken from it along the edge's centre line, the attributes and the keep rule on
those integers — on the host.  numpy and the stdlib only; the device (csrc/road_width.hip) must equal road_dist_ref and road_width_ref
exactly.  The reference has no such step.

    ROAD_WIDTH: {on: T,               # float 0 .. 1, default ROAD_THRESHOLD; on_level = floor(T * 255), as EDGE_SUPPORT
                 max_radius: R,       # int 1 .. 254, default 32: distances are exact up to R and capped there
                 min_width: w,        # optional, float >= 0 (px)
                 max_width: w,        # optional, float >= 0 (px)
                 min_in: f,           # optional, float 0 .. 1
                 drop_isolated: bool} # default false
    absent / None / {}: nothing is computed, nothing is launched.  A key that states no condition is valid: it yields attributes only.

THE DISTANCE MAP (road_dist_ref).  F is the set of pixels with mask > on_level.  D2[x] = 0 for x outside F, else
    D2[x] = min(R^2, min over the pixels y OF THE IMAGE outside F of |x - y|^2)
— a uint16 [H, W], since R <= 254 gives D2 <= 64516.  Pixels OUTSIDE the image are not background, so a road that runs off the scene is
not narrowed by the scene's edge (scipy.ndimage.distance_transform_edt's convention).  Nodata pixels carry mask 0 and are background.
For a pixel on the road, sqrt(D2) = d is the local half-width: width ~ 2 d - 1.

ITS SEPARABLE FORM, which the device mirrors:
    G[y, x]  = min(R + 1, vertical distance in column x to the nearest background pixel)                 (0 on background)
    D2[y, x] = min(R^2, min over |dx| <= R, 0 <= x + dx < W of dx^2 + G[y, x + dx]^2)
The capped search is exact: a background pixel nearer than R lies within R in both axes, so its column is searched and G of that column
is not capped below it; a candidate that a cap distorts has G = R + 1 and is at least (R + 1)^2 > R^2, where the outer cap cuts it.

THE STATISTICS (road_width_ref).  C_e is EDGE_SUPPORT's covered set of edge e at width 1, the 8-connected centre line
(edge_support.covered_sets; the graph is checked by graph_raster.check_graph as it is).  Q[x] = isqrt(256 D2[x]) = floor(16 sqrt(D2[x])),
at most floor(16 * 254) = 4064.  An edge has eight int32 {n, n_in, s_q, n_cap, d2_min, d2_max, 0, 0}:
    n      = |C_e|                            n_in   = #{x in C_e : D2[x] > 0}
    s_q    = sum of Q[x] over C_e             n_cap  = #{x in C_e : D2[x] = R^2}
    d2_min = min of D2 over the pixels of C_e with D2 > 0, 0 when n_in = 0
    d2_max = max of D2 over C_e

THE 32-BIT BOUND.  By the lattice-point bound of edge_support.py at t = 1 — a stadium of length l <= 16383 sqrt(2) < 23170 and width 1
holds at most l + pi / 4 + (2 l + pi) / 2 + 1 < 46343 lattice points — n <= 46343 (MAX_COVERED), so s_q <= 4064 * 46343 = 188 337 952
< 2^31: the statistics fit int32, and a lane's partial sums fit 32 bits in any order.

THE ATTRIBUTES (width_attrs), per edge: width_px = 2 s_q / (16 n_in) - 1, width_min_px = 2 sqrt(d2_min) - 1, width_max_px =
2 sqrt(d2_max) - 1 (each None when n_in = 0), in_frac = n_in / n (None when n = 0), width_capped = n_cap > 0 (the width is then a lower
bound), and length_px.

THE KEEP RULE (width_keep), on the integers alone.  An edge is kept iff every condition the key states holds:
    min_width w:  n_in > 0 and 2 s_q >= 16 (w + 1) n_in          (the mean of 2 Q / 16 - 1 over the in-road pixels, at least w)
    max_width w:  n_in > 0 and 2 s_q <= 16 (w + 1) n_in
    min_in f:     n > 0 and n_in >= f n
An edge with n = 0 fails every stated condition.  The kept graph is edge_support.filter_graph's, drop_isolated included.

Masks and nodes of a result are already in the real scene's frame under SCENE_SCALE and SCENE_PAD: the width is in scene pixels."""
import collections
import math

import numpy as np

from .edge_support import _is_int, _is_num, _ops, check_on_level, covered_sets, filter_graph, on_level_of
from .graph_raster import _check_shape, check_graph

MAX_RADIUS = 254
MAX_COVERED = 46343                                       # |C_e| at width 1 at most, from the bound above
MAX_Q = 4064                                              # isqrt(256 * 254^2)
assert MAX_Q == math.isqrt(256 * MAX_RADIUS ** 2) and MAX_Q * MAX_COVERED < 2 ** 31
STATS = ("n", "n_in", "s_q", "n_cap", "d2_min", "d2_max")
_KEYS = ("on", "max_radius", "min_width", "max_width", "min_in", "drop_isolated")

# on_level: int 0 .. 255; max_radius: int; min_width / max_width / min_in: float or None; drop_isolated: bool
RoadWidth = collections.namedtuple("RoadWidth", "on_level max_radius min_width max_width min_in drop_isolated")


def check_radius(R):
    if not _is_int(R) or not 1 <= R <= MAX_RADIUS:
        raise ValueError(f"ROAD_WIDTH: max_radius must be an int 1 .. {MAX_RADIUS}, got {R!r}")
    return int(R)


def _width(name, v):
    if not _is_num(v) or not np.isfinite(v) or v < 0:
        raise ValueError(f"ROAD_WIDTH: {name} must be a number >= 0, got {v!r}")
    return float(v)


def _on_level(threshold):
    try:
        return on_level_of(threshold)
    except ValueError:
        raise ValueError(f"ROAD_WIDTH: on must be a number 0 .. 1, got {threshold!r}") from None


def road_width_key_of(v, road_threshold=0.5):
    """A ROAD_WIDTH value (the mapping of the module's docstring) as a RoadWidth tuple; None for None / {}.  road_threshold: the default
    of `on`.  ValueError for anything else: unknown keys, bools used as numbers, values outside their range, min_width > max_width."""
    if v is None or (isinstance(v, dict) and not v):
        return None
    if isinstance(v, RoadWidth):
        return v
    if not isinstance(v, dict):
        raise ValueError(f"ROAD_WIDTH must be a mapping with {', '.join(_KEYS)}, got {v!r}")
    unknown = sorted(set(v) - set(_KEYS), key=str)
    if unknown:
        raise ValueError(f"ROAD_WIDTH: unknown key {unknown[0]!r} ({', '.join(_KEYS)})")
    on = v.get("on")
    level = _on_level(road_threshold if on is None else on)
    R = check_radius(v.get("max_radius", 32) if v.get("max_radius") is not None else 32)
    lo = None if v.get("min_width") is None else _width("min_width", v["min_width"])
    hi = None if v.get("max_width") is None else _width("max_width", v["max_width"])
    if lo is not None and hi is not None and lo > hi:
        raise ValueError(f"ROAD_WIDTH: min_width {lo!r} is above max_width {hi!r}")
    f = v.get("min_in")
    if f is not None:
        if not _is_num(f) or not np.isfinite(f) or not 0 <= f <= 1:
            raise ValueError(f"ROAD_WIDTH: min_in must be a number 0 .. 1, got {f!r}")
        f = float(f)
    drop = v.get("drop_isolated", False)
    if not isinstance(drop, (bool, np.bool_)):
        raise ValueError(f"ROAD_WIDTH: drop_isolated must be true or false, got {drop!r}")
    return RoadWidth(level, R, lo, hi, f, bool(drop))


def road_width_key(config):
    """config.ROAD_WIDTH as a RoadWidth tuple, None without the key; ValueError before any device is touched."""
    thr = config.get("ROAD_THRESHOLD", 0.5)
    return road_width_key_of(config.get("ROAD_WIDTH"), 0.5 if thr is None else thr)


def filters(key):
    """Does the key state a condition?"""
    return key is not None and (key.min_width is not None or key.max_width is not None or key.min_in is not None)


def road_width_override(config, enable=None, on=None, max_radius=None, min_width=None, max_width=None, min_in=None, drop_isolated=None):
    """The ROAD_WIDTH mapping with the CLI's flags laid over the config's key: a flag that is given replaces that field, the others stay
    as the config has them; `enable` alone (--road-width) turns an absent key into one with the defaults, {max_radius: 32}.  The result is
    validated."""
    base = config.get("ROAD_WIDTH")
    thr = config.get("ROAD_THRESHOLD", 0.5)
    thr = 0.5 if thr is None else thr
    road_width_key_of(base, thr)
    out = dict(base) if isinstance(base, dict) else {}
    for field, val in (("on", on), ("max_radius", max_radius), ("min_width", min_width), ("max_width", max_width), ("min_in", min_in)):
        if val is not None:
            out[field] = val
    if drop_isolated:
        out["drop_isolated"] = True
    if enable and not out:
        out["max_radius"] = 32
    road_width_key_of(out, thr)
    return out


# ---- the rule --------------------------------------------------------------------------------------------------------------------------------
def _mask(mask):
    mask = np.asarray(mask)
    H, W = _check_shape(mask.shape[:2] if mask.ndim == 2 else (0, 0))
    if mask.dtype != np.uint8:
        raise ValueError(f"ROAD_WIDTH: the mask must be uint8 [H, W], got {mask.dtype} {mask.shape}")
    return mask, H, W


def column_distance_ref(mask, on_level, R):
    """G of the separable form: uint8 [H, W], min(R + 1, vertical distance to the nearest background pixel of the column)."""
    mask, H, W = _mask(mask)
    level, R = check_on_level(on_level), check_radius(R)
    F = mask > level
    G = np.empty((H, W), np.int32)
    d = np.full(W, R + 1, np.int32)
    for y in range(H):                                    # the sweep down: rows above the image hold no background
        d = np.where(F[y], np.minimum(d + 1, R + 1), 0)
        G[y] = d
    d = np.full(W, R + 1, np.int32)
    for y in range(H - 1, -1, -1):                        # the sweep up
        d = np.where(F[y], np.minimum(d + 1, R + 1), 0)
        G[y] = np.minimum(G[y], d)
    return G.astype(np.uint8)


def road_dist_ref(mask, on_level, R):
    """THE DISTANCE MAP of the module's docstring in its separable form: uint16 [H, W]."""
    G = column_distance_ref(mask, on_level, R).astype(np.int32)
    R = int(R)
    H, W = G.shape
    G2 = G * G
    best = np.minimum(G2, R * R)
    for dx in range(1, min(R, W - 1) + 1):                # columns outside the image are not searched
        c = G2[:, dx:] + dx * dx
        np.minimum(best[:, :-dx], c, out=best[:, :-dx])   # x + dx
        c = G2[:, :-dx] + dx * dx
        np.minimum(best[:, dx:], c, out=best[:, dx:])     # x - dx
    best[G == 0] = 0
    return best.astype(np.uint16)


def q_table(R=MAX_RADIUS):
    """Q of every D2 0 .. R^2: uint16 [R^2 + 1], isqrt(256 D2)."""
    return np.array([math.isqrt(256 * v) for v in range(check_radius(R) ** 2 + 1)], np.uint16)


def road_width_ref(nodes, edges, mask, on_level, R, d2=None):
    """THE STATISTICS of the module's docstring on the host: int32 [E, 8], rows {n, n_in, s_q, n_cap, d2_min, d2_max, 0, 0}.  d2: the
    distance map where the caller has it already (uint16 [H, W], road_dist_ref(mask, on_level, R))."""
    mask, H, W = _mask(mask)
    n, e = check_graph(nodes, edges)
    R = check_radius(R)
    D2 = road_dist_ref(mask, on_level, R) if d2 is None else np.asarray(d2)
    if D2.dtype != np.uint16 or D2.shape != (H, W):
        raise ValueError(f"ROAD_WIDTH: the distance map must be uint16 [{H}, {W}], got {D2.dtype} {D2.shape}")
    Q = q_table(R)
    out = np.zeros((e.shape[0], 8), np.int32)
    for k, box, cov in covered_sets(n, e, H, W, 1):
        d = D2[box][cov].astype(np.int64)
        inside = d[d > 0]
        out[k, :6] = (d.size, inside.size, int(Q[d].sum(dtype=np.int64)), int((d == R * R).sum()), int(inside.min()) if inside.size else 0,
                      int(d.max()) if d.size else 0)
    return out


def _stats(stats):
    s = np.asarray(stats)
    if s.size == 0:
        s = np.zeros((0, 8), np.int32)
    if s.ndim != 2 or s.shape[1] != 8 or s.dtype.kind not in "iu":
        raise ValueError(f"ROAD_WIDTH: the statistics must be an integer [E, 8] array, got {s.dtype} {s.shape}")
    return s.astype(np.int64)


def width_keep(stats, key):
    """THE KEEP RULE: bool [E].  Exact: the thresholds are taken as the rationals their floats are, the comparisons are in integers."""
    from fractions import Fraction
    s = _stats(stats)
    key = road_width_key_of(key)
    keep = np.ones(s.shape[0], bool)
    if key is None:
        return keep
    n, n_in, s_q = (s[:, k].astype(object) for k in range(3))          # Python ints: a float's denominator may exceed 64 bits
    if key.min_width is not None:                          # 2 s_q >= 16 (w + 1) n_in  <=>  2 s_q q >= 16 p n_in  with w + 1 = p / q
        w = Fraction(key.min_width) + 1
        keep &= ((n_in > 0) & (2 * s_q * w.denominator >= 16 * w.numerator * n_in)).astype(bool)
    if key.max_width is not None:
        w = Fraction(key.max_width) + 1
        keep &= ((n_in > 0) & (2 * s_q * w.denominator <= 16 * w.numerator * n_in)).astype(bool)
    if key.min_in is not None:                             # n_in >= f n  <=>  n_in q >= p n  with f = p / q
        f = Fraction(key.min_in)
        keep &= ((n > 0) & (n_in * f.denominator >= f.numerator * n)).astype(bool)
    return keep


def width_attrs(nodes, edges, stats):
    """THE ATTRIBUTES: a list of {width_px, width_min_px, width_max_px, in_frac, width_capped, length_px}, one per edge."""
    n, e = check_graph(nodes, edges)
    s = _stats(stats)
    if s.shape[0] != e.shape[0]:
        raise ValueError(f"ROAD_WIDTH: {s.shape[0]} rows of statistics for {e.shape[0]} edges")
    d = (n[e[:, 1]].astype(np.float64) - n[e[:, 0]].astype(np.float64)).reshape(-1, 2)
    length = np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1])
    return [dict(width_px=None if i == 0 else 2 * q / (16 * i) - 1, width_min_px=None if i == 0 else 2 * math.sqrt(lo) - 1,
                 width_max_px=None if i == 0 else 2 * math.sqrt(hi) - 1, in_frac=None if c == 0 else i / c, width_capped=cap > 0, length_px=float(ln))
            for (c, i, q, cap, lo, hi, _, _), ln in zip(s.tolist(), length.tolist())]


# ---- the device ------------------------------------------------------------------------------------------------------------------------------
def distance_map(mask, on_level=127, R=32, device=None, net=None):
    """THE DISTANCE MAP on the device (srh_road_dist): a uint16 [H, W] tensor ON THE DEVICE equal to road_dist_ref.  mask: a numpy array or
    a tensor on the device.  net: the model whose device is used; without one the device `device` (default cuda).  Runs on torch's
    current stream."""
    return _ops(device, net).road_dist(mask, on_level=on_level, radius=R)


def edge_widths(nodes, edges, mask, on_level=127, R=32, device=None, net=None):
    """THE STATISTICS on the device (srh_road_dist, srh_graph_edge_widths): an int32 [E, 8] HOST array equal to road_width_ref.  Runs on
    torch's current stream and waits for that stream alone."""
    ops = _ops(device, net)
    d2 = ops.road_dist(mask, on_level=on_level, radius=R)
    return ops.graph_edge_widths(nodes, edges, d2, radius=R).cpu().numpy()


def _finish(key, result, stats):
    nodes, edges, kp_mask, road_mask = result
    keep = width_keep(stats, key)
    new_nodes, new_edges, _ = filter_graph(nodes, edges, keep, key.drop_isolated)
    return (new_nodes, new_edges, kp_mask, road_mask), width_attrs(new_nodes, new_edges, stats[keep]), keep


def apply(key, result, net=None, device=None, return_keep=False):
    """The key applied to `result`, the 4-tuple (nodes, edges, kp_mask, road_mask) of infer_one_img:
    ((nodes, edges, kp_mask, road_mask), attrs) with the filtered graph and the attributes of its edges.  key None returns the result
    object itself (and no attributes) and calls nothing.  return_keep: a third element, bool [E] over the edges that came in (None
    without a key), for a caller that carries other per-edge data along."""
    if key is None:
        return (result, None, None) if return_keep else (result, None)
    nodes, edges, _, road_mask = result
    road, _, _ = _mask(road_mask)
    n, e = check_graph(nodes, edges)
    stats = edge_widths(n, e, road, key.on_level, key.max_radius, device=device, net=net) if e.shape[0] else np.zeros((0, 8), np.int32)
    out = _finish(key, result, stats)
    return out if return_keep else out[:2]


def apply_ref(key, result):
    """apply() on the host statement alone."""
    if key is None:
        return result, None
    nodes, edges, _, road_mask = result
    return _finish(key, result, road_width_ref(nodes, edges, np.asarray(road_mask), key.on_level, key.max_radius))[:2]
