"""SCENE_AOI: the one statement of how a validity mask follows from the POLYGONS of an area of interest, on the host, in
integers.  No torch, no device: numpy (and the stdlib json for the GeoJSON reader) only.

    SCENE_AOI: {include: [polygon, ...],     # optional; absent / empty: the whole scene is inside
                exclude: [polygon, ...],     # optional
                order: rc | xy,              # default rc: a vertex is [row, col], as the nodes are; xy: [x, y] = [col, row] (GeoJSON)
                geotransform: [g0 .. g5],    # optional, implies xy: X = g0 + col g1 + row g2, Y = g3 + col g4 + row g5
                buffer: b}                   # int -16 .. 16, default 0
    polygon = [ring, ...]                    # GeoJSON's layout: first ring and holes alike, even-odd over all rings of the polygon
    ring    = [[a, b], ...]                  # >= 3 vertices, ints or finite floats; a repeated closing vertex is allowed

A bare list means {include: ...}; the nesting is always polygons -> rings -> vertices (a GeoJSON MultiPolygon's coordinates).

Coordinates are continuous pixel-corner coordinates of the RAW scene: pixel (r, c) covers [r, r + 1) x [c, c + 1), its centre is
(r + 1/2, c + 1/2).  Every coordinate is quantised ONCE, q = int(rint(float64(v) * 256)) (half to even); from there on everything is integers,
in 1/256 px.  For one ring:
  1. horizontal edges are dropped, every other edge is oriented so that y0 < y1; dy = y1 - y0, dx = x1 - x0
  2. an edge crosses row y iff y0 <= yc < y1, yc = 256 y + 128
  3. a crossing edge toggles every pixel of that row from column j = max(0, ceil(((x0 - 128) dy + (yc - y0) dx) / (256 dy))) on (the
     crossing lies at or left of the centre); j >= W toggles nothing
A pixel is inside a polygon iff the number of toggles over all edges of all its rings is odd.  So a centre exactly on a left or top edge is
inside, on a right or bottom edge outside.
  aoi = (include absent ? 1 : OR over include of inside) AND NOT (OR over exclude of inside)          # a union, not an XOR
  buffer b > 0: grow_ref(aoi, b); b < 0: 1 - grow_ref(1 - aoi, -b)                                    # nodata.grow_ref: Chebyshev
  valid_out = aoi, ANDed with the caller's valid != 0 where one is given: u8 [H, W], 0 / 1

A run with the key equals, bit for bit, the pipeline called with valid = aoi_ref(shape, key, valid).  The device kernel
(csrc/scene_aoi.hip) must equal aoi_ref byte for byte; it reads the table of aoi_edges."""
import collections
import json

import numpy as np

from .nodata import grow_ref

FRAC = 256                                                # quantisation steps per pixel
MAX_COORD_PX = 1 << 20                                    # a coordinate lies within +- 2^20 px
MAX_POLYGONS = 64
MAX_EDGES = 16384                                         # non-horizontal edges, over all polygons
MAX_BUFFER = 16
_KEYS = ("include", "exclude", "order", "geotransform", "buffer")

# include: None (the whole scene) or a tuple of polygons; exclude: a tuple of polygons (may be empty); a polygon is a tuple of rings, a
# ring a tuple of (y, x) in 1/256 px — quantised, in the (row, col) frame whatever the key's order was; buffer: int
SceneAoi = collections.namedtuple("SceneAoi", "include exclude buffer")


def _absent(v):
    return v is None or (isinstance(v, dict) and not v)


def _is_int(v):
    return isinstance(v, (int, np.integer)) and not isinstance(v, (bool, np.bool_))


def _is_num(v):
    return (isinstance(v, (int, float, np.integer, np.floating)) and not isinstance(v, (bool, np.bool_)))


def _quantise(v):
    if not np.isfinite(v) or abs(v) > MAX_COORD_PX:
        raise ValueError(f"SCENE_AOI: a coordinate must be finite and within +-2^20 px, got {v!r}")
    return int(np.rint(np.float64(v) * FRAC))


def _polygons(name, polys, xy, inverse):
    if not isinstance(polys, (list, tuple)):
        raise ValueError(f"SCENE_AOI: {name} must be a list of polygons (polygon = list of rings, ring = list of [a, b] vertices), got {polys!r}")
    out = []
    for poly in polys:
        if not isinstance(poly, (list, tuple)) or not poly:
            raise ValueError(f"SCENE_AOI: a polygon of {name} must be a non-empty list of rings, got {poly!r}")
        rings = []
        for ring in poly:
            if not isinstance(ring, (list, tuple)) or not all(isinstance(p, (list, tuple)) and len(p) == 2 and _is_num(p[0]) and _is_num(p[1]) for p in ring):
                raise ValueError(f"SCENE_AOI: a ring of {name} must be a list of [a, b] vertices (ints or floats); the nesting is polygons -> rings -> "
                                 f"vertices, got {ring!r}")
            pts = []
            for a, b in ring:
                a, b = np.float64(a), np.float64(b)
                if not (np.isfinite(a) and np.isfinite(b)):
                    raise ValueError(f"SCENE_AOI: a coordinate must be finite, got {[a, b]!r}")
                if inverse is not None:                    # map (X, Y) -> (col, row) in float64
                    g0, g1, g2, g3, g4, g5, det = inverse
                    dX, dY = a - g0, b - g3
                    a, b = (dX * g5 - dY * g2) / det, (dY * g1 - dX * g4) / det
                row, col = (b, a) if xy else (a, b)
                pts.append((_quantise(row), _quantise(col)))
            if len(pts) > 1 and pts[0] == pts[-1]:         # a repeated closing vertex
                pts.pop()
            if len(pts) < 3:
                raise ValueError(f"SCENE_AOI: a ring has at least 3 vertices, got {ring!r}")
            rings.append(tuple(pts))
        out.append(tuple(rings))
    return tuple(out)


def _ring_edges(ring):
    """The non-horizontal edges of one quantised ring, oriented y0 < y1: rows {y0, x0, y1, x1}."""
    out = []
    for (ya, xa), (yb, xb) in zip(ring, ring[1:] + ring[:1]):
        if ya == yb:
            continue
        out.append((ya, xa, yb, xb) if ya < yb else (yb, xb, ya, xa))
    return out


def aoi_key_of(v):
    """A SCENE_AOI value (the mapping of the module's docstring, or a bare list of polygons) as a SceneAoi tuple, quantised; None for None /
    {}.  ValueError for anything else: unknown keys, bools, an order other than rc / xy, a geotransform with order rc or with determinant 0,
    a ring of fewer than 3 vertices, a non-finite or out-of-range coordinate, a buffer that is not an int in -16 .. 16, more than 64
    polygons or more than 16384 non-horizontal edges."""
    if _absent(v):
        return None
    if isinstance(v, SceneAoi):
        return v
    if isinstance(v, (list, tuple)):
        v = {"include": v}
    if not isinstance(v, dict):
        raise ValueError(f"SCENE_AOI must be a list of polygons or a mapping with include / exclude / order / geotransform / buffer, got {v!r}")
    unknown = sorted(set(v) - set(_KEYS), key=str)
    if unknown:
        raise ValueError(f"SCENE_AOI: unknown key {unknown[0]!r} ({', '.join(_KEYS)})")
    gt = v.get("geotransform")
    order = v.get("order", "rc" if gt is None else "xy")
    name = order.strip().lower() if isinstance(order, str) else order
    if not isinstance(name, str) or name not in ("rc", "xy"):
        raise ValueError(f"SCENE_AOI: order must be 'rc' or 'xy', got {order!r}")
    inverse = None
    if gt is not None:
        if name == "rc":
            raise ValueError("SCENE_AOI: a geotransform maps (X, Y) map coordinates, it does not combine with order rc")
        if not isinstance(gt, (list, tuple)) or len(gt) != 6 or not all(_is_num(g) and np.isfinite(g) for g in gt):
            raise ValueError(f"SCENE_AOI: geotransform must be six finite numbers [g0 .. g5], got {gt!r}")
        g = [np.float64(x) for x in gt]
        det = g[1] * g[5] - g[2] * g[4]
        if det == 0 or not np.isfinite(det):
            raise ValueError(f"SCENE_AOI: geotransform {list(gt)!r} cannot be inverted (g1 g5 - g2 g4 = 0)")
        inverse = (*g, det)
    buf = v.get("buffer", 0)
    if not _is_int(buf) or not -MAX_BUFFER <= buf <= MAX_BUFFER:
        raise ValueError(f"SCENE_AOI: buffer must be an int in -{MAX_BUFFER}..{MAX_BUFFER}, got {buf!r}")
    include = v.get("include")
    include = _polygons("include", include, name == "xy", inverse) if include is not None else None
    if include is not None and not include:                # an empty list: the whole scene, as an absent one
        include = None
    exclude = v.get("exclude")
    exclude = _polygons("exclude", exclude, name == "xy", inverse) if exclude is not None else ()
    n_polys = len(include or ()) + len(exclude)
    if n_polys > MAX_POLYGONS:
        raise ValueError(f"SCENE_AOI: at most {MAX_POLYGONS} polygons (include and exclude together), got {n_polys}")
    n_edges = sum(len(_ring_edges(r)) for p in (include or ()) + exclude for r in p)
    if n_edges > MAX_EDGES:
        raise ValueError(f"SCENE_AOI: at most {MAX_EDGES} non-horizontal edges in all, got {n_edges}")
    return SceneAoi(include, exclude, int(buf))


def scene_aoi_key(config):
    """config.SCENE_AOI as a SceneAoi tuple, or None for a missing key / None / {}: nothing changes anywhere.  ValueError — before the device is
    touched — for anything that is not the mapping of the module's docstring (aoi_key_of)."""
    return aoi_key_of(config.SCENE_AOI)


def scene_aoi_override(config, include=None, exclude=None, geotransform=None, buffer=None):
    """The SCENE_AOI mapping of the command line's --aoi, --aoi-exclude, --aoi-geotransform and --aoi-buffer laid over the config's key: a
    flag that is given replaces that field, the others stay as the config has them.  include / exclude: lists of polygons in xy (what the
    GeoJSON reader returns), so the key's order becomes xy; polygons the config keeps in order rc beside them are a ValueError."""
    v = config.SCENE_AOI
    if isinstance(v, (list, tuple)):
        v = {"include": list(v)}
    if not _absent(v) and not isinstance(v, dict):
        raise ValueError(f"SCENE_AOI must be a list of polygons or a mapping, got {v!r}")
    new = dict(v or {})
    if include is not None or exclude is not None:
        kept = [f for f, given in (("include", include), ("exclude", exclude)) if given is None and new.get(f)]
        if kept and "geotransform" not in new and str(new.get("order", "rc")).strip().lower() != "xy":
            raise ValueError(f"SCENE_AOI: the command line's polygons are xy, the config's {kept[0]} is in order rc: give both on one side")
        new["order"] = "xy"
    for field, val in (("include", include), ("exclude", exclude), ("geotransform", geotransform), ("buffer", buffer)):
        if val is not None:
            new[field] = list(val) if field != "buffer" else val
    return new


def read_geojson(path):
    """The polygons of a GeoJSON file, read with the stdlib json: a list of polygons (list of rings of [x, y]) from a Polygon, MultiPolygon,
    Feature, FeatureCollection or GeometryCollection, nested as deep as they come.  Any other geometry type is a ValueError naming it."""
    with open(path) as f:
        doc = json.load(f)
    out = []

    def walk(node):
        kind = node.get("type") if isinstance(node, dict) else None
        if kind == "Polygon":
            out.append([[list(p[:2]) for p in ring] for ring in node["coordinates"]])
        elif kind == "MultiPolygon":
            for poly in node["coordinates"]:
                out.append([[list(p[:2]) for p in ring] for ring in poly])
        elif kind == "Feature":
            if node.get("geometry") is not None:
                walk(node["geometry"])
        elif kind == "FeatureCollection":
            for feat in node.get("features", []):
                walk(feat)
        elif kind == "GeometryCollection":
            for geom in node.get("geometries", []):
                walk(geom)
        else:
            raise ValueError(f"SCENE_AOI: {path}: geometry type {kind!r} is not supported (Polygon, MultiPolygon, Feature, FeatureCollection, "
                             f"GeometryCollection)")

    walk(doc)
    return out


def aoi_edges(key, H, W):
    """The table the device reads: (edges int32 [E, 4] rows {y0, x0, y1, x1} in 1/256 px with y0 < y1, polygon offsets int32 [n + 1] — polygon
    k owns edges offsets[k] .. offsets[k + 1] —, n_include, n_exclude), include first.  Horizontal edges are dropped (rule 1), and so are
    the edges that cross no row of 0 .. H - 1 (they toggle nothing)."""
    H, W = int(H), int(W)
    rows, offsets = [], [0]
    for poly in (key.include or ()) + key.exclude:
        for ring in poly:
            for y0, x0, y1, x1 in _ring_edges(ring):
                first, last = -((128 - y0) // FRAC), -((128 - y1) // FRAC) - 1          # ceil((y - 128) / 256)
                if max(first, 0) <= min(last, H - 1):
                    rows.append((y0, x0, y1, x1))
        offsets.append(len(rows))
    return (np.asarray(rows, dtype=np.int32).reshape(-1, 4), np.asarray(offsets, dtype=np.int32), len(key.include or ()), len(key.exclude))


def aoi_pack(edges, polys):
    """Both tables as ONE flat int32 array, so that they travel in one upload: the edges (at least one row, zeros without any, so that the
    array's start is the 16-byte aligned edge table) and behind them, at int offset 4 max(E, 1), the polygon offsets."""
    edges = np.ascontiguousarray(edges, dtype=np.int32).reshape(-1, 4)
    if edges.shape[0] == 0:
        edges = np.zeros((1, 4), np.int32)
    return np.concatenate([edges.reshape(-1), np.ascontiguousarray(polys, dtype=np.int32).reshape(-1)])


def _inside(polys, H, W):
    """OR over the polygons of the even-odd fill: bool [H, W]."""
    out = np.zeros((H, W), bool)
    for poly in polys:
        diff = np.zeros((H, W + 1), np.int64)              # column W collects the toggles that lie right of the scene
        for ring in poly:
            for y0, x0, y1, x1 in _ring_edges(ring):
                dy, dx = y1 - y0, x1 - x0
                first, last = max(-((128 - y0) // FRAC), 0), min(-((128 - y1) // FRAC) - 1, H - 1)
                if first > last:
                    continue
                y = np.arange(first, last + 1, dtype=np.int64)
                num = (x0 - 128) * dy + (FRAC * y + 128 - y0) * dx
                j = np.clip(-((-num) // (FRAC * dy)), 0, W)
                np.add.at(diff, (y, j), 1)
        out |= (np.cumsum(diff[:, :W], axis=1) & 1).astype(bool)
    return out


def aoi_fill_ref(shape, key):
    """aoi before the buffer: u8 [H, W], 0 / 1."""
    H, W = int(shape[0]), int(shape[1])
    aoi = np.ones((H, W), bool) if key.include is None else _inside(key.include, H, W)
    if key.exclude:
        aoi &= ~_inside(key.exclude, H, W)
    return aoi.astype(np.uint8)


def aoi_ref(shape, key, valid=None):
    """The rule on a scene of `shape` = (H, W[, C]) under a SceneAoi key: valid_out, a NEW uint8 [H, W] array of 0 / 1.  valid: the caller's
    mask (bool / uint8 [H, W], non-zero = valid) or None."""
    H, W = int(shape[0]), int(shape[1])
    out = aoi_fill_ref((H, W), key)
    if key.buffer > 0:
        out = grow_ref(out, key.buffer)
    elif key.buffer < 0:
        out = 1 - grow_ref(1 - out, -key.buffer)
    if valid is not None:
        valid = np.asarray(valid)
        if tuple(valid.shape) != (H, W):
            raise ValueError(f"valid must have the scene's shape {(H, W)}, got {tuple(valid.shape)}")
        out = out & (valid != 0)
    return np.ascontiguousarray(out, dtype=np.uint8)
