"""What the SCENE_AOI tests share (tests/test_scene_aoi_host.py, tests/test_gpu_scene_aoi.py): the polygon menu, two independent statements
of the rule (a fractions.Fraction crossing-number brute force from the vertices, and a division-free numpy fill from the edge TABLE), and
the CPU stand-in with a numpy body of the new method.  A plain module (not collected); importing it does not touch the GPU."""
from fractions import Fraction

import numpy as np
import torch

from scene_nodata_kit import NodataStandIn

Q = 256


def quantise(v):
    return int(np.rint(np.float64(v) * Q))


# ---- the rule from the VERTICES, exact rational arithmetic ---------------------------------------------------------------------------------------
def fraction_inside(shape, polygon):
    """bool [H, W]: even-odd over all rings of one polygon (rings of (row, col) floats).  The vertices are quantised to 1 / 256 px as the
    rule says; from there a pixel is inside iff an odd number of non-horizontal edges cross its centre's row (y0 <= yc < y1) with the
    crossing's exact x, a Fraction, at or left of the centre.  No rounding anywhere, no table, none of the library."""
    H, W = shape
    edges = []
    for ring in polygon:
        pts = [(quantise(r), quantise(c)) for r, c in ring]
        for (ya, xa), (yb, xb) in zip(pts, pts[1:] + pts[:1]):
            if ya != yb:
                edges.append((ya, xa, yb, xb) if ya < yb else (yb, xb, ya, xa))
    out = np.zeros((H, W), bool)
    for y in range(H):
        yc = Q * y + Q // 2
        xs = [Fraction(x0) + Fraction((yc - y0) * (x1 - x0), y1 - y0) for y0, x0, y1, x1 in edges if y0 <= yc < y1]
        for x in range(W):
            xc = Q * x + Q // 2
            out[y, x] = sum(1 for s in xs if s <= xc) & 1
    return out


def fraction_ref(shape, include=None, exclude=()):
    aoi = np.ones(shape, bool)
    if include:
        aoi = np.zeros(shape, bool)
        for poly in include:
            aoi |= fraction_inside(shape, poly)
    for poly in exclude:
        aoi &= ~fraction_inside(shape, poly)
    return aoi.astype(np.uint8)


# ---- the rule from the TABLE, without a division ---------------------------------------------------------------------------------------------------
def table_fill(shape, edges, polys, n_include, n_exclude):
    """u8 [H, W] from the tables of aoi_edges: an edge that crosses row y toggles pixel x iff (x0 - 128) dy + (yc - y0) dx <= 256 x dy."""
    H, W = shape
    edges = np.asarray(edges, np.int64).reshape(-1, 4)
    yc = (Q * np.arange(H, dtype=np.int64) + Q // 2)[:, None]
    x = np.arange(W, dtype=np.int64)[None, :]
    inc, exc = np.zeros((H, W), bool) if n_include else np.ones((H, W), bool), np.zeros((H, W), bool)
    for k in range(n_include + n_exclude):
        toggles = np.zeros((H, W), np.int64)
        for y0, x0, y1, x1 in edges[polys[k]:polys[k + 1]].tolist():
            dy, dx = y1 - y0, x1 - x0
            toggles += ((yc >= y0) & (yc < y1)) & ((x0 - Q // 2) * dy + (yc - y0) * dx <= Q * x * dy)
        (inc if k < n_include else exc)[...] |= (toggles & 1).astype(bool)
    return (inc & ~exc).astype(np.uint8)


# ---- the polygon menu ------------------------------------------------------------------------------------------------------------------------------
def circle(cy, cx, r, n=1000):
    a = 2 * np.pi * np.arange(n) / n
    return [[[float(cy + r * np.sin(t)), float(cx + r * np.cos(t))] for t in a]]


def star(H, W, frac, points=7):
    """One polygon, a star around the scene's centre whose area is about frac H W: (row, col) floats.  Area of a 2 n-gon with alternating
    radii R and R / 2 (as fractions of the half axes): n sin(pi / n) R (R / 2) (H / 2) (W / 2)."""
    n = points
    R = np.sqrt(frac * 8.0 / (n * np.sin(np.pi / n)))
    ring = []
    for i in range(2 * n):
        rad, t = (R if i % 2 == 0 else R / 2), np.pi * i / n
        ring.append([float(H / 2 * (1 + rad * np.sin(t))), float(W / 2 * (1 + rad * np.cos(t)))])
    return [ring]


def menu(H, W):
    """name -> SCENE_AOI value, scaled to the scene: the cases of the issue's list."""
    h, w = float(H), float(W)
    box = lambda r0, c0, r1, c1: [[[r0, c0], [r0, c1], [r1, c1], [r1, c0]]]
    return {
        "rect_int": [box(2, 3, 5, 9)],
        "rect_half": [box(2.5, 3.5, 5.5, 9.5)],
        "bowtie": [[[[0.1 * h, 0.1 * w], [0.9 * h, 0.9 * w], [0.1 * h, 0.9 * w], [0.9 * h, 0.1 * w]]]],
        "hole": [[box(0.1 * h, 0.1 * w, 0.9 * h, 0.9 * w)[0], box(0.3 * h, 0.35 * w, 0.6 * h, 0.7 * w)[0]]],
        "union": [box(0.05 * h, 0.05 * w, 0.6 * h, 0.6 * w), [[[0.4 * h, 0.3 * w], [0.95 * h, 0.5 * w], [0.5 * h, 0.97 * w]]]],
        "exclude": {"include": [box(0.1 * h, 0.05 * w, 0.95 * h, 0.9 * w)], "exclude": [[[[0.2 * h, 0.2 * w], [0.8 * h, 0.4 * w], [0.5 * h, 0.8 * w]]]]},
        "exclude_only": {"exclude": [box(0.25 * h, 0.25 * w, 0.75 * h, 0.75 * w)]},
        "sliver": [[[[0.6, 0.1], [0.6, w - 0.1], [0.9, w - 0.1], [0.9, 0.1]]]],              # between two rows of centres: holds none
        "partly_outside": [[[[-0.5 * h, -0.3 * w], [0.7 * h, 0.2 * w], [1.4 * h, 1.5 * w], [0.2 * h, 0.8 * w]]]],
        "wholly_outside": [box(-30.0, -40.0, -2.0, -3.0), box(h + 1, w + 1, h + 20, w + 30)],
        "covers": [box(-5.0, -5.0, h + 5, w + 5)],
        "xy": {"order": "xy", "include": [[[[0.1 * w, 0.2 * h], [0.9 * w, 0.3 * h], [0.5 * w, 0.95 * h]]]]},
        "centre_vertex": [[[[0.5, 0.5], [H + 0.5, W // 2 + 0.5], [H // 2 + 0.5, W + 1.5]]]],      # every vertex on the lattice of pixel centres
        "diagonal": [[[[0.0, 0.0], [min(h, w), min(h, w)], [min(h, w), 0.0]]]],             # its long edge passes exactly through centres
    }


def many_polygons(H, W, n=64):
    """n small boxes on a grid, the odd ones excluded from a big box that is include polygon 0: the polygon limit."""
    per = int(np.ceil(np.sqrt(n)))
    sy, sx = H / per, W / per
    inc, exc = [[[[0.0, 0.0], [0.0, 0.55 * W], [0.8 * H, 0.55 * W], [0.8 * H, 0.0]]]], []
    for k in range(1, n):
        r0, c0 = (k // per) * sy + 0.2 * sy, (k % per) * sx + 0.15 * sx
        (exc if k & 1 else inc).append([[[r0, c0], [r0, c0 + 0.6 * sx], [r0 + 0.55 * sy, c0 + 0.6 * sx], [r0 + 0.55 * sy, c0]]])
    return {"include": inc, "exclude": exc}


def many_edges(H, W, n=16384):
    """One ring of exactly n non-horizontal edges, each crossing rows of the scene: a zigzag of n - 1 vertices between the scene's upper and
    its middle rows (n - 2 edges), closed along a horizontal edge (dropped) near the bottom by two more (the edge limit)."""
    ring = [[(0.05 if i % 2 == 0 else 0.6) * H + (i % 7) / 256.0, (i + 0.5) * W / (n - 1)] for i in range(n - 1)]
    return [[ring + [[0.9 * H, float(W)], [0.9 * H, 0.0]]]]


# ---- the CPU stand-in --------------------------------------------------------------------------------------------------------------------------------
class AoiStandIn(NodataStandIn):
    """The stand-in with the method this feature adds, its body the division-free numpy fill of the TABLE it is handed.  Every call is
    logged: a run without the key must log none."""

    def scene_aoi_fill(self, shape, edges, polys, n_include, n_exclude, and_with=None, invert=False, table_dev=None, out=None):
        from sam_road_amd.aoi import aoi_pack
        edges, polys = np.asarray(edges), np.asarray(polys)
        assert edges.dtype == np.int32 and edges.ndim == 2 and edges.shape[1] == 4 and polys.dtype == np.int32 and polys.shape == (n_include + n_exclude + 1,) and out is None
        assert table_dev is None or (table_dev.dtype == torch.int32 and np.array_equal(table_dev.numpy(), aoi_pack(edges, polys)))
        self.calls.append(("aoi_fill", tuple(shape), int(edges.shape[0]), n_include, n_exclude, and_with is not None, bool(invert)))
        v = table_fill(tuple(shape), edges, polys, n_include, n_exclude).astype(bool)
        if invert:
            v = ~v
        if and_with is not None:
            assert tuple(and_with.shape) == tuple(shape)
            v = v & (and_with.numpy() != 0)
        return torch.from_numpy(np.ascontiguousarray(v.astype(np.uint8)))


def aoi_calls(net):
    return [c for c in net.calls if c[0] == "aoi_fill"]
