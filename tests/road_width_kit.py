"""What the ROAD_WIDTH tests share: the masks at which a distance map can go wrong, independent restatements of the rule (a brute force over
every pair of pixels; scipy's exact Euclidean transform), and the CPU stand-in with the two methods the feature adds.  A plain module (not
collected); importing it does not touch the GPU."""
import math

import numpy as np
import torch

import edge_support_kit as ek
from edge_support_kit import grid_graph, random_graph, star  # noqa: F401

from sam_road_amd.road_width import road_dist_ref, road_width_ref

# the sizes of the kernels' own tiling (csrc/road_width_piece.hpp), restated: a test at these sizes and one off them crosses every boundary
COL_ROWS, COL_STRIP, ROW_SEG = 32, 256, 1024


# ---- masks ---------------------------------------------------------------------------------------------------------------------------------
def level_values(on_level):
    """(a background value, a road value) for this level; road is None at 255, where nothing is road."""
    return on_level, None if on_level == 255 else on_level + 1


def random_mask(rng, H, W, on_level, density=0.9):
    """Road with probability `density`; both sides of the level take every value they have."""
    road = rng.random((H, W)) < density
    lo = rng.integers(0, on_level + 1, (H, W))
    hi = rng.integers(min(on_level + 1, 255), 256, (H, W))
    return np.where(road, hi, lo).astype(np.uint8)


def solid_with_holes(H, W, on_level):
    """All road but single background pixels at the four corners, at the centre and on either side of the chunk / strip / segment
    boundaries of both passes: the circle dx^2 + dy^2 = R^2 lies exactly on the cap, R^2 + 1 exactly behind it, across workgroups."""
    bg, road = level_values(on_level)
    m = np.full((H, W), bg if road is None else road, np.uint8)
    ys = {0, H - 1, H // 2, COL_ROWS - 1, COL_ROWS, 2 * COL_ROWS}
    xs = {0, W - 1, W // 2, COL_STRIP - 1, COL_STRIP, ROW_SEG - 3, ROW_SEG}
    for y, x in [(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1), (H // 2, W // 2)] + [(y, x) for y in sorted(ys) for x in sorted(xs) if (y + x) % 5 == 0]:
        if 0 <= y < H and 0 <= x < W:
            m[y, x] = bg
    return m


def shape_mask(kind, half, H, W):
    """A horizontal and a vertical bar ("bars"), a disc or a cross of half-width `half` (thickness 2 half + 1) around the centre, 0 / 255."""
    yy, xx = np.mgrid[0:H, 0:W]
    cy, cx = H // 2, W // 2
    if kind == "bars":
        m = (np.abs(yy - cy) <= half) | (np.abs(xx - W // 4) <= half)
    elif kind == "disc":
        m = (yy - cy) ** 2 + (xx - cx) ** 2 <= half * half
    elif kind == "cross":
        m = (np.abs(yy - cy) <= half) | (np.abs(xx - cx) <= half)
    else:
        raise KeyError(kind)
    return (m * 255).astype(np.uint8)


# ---- the rule, restated --------------------------------------------------------------------------------------------------------------------
def brute_dist(mask, on_level, R):
    """uint16 [H, W] by brute force: for every road pixel the squared distance to every background pixel of the image, in Python ints."""
    H, W = mask.shape
    bg = [(y, x) for y in range(H) for x in range(W) if mask[y, x] <= on_level]
    out = np.zeros((H, W), np.uint16)
    for y in range(H):
        for x in range(W):
            if mask[y, x] > on_level:
                out[y, x] = min([R * R] + [(y - by) ** 2 + (x - bx) ** 2 for by, bx in bg])
    return out


def scipy_dist(mask, on_level, R):
    """uint16 [H, W] from scipy's exact Euclidean transform; the mask must have a background pixel (without one scipy's result is not defined
    by the rule)."""
    from scipy.ndimage import distance_transform_edt
    F = mask > on_level
    assert not F.all()
    return np.minimum(np.rint(distance_transform_edt(F) ** 2), R * R).astype(np.uint16)


def brute_widths(nodes, edges, d2, R):
    """int64 [E, 8] from graph_raster_kit.brute_raster of every edge ALONE at width 1 and plain Python over its pixels."""
    H, W = d2.shape
    out = np.zeros((len(edges), 8), np.int64)
    for k, e in enumerate(np.asarray(edges).tolist()):
        vals = [int(v) for v in d2[ek.gk.brute_raster(nodes, [e], (H, W), 1) == 1].tolist()]
        inside = [v for v in vals if v > 0]
        out[k, :6] = (len(vals), len(inside), sum(math.isqrt(256 * v) for v in vals), sum(v == R * R for v in vals), min(inside, default=0), max(vals, default=0))
    return out


# ---- the CPU stand-in --------------------------------------------------------------------------------------------------------------------------
class WidthStandIn(ek.SupportStandIn):
    """The stand-in with road_dist and graph_edge_widths on the host statement of the rule.  Every call is logged: a run without the key
    must log none."""

    def road_dist(self, mask, on_level=127, radius=32):
        mask = mask.numpy() if torch.is_tensor(mask) else np.asarray(mask)
        self.calls.append(("road_dist", tuple(mask.shape), int(on_level), int(radius)))
        return torch.from_numpy(road_dist_ref(mask, on_level, radius))

    def graph_edge_widths(self, nodes, edges, d2, radius=32):
        d2 = d2.numpy() if torch.is_tensor(d2) else np.asarray(d2)
        self.calls.append(("graph_edge_widths", tuple(d2.shape), int(radius)))
        H, W = d2.shape
        return torch.from_numpy(road_width_ref(nodes, edges, np.zeros((H, W), np.uint8), 0, radius, d2=d2))


def width_calls(net):
    return [c for c in net.calls if c[0] in ("road_dist", "graph_edge_widths")]
