"""What the GRAPH_RASTER tests share: graphs, independent restatements of the rule (exact rationals; float64), the CPU stand-in with the
three methods the feature adds, and the numpy statement of the comparison.  A plain module (not collected); importing it does not touch
the GPU."""
from fractions import Fraction

import numpy as np
import torch

from scene_kit import SceneStandIn

from sam_road_amd.graph_raster import EDGE_COLOR, NODE_COLOR, composite_ref, graph_raster_ref


# ---- graphs ----------------------------------------------------------------------------------------------------------------------------------
def random_graph(rng, H, W, n_nodes, n_edges, margin=8, zero_length=2):
    """(nodes int64 [N, 2], edges int64 [E, 2]): nodes up to `margin` pixels outside the image, the first `zero_length` edges of length 0."""
    nodes = np.stack([rng.integers(-margin, H + margin, n_nodes), rng.integers(-margin, W + margin, n_nodes)], axis=1)
    edges = rng.integers(0, n_nodes, (n_edges, 2))
    edges[:zero_length, 1] = edges[:zero_length, 0]
    return nodes.astype(np.int64), edges.astype(np.int64)


def star(H, W, n=500, seed=3):
    """n edges from one node near the centre to n nodes around it: many writers on the pixels at the hub."""
    rng = np.random.default_rng(seed)
    ang = rng.uniform(0, 2 * np.pi, n)
    rad = rng.uniform(2, 0.6 * max(H, W), n)
    nodes = np.concatenate([[[H // 2, W // 2]], np.stack([H // 2 + rad * np.sin(ang), W // 2 + rad * np.cos(ang)], axis=1).astype(np.int64)])
    return nodes.astype(np.int64), np.stack([np.zeros(n, np.int64), np.arange(1, n + 1)], axis=1)


def grid_graph(H, W, step=24, jitter=5, seed=5):
    """A synthetic road grid: nodes on a jittered lattice, edges to the right and the lower neighbour."""
    rng = np.random.default_rng(seed)
    rows, cols = np.arange(step // 2, H, step), np.arange(step // 2, W, step)
    rr, cc = np.meshgrid(rows, cols, indexing="ij")
    nodes = np.stack([rr + rng.integers(-jitter, jitter + 1, rr.shape), cc + rng.integers(-jitter, jitter + 1, cc.shape)], axis=-1).reshape(-1, 2)
    idx = np.arange(nodes.shape[0]).reshape(rr.shape)
    edges = np.concatenate([np.stack([idx[:, :-1].ravel(), idx[:, 1:].ravel()], axis=1), np.stack([idx[:-1].ravel(), idx[1:].ravel()], axis=1)])
    return nodes.astype(np.int64), edges.astype(np.int64)


# ---- the rule, restated --------------------------------------------------------------------------------------------------------------------
def dist2_fraction(a, b, x):
    """The squared distance of point x to the segment a b, as an exact rational."""
    d = (b[0] - a[0], b[1] - a[1])
    L = d[0] * d[0] + d[1] * d[1]
    s = Fraction(0) if L == 0 else min(max(Fraction((x[0] - a[0]) * d[0] + (x[1] - a[1]) * d[1], L), Fraction(0)), Fraction(1))
    q = (a[0] + s * d[0], a[1] + s * d[1])
    return (x[0] - q[0]) ** 2 + (x[1] - q[1]) ** 2


def brute_raster(nodes, edges, shape, t, mark="none", r=0):
    """The class map by brute force over every pixel and every edge: distance^2 to the segment against t^2 / 4 in fractions.Fraction."""
    H, W = shape
    out = np.zeros((H, W), np.uint8)
    nodes, lim = [tuple(int(v) for v in n) for n in np.asarray(nodes).tolist()], Fraction(t * t, 4)
    for a, b in np.asarray(edges).tolist():
        for y in range(H):
            for x in range(W):
                if dist2_fraction(nodes[a], nodes[b], (y, x)) <= lim:
                    out[y, x] = 1
    if mark != "none":
        for ar, ac in nodes:
            for y in range(H):
                for x in range(W):
                    if (max(abs(y - ar), abs(x - ac)) <= r) if mark == "square" else ((y - ar) ** 2 + (x - ac) ** 2 <= r * r):
                        out[y, x] = 2
    return out


def float_distance(nodes, edges, shape):
    """float64 [H, W]: every pixel's distance to the nearest edge of the graph (inf without edges)."""
    H, W = shape
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    best = np.full((H, W), np.inf)
    nodes = np.asarray(nodes, np.float64)
    for a, b in np.asarray(edges).tolist():
        d = nodes[b] - nodes[a]
        L = float(d @ d)
        s = np.zeros((H, W)) if L == 0 else np.clip(((yy - nodes[a][0]) * d[0] + (xx - nodes[a][1]) * d[1]) / L, 0.0, 1.0)
        best = np.minimum(best, np.hypot(yy - (nodes[a][0] + s * d[0]), xx - (nodes[a][1] + s * d[1])))
    return best


def np_compare(pt, pw, gt, gw, valid=None, img=None):
    """The comparison in numpy from four maps: ([n_pred, n_fp, n_gt, n_missed], diff image)."""
    v = np.ones(pt.shape, bool) if valid is None else np.asarray(valid) != 0
    pred, truth = (pt != 0) & v, (gt != 0) & v
    fp, missed = pred & (gw == 0), truth & (pw == 0)
    out = np.zeros(pt.shape + (3,), np.uint8) if img is None else img.copy()
    out[fp] = (0, 0, 255)
    out[missed] = (255, 0, 0)
    return [int(pred.sum()), int(fp.sum()), int(truth.sum()), int(missed.sum())], out


# ---- the CPU stand-in --------------------------------------------------------------------------------------------------------------------------
class RasterStandIn(SceneStandIn):
    """The stand-in with the three methods this feature adds, on the host statement of the rule.  Every call is logged: a run without the
    key must log none."""

    def graph_raster(self, shape, nodes, edges, width, mark="none", radius=0, values=(1, 2), out=None):
        assert out is None
        self.calls.append(("graph_raster", tuple(shape), int(width), mark, int(radius), tuple(values)))
        return torch.from_numpy(graph_raster_ref(nodes, edges, shape, width, mark, radius, values))

    def graph_composite(self, cls, img=None, edge_color=EDGE_COLOR, node_color=NODE_COLOR, background=(0, 0, 0), out=None):
        assert out is None
        self.calls.append(("graph_composite", tuple(cls.shape), img is not None))
        return torch.from_numpy(composite_ref(cls.numpy(), None if img is None else img.numpy(), edge_color, node_color, background))

    def graph_compare(self, pred_thin, pred_wide, gt_thin, gt_wide, valid=None, img=None, diff=False):
        self.calls.append(("graph_compare", tuple(pred_thin.shape), valid is not None, img is not None, bool(diff)))
        counts, image = np_compare(pred_thin.numpy(), pred_wide.numpy(), gt_thin.numpy(), gt_wide.numpy(), None if valid is None else valid.numpy(),
                                   None if img is None else img.numpy())
        return torch.tensor(counts, dtype=torch.int64), torch.from_numpy(image) if diff else None


def raster_calls(net):
    return [c for c in net.calls if c[0].startswith("graph_")]
