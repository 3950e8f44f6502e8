"""GRAPH_RASTER: the one statement of how a road graph becomes a raster — the graph drawn over the scene (the reference's
viz/, triage.py:8-35), the graph as a mask (triage.py:38-71) and the pixel comparison of a predicted graph with a ground-truth one (the
comparison the reference carries commented out, inferencer.py:305-322) — on the host, in integers.  cv2's bytes are NOT reproduced: its
thick lines are fixed-point polygon fills; the rule here is exact and is what the device kernels (csrc/graph_raster.hip) must equal byte
for byte.

    GRAPH_RASTER: {viz:  true | {width: 4, mark: disc, radius: 4, edge_color: [253, 160, 15], node_color: [255, 255, 0]},
                   mask: RHO | {radius: RHO},                    # 1 .. 127
                   diff: true | {thin: 1, wide: 5}}              # 1 <= thin <= wide <= 127
    absent / None / {} / every product absent, None or false: nothing is rendered, nothing is launched.

THE RULE.  Nodes are (row, col) integers; a pixel is the point at its own integer coordinates, the frame the nodes already live in.  A float
node array is truncated toward zero, as the reference's int() does.  Nodes may lie outside the image (ground-truth graphs and the SpaceNet
flip produce such nodes): everything is clipped to [0, H) x [0, W).  For an edge a -> b of width t (int, 1 .. 255) let d = b - a, p = x - a,
u = p . d and L = d . d.  Pixel x is covered iff
    4 (p . p)     <= t^2      when L = 0 or u <= 0       (the end a, or a zero-length edge)
    4 |p - d|^2   <= t^2      when u >= L                (the end b)
    4 (p x d)^2   <= t^2 L    otherwise                  (the inside: the distance to the line)
— the pixel centres within t / 2 of the segment; at t = 1 still an 8-connected line.  A node mark is `none`, `square` (Chebyshev distance
<= r, the reference's rasterize_graph) or `disc` (p . p <= r^2, the reference's viz circle), 0 <= r <= 127.  The CLASS MAP is uint8 [H, W]:
0 background, 1 covered by an edge, 2 covered by a node mark; a node mark wins over an edge.

THE SPAN BOUND.  An edge spans at most MAX_SPAN = 16383 pixels per axis and coordinates lie within +-2^28.  Every covered pixel lies in the
edge's bounding box grown by g = ceil(t / 2) <= 128, so |p| <= 16383 + 128 = 16511 per axis and |d| <= 16383.  Then |u| and |p x d| are at
most 2 * 16511 * 16383 = 540 999 426 < 2^30, L <= 2 * 16383^2 = 536 805 378 < 2^29, p . p and |p - d|^2 <= 2 * 16511^2 < 2^30, and the
largest products are 4 (p x d)^2 <= 1.18e18 < 2^62 and t^2 L <= 65025 * 536 805 378 < 2^45: all inside a signed 64-bit integer.  Longer
edges, coordinates outside +-2^28 and edge indices outside [0, N) are a ValueError here and SRH_ERR_BAD_ARG in the entry.

THE PRODUCTS.
  viz   uint8 [H, W, 3]: the scene with class 1 in the edge colour and class 2 in the node colour.  Defaults are the reference's: width
        4, discs of radius 4, RGB (253, 160, 15) and (255, 255, 0).  A rectangular scene renders at its own size (the reference resizes
        the image to a square of its own height, which leaves a square scene unchanged).  Without a uint8 RGB scene: on black.
  mask  radius rho: the class map at width 2 rho with squares of half-side rho, written as 0 / 255 — rasterize_graph(..., dilation_radius=rho).
  diff  {thin, wide} and a ground-truth graph: pred_thin, pred_wide, gt_thin, gt_wide are the mask products at radius thin / wide;
        fp = pred_thin & ~gt_wide, missed = gt_thin & ~pred_wide.  Four exact counts over the pixels of `valid` (all pixels without one):
        n_pred = #pred_thin, n_fp = #fp, n_gt = #gt_thin, n_missed = #missed; precision = 1 - n_fp / n_pred, recall = 1 - n_missed / n_gt,
        computed on the host from the integers, None for a zero denominator.  The diff image is the scene with the counted fp pixels blue
        (0, 0, 255) and the counted missed pixels red (255, 0, 0), red first in priority.  thin <= wide is required: coverage grows with
        the width and the squares with their half-side, so thin is a subset of wide and a graph compared with itself has no fp and nothing
        missed.

Renders are in the frame the nodes are in; under SCENE_SCALE and SCENE_PAD that is the real scene."""
import collections

import numpy as np

MAX_SPAN = 16383                                          # |b - a| per axis
MAX_COORD = 1 << 28
MAX_WIDTH, MAX_RADIUS = 255, 127
MARKS = ("none", "square", "disc")
EDGE_COLOR, NODE_COLOR = (253, 160, 15), (255, 255, 0)    # triage.py:26,33 (BGR there)
FP_COLOR, MISSED_COLOR = (0, 0, 255), (255, 0, 0)         # inferencer.py:315-317
_KEYS = ("viz", "mask", "diff")
_VIZ_KEYS = ("width", "mark", "radius", "edge_color", "node_color")

VizStyle = collections.namedtuple("VizStyle", "width mark radius edge_color node_color")
VIZ_DEFAULT = VizStyle(4, "disc", 4, EDGE_COLOR, NODE_COLOR)
# viz: a VizStyle or None; mask: the radius rho or None; diff: (thin, wide) or None
GraphRaster = collections.namedtuple("GraphRaster", "viz mask diff")


def _is_int(v):
    return isinstance(v, (int, np.integer)) and not isinstance(v, (bool, np.bool_))


def _off(v):
    return v is None or v is False or (isinstance(v, dict) and not v)


def _colour(name, v):
    if not isinstance(v, (list, tuple)) or len(v) != 3 or not all(_is_int(c) and 0 <= c <= 255 for c in v):
        raise ValueError(f"GRAPH_RASTER: {name} must be three ints 0 .. 255 [r, g, b], got {v!r}")
    return tuple(int(c) for c in v)


def check_style(width, mark, radius):
    """ValueError unless width is an int 1 .. 255, mark one of none / square / disc and radius an int 0 .. 127."""
    if not _is_int(width) or not 1 <= width <= MAX_WIDTH:
        raise ValueError(f"GRAPH_RASTER: a width must be an int 1 .. {MAX_WIDTH}, got {width!r}")
    if not isinstance(mark, str) or mark not in MARKS:
        raise ValueError(f"GRAPH_RASTER: a mark must be one of {', '.join(MARKS)}, got {mark!r}")
    if not _is_int(radius) or not 0 <= radius <= MAX_RADIUS:
        raise ValueError(f"GRAPH_RASTER: a radius must be an int 0 .. {MAX_RADIUS}, got {radius!r}")


def _radius(name, v):
    if not _is_int(v) or not 1 <= v <= MAX_RADIUS:
        raise ValueError(f"GRAPH_RASTER: {name} must be an int 1 .. {MAX_RADIUS}, got {v!r}")
    return int(v)


def graph_raster_key_of(v):
    """A GRAPH_RASTER value (the mapping of the module's docstring) as a GraphRaster tuple; None when nothing is to be rendered.
    ValueError for anything else: unknown keys, a width / radius / colour outside its range, an unknown mark, thin > wide."""
    if _off(v):
        return None
    if isinstance(v, GraphRaster):
        return v
    if not isinstance(v, dict):
        raise ValueError(f"GRAPH_RASTER must be a mapping with viz / mask / diff, got {v!r}")
    unknown = sorted(set(v) - set(_KEYS), key=str)
    if unknown:
        raise ValueError(f"GRAPH_RASTER: unknown key {unknown[0]!r} ({', '.join(_KEYS)})")
    viz = v.get("viz")
    if _off(viz):
        viz = None
    elif viz is True:
        viz = VIZ_DEFAULT
    elif isinstance(viz, dict):
        unknown = sorted(set(viz) - set(_VIZ_KEYS), key=str)
        if unknown:
            raise ValueError(f"GRAPH_RASTER: unknown key {unknown[0]!r} of viz ({', '.join(_VIZ_KEYS)})")
        mark = viz.get("mark", VIZ_DEFAULT.mark)
        mark = mark.strip().lower() if isinstance(mark, str) else mark
        check_style(viz.get("width", VIZ_DEFAULT.width), mark, viz.get("radius", VIZ_DEFAULT.radius))
        viz = VizStyle(int(viz.get("width", VIZ_DEFAULT.width)), mark, int(viz.get("radius", VIZ_DEFAULT.radius)),
                       _colour("edge_color", viz.get("edge_color", EDGE_COLOR)), _colour("node_color", viz.get("node_color", NODE_COLOR)))
    else:
        raise ValueError(f"GRAPH_RASTER: viz must be true or a mapping with {', '.join(_VIZ_KEYS)}, got {viz!r}")
    mask = v.get("mask")
    if _off(mask):
        mask = None
    elif isinstance(mask, dict):
        if set(mask) != {"radius"}:
            raise ValueError(f"GRAPH_RASTER: mask must be a radius or {{radius: RHO}}, got {mask!r}")
        mask = _radius("the radius of mask", mask["radius"])
    else:
        mask = _radius("the radius of mask", mask)
    diff = v.get("diff")
    if _off(diff):
        diff = None
    elif diff is True:
        diff = (1, 5)
    elif isinstance(diff, dict):
        unknown = sorted(set(diff) - {"thin", "wide"}, key=str)
        if unknown:
            raise ValueError(f"GRAPH_RASTER: unknown key {unknown[0]!r} of diff (thin, wide)")
        diff = (_radius("thin", diff.get("thin", 1)), _radius("wide", diff.get("wide", 5)))
    else:
        raise ValueError(f"GRAPH_RASTER: diff must be true or {{thin: T, wide: W}}, got {diff!r}")
    if diff is not None and diff[0] > diff[1]:
        raise ValueError(f"GRAPH_RASTER: thin <= wide is required (a graph compared with itself must have no false positive), got thin {diff[0]}, wide {diff[1]}")
    if viz is None and mask is None and diff is None:
        return None
    return GraphRaster(viz, mask, diff)


def graph_raster_key(config):
    """config.GRAPH_RASTER as a GraphRaster tuple, None without the key; ValueError before any device is touched."""
    return graph_raster_key_of(config.get("GRAPH_RASTER"))


def graph_raster_override(config, viz=None, mask=None, diff=None):
    """The GRAPH_RASTER mapping with the CLI's flags laid over the config's key: viz True switches the viz product on (the config's style
    stays), mask an int replaces the radius, diff True switches the comparison on (the config's thin / wide stay) and a (thin, wide) pair
    replaces them.  The result is validated."""
    base = config.get("GRAPH_RASTER")
    graph_raster_key_of(base)
    out = dict(base) if isinstance(base, dict) else {}
    if viz and _off(out.get("viz")):
        out["viz"] = True
    if mask is not None:
        out["mask"] = {"radius": mask}
    if diff is True and _off(out.get("diff")):
        out["diff"] = True
    elif diff is not None and diff is not True:
        if len(diff) != 2:
            raise ValueError(f"GRAPH_RASTER: --diff takes no value or THIN WIDE, got {diff!r}")
        out["diff"] = {"thin": diff[0], "wide": diff[1]}
    graph_raster_key_of(out)
    return out


# ---- the graph -------------------------------------------------------------------------------------------------------------------------------
def check_graph(nodes, edges):
    """(nodes int32 [N, 2], edges int32 [E, 2]), contiguous, as the device takes them.  A float node array is truncated toward zero (the
    reference's int()).  ValueError for a shape other than [N, 2] / [E, 2], a non-finite coordinate or one outside +-2^28, a non-integer
    edge array, an edge index outside [0, N) or an edge spanning more than MAX_SPAN pixels on an axis."""
    n = np.asarray(nodes)
    if n.size == 0:
        n = np.zeros((0, 2), np.int32)
    if n.ndim != 2 or n.shape[1] != 2 or n.dtype.kind not in "iuf":
        raise ValueError(f"GRAPH_RASTER: nodes must be a numeric [N, 2] array of (row, col), got {n.dtype} {n.shape}")
    if n.dtype.kind == "f":
        if not np.isfinite(n).all():
            raise ValueError("GRAPH_RASTER: a node coordinate is not finite")
        n = np.trunc(n)
    if n.size and (n.min() < -MAX_COORD or n.max() > MAX_COORD):
        raise ValueError("GRAPH_RASTER: a node coordinate lies outside +-2^28")
    n = np.ascontiguousarray(n.astype(np.int32))
    e = np.asarray(edges)
    if e.size == 0:
        e = np.zeros((0, 2), np.int32)
    if e.ndim != 2 or e.shape[1] != 2 or e.dtype.kind not in "iu":
        raise ValueError(f"GRAPH_RASTER: edges must be an integer [E, 2] array of node indices, got {e.dtype} {e.shape}")
    if e.size and (e.min() < 0 or e.max() >= n.shape[0]):
        raise ValueError(f"GRAPH_RASTER: an edge index lies outside [0, {n.shape[0]})")
    e = np.ascontiguousarray(e.astype(np.int32))
    if e.size:
        span = np.abs(n[e[:, 1]].astype(np.int64) - n[e[:, 0]].astype(np.int64)).max()
        if span > MAX_SPAN:
            raise ValueError(f"GRAPH_RASTER: an edge spans {int(span)} pixels on an axis, at most {MAX_SPAN} (with it every product of the rule fits 64 bits)")
    return n, e


def _check_shape(shape):
    H, W = int(shape[0]), int(shape[1])
    if H < 1 or W < 1 or H * W > 2 ** 31 - 1:
        raise ValueError(f"GRAPH_RASTER: the image must have at least 1 x 1 and at most 2^31 - 1 pixels, got {H} x {W}")
    return H, W


def graph_raster_ref(nodes, edges, shape, width, mark="none", radius=0, values=(1, 2)):
    """THE RULE of the module's docstring on the host: the class map uint8 [H, W] (values = (edge byte, node byte), (1, 2) by default)."""
    H, W = _check_shape(shape)
    n, e = check_graph(nodes, edges)
    check_style(width, mark, radius)
    out = np.zeros((H, W), np.uint8)
    n = n.astype(np.int64)
    t, g, tt = int(width), (int(width) + 1) // 2, int(width) * int(width)
    for ia, ib in e.tolist():
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
        out[y0:y1 + 1, x0:x1 + 1][cov] = values[0]
    if mark != "none":
        r = int(radius)
        for ar, ac in n.tolist():
            y0, y1, x0, x1 = max(ar - r, 0), min(ar + r, H - 1), max(ac - r, 0), min(ac + r, W - 1)
            if y0 > y1 or x0 > x1:
                continue
            if mark == "square":
                out[y0:y1 + 1, x0:x1 + 1] = values[1]
            else:
                pr = (np.arange(y0, y1 + 1, dtype=np.int64) - ar)[:, None]
                pc = (np.arange(x0, x1 + 1, dtype=np.int64) - ac)[None, :]
                out[y0:y1 + 1, x0:x1 + 1][pr * pr + pc * pc <= r * r] = values[1]
    return out


def graph_mask_ref(nodes, edges, shape, radius):
    """The mask product on the host: 0 / 255, width 2 rho, squares of half-side rho."""
    return graph_raster_ref(nodes, edges, shape, 2 * radius, "square", radius, values=(255, 255))


def composite_ref(cls, img=None, edge_color=EDGE_COLOR, node_color=NODE_COLOR, background=(0, 0, 0)):
    """The viz composition on the host: uint8 [H, W, 3]."""
    out = np.empty(cls.shape + (3,), np.uint8)
    out[:] = np.asarray(background, np.uint8) if img is None else img
    out[cls == 1] = np.asarray(edge_color, np.uint8)
    out[cls >= 2] = np.asarray(node_color, np.uint8)
    return out


def metrics(counts):
    """{n_pred, n_fp, n_gt, n_missed, precision, recall} from the four integers; a ratio with a zero denominator is None."""
    n_pred, n_fp, n_gt, n_missed = (int(c) for c in counts)
    return dict(n_pred=n_pred, n_fp=n_fp, n_gt=n_gt, n_missed=n_missed, precision=None if n_pred == 0 else 1 - n_fp / n_pred,
                recall=None if n_gt == 0 else 1 - n_missed / n_gt)


def compare_ref(pred, gt, shape, thin=1, wide=5, valid=None, img=None, diff=True):
    """The diff product on the host: (metrics, diff image uint8 [H, W, 3] or None).  pred and gt are (nodes, edges)."""
    if not (_is_int(thin) and _is_int(wide) and 1 <= thin <= wide <= MAX_RADIUS):
        raise ValueError(f"GRAPH_RASTER: 1 <= thin <= wide <= {MAX_RADIUS} is required, got thin {thin!r}, wide {wide!r}")
    pt, pw, gtn, gw = (graph_mask_ref(*g, shape, r) != 0 for g, r in ((pred, thin), (pred, wide), (gt, thin), (gt, wide)))
    v = np.ones(pt.shape, bool) if valid is None else np.asarray(valid) != 0
    fp, missed = pt & ~gw & v, gtn & ~pw & v
    m = metrics(((pt & v).sum(), fp.sum(), (gtn & v).sum(), missed.sum()))
    if not diff:
        return m, None
    out = np.zeros(pt.shape + (3,), np.uint8) if img is None else np.array(img, np.uint8)
    out[fp] = np.asarray(FP_COLOR, np.uint8)
    out[missed] = np.asarray(MISSED_COLOR, np.uint8)
    return m, out


def read_gt_graph(path, spacenet=False):
    """A sat2graph pickle (formats.convert_from_sat2graph_format) as (nodes int [N, 2] (row, col), edges [E, 2]).  spacenet: the reference's
    coordinate handling (inferencer.py:289-292), (row, col) = (400 - n0, n1)."""
    import pickle
    from .formats import convert_from_sat2graph_format
    with open(path, "rb") as f:
        nodes, edges = convert_from_sat2graph_format(pickle.load(f))
    nodes = np.asarray(nodes).reshape(-1, 2)
    if spacenet and nodes.shape[0]:
        nodes = np.stack([400 - nodes[:, 0], nodes[:, 1]], axis=1)
    return nodes, np.asarray(edges, np.int64).reshape(-1, 2)


# ---- the device ------------------------------------------------------------------------------------------------------------------------------
def _ops(device, net):
    if net is not None:
        return net
    from .model import DeviceGraphOps
    return DeviceGraphOps("cuda" if device is None else device)


def _scene(img, shape, device):
    """img (uint8 [H, W, 3], numpy or a tensor on the device) as a device tensor, or None."""
    import torch
    if img is None:
        return None
    if not torch.is_tensor(img):
        img = np.asarray(img)
        if img.dtype != np.uint8 or img.shape != (shape[0], shape[1], 3):
            raise ValueError(f"GRAPH_RASTER: the scene must be uint8 [{shape[0]}, {shape[1]}, 3], got {img.dtype} {img.shape}")
        img = torch.from_numpy(np.ascontiguousarray(img)).to(device)
    return img


def rasterize_graph(nodes, edges, shape, width=VIZ_DEFAULT.width, mark="none", radius=0, values=(1, 2), device=None, net=None):
    """The class map on the device (srh_graph_raster): a uint8 [H, W] tensor equal to graph_raster_ref byte for byte.  net: the model whose
    device is used; without one the device `device` (default cuda)."""
    H, W = _check_shape(shape)
    return _ops(device, net).graph_raster((H, W), nodes, edges, width, mark, radius, values=values)


def render_mask(nodes, edges, shape, radius, device=None, net=None):
    """The mask product on the device: uint8 [H, W] of 0 / 255."""
    return rasterize_graph(nodes, edges, shape, 2 * _radius("the radius of mask", radius), "square", radius, (255, 255), device, net)


def render_viz(img, nodes, edges, width=VIZ_DEFAULT.width, mark=VIZ_DEFAULT.mark, radius=VIZ_DEFAULT.radius, edge_color=EDGE_COLOR,
               node_color=NODE_COLOR, shape=None, device=None, net=None):
    """The viz product on the device: uint8 [H, W, 3].  img: the scene, uint8 [H, W, 3] (numpy or a device tensor), or None with a shape:
    the graph on black."""
    ops = _ops(device, net)
    shape = tuple(img.shape[:2]) if img is not None else shape
    cls = ops.graph_raster(_check_shape(shape), nodes, edges, width, mark, radius)
    return ops.graph_composite(cls, _scene(img, shape, cls.device), _colour("edge_color", edge_color), _colour("node_color", node_color))


def compare_graphs(pred, gt, shape, thin=1, wide=5, valid=None, img=None, diff=None, device=None, net=None):
    """The diff product on the device: (metrics, diff image tensor uint8 [H, W, 3] or None).  pred and gt are (nodes, edges); valid uint8 /
    bool [H, W] (numpy or a device tensor) or None; diff: make the image (default: iff img is given).  The four counts are summed on the
    device and read back here, 32 bytes."""
    import torch
    if not (_is_int(thin) and _is_int(wide) and 1 <= thin <= wide <= MAX_RADIUS):
        raise ValueError(f"GRAPH_RASTER: 1 <= thin <= wide <= {MAX_RADIUS} is required, got thin {thin!r}, wide {wide!r}")
    H, W = _check_shape(shape)
    pred, gt = check_graph(*pred), check_graph(*gt)
    ops = _ops(device, net)
    maps = [ops.graph_raster((H, W), *g, 2 * r, "square", r, values=(255, 255)) for g, r in ((pred, thin), (pred, wide), (gt, thin), (gt, wide))]
    dev = maps[0].device
    if valid is not None and not torch.is_tensor(valid):
        valid = np.asarray(valid)
        if valid.shape != (H, W) or valid.dtype not in (np.uint8, np.bool_):
            raise ValueError(f"GRAPH_RASTER: valid must be uint8 / bool [{H}, {W}], got {valid.dtype} {valid.shape}")
        valid = torch.from_numpy(np.ascontiguousarray(valid)).to(dev)
    counts, image = ops.graph_compare(*maps, valid=valid, img=_scene(img, (H, W), dev), diff=img is not None if diff is None else bool(diff))
    return metrics(counts.cpu().tolist()), image


def render(key, nodes, edges, shape, img=None, gt=None, valid=None, device=None, net=None):
    """Every product the key asks for, as host arrays: {"viz": uint8 [H, W, 3], "mask": uint8 [H, W], "diff": uint8 [H, W, 3],
    "metrics": {...}} — diff and metrics only with a ground-truth graph gt = (nodes, edges).  The scene is uploaded once.  Runs on torch's
    current stream and waits for that stream alone."""
    out = {}
    if key is None:
        return out
    H, W = _check_shape(shape)
    ops = _ops(device, net)
    if img is not None and (img.dtype != np.uint8 or tuple(img.shape) != (H, W, 3)):
        img = None                                        # a raw multi-band / 16-bit / float scene has no RGB to draw on: black
    scene = None
    if key.viz is not None:
        cls = ops.graph_raster((H, W), nodes, edges, key.viz.width, key.viz.mark, key.viz.radius)
        scene = _scene(img, (H, W), cls.device)
        out["viz"] = ops.graph_composite(cls, scene, key.viz.edge_color, key.viz.node_color).cpu().numpy()
    if key.mask is not None:
        out["mask"] = render_mask(nodes, edges, (H, W), key.mask, net=ops).cpu().numpy()
    if key.diff is not None and gt is not None:
        m, image = compare_graphs((nodes, edges), gt, (H, W), key.diff[0], key.diff[1], valid=valid, img=scene if scene is not None else img,
                                  diff=True, net=ops)
        out["metrics"], out["diff"] = m, image.cpu().numpy()
    return out


def total_metrics(per_scene):
    """The totals over scenes: the counts summed, precision and recall from the sums."""
    keys = ("n_pred", "n_fp", "n_gt", "n_missed")
    return metrics([sum(m[k] for m in per_scene) for k in keys])
