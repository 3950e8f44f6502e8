"""SCENE_SCALE: the one statement of the resampling rule, on the host, in integers.

A scene at another ground resolution than the model's is resampled by the fraction p/q (model pixels per scene pixel, reduced, 1 <= p, q
<= 16, 1/8 <= p/q <= 4) in front of pass 1, and the masks are resampled back by q/p behind it.  Everything here is exact: the device
kernel (csrc/scene_scale.hip) reads the tables built here and must equal resample_ref byte for byte, so a run with the key equals the
existing pipeline on resample_ref(scene), bit for bit.  No float enters the rule.

Per axis an input of n pixels becomes n_out = ceil(n p / q) pixels (or the n_out that is given: the way back to the scene's own size).
Output pixel j has a start index s[j] and T integer weights w[j][0..T) that sum to D; tap t reads input clamp(s[j] + t, 0, n - 1).

  p < q, area:      on a lattice where an input pixel is p long and an output pixel q long, s[j] = (j q) // p,
                    w[j][t] = |[j q, (j + 1) q) ∩ [(s[j] + t) p, (s[j] + t + 1) p)|, D = q, T = ceil(q / p) + 1
  p > q, bilinear   at pixel centres: num = (2 j + 1) q - p, D = 2 p, s[j] = floor(num / D) (-1 at the border: the clamp handles it),
                    f = num - s[j] D, w[j] = (D - f, f), T = 2
  2-D:              out = (sum_y sum_x wy wx v + (Dy Dx) // 2) // (Dy Dx) per channel — ONE rounding; the sum is at most 255 * 1024
  validity masks:   an output pixel is valid iff every tap with a non-zero weight is valid, on both axes
  nodes:            a graph point at model-frame (r, c) is reported at scene-frame (min(H - 1, ((2 r + 1) q) // (2 p)), the same for c):
                    one of the point's own non-zero taps of the way back, so under the validity rule no node lies on nodata
"""
import math

import numpy as np

SCALE_MAX_TERM = 16                     # 1 <= p, q <= 16
SCALE_RANGE = ((1, 8), (4, 1))          # 1/8 <= p/q <= 4
_GSD_KEYS = ("scene_gsd", "model_gsd")


def _absent(v):
    return v is None or (isinstance(v, dict) and not v)


def _is_int(v):
    return isinstance(v, (int, np.integer)) and not isinstance(v, (bool, np.bool_))


def _is_num(v):
    return (_is_int(v) or isinstance(v, (float, np.floating))) and math.isfinite(float(v))


def _reduced(p, q, what):
    """(p, q) reduced and inside the limits, or ValueError."""
    g = math.gcd(p, q)
    p, q = p // g, q // g
    (lo_p, lo_q), (hi_p, hi_q) = SCALE_RANGE
    if not (1 <= p <= SCALE_MAX_TERM and 1 <= q <= SCALE_MAX_TERM) or p * lo_q < lo_p * q or p * hi_q > hi_p * q:
        raise ValueError(f"SCENE_SCALE: {what} reduces to {p}/{q}; the fraction must have 1 <= p, q <= {SCALE_MAX_TERM} and lie in [1/8, 4]")
    return p, q


def _from_gsd(a, b):
    """The fraction inside the limits that equals a / b to 1e-9 relative, or ValueError asking for [p, q]."""
    r = float(a) / float(b)
    for q in range(1, SCALE_MAX_TERM + 1):
        p = int(round(r * q))
        if 1 <= p <= SCALE_MAX_TERM and abs(p / q - r) <= 1e-9 * r:
            return _reduced(p, q, f"scene_gsd / model_gsd = {a!r} / {b!r}")
    raise ValueError(f"SCENE_SCALE: scene_gsd / model_gsd = {a!r} / {b!r} is no fraction p/q with 1 <= p, q <= {SCALE_MAX_TERM}; give the "
                     f"scale as [p, q] (model pixels per scene pixel)")


def scene_scale_key(config):
    """config.SCENE_SCALE (extension key) as the reduced fraction (p, q), model pixels per scene pixel, or None for a missing
    key, None and a scale that reduces to 1/1: nothing changes anywhere.  [p, q]: two ints >= 1; or a mapping {scene_gsd: a, model_gsd: b}
    (two positive numbers, model_gsd default 1.0) whose quotient equals such a fraction to 1e-9 relative.  ValueError — before the device
    is touched — for anything else, unknown mapping keys included, for a fraction outside 1 <= p, q <= 16 and [1/8, 4], for NMS radii so
    small that two graph points could map to one scene pixel (min(ITSC_NMS_RADIUS, ROAD_NMS_RADIUS) q < 2 p), and together with
    SCENE_GROUP > 1."""
    v = config.SCENE_SCALE
    if _absent(v):
        return None
    if isinstance(v, dict):
        unknown = sorted(set(v) - set(_GSD_KEYS), key=str)
        if unknown:
            raise ValueError(f"SCENE_SCALE: unknown key {unknown[0]!r} (scene_gsd, model_gsd)")
        a, b = v.get("scene_gsd"), v.get("model_gsd", 1.0)
        if not (_is_num(a) and _is_num(b) and a > 0 and b > 0):
            raise ValueError(f"SCENE_SCALE: scene_gsd and model_gsd must be positive numbers, got {v.get('scene_gsd')!r} and {b!r}")
        p, q = _from_gsd(a, b)
    elif isinstance(v, (list, tuple)) and len(v) == 2 and all(_is_int(x) and x >= 1 for x in v):
        p, q = _reduced(int(v[0]), int(v[1]), f"[{v[0]}, {v[1]}]")
    else:
        raise ValueError(f"SCENE_SCALE must be [p, q] (two ints >= 1: model pixels per scene pixel) or a mapping with scene_gsd / model_gsd, got {v!r}")
    if (p, q) == (1, 1):
        return None
    radii = [r for r in (config.ITSC_NMS_RADIUS, config.ROAD_NMS_RADIUS) if _is_num(r)]
    if radii and min(radii) * q < 2 * p:
        raise ValueError(f"SCENE_SCALE {p}/{q}: min(ITSC_NMS_RADIUS, ROAD_NMS_RADIUS) = {min(radii)} model pixels is less than {2 * p}/{q}: two graph "
                         f"points could map to one scene pixel; raise the NMS radii or lower the scale")
    g = config.SCENE_GROUP
    if _is_int(g) and g > 1:
        raise ValueError(f"SCENE_SCALE does not combine with SCENE_GROUP = {g} (a group's stack holds scenes of one frame): drop one of the keys")
    return p, q


def scene_scale_override(config, scale=None, scene_gsd=None, model_gsd=None):
    """The SCENE_SCALE value of the command line's --scene-scale P Q, or --scene-gsd A [--model-gsd B], laid over the config's key: the
    fraction replaces the key; a gsd flag replaces that field of a mapping key and keeps the other (model_gsd default 1.0)."""
    if scale is not None:
        if scene_gsd is not None or model_gsd is not None:
            raise ValueError("SCENE_SCALE: give --scene-scale P Q or --scene-gsd A [--model-gsd B], not both")
        return [int(scale[0]), int(scale[1])]
    v = config.SCENE_SCALE
    old = dict(v) if isinstance(v, dict) else {}
    if scene_gsd is None and "scene_gsd" not in old:
        raise ValueError("SCENE_SCALE: --model-gsd needs --scene-gsd (or a scene_gsd in the config's key)")
    return {"scene_gsd": old.get("scene_gsd") if scene_gsd is None else scene_gsd,
            "model_gsd": old.get("model_gsd", 1.0) if model_gsd is None else model_gsd}


def out_size(n, p, q):
    """ceil(n p / q): the pixels an axis of n pixels has after resampling by p/q."""
    return -(-int(n) * int(p) // int(q))


def model_shape(shape, scale):
    """(H, W) of the model frame of a scene of `shape` = (H, W[, C]) under scale = (p, q), or of the scene itself for None."""
    H, W = int(shape[0]), int(shape[1])
    return (H, W) if scale is None else (out_size(H, *scale), out_size(W, *scale))


def axis_tables(n_in, p, q, n_out=None):
    """One axis of the rule: (start int32 [n_out], weights uint8 [n_out, T], T, D) for an input of n_in pixels resampled by p/q (any two
    ints >= 1, p != q) to n_out pixels (None: ceil(n_in p / q)).  Every row of weights sums to D; tap t of output j reads input
    clamp(start[j] + t, 0, n_in - 1)."""
    n_in, p, q = int(n_in), int(p), int(q)
    if n_in < 1 or p < 1 or q < 1 or p == q:
        raise ValueError(f"axis_tables: n_in, p, q >= 1 and p != q, got {n_in}, {p}, {q}")
    n_out = out_size(n_in, p, q) if n_out is None else int(n_out)
    if n_out < 1:
        raise ValueError(f"axis_tables: n_out >= 1, got {n_out}")
    j = np.arange(n_out, dtype=np.int64)
    if p < q:
        T, D = -(-q // p) + 1, q
        s = (j * q) // p
        lo = (s[:, None] + np.arange(T, dtype=np.int64)[None, :]) * p
        w = np.clip(np.minimum(lo + p, ((j + 1) * q)[:, None]) - np.maximum(lo, (j * q)[:, None]), 0, None)
    else:
        T, D = 2, 2 * p
        num = (2 * j + 1) * q - p
        s = num // D                                        # numpy's // on int64 floors, as Python's
        f = num - s * D
        w = np.stack([D - f, f], axis=1)
    assert (w.sum(axis=1) == D).all() and w.min() >= 0 and w.max() <= 255
    return s.astype(np.int32), np.ascontiguousarray(w.astype(np.uint8)), T, D


def _taps(n_in, p, q, n_out):
    """(clamped tap indices int64 [n_out, T], weights int64 [n_out, T], D)."""
    s, w, T, D = axis_tables(n_in, p, q, n_out)
    idx = np.clip(s.astype(np.int64)[:, None] + np.arange(T, dtype=np.int64)[None, :], 0, n_in - 1)
    return idx, w.astype(np.int64), D


def _weighted(v, idx, w, axis):
    """sum_t w[:, t] * v taken at idx[:, t] along `axis` (int64)."""
    shape = [1] * v.ndim
    shape[axis] = -1
    return sum(np.take(v, idx[:, t], axis=axis) * w[:, t].astype(np.int64).reshape(shape) for t in range(idx.shape[1]))


def resample_ref(arr, p, q, out_shape=None, valid_rule=False, zero_where=None):
    """The rule in int64 numpy: arr [H, W] or [H, W, C] (uint8, or bool for a mask) resampled by p/q to out_shape = (Ho, Wo) (None:
    ceil(H p / q) x ceil(W p / q)); the result has arr's dtype.  valid_rule: arr is a validity mask (non-zero = valid) and an output pixel
    is 1 iff every tap with a non-zero weight is valid, on both axes; else the weighted sum with the single rounding.  zero_where [Ho, Wo]:
    the result is 0 wherever it is 0."""
    arr = np.asarray(arr)
    if arr.ndim not in (2, 3) or arr.dtype not in (np.dtype(np.uint8), np.dtype(bool)):
        raise ValueError(f"resample_ref takes a uint8 / bool [H,W] or [H,W,C] array, got {arr.dtype} {tuple(arr.shape)}")
    H, W = arr.shape[:2]
    Ho, Wo = (out_size(H, p, q), out_size(W, p, q)) if out_shape is None else (int(out_shape[0]), int(out_shape[1]))
    iy, wy, Dy = _taps(H, p, q, Ho)
    ix, wx, Dx = _taps(W, p, q, Wo)
    if valid_rule:                                          # count the invalid taps whose weights are non-zero on both axes
        out = (_weighted(_weighted((arr == 0).astype(np.int64), ix, wx != 0, 1), iy, wy != 0, 0) == 0).astype(np.int64)
    else:                                                   # integer sums are exact in any order: columns first, then rows
        out = (_weighted(_weighted(arr.astype(np.int64), ix, wx, 1), iy, wy, 0) + (Dy * Dx) // 2) // (Dy * Dx)
    if zero_where is not None:
        z = np.asarray(zero_where)
        if z.shape != (Ho, Wo):
            raise ValueError(f"zero_where must have the output's shape {(Ho, Wo)}, got {tuple(z.shape)}")
        out[z == 0] = 0
    return np.ascontiguousarray(out.astype(arr.dtype))


def map_nodes(nodes, scene_shape, p, q):
    """Graph points (row, col) of the model frame -> the scene frame of `scene_shape` = (H, W): (min(H - 1, ((2 r + 1) q) // (2 p)), the same
    for the column with W).  Keeps the dtype; an empty array passes through."""
    nodes = np.asarray(nodes)
    if nodes.shape[0] == 0:
        return nodes
    hi = np.array([int(scene_shape[0]) - 1, int(scene_shape[1]) - 1], dtype=np.int64)
    out = np.minimum(((2 * nodes.astype(np.int64) + 1) * int(q)) // (2 * int(p)), hi[None, :])
    return np.ascontiguousarray(out.astype(nodes.dtype))


# ---- how the device kernel is cut (csrc/scene_scale.hip) ---------------------------------------------------------------------------------
LDS_BUDGET = 32 * 1024                  # per workgroup; the entry itself accepts up to 64 KiB
_BLOCKS = (64, 48, 32, 24, 16, 12, 8, 6, 4, 3, 2, 1)


def window_span(b, T, p, q):
    """An upper bound of the input pixels the taps of b consecutive outputs span on one axis: consecutive starts differ by at most
    ceil(q / p), so the last tap lies at most ceil((b - 1) q / p) + T - 1 behind the first start (+ 1 for the floor of the first)."""
    return -(-(b - 1) * q // p) + T + 1


def lds_bytes(win_h, win_w, block_w, C):
    """The workgroup's LDS under the kernel's layout: win_h rows of a 16-byte-pitched u8 window (a row is staged from its 16-byte-aligned
    address, so up to 15 bytes precede it) and win_h rows of block_w C u16 row sums."""
    pitch = (win_w * C + 15 + 15) // 16 * 16
    return win_h * (pitch + 2 * block_w * C)


def block_plan(Ty, Tx, p, q, C):
    """(block_h, block_w, win_h, win_w): the largest square output block whose source window plus row-pass buffer stays inside LDS_BUDGET."""
    for b in _BLOCKS:
        win_h, win_w = window_span(b, Ty, p, q), window_span(b, Tx, p, q)
        if lds_bytes(win_h, win_w, b, C) <= LDS_BUDGET:
            return b, b, win_h, win_w
    raise ValueError(f"no output block fits {LDS_BUDGET} bytes of LDS at scale {p}/{q}")
