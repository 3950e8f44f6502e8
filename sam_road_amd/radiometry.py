"""16-bit and multi-band scenes (config key SCENE_BANDS): the host side, and the single statement of what the key means.
No torch, no device: numpy only.  The device gathers from the tables built here and counts the histogram read here; nothing is computed
twice in two places.

A scene under the key is uint8 (levels = 256) or uint16 (levels = 65536), [H, W, C] with 1 <= C <= 16.  Output channel b of a pixel is
LUT[b][pixel[select[b]]], and

    t = clip((v - lo_b) / (hi_b - lo_b), 0, 1)            (float64)
    LUT[b][v] = uint8(floor(255 * t ** (1 / gamma) + 0.5))   for v in 0 .. levels - 1

With a percentile stretch lo_b / hi_b are read off the exact integer histogram of band select[b] over the scene's valid pixels: the
values at sorted index floor(p / 100 * (N - 1)) — numpy.percentile(..., method="lower")."""
import collections
import math

import numpy as np

MAX_BANDS = 16
LEVELS = {np.dtype(np.uint8): 256, np.dtype(np.uint16): 65536}
_KEYS = ("select", "stretch", "gamma")

# select: three band indices; ranges: None (the whole range of the dtype) or three (lo, hi); percentile: None or (p_lo, p_hi); gamma
SceneBands = collections.namedtuple("SceneBands", "select ranges percentile gamma")


def _absent(v):
    return v is None or (isinstance(v, dict) and not v)


def _is_int(v):
    return isinstance(v, (int, np.integer)) and not isinstance(v, (bool, np.bool_))


def _is_num(v):
    return (_is_int(v) or isinstance(v, (float, np.floating))) and math.isfinite(float(v))


def _pair(v):
    return isinstance(v, (list, tuple)) and len(v) == 2 and all(_is_int(x) for x in v)


def scene_bands_key(config):
    """config.SCENE_BANDS as a SceneBands tuple, or None for a missing key / None: nothing changes anywhere.  The key is a mapping with
    `select` (three band indices >= 0, repeats allowed, default [0, 1, 2]), `stretch` ([lo, hi] or three such pairs, ints with 0 <= lo <
    hi, or {percentile: [p_lo, p_hi]} with 0 <= p_lo < p_hi <= 100; default: the whole range of the scene's dtype) and `gamma` (a finite
    number > 0, default 1).  ValueError — before the device is touched — for anything else, unknown keys included.  What depends on the
    scene (select against C, a range against the dtype's levels) is checked per scene: scene_bands_check."""
    v = config.SCENE_BANDS
    if _absent(v):                                       # None, or the empty node of a missing key (an empty mapping written out counts as that)
        return None
    if not isinstance(v, dict):
        raise ValueError(f"SCENE_BANDS must be a mapping with select / stretch / gamma, got {v!r}")
    unknown = sorted(set(v) - set(_KEYS), key=str)
    if unknown:
        raise ValueError(f"SCENE_BANDS: unknown key {unknown[0]!r} (select, stretch, gamma)")
    select = v.get("select", [0, 1, 2])
    if not isinstance(select, (list, tuple)) or len(select) != 3 or not all(_is_int(b) and 0 <= b < MAX_BANDS for b in select):
        raise ValueError(f"SCENE_BANDS: select must be three band indices in 0..{MAX_BANDS - 1}, got {select!r}")
    stretch, ranges, percentile = v.get("stretch"), None, None
    if isinstance(stretch, dict) and stretch:
        if set(stretch) != {"percentile"}:
            raise ValueError(f"SCENE_BANDS: a stretch mapping has the one key 'percentile', got {sorted(stretch, key=str)!r}")
        p = stretch["percentile"]
        if not isinstance(p, (list, tuple)) or len(p) != 2 or not all(_is_num(x) for x in p) or not 0 <= p[0] < p[1] <= 100:
            raise ValueError(f"SCENE_BANDS: stretch percentile must be [p_lo, p_hi] with 0 <= p_lo < p_hi <= 100, got {p!r}")
        percentile = (float(p[0]), float(p[1]))
    elif not _absent(stretch):
        pairs = [stretch] * 3 if _pair(stretch) else stretch
        if not isinstance(pairs, (list, tuple)) or len(pairs) != 3 or not all(_pair(q) and 0 <= q[0] < q[1] <= 65535 for q in pairs):
            raise ValueError(f"SCENE_BANDS: stretch must be [lo, hi] or three such pairs of ints with 0 <= lo < hi <= levels - 1, or "
                             f"{{percentile: [p_lo, p_hi]}}, got {stretch!r}")
        ranges = tuple((int(q[0]), int(q[1])) for q in pairs)
    gamma = v.get("gamma", 1)
    if not _is_num(gamma) or not float(gamma) > 0:
        raise ValueError(f"SCENE_BANDS: gamma must be a finite number > 0, got {gamma!r}")
    return SceneBands(tuple(int(b) for b in select), ranges, percentile, float(gamma))


def scene_bands_check(img, key):
    """The per-scene half of the key's validation: img is uint8 / uint16 [H, W, C], 1 <= C <= 16, C > max(select), and a fixed range lies
    inside the dtype's levels.  Returns levels.  ValueError otherwise."""
    if img.ndim != 3 or img.dtype not in LEVELS or not 1 <= img.shape[2] <= MAX_BANDS:
        raise ValueError(f"with SCENE_BANDS infer_one_img expects an HxWxC uint8 or uint16 scene with 1 <= C <= {MAX_BANDS}, got {img.dtype} {tuple(img.shape)}")
    levels = LEVELS[img.dtype]
    if img.shape[2] <= max(key.select):
        raise ValueError(f"SCENE_BANDS: select {list(key.select)} needs more than the {img.shape[2]} band(s) of the scene")
    if key.ranges is not None and any(hi > levels - 1 for _, hi in key.ranges):
        raise ValueError(f"SCENE_BANDS: stretch {[list(q) for q in key.ranges]} leaves the {levels} levels of a {img.dtype} scene (0 <= lo < hi <= {levels - 1})")
    return levels


def band_lut(lo, hi, gamma, levels):
    """The table of one output channel, uint8 [levels]: LUT[v] = floor(255 * clip((v - lo) / (hi - lo), 0, 1) ** (1 / gamma) + 0.5) in
    float64.  lo < hi; hi may be `levels` (a degenerate percentile range)."""
    lo, hi, gamma, levels = int(lo), int(hi), float(gamma), int(levels)
    if not lo < hi or not gamma > 0 or not math.isfinite(gamma):
        raise ValueError(f"band_lut needs lo < hi and a finite gamma > 0, got {lo}, {hi}, {gamma}")
    t = np.clip((np.arange(levels, dtype=np.float64) - lo) / np.float64(hi - lo), 0.0, 1.0)
    return np.floor(255.0 * t ** (1.0 / gamma) + 0.5).astype(np.uint8)


def stretch_from_hist(hist, p_lo, p_hi):
    """(lo, hi) of every row of hist (integer counts [k, levels] -> a list of k pairs; [levels] -> one pair): the values at sorted index
    floor(p / 100 * (N - 1)) of the N counted pixels, float64 arithmetic — numpy.percentile(method="lower") — read off the cumulative
    histogram.  hi <= lo becomes hi = lo + 1 (it may equal levels); N = 0 gives (0, levels - 1)."""
    hist = np.asarray(hist)
    if hist.ndim == 1:
        return stretch_from_hist(hist[None], p_lo, p_hi)[0]
    out = []
    for h in hist.astype(np.int64):
        cum = np.cumsum(h)
        N = int(cum[-1])
        if N == 0:
            out.append((0, int(h.shape[0]) - 1))
            continue
        lo, hi = (int(np.searchsorted(cum, min(max(int(np.floor(np.float64(p) / 100.0 * (N - 1))), 0), N - 1), side="right"))
                  for p in (p_lo, p_hi))
        out.append((lo, hi if hi > lo else lo + 1))
    return out


def band_luts(ranges, gamma, levels):
    """The three tables of a scene, uint8 [3, levels], from its three (lo, hi); equal ranges share one computation."""
    memo = {}
    return np.stack([memo.setdefault(tuple(q), band_lut(q[0], q[1], gamma, levels)) for q in ranges])


def fixed_ranges(key, levels):
    """The three (lo, hi) of a key without a percentile: its ranges, or the whole range of the dtype."""
    return key.ranges if key.ranges is not None else ((0, levels - 1),) * 3


def apply_luts(img, select, luts):
    """The definition applied on the host (numpy): uint8 [H, W, 3], channel b = luts[b][img[..., select[b]]].  What the device step must
    equal byte for byte; the tests and the cost comparison of tools/scene_bench.py use it, the pipeline does not."""
    return np.stack([luts[b][img[..., select[b]]] for b in range(3)], axis=-1)


def scene_bands_override(config, bands=None, stretch_range=None, stretch_percentile=None, gamma=None):
    """The SCENE_BANDS mapping of the command line's --bands / --stretch-range / --stretch-percentile / --gamma laid over the config's
    key: a flag that is given replaces that field (either stretch flag replaces the stretch), the others stay as the config has them."""
    key = scene_bands_key(config)
    out = {}
    if key is not None:
        out["select"], out["gamma"] = list(key.select), key.gamma
        if key.ranges is not None:
            out["stretch"] = [list(q) for q in key.ranges]
        if key.percentile is not None:
            out["stretch"] = {"percentile": list(key.percentile)}
    if bands is not None:
        out["select"] = list(bands)
    if stretch_range is not None and stretch_percentile is not None:
        raise ValueError("--stretch-range and --stretch-percentile exclude each other")
    if stretch_range is not None:
        out["stretch"] = list(stretch_range)
    if stretch_percentile is not None:
        out["stretch"] = {"percentile": list(stretch_percentile)}
    if gamma is not None:
        out["gamma"] = gamma
    return out
