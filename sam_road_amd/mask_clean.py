"""MASK_CLEAN: the one statement of the connected-component filter of the scene masks, on the host, in integers.

Between pass 1 and the point extraction the two fused uint8 masks are thresholded and every blob above the threshold becomes graph
points.  The optional key drops the blobs that are too small or never reach a confident level:

    MASK_CLEAN:
      road:     {min_area: 200, min_peak: 0.6}   # either may be missing
      keypoint: {min_peak: 0.5}                  # the whole entry may be missing
      connectivity: 8                            # 8 (default) or 4

For a mask m (uint8 [H, W]):
  foreground   m >= t_on, t_on = floor(T * 255) + 1 with T = ROAD_THRESHOLD / ITSC_THRESHOLD: exactly the pixels that
               graph_points.points_and_scores_from_mask takes (mask > T * 255); t_on > 255: no foreground, nothing happens
  components   the connected components of the foreground under 8- or 4-connectivity; area = pixel count, peak = highest level
  keep         iff area >= min_area (an int >= 1, default 1) and peak >= t_peak = floor(min_peak * 255) + 1 (min_peak a number in
               [0, 1); missing: t_peak = 0, every component passes)
  output       m with the pixels of the dropped components set to 0; every other byte, those below the threshold included, untouched

The device kernels (csrc/mask_clean.hip) must equal mask_clean_ref byte for byte, so a run with the key equals the existing pipeline
with its two masks replaced by mask_clean_ref of them before the point extraction, bit for bit.  No float enters the rule after the
three levels have been taken.
"""
import collections
import math

import numpy as np

_ENTRY_KEYS = ("min_area", "min_peak")
_TOP_KEYS = ("road", "keypoint", "connectivity")

# what one mask is filtered with; (t_on, 1, 0) filters nothing
MaskRule = collections.namedtuple("MaskRule", "t_on min_area t_peak")
# the parsed key: the two rules and the connectivity.  order: the masks as the scene path holds them (keypoint, road)
MaskCleanPlan = collections.namedtuple("MaskCleanPlan", "keypoint road connectivity")


def _absent(v):
    return v is None or (isinstance(v, dict) and not v)


def _is_int(v):
    return isinstance(v, (int, np.integer)) and not isinstance(v, (bool, np.bool_))


def _is_num(v):
    return (_is_int(v) or isinstance(v, (float, np.floating))) and math.isfinite(float(v))


def level_above(fraction):
    """floor(fraction * 255) + 1 clipped to 0 .. 256: the lowest uint8 level that is > fraction * 255 (256: none is)."""
    return int(min(256, max(0, math.floor(float(fraction) * 255) + 1)))


def _entry(name, v):
    """(min_area, t_peak) of one mask's entry, or ValueError."""
    if _absent(v):
        return 1, 0
    if not isinstance(v, dict):
        raise ValueError(f"MASK_CLEAN: {name} must be a mapping with min_area and / or min_peak, got {v!r}")
    unknown = sorted(set(v) - set(_ENTRY_KEYS), key=str)
    if unknown:
        raise ValueError(f"MASK_CLEAN: unknown key {unknown[0]!r} in {name} (min_area, min_peak)")
    area, peak = v.get("min_area"), v.get("min_peak")
    if area is None:
        area = 1
    elif not _is_int(area) or area < 1:
        raise ValueError(f"MASK_CLEAN: {name}.min_area must be an int >= 1, got {area!r}")
    if peak is None:
        t_peak = 0
    elif not _is_num(peak) or not 0 <= float(peak) < 1:
        raise ValueError(f"MASK_CLEAN: {name}.min_peak must be a number in [0, 1), got {peak!r}")
    else:
        t_peak = level_above(peak)
    return int(area), t_peak


def mask_clean_key(config):
    """config.MASK_CLEAN (extension key) as a MaskCleanPlan, or None when nothing is to be filtered: a missing key, None,
    an empty mapping, and entries that name nothing but min_area: 1.  ValueError — before the device is touched — for anything else
    that is not the mapping of the module's docstring: unknown keys, a bool, min_area < 1 or no int, min_peak outside [0, 1) or not
    finite, a connectivity other than 4 or 8.  The thresholds come from ITSC_THRESHOLD and ROAD_THRESHOLD."""
    v = config.MASK_CLEAN
    if _absent(v):
        return None
    if not isinstance(v, dict):
        raise ValueError(f"MASK_CLEAN must be a mapping with road / keypoint / connectivity, got {v!r}")
    unknown = sorted(set(v) - set(_TOP_KEYS), key=str)
    if unknown:
        raise ValueError(f"MASK_CLEAN: unknown key {unknown[0]!r} (road, keypoint, connectivity)")
    conn = v.get("connectivity", 8)
    if not _is_int(conn) or conn not in (4, 8):
        raise ValueError(f"MASK_CLEAN: connectivity must be 4 or 8, got {conn!r}")
    rules = {}
    for name, thr in (("keypoint", config.ITSC_THRESHOLD), ("road", config.ROAD_THRESHOLD)):
        min_area, t_peak = _entry(name, v.get(name))
        if (min_area, t_peak) != (1, 0) and not _is_num(thr):
            raise ValueError(f"MASK_CLEAN: {name} needs its threshold ({'ITSC' if name == 'keypoint' else 'ROAD'}_THRESHOLD) in the config, got {thr!r}")
        rules[name] = MaskRule(level_above(thr) if _is_num(thr) else 256, min_area, t_peak)
    if all(idle(r) for r in rules.values()):
        return None
    return MaskCleanPlan(rules["keypoint"], rules["road"], int(conn))


def idle(rule):
    """The rule drops nothing whatever the mask holds: no foreground, or every component passes (a peak is >= t_on)."""
    return rule.t_on > 255 or (rule.min_area <= 1 and rule.t_peak <= rule.t_on)


def mask_clean_override(config, min_area=None, min_peak=None, connectivity=None):
    """The MASK_CLEAN value of the command line's --mask-min-area ROAD [KEYPOINT], --mask-min-peak ROAD [KEYPOINT] and
    --mask-connectivity N laid over the config's key: a flag replaces that field and keeps the others."""
    v = config.MASK_CLEAN
    if not _absent(v) and not isinstance(v, dict):
        raise ValueError(f"MASK_CLEAN must be a mapping with road / keypoint / connectivity, got {v!r}")
    new = {k: (dict(e) if isinstance(e, dict) else e) for k, e in (v or {}).items()}
    for field, values in (("min_area", min_area), ("min_peak", min_peak)):
        if values is None:
            continue
        if not 1 <= len(values) <= 2:
            raise ValueError(f"MASK_CLEAN: --mask-{field.replace('_', '-')} takes ROAD [KEYPOINT], got {list(values)!r}")
        for name, val in zip(("road", "keypoint"), values):
            if not isinstance(new.get(name), dict):
                new[name] = {}
            new[name][field] = val
    if connectivity is not None:
        new["connectivity"] = connectivity
    return new


def mask_clean_ref(m, t_on, min_area=1, t_peak=0, connectivity=8):
    """The rule on one uint8 [H, W] array: a NEW array, m with the pixels of every dropped component set to 0."""
    from scipy import ndimage
    m = np.asarray(m)
    if m.dtype != np.uint8 or m.ndim != 2:
        raise ValueError(f"mask_clean_ref takes a uint8 [H, W] array, got {m.dtype} {m.shape}")
    if connectivity not in (4, 8):
        raise ValueError(f"connectivity must be 4 or 8, got {connectivity!r}")
    out = np.array(m, copy=True, order="C")
    fg = m.astype(np.int64) >= int(t_on)
    if not fg.any():
        return out
    structure = np.ones((3, 3), bool) if connectivity == 8 else ndimage.generate_binary_structure(2, 1)
    labels, n = ndimage.label(fg, structure=structure)
    area = np.bincount(labels.ravel(), minlength=n + 1)
    peak = np.asarray(ndimage.maximum(m, labels=labels, index=np.arange(n + 1))).astype(np.int64)
    keep = (area >= int(min_area)) & (peak >= int(t_peak))
    keep[0] = True                                    # label 0 is the background: untouched
    out[~keep[labels]] = 0
    return out


def mask_clean_stats(m, t_on, connectivity=8):
    """(areas, peaks) int64 [n] of the components of m's foreground, for choosing and checking parameters."""
    from scipy import ndimage
    m = np.asarray(m)
    structure = np.ones((3, 3), bool) if connectivity == 8 else ndimage.generate_binary_structure(2, 1)
    labels, n = ndimage.label(m.astype(np.int64) >= int(t_on), structure=structure)
    if n == 0:
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    return (np.bincount(labels.ravel(), minlength=n + 1)[1:].astype(np.int64),
            np.asarray(ndimage.maximum(m, labels=labels, index=np.arange(1, n + 1))).astype(np.int64))


MC_COLS = 8     # = csrc/mask_clean_piece.hpp: {OFF, H, W, T_ON, MIN_AREA, T_PEAK, BASE, SEG0}


def mask_clean_table(images):
    """The int64 [n, 8] table of srh_mask_clean for images = [(byte offset, H, W, MaskRule), ...] in the order given."""
    t = np.zeros((len(images), MC_COLS), dtype=np.int64)
    base = seg0 = 0
    for k, (off, H, W, rule) in enumerate(images):
        H, W = int(H), int(W)
        t[k] = (int(off), H, W, rule.t_on, rule.min_area, rule.t_peak, base, seg0)
        base += H * W
        seg0 += H * ((W + 63) // 64)
    return t
