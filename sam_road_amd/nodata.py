"""SCENE_NODATA: the one statement of how a validity mask follows from a nodata VALUE, on the host, in integers.
No torch, no device: numpy (and, for the area rule, mask_clean_ref) only.

    SCENE_NODATA: {value: v | [v_0 .. v_{C-1}],    # level(s) of the RAW scene (u8: 0..255, u16: 0..65535); an int serves every band
                   tolerance: t,                   # int >= 0, default 0: band c hits iff |pixel_c - v_c| <= t
                   match: all | any,               # default all: over ALL C bands of the raw scene, not only SCENE_BANDS.select
                   min_area: a, connectivity: 8|4, # int >= 1, default 1; 8: a connected set of hit pixels smaller than a is NOT nodata
                   grow: r}                        # int 0..16, default 0: nodata grown by r px (Chebyshev)

A bare int or list means {value: ...}.  For a raw scene raw [H, W, C] of `levels` levels:
  1. hit[y, x] = all / any over c of lo_c <= raw[y, x, c] <= hi_c, lo_c = max(0, v_c - t), hi_c = min(levels - 1, v_c + t)
  2. min_area > 1: the connected components of hit with fewer than min_area pixels are cleared — mask_clean_ref on the 0 / 1 image with
     t_on = 1, that min_area and no peak test
  3. grow > 0: nodata[y, x] = any hit within Chebyshev distance r INSIDE the image (pixels outside the image are not nodata); else
     nodata = hit
  4. valid_out = not nodata, ANDed with the caller's valid != 0 where one is given: u8, 0 / 1

A run with the key equals, bit for bit, the pipeline called with valid = nodata_ref(raw, key, valid).  The device kernels
(csrc/scene_nodata.hip, and csrc/mask_clean.hip as it is) must equal nodata_ref byte for byte."""
import collections

import numpy as np

from .mask_clean import MaskRule, mask_clean_ref, mask_clean_table

LEVELS = {np.dtype(np.uint8): 256, np.dtype(np.uint16): 65536}
MAX_BANDS = 16
MAX_GROW = 16
_KEYS = ("value", "tolerance", "match", "min_area", "connectivity", "grow")

# value: one int (every band) or a tuple of C ints; any: False = all bands must hit, True = one is enough
SceneNodata = collections.namedtuple("SceneNodata", "value tolerance any min_area connectivity grow")


def _absent(v):
    return v is None or (isinstance(v, dict) and not v)


def _is_int(v):
    return isinstance(v, (int, np.integer)) and not isinstance(v, (bool, np.bool_))


def scene_nodata_key(config):
    """config.SCENE_NODATA as a SceneNodata tuple, or None for a missing key / None: nothing changes anywhere.  ValueError — before the
    device is touched — for anything that is not the mapping of the module's docstring: unknown keys, bools, non-ints, a value outside
    0 .. 65535, tolerance < 0, min_area < 1, grow outside 0 .. 16, a connectivity other than 4 or 8, a match other than all / any.  What
    depends on the scene (the value against the dtype's levels, a list against the band count) is checked per scene: scene_nodata_check."""
    v = config.SCENE_NODATA
    if _absent(v):                                       # None, or the empty node of a missing key
        return None
    if _is_int(v) or isinstance(v, (list, tuple)):
        v = {"value": v}
    if not isinstance(v, dict):
        raise ValueError(f"SCENE_NODATA must be an int, a list of ints or a mapping with value / tolerance / match / min_area / connectivity / grow, got {v!r}")
    unknown = sorted(set(v) - set(_KEYS), key=str)
    if unknown:
        raise ValueError(f"SCENE_NODATA: unknown key {unknown[0]!r} ({', '.join(_KEYS)})")
    if "value" not in v:
        raise ValueError("SCENE_NODATA: value is required (an int, or one int per band of the raw scene)")
    value = v["value"]
    if isinstance(value, (list, tuple)):
        if not 1 <= len(value) <= MAX_BANDS or not all(_is_int(x) and 0 <= x <= 65535 for x in value):
            raise ValueError(f"SCENE_NODATA: value must be an int or a list of 1 to {MAX_BANDS} ints in 0..65535, got {value!r}")
        value = tuple(int(x) for x in value)
    elif _is_int(value) and 0 <= value <= 65535:
        value = int(value)
    else:
        raise ValueError(f"SCENE_NODATA: value must be an int or a list of 1 to {MAX_BANDS} ints in 0..65535, got {value!r}")
    tol = v.get("tolerance", 0)
    if not _is_int(tol) or tol < 0:
        raise ValueError(f"SCENE_NODATA: tolerance must be an int >= 0, got {tol!r}")
    match = v.get("match", "all")
    name = match.strip().lower() if isinstance(match, str) else match
    if not isinstance(name, str) or name not in ("all", "any"):
        raise ValueError(f"SCENE_NODATA: match must be 'all' or 'any', got {match!r}")
    area = v.get("min_area", 1)
    if not _is_int(area) or area < 1:
        raise ValueError(f"SCENE_NODATA: min_area must be an int >= 1, got {area!r}")
    conn = v.get("connectivity", 8)
    if not _is_int(conn) or conn not in (4, 8):
        raise ValueError(f"SCENE_NODATA: connectivity must be 4 or 8, got {conn!r}")
    grow = v.get("grow", 0)
    if not _is_int(grow) or not 0 <= grow <= MAX_GROW:
        raise ValueError(f"SCENE_NODATA: grow must be an int in 0..{MAX_GROW}, got {grow!r}")
    return SceneNodata(value, int(min(tol, 65535)), name == "any", int(area), int(conn), int(grow))


def scene_nodata_override(config, value=None, tolerance=None, match=None, min_area=None, grow=None):
    """The SCENE_NODATA mapping of the command line's --nodata V [V ...], --nodata-tolerance T, --nodata-match all|any, --nodata-min-area A
    and --nodata-grow R laid over the config's key: a flag that is given replaces that field, the others stay as the config has them."""
    v = config.SCENE_NODATA
    if _is_int(v) or isinstance(v, (list, tuple)):
        v = {"value": v}
    if not _absent(v) and not isinstance(v, dict):
        raise ValueError(f"SCENE_NODATA must be an int, a list of ints or a mapping, got {v!r}")
    new = dict(v or {})
    if value is not None:
        value = list(value)
        new["value"] = value[0] if len(value) == 1 else value
    for field, val in (("tolerance", tolerance), ("match", match), ("min_area", min_area), ("grow", grow)):
        if val is not None:
            new[field] = val
    return new


def scene_nodata_check(img, key):
    """The per-scene half of the key's validation: the raw scene is uint8 / uint16 [H, W, C] with 1 <= C <= 16, every value lies inside the
    dtype's levels and a list of values has one entry per band.  Returns (lo, hi): two lists of C ints, the inclusive range of every band
    (rule 1 of the module's docstring).  ValueError otherwise."""
    img = np.asarray(img) if not hasattr(img, "dtype") else img
    if img.ndim != 3 or np.dtype(img.dtype) not in LEVELS or not 1 <= img.shape[2] <= MAX_BANDS:
        raise ValueError(f"with SCENE_NODATA a scene is HxWxC uint8 or uint16 with 1 <= C <= {MAX_BANDS}, got {img.dtype} {tuple(img.shape)}")
    levels, C = LEVELS[np.dtype(img.dtype)], int(img.shape[2])
    values = key.value if isinstance(key.value, tuple) else (key.value,) * C
    if len(values) != C:
        raise ValueError(f"SCENE_NODATA: value lists {len(values)} level(s), the scene has {C} band(s)")
    if any(x > levels - 1 for x in values):
        raise ValueError(f"SCENE_NODATA: value {list(values)} leaves the {levels} levels of a {img.dtype} scene (0..{levels - 1})")
    return [max(0, x - key.tolerance) for x in values], [min(levels - 1, x + key.tolerance) for x in values]


def nodata_rule(key):
    """The MaskRule of step 2 for srh_mask_clean / mask_clean_ref: foreground = hit (level >= 1), min_area, no peak test."""
    return MaskRule(1, key.min_area, 0)


def nodata_table(blocks, key):
    """The int64 [n, 8] table that srh_mask_clean (step 2) and srh_scene_nodata_grow (step 3; it reads columns 0..2) share, for blocks =
    [(byte offset, H, W), ...]."""
    return mask_clean_table([(off, H, W, nodata_rule(key)) for off, H, W in blocks])


def nodata_hit(raw, key):
    """Steps 1 and 2: hit as a uint8 [H, W] 0 / 1 array."""
    raw = np.asarray(raw)
    lo, hi = scene_nodata_check(raw, key)
    r = raw.astype(np.int64)
    per_band = (r >= np.asarray(lo, np.int64)) & (r <= np.asarray(hi, np.int64))
    hit = (per_band.any(-1) if key.any else per_band.all(-1)).astype(np.uint8)
    if key.min_area > 1:
        hit = mask_clean_ref(hit, 1, key.min_area, 0, key.connectivity)
    return hit


def grow_ref(hit, r):
    """Step 3: uint8 [H, W] 0 / 1, 1 iff any pixel of hit within Chebyshev distance r inside the image is non-zero."""
    h = np.asarray(hit) != 0
    r = int(r)
    if r <= 0:
        return h.astype(np.uint8)
    H, W = h.shape
    rows = np.zeros_like(h)
    for d in range(-min(r, W - 1), min(r, W - 1) + 1):                     # a shift of W or more brings nothing into the image
        if d >= 0:
            rows[:, d:] |= h[:, :W - d]
        else:
            rows[:, :W + d] |= h[:, -d:]
    out = np.zeros_like(h)
    for d in range(-min(r, H - 1), min(r, H - 1) + 1):
        if d >= 0:
            out[d:] |= rows[:H - d]
        else:
            out[:H + d] |= rows[-d:]
    return out.astype(np.uint8)


def nodata_ref(raw, key, valid=None):
    """The rule on one raw scene (uint8 / uint16 [H, W, C]) under a SceneNodata key: valid_out, a NEW uint8 [H, W] array of 0 / 1.  valid:
    the caller's mask (bool / uint8 [H, W], non-zero = valid) or None."""
    raw = np.asarray(raw)
    out = 1 - grow_ref(nodata_hit(raw, key), key.grow)
    if valid is not None:
        valid = np.asarray(valid)
        if tuple(valid.shape) != tuple(raw.shape[:2]):
            raise ValueError(f"valid must have the scene's shape {tuple(raw.shape[:2])}, got {tuple(valid.shape)}")
        out = out & (valid != 0)
    return np.ascontiguousarray(out, dtype=np.uint8)
