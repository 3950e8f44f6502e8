"""Float32 scenes (config key SCENE_FLOAT): the host side, and the single statement of what the key means.  No torch, no
device: numpy only.  The device compares integers against the tables built here and counts the histograms read here; pow, exp and log
run on the host alone, 255 times per band.

    SCENE_FLOAT: {select:   [i, j, k],                        # band indices 0..15, repeats allowed, default [0, 1, 2]
                  stretch:  [lo, hi] | three such pairs | {percentile: [p_lo, p_hi]},    # REQUIRED (a float has no "whole range")
                  gamma:    g,                                # finite > 0, default 1
                  transfer: linear | log,                     # default linear
                  nodata:   v | [v, ...]}                     # up to 4 finite numbers, default none

A scene under the key is float32 [H, W, C] with 1 <= C <= 16.  Everything is defined on a value's 32-bit pattern through the ordered key
(float_keys): b = bits(x), with 0x80000000 (-0.0) read as 0; key = ~b if the sign bit is set, else b | 0x80000000.  Over the non-NaN
values the key is a strictly monotone map from float order to unsigned order; x is finite iff its exponent field is not 0xff.

1. Validity.  A pixel is valid iff all three selected bands are finite, none of them has the key of float32(v) for a nodata value v, with
   transfer log every one of them is > 0, and the caller's mask (or SCENE_AOI's) is non-zero there.  A float scene is always a masked scene.
2. Ranges.  Fixed: lo and hi cast to float32, lo32 < hi32 (log: lo32 > 0).  Percentile: for output channel b, s = the sorted values of band
   select[b] over the valid pixels (N of them, the same for all three), lo = s[floor(float64(p_lo) / 100 (N - 1))] and hi likewise;
   hi <= lo becomes nextafter(lo, +inf) in float32 (where that is +inf, lo being the largest finite float32, the range is (nextafter(lo,
   -inf), lo) instead: every range is finite, and no scene can fail after the key has passed); N = 0 gives (0, 1), or (1, 2) under log.
3. Thresholds T_b[j], j = 1 .. 255, in float64: u = ((j - 0.5) / 255) ** gamma; t = lo + (hi - lo) u (linear) or exp(ln lo + (ln hi -
   ln lo) u) (log); T_b[j] = the smallest float32 >= t; then a running maximum over j.  This table is the definition.
4. Output.  Channel b of a valid pixel is #{j : x >= T_b[j]} = searchsorted(T_b, x, side="right"); an invalid pixel is 0, 0, 0 (the
   nodata fill of the masked pipeline then writes NODATA_FILL there)."""
import collections
import math

import numpy as np

MAX_BANDS = 16
MAX_NODATA = 4
MAX_TARGETS = 6
_KEYS = ("select", "stretch", "gamma", "transfer", "nodata")

# select: three band indices; ranges: None or three (lo, hi) of float32; percentile: None or (p_lo, p_hi); gamma; log: transfer is log;
# nodata: a tuple of up to 4 float32 values
SceneFloat = collections.namedtuple("SceneFloat", "select ranges percentile gamma log nodata")


def _absent(v):
    return v is None or (isinstance(v, dict) and not v)


def _is_int(v):
    return isinstance(v, (int, np.integer)) and not isinstance(v, (bool, np.bool_))


def _is_num(v):
    return (_is_int(v) or isinstance(v, (float, np.floating))) and math.isfinite(float(v))


def _f32(v):
    with np.errstate(over="ignore"):
        return np.float32(v)


def _is_f32(v):
    return _is_num(v) and bool(np.isfinite(_f32(v)))


def _pair(v):
    return isinstance(v, (list, tuple)) and len(v) == 2 and all(_is_f32(x) for x in v)


def scene_float_key(config):
    """config.SCENE_FLOAT as a SceneFloat tuple, or None for a missing key / None / {}: nothing changes anywhere.  ValueError — before the
    device is touched — for anything the module's docstring does not name, unknown keys and a missing stretch included.  What depends on
    the scene (dtype, select against C) is checked per scene: scene_float_check."""
    v = config.SCENE_FLOAT if not isinstance(config, dict) else config.get("SCENE_FLOAT")
    if _absent(v):
        return None
    if not isinstance(v, dict):
        raise ValueError(f"SCENE_FLOAT must be a mapping with select / stretch / gamma / transfer / nodata, got {v!r}")
    unknown = sorted(set(v) - set(_KEYS), key=str)
    if unknown:
        raise ValueError(f"SCENE_FLOAT: unknown key {unknown[0]!r} (select, stretch, gamma, transfer, nodata)")
    select = v.get("select", [0, 1, 2])
    if not isinstance(select, (list, tuple)) or len(select) != 3 or not all(_is_int(b) and 0 <= b < MAX_BANDS for b in select):
        raise ValueError(f"SCENE_FLOAT: select must be three band indices in 0..{MAX_BANDS - 1}, got {select!r}")
    transfer = v.get("transfer", "linear")
    if transfer not in ("linear", "log"):
        raise ValueError(f"SCENE_FLOAT: transfer must be 'linear' or 'log', got {transfer!r}")
    log = transfer == "log"
    stretch, ranges, percentile = v.get("stretch"), None, None
    if _absent(stretch):
        raise ValueError("SCENE_FLOAT: stretch is required ([lo, hi], three such pairs or {percentile: [p_lo, p_hi]}): a float has no whole range")
    if isinstance(stretch, dict):
        if set(stretch) != {"percentile"}:
            raise ValueError(f"SCENE_FLOAT: a stretch mapping has the one key 'percentile', got {sorted(stretch, key=str)!r}")
        p = stretch["percentile"]
        if not isinstance(p, (list, tuple)) or len(p) != 2 or not all(_is_num(x) for x in p) or not 0 <= p[0] < p[1] <= 100:
            raise ValueError(f"SCENE_FLOAT: stretch percentile must be [p_lo, p_hi] with 0 <= p_lo < p_hi <= 100, got {p!r}")
        percentile = (float(p[0]), float(p[1]))
    else:
        pairs = [stretch] * 3 if _pair(stretch) else stretch
        if (not isinstance(pairs, (list, tuple)) or len(pairs) != 3 or not all(_pair(q) for q in pairs)
                or not all(_f32(q[0]) < _f32(q[1]) and (not log or _f32(q[0]) > 0) for q in pairs)):
            raise ValueError(f"SCENE_FLOAT: stretch must be [lo, hi] or three such pairs of finite numbers with float32(lo) < float32(hi) (and "
                             f"lo > 0 with transfer log), or {{percentile: [p_lo, p_hi]}}, got {stretch!r}")
        ranges = tuple((_f32(q[0]), _f32(q[1])) for q in pairs)
    gamma = v.get("gamma", 1)
    if not _is_num(gamma) or not float(gamma) > 0:
        raise ValueError(f"SCENE_FLOAT: gamma must be a finite number > 0, got {gamma!r}")
    nodata = v.get("nodata")
    if nodata is None or (isinstance(nodata, (list, tuple, dict)) and not nodata):
        nodata = ()
    elif _is_f32(nodata):
        nodata = (nodata,)
    if not isinstance(nodata, (list, tuple)) or len(nodata) > MAX_NODATA or not all(_is_f32(x) for x in nodata):
        raise ValueError(f"SCENE_FLOAT: nodata must be a finite number or a list of up to {MAX_NODATA} of them (float32), got {v.get('nodata')!r}")
    return SceneFloat(tuple(int(b) for b in select), ranges, percentile, float(gamma), log, tuple(_f32(x) for x in nodata))


def as_key(key):
    """A SceneFloat from a SceneFloat or from the mapping a config would hold."""
    if isinstance(key, SceneFloat):
        return key
    k = scene_float_key({"SCENE_FLOAT": key})
    if k is None:
        raise ValueError("SCENE_FLOAT: an absent key has no meaning here")
    return k


def scene_float_check(img, key):
    """The per-scene half of the key's validation: img is float32 [H, W, C], 1 <= C <= 16, C > max(select).  ValueError otherwise."""
    if img.dtype in (np.dtype(np.float64), np.dtype(np.float16)):
        raise ValueError(f"with SCENE_FLOAT a scene is float32, got {img.dtype}: cast it with .astype(numpy.float32) (the rule is stated on "
                         f"float32 bit patterns)")
    if img.ndim != 3 or img.dtype != np.float32 or not 1 <= img.shape[2] <= MAX_BANDS:
        raise ValueError(f"with SCENE_FLOAT infer_one_img expects an HxWxC float32 scene with 1 <= C <= {MAX_BANDS}, got {img.dtype} {tuple(img.shape)}")
    if img.shape[2] <= max(key.select):
        raise ValueError(f"SCENE_FLOAT: select {list(key.select)} needs more than the {img.shape[2]} band(s) of the scene")


# ---- the ordered key ---------------------------------------------------------------------------------------------------------------------
def float_keys(x):
    """uint32 keys of float32 values (any shape): -0.0 read as +0.0; ~bits for a set sign bit, else bits | 0x80000000."""
    b = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)
    b = np.where(b == np.uint32(0x80000000), np.uint32(0), b)
    return np.where(b & np.uint32(0x80000000) != 0, ~b, b | np.uint32(0x80000000)).astype(np.uint32)


def keys_to_float(k):
    """The float32 values of keys (the inverse of float_keys, +0.0 for the key of zero)."""
    k = np.asarray(k, dtype=np.uint32)
    return np.where(k & np.uint32(0x80000000) != 0, k ^ np.uint32(0x80000000), ~k).astype(np.uint32).view(np.float32)


def _finite_bits(x):
    return (np.ascontiguousarray(x, dtype=np.float32).view(np.uint32) >> np.uint32(23)) & np.uint32(0xff) != np.uint32(0xff)


def nodata_keys(key):
    """The keys of the nodata values, uint32 [k], k <= 4."""
    return float_keys(np.array(as_key(key).nodata, dtype=np.float32))


# ---- rule 1 ------------------------------------------------------------------------------------------------------------------------------
def float_valid_ref(raw, key, valid=None):
    """Rule 1: uint8 [H, W] (0 / 1) for raw float32 [..., C]; valid: the caller's mask (non-zero = valid) or None."""
    key = as_key(key)
    ok = np.ones(raw.shape[:-1], bool) if valid is None else np.asarray(valid) != 0
    nd = nodata_keys(key)
    zero = np.uint32(0x80000000)
    for b in key.select:
        x = np.ascontiguousarray(raw[..., b])
        k = float_keys(x)
        ok = ok & _finite_bits(x)
        for v in nd:
            ok = ok & (k != v)
        if key.log:
            ok = ok & (k > zero)
    return ok.astype(np.uint8)


# ---- rule 2 ------------------------------------------------------------------------------------------------------------------------------
def _rank(p, N):
    return min(max(int(np.floor(np.float64(p) / 100.0 * (N - 1))), 0), N - 1)


def _fix_range(lo, hi):
    lo, hi = np.float32(lo), np.float32(hi)
    if hi > lo:
        return lo, hi
    with np.errstate(over="ignore"):
        hi = np.nextafter(lo, np.float32(np.inf), dtype=np.float32)
    if np.isfinite(hi):
        return lo, hi
    return np.nextafter(lo, np.float32(-np.inf), dtype=np.float32), lo      # lo is the largest finite float32: the range steps down instead


def empty_range(key):
    return (np.float32(1), np.float32(2)) if as_key(key).log else (np.float32(0), np.float32(1))


def float_ranges_ref(raw, key, valid=None):
    """Rule 2: the three (lo, hi) of float32 — the key's fixed ranges, or np.sort plus the index rule over the valid pixels (rule 1)."""
    key = as_key(key)
    if key.percentile is None:
        return list(key.ranges)
    ok = float_valid_ref(raw, key, valid) != 0
    out = []
    for b in key.select:
        x = raw[..., b][ok]
        if x.size == 0:
            out.append(empty_range(key))
            continue
        s = keys_to_float(np.sort(float_keys(x)))       # sorted by key: float order, -0.0 and +0.0 one value
        out.append(_fix_range(*(s[_rank(p, x.size)] for p in key.percentile)))
    return out


# the percentile on the device: two 65536-bin histograms of the keys (pass 1 over key >> 16, pass 2 over key & 0xffff of the values whose
# band and top half match a target) and the rank arithmetic here, in one place
def float_hist_targets(hist1, key):
    """hist1: integer counts [3, 65536] over key >> 16 of the selected bands of the valid pixels.  Returns (targets, picks): targets, the
    de-duplicated (band, prefix) pairs of pass 2, at most 6, and picks[b] = ((target index, residual rank) for p_lo, the same for p_hi),
    or None when nothing was counted."""
    key = as_key(key)
    hist1 = np.asarray(hist1).astype(np.int64)
    N = int(hist1[0].sum())
    if N == 0:
        return [], None
    targets, picks = [], []
    for b in range(3):
        cum = np.cumsum(hist1[b])
        assert int(cum[-1]) == N, "the three channels count the same pixels"
        pick = []
        for p in key.percentile:
            r = _rank(p, N)
            bucket = int(np.searchsorted(cum, r, side="right"))
            t = (key.select[b], bucket)
            if t not in targets:
                targets.append(t)
            pick.append((targets.index(t), r - (int(cum[bucket - 1]) if bucket else 0)))
        picks.append(tuple(pick))
    assert len(targets) <= MAX_TARGETS
    return targets, picks


def float_ranges_from_hists(targets, picks, hist2, key):
    """The three (lo, hi) from pass 2's counts hist2 [n_targets, 65536] over key & 0xffff; picks None (N = 0): the empty range."""
    key = as_key(key)
    if picks is None:
        return [empty_range(key)] * 3
    cum = np.cumsum(np.asarray(hist2).astype(np.int64), axis=1)
    out = []
    for pick in picks:
        lo, hi = (keys_to_float(np.uint32((targets[t][1] << 16) | int(np.searchsorted(cum[t], r, side="right"))))[()] for t, r in pick)
        out.append(_fix_range(lo, hi))
    return out


def radix_select_ref(raw, key, valid=None):
    """float_ranges_ref the way the device path computes it: both histograms from numpy, the host arithmetic above."""
    key = as_key(key)
    ok = float_valid_ref(raw, key, valid).reshape(-1) != 0
    k = float_keys(raw.reshape(-1, raw.shape[-1]))[ok]
    hist1 = np.stack([np.bincount(k[:, b] >> np.uint32(16), minlength=65536) for b in key.select])
    targets, picks = float_hist_targets(hist1, key)
    hist2 = np.stack([np.bincount(k[k[:, b] >> np.uint32(16) == pre, b] & np.uint32(0xffff), minlength=65536) for b, pre in targets]) if targets else None
    return float_ranges_from_hists(targets, picks, hist2, key)


# ---- rules 3 and 4 -----------------------------------------------------------------------------------------------------------------------
def float_thresholds(ranges, key):
    """Rule 3: float32 [3, 255], row b = T_b[1 .. 255] for the three (lo, hi) of `ranges`; equal ranges share one computation."""
    key = as_key(key)
    u = ((np.arange(1, 256, dtype=np.float64) - 0.5) / 255.0) ** np.float64(key.gamma)
    memo = {}
    rows = []
    for lo, hi in ranges:
        lo32, hi32 = np.float32(lo), np.float32(hi)
        if not (np.isfinite(lo32) and np.isfinite(hi32) and lo32 < hi32) or (key.log and not lo32 > 0):
            raise ValueError(f"float_thresholds needs finite float32 lo < hi (lo > 0 with transfer log), got {lo!r}, {hi!r}")
        k = (lo32.tobytes(), hi32.tobytes())
        if k not in memo:
            lo64, hi64 = np.float64(lo32), np.float64(hi32)
            t = np.exp(np.log(lo64) + (np.log(hi64) - np.log(lo64)) * u) if key.log else lo64 + (hi64 - lo64) * u
            with np.errstate(over="ignore"):
                T = t.astype(np.float32)
            down = T.astype(np.float64) < t
            T[down] = np.nextafter(T[down], np.float32(np.inf), dtype=np.float32)
            memo[k] = np.maximum.accumulate(T)
        rows.append(memo[k])
    return np.stack(rows)


def threshold_keys(T):
    """What the device compares against: uint32 [3, 256], the keys of the thresholds with 0xffffffff as entry 255."""
    out = np.full((3, 256), 0xffffffff, dtype=np.uint32)
    out[:, :255] = float_keys(np.asarray(T, dtype=np.float32))
    return out


def apply_thresholds(raw, select, T, valid):
    """Rule 4 on the host: uint8 [..., 3], channel b = searchsorted(T[b], raw[..., select[b]], side="right") on the keys, 0 where valid is 0."""
    tk = float_keys(T)
    out = np.stack([np.searchsorted(tk[b], float_keys(raw[..., select[b]]), side="right") for b in range(3)], axis=-1).astype(np.uint8)
    out[np.asarray(valid) == 0] = 0
    return out


def float_scene_ref(raw, key, valid=None):
    """The whole rule: (uint8 [H, W, 3], valid uint8 [H, W]) of a float32 scene [H, W, C] under the key (a mapping or a SceneFloat)."""
    key = as_key(key)
    raw = np.asarray(raw)
    scene_float_check(raw, key)
    ok = float_valid_ref(raw, key, valid)
    T = float_thresholds(float_ranges_ref(raw, key, valid), key)
    return np.ascontiguousarray(apply_thresholds(raw, key.select, T, ok)), ok


def scene_float_override(config, bands=None, float_range=None, float_percentile=None, gamma=None, transfer=None, nodata=None):
    """The SCENE_FLOAT mapping of the command line's --float-bands / --float-range / --float-percentile / --float-gamma / --float-transfer /
    --float-nodata laid over the config's key: a flag that is given replaces that field (either stretch flag replaces the stretch), the
    others stay as the config has them."""
    if float_range is not None and float_percentile is not None:
        raise ValueError("--float-range and --float-percentile exclude each other")
    v = config.SCENE_FLOAT
    out = {} if _absent(v) else dict(v) if isinstance(v, dict) else v
    if not isinstance(out, dict):
        raise ValueError(f"SCENE_FLOAT must be a mapping with select / stretch / gamma / transfer / nodata, got {v!r}")
    if bands is not None:
        out["select"] = list(bands)
    if float_range is not None:
        out["stretch"] = list(float_range)
    if float_percentile is not None:
        out["stretch"] = {"percentile": list(float_percentile)}
    if gamma is not None:
        out["gamma"] = gamma
    if transfer is not None:
        out["transfer"] = transfer
    if nodata is not None:
        out["nodata"] = list(nodata)
    return out
