"""What the SCENE_NODATA tests share (tests/test_scene_nodata_host.py, tests/test_gpu_scene_nodata.py): the test scenes, a second plain
statement of the rule, and the CPU stand-in with numpy bodies of the two new methods, of mask_clean and of the entries the feature must
compose with.  A plain module (not collected); importing it does not touch the GPU."""
import collections

import numpy as np
import torch

from sam_road_amd.mask_clean import mask_clean_ref
from sam_road_amd.radiometry import apply_luts
from sam_road_amd.resample import resample_ref

from scene_kit import SceneStandIn, np_pad, rect_scene

BLOBS = ((1, 5), (3, 4), (5, 5), (5, 8))                  # interior blobs of 5, 12, 25 and 40 hit pixels
N_SINGLES = 12
COLLAR = 0.42                                             # the collar: the triangle y / H + x / W < COLLAR at the scene's origin


def collar_of(H, W, frac=COLLAR, shift=0):
    yy, xx = np.mgrid[0:H, 0:W]
    return (yy - shift) * W + (xx - shift) * H < frac * H * W


def paint(raw, value, fringe, seed, frac=COLLAR):
    """raw [H,W,C] IN PLACE: a triangular collar of `value` (every band), a 2-3 px fringe of the levels `fringe` beside it, N_SINGLES
    isolated single pixels and the four BLOBS of the value in the interior.  Returns the bool [H,W] of the pixels that now hold the
    value (collar, singles and blobs; natural pixels that happen to hold it are not listed)."""
    H, W, C = raw.shape
    rng = np.random.default_rng(seed)
    collar = collar_of(H, W, frac)
    edge = collar_of(H, W, frac, 3) & ~collar
    painted = collar.copy()
    raw[collar] = value
    raw[edge] = np.asarray(fringe)[rng.integers(0, len(fringe), size=(int(edge.sum()), C))]
    free = ~collar_of(H, W, frac, 12)                     # the interior, well away from the fringe
    free[:6] = free[-6:] = False
    free[:, :6] = free[:, -6:] = False
    spots = []
    for h, w in BLOBS + ((1, 1),) * N_SINGLES:
        for _ in range(1000):
            y, x = int(rng.integers(6, H - 6 - h)), int(rng.integers(6, W - 6 - w))
            if free[y - 3:y + h + 3, x - 3:x + w + 3].all():
                break
        else:
            raise AssertionError("no room for a blob")
        raw[y:y + h, x:x + w] = value
        painted[y:y + h, x:x + w] = True
        free[y - 3:y + h + 3, x - 3:x + w + 3] = False
        spots.append((y, x, h, w))
    return painted


def collar_scene(H, W, seed, value=0):
    """The kit scene of the feature: rect_scene (its natural pixels lifted to >= 8, so that only what is painted hits at tolerance <= 3)
    with paint()'s collar, fringe of levels 1..3, singles and blobs of `value`.  (u8 [H,W,3], painted bool [H,W])"""
    img = np.maximum(rect_scene(H, W, seed), 8)
    painted = paint(img, value, (1, 2, 3), seed)
    return np.ascontiguousarray(img), painted


def plain_scene(H, W, seed):
    """A scene without a hit pixel at value 0, tolerance <= 3."""
    return np.ascontiguousarray(np.maximum(rect_scene(H, W, seed), 8))


def raw16_scene(H, W, seed, value=65535, select=(2, 1, 0)):
    """u16 [H,W,4]: band select[b] = channel b of rect_scene times 200 plus 1000 (well inside the range), the fourth band their mean; the
    collar, singles and blobs hold `value`, the fringe the three levels next to it."""
    u8 = rect_scene(H, W, seed).astype(np.uint16)
    raw = np.zeros((H, W, 4), np.uint16)
    for b, s in enumerate(select):
        raw[..., s] = u8[..., b] * 200 + 1000
    raw[..., 3] = (u8.sum(-1) // 3) * 200 + 1000
    near = (value - 1, value - 2, value - 3) if value > 3 else (value + 1, value + 2, value + 3)
    painted = paint(raw, value, near, seed)
    return np.ascontiguousarray(raw), painted


# ---- the rule, restated in plain loops ---------------------------------------------------------------------------------------------------------
def loops_ref(raw, value, tolerance=0, any_band=False, min_area=1, connectivity=8, grow=0, valid=None):
    """valid_out of DESIGN.md §6l: per-pixel loops for the match, a breadth-first flood fill for the area rule, a brute-force window maximum
    for the grow.  Independent of sam_road_amd/nodata.py, of scipy and of the kernels."""
    H, W, C = raw.shape
    levels = 256 if raw.dtype == np.uint8 else 65536
    values = [value] * C if isinstance(value, int) else list(value)
    hit = np.zeros((H, W), bool)
    for y in range(H):
        for x in range(W):
            n = 0
            for c in range(C):
                lo, hi = max(0, values[c] - tolerance), min(levels - 1, values[c] + tolerance)
                n += lo <= int(raw[y, x, c]) <= hi
            hit[y, x] = n > 0 if any_band else n == C
    if min_area > 1:
        steps = [(dy, dx) for dy in (-1, 0, 1) for dx in (-1, 0, 1) if (dy or dx) and (connectivity == 8 or not (dy and dx))]
        seen = np.zeros((H, W), bool)
        for sy in range(H):
            for sx in range(W):
                if seen[sy, sx] or not hit[sy, sx]:
                    continue
                seen[sy, sx] = True
                queue, comp = collections.deque([(sy, sx)]), []
                while queue:
                    y, x = queue.popleft()
                    comp.append((y, x))
                    for dy, dx in steps:
                        yy, xx = y + dy, x + dx
                        if 0 <= yy < H and 0 <= xx < W and not seen[yy, xx] and hit[yy, xx]:
                            seen[yy, xx] = True
                            queue.append((yy, xx))
                if len(comp) < min_area:
                    for p in comp:
                        hit[p] = False
    nodata = hit
    if grow > 0:
        nodata = np.zeros((H, W), bool)
        for y in range(H):
            for x in range(W):
                nodata[y, x] = hit[max(0, y - grow):y + grow + 1, max(0, x - grow):x + grow + 1].any()
    out = ~nodata
    if valid is not None:
        out &= np.asarray(valid) != 0
    return out.astype(np.uint8)


def window_max(src, r):
    """The grow alone, brute force: 1 iff any pixel of the uint8 [H, W] image within Chebyshev distance r inside it is non-zero."""
    H, W = src.shape
    s = src != 0
    out = np.zeros((H, W), np.uint8)
    for y, x in zip(*np.nonzero(s)):
        out[max(0, y - r):y + r + 1, max(0, x - r):x + r + 1] = 1
    return out


# ---- the CPU stand-in --------------------------------------------------------------------------------------------------------------------------
def _np_stack(ragged, table, C, Ha, Wa, mode, fill):
    out = np.zeros((Ha, Wa, 3) if C == 3 else (Ha, Wa), dtype=ragged.dtype)
    for off, H, W, top, left, Hv, Wv, row0 in np.asarray(table).tolist():
        block = ragged[off:off + H * W * C].reshape((H, W, 3) if C == 3 else (H, W))
        out[row0:row0 + Hv, :Wv] = np_pad(block, (top, Hv - H - top, left, Wv - W - left), mode, fill)
    return out


class NodataStandIn(SceneStandIn):
    """The stand-in with the two methods this feature adds, their bodies plain numpy, and — for the paths it must compose with — the
    numpy bodies of mask_clean, scene_resample, the two group entries and the two SCENE_BANDS entries, as their own suites state them.
    Every call of a new method is logged: a run without the key must log none."""

    def __init__(self, cfg, features=()):
        super().__init__(cfg, features)
        self.tables = []

    def scene_nodata_match(self, src, lo, hi, match="all", and_with=None, invert=False, out=None):
        assert src.dtype in (torch.uint8, torch.uint16) and src.is_contiguous() and len(lo) == len(hi) == src.shape[-1] and out is None
        self.calls.append(("nodata_match", tuple(src.shape), tuple(lo), tuple(hi), match, and_with is not None, bool(invert)))
        a = src.numpy().astype(np.int64)
        per = (a >= np.asarray(lo)) & (a <= np.asarray(hi))
        v = per.any(-1) if match == "any" else per.all(-1)
        if invert:
            v = ~v
        if and_with is not None:
            assert and_with.numel() == v.size
            v = v & (and_with.numpy().reshape(v.shape) != 0)
        return torch.from_numpy(np.ascontiguousarray(v.astype(np.uint8)))

    def scene_nodata_grow(self, src, table, r, and_with=None, invert=False, table_dev=None, out=None):
        t = torch.as_tensor(table)
        assert src.dim() == 1 and src.dtype == torch.uint8 and t.dtype == torch.int64 and tuple(t.shape[1:]) == (8,) and 1 <= r <= 16 and out is None
        assert table_dev is None or torch.equal(table_dev, t)
        self.calls.append(("nodata_grow", [tuple(row[:3]) for row in t.tolist()], int(r), and_with is not None, bool(invert)))
        s, res = src.numpy(), np.full(src.numel(), 0xEE, np.uint8)
        for off, H, W in (row[:3] for row in t.tolist()):
            g = window_max(s[off:off + H * W].reshape(H, W), r).astype(bool)
            if invert:
                g = ~g
            if and_with is not None:
                g = g & (and_with.numpy()[off:off + H * W].reshape(H, W) != 0)
            res[off:off + H * W] = g.reshape(-1)
        return torch.from_numpy(res)

    def mask_clean(self, buf, table, table_dev=None, connectivity=8):
        t = torch.as_tensor(table)
        assert buf.dim() == 1 and buf.dtype == torch.uint8 and buf.is_contiguous() and t.dtype == torch.int64 and tuple(t.shape[1:]) == (8,)
        assert table_dev is None or torch.equal(table_dev, t)
        self.calls.append(("mask_clean", [tuple(r[1:6]) for r in t.tolist()], connectivity))
        flat = buf.numpy()                                                   # shares the tensor's memory: in place
        for off, H, W, t_on, min_area, t_peak, _, _ in t.tolist():
            block = flat[off:off + H * W].reshape(H, W)
            block[...] = mask_clean_ref(block.copy(), t_on, min_area, t_peak, connectivity)
        return buf

    def scene_resample(self, t, p, q, out_shape=None, valid_rule=False, zero_where=None):
        self.calls.append(("resample", p, q))
        return torch.from_numpy(resample_ref(t.numpy(), p, q, out_shape, valid_rule, None if zero_where is None else zero_where.numpy()))

    def scene_group_pack(self, ragged, table, C, Ha, Wa, mode="reflect", fill=(0, 0, 0), table_dev=None):
        self.calls.append(("group_pack", int(table.shape[0]), C))
        return torch.from_numpy(_np_stack(ragged.numpy(), table.numpy(), C, int(Ha), int(Wa), mode, fill))

    def scene_group_crop(self, kp, road, table, table_dev=None):
        self.calls.append(("group_crop", int(table.shape[0])))
        t = table.numpy()
        out = np.full((2, int((t[:, 1] * t[:, 2]).sum())), 0xEE, np.uint8)
        for off, H, W, top, left, _, _, row0 in t.tolist():
            for j, m in enumerate((kp, road)):
                out[j, off:off + H * W] = m.numpy()[row0 + top:row0 + top + H, left:left + W].reshape(-1)
        return torch.from_numpy(out)

    def scene_bands_hist(self, src, select, valid=None):
        a = src.numpy().reshape(-1, src.shape[-1])
        levels = 256 if a.dtype == np.uint8 else 65536
        keep = slice(None) if valid is None else valid.numpy().reshape(-1) != 0
        self.calls.append(("bands_hist", tuple(select), valid is not None))
        return torch.from_numpy(np.stack([np.bincount(a[keep, b], minlength=levels) for b in select]).astype(np.uint32))

    def scene_bands_apply(self, src, select, lut):
        self.calls.append(("bands_apply", tuple(select), str(src.dtype)))
        self.tables.append(lut.numpy().copy())
        return torch.from_numpy(np.ascontiguousarray(apply_luts(src.numpy(), list(select), lut.numpy())))


def nodata_calls(net):
    return [c for c in net.calls if c[0] in ("nodata_match", "nodata_grow")]
