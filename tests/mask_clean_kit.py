"""What the MASK_CLEAN tests share (tests/test_mask_clean_host.py, tests/test_gpu_mask_clean.py): a second statement of the rule, the
mask patterns, and the composition that pins the feature.  A plain module (not collected); importing it does not touch the GPU."""
import collections
import contextlib

import numpy as np

from sam_road_amd import inferencer as inf
from sam_road_amd.mask_clean import mask_clean_ref

SEGMENT = 64             # csrc/mask_clean_piece.hpp: a wave owns 64 consecutive pixels of a row
WORKGROUP = 4            # and a workgroup four consecutive segments


def flood_clean(m, t_on, min_area=1, t_peak=0, connectivity=8):
    """The rule of DESIGN.md §6k by a breadth-first flood fill: independent of scipy.ndimage and of the kernels' union-find."""
    H, W = m.shape
    out, seen = m.copy(), np.zeros((H, W), bool)
    steps = [(dy, dx) for dy in (-1, 0, 1) for dx in (-1, 0, 1) if (dy or dx) and (connectivity == 8 or not (dy and dx))]
    for sy in range(H):
        for sx in range(W):
            if seen[sy, sx] or m[sy, sx] < t_on:
                continue
            seen[sy, sx] = True
            queue = collections.deque([(sy, sx)])
            comp = []
            while queue:
                y, x = queue.popleft()
                comp.append((y, x))
                for dy, dx in steps:
                    yy, xx = y + dy, x + dx
                    if 0 <= yy < H and 0 <= xx < W and not seen[yy, xx] and m[yy, xx] >= t_on:
                        seen[yy, xx] = True
                        queue.append((yy, xx))
            if len(comp) < min_area or max(int(m[p]) for p in comp) < t_peak:
                for p in comp:
                    out[p] = 0
    return out


def spiral(H, W):
    """A 1-pixel path wound inwards from (0, 0) with one pixel of background between its turns: ONE component, the longest chain."""
    f = np.zeros((H, W), bool)
    inside = lambda y, x: 0 <= y < H and 0 <= x < W
    y = x = d = turns = 0
    f[0, 0] = True
    step = ((0, 1), (1, 0), (0, -1), (-1, 0))
    while turns < 2:
        ny, nx = y + step[d][0], x + step[d][1]
        my, mx = ny + step[d][0], nx + step[d][1]
        if inside(ny, nx) and not f[ny, nx] and not (inside(my, mx) and f[my, mx]):
            y, x, turns = ny, nx, 0
            f[y, x] = True
        else:
            d, turns = (d + 1) % 4, turns + 1
    return f


def pattern(kind, H, W, seed=0):
    """bool [H, W], True = foreground."""
    yy, xx = np.mgrid[0:H, 0:W]
    if kind == "all":                                     # one component of H * W pixels
        return np.ones((H, W), bool)
    if kind == "checker":                                 # one component under 8, all singletons under 4
        return (yy + xx) % 2 == 1
    if kind == "spiral":
        return spiral(H, W)
    if kind == "comb":                                    # teeth in every second column, joined by the LAST row only: labels merge late
        return (xx % 2 == 0) | (yy == H - 1)
    if kind == "u":                                       # two arms at the left and right edge that meet only in the last row
        return (xx == 0) | (xx == W - 1) | (yy == H - 1)
    if kind == "diag":                                    # diagonals of both directions
        return ((xx + yy) % 5 == 0) | ((xx - yy) % 7 == 0)
    if kind == "corner":                                  # 3 x 3 blobs left and right of every 64-column border that touch only diagonally:
        f = np.zeros((H, W), bool)                        # segment corners everywhere, workgroup corners where the segment number is 4 j
        for cx in range(SEGMENT, W + 3, SEGMENT):
            for k in range((H + 2) // 3):
                x0 = cx if k % 2 else cx - 3
                f[3 * k:3 * k + 3, max(0, x0):max(0, min(W, x0 + 3))] = True
        return f
    if kind.startswith("r"):                              # random at density 0.NN
        return np.random.default_rng(1000 + seed).random((H, W)) < int(kind[1:]) / 100.0
    raise KeyError(kind)


PATTERNS = ("all", "checker", "spiral", "comb", "u", "diag", "corner", "r30", "r41", "r50", "r60")


def levels(fg, t_on, seed=0):
    """A uint8 mask whose foreground is exactly fg at threshold t_on (1 <= t_on <= 255): levels t_on .. 255 on it, 0 .. t_on - 1 elsewhere."""
    rng = np.random.default_rng(2000 + seed)
    hi, lo = rng.integers(t_on, 256, size=fg.shape), rng.integers(0, t_on, size=fg.shape)
    return np.where(fg, hi, lo).astype(np.uint8)


def clean_pair(plan, kp, road):
    """mask_clean_ref of the two masks of a scene under a MaskCleanPlan."""
    return (mask_clean_ref(kp, *plan.keypoint, plan.connectivity), mask_clean_ref(road, *plan.road, plan.connectivity))


@contextlib.contextmanager
def cleaned_before_extraction(plan, seen=None):
    """The composition that pins the feature: inside the block the EXISTING pipeline (no key) extracts its graph points from
    mask_clean_ref of its two masks — everything else, pass 2 included, is the code as it stands.  seen: a list that receives the
    cleaned (kp, road) pairs in call order."""
    orig = inf.extract_graph_points

    def wrapped(kp, road, config, **kw):
        pair = clean_pair(plan, np.asarray(kp), np.asarray(road))
        if seen is not None:
            seen.append(pair)
        return orig(pair[0], pair[1], config, **kw)

    inf.extract_graph_points = wrapped
    try:
        yield
    finally:
        inf.extract_graph_points = orig


def composed(plan, run):
    """run() -> list of (nodes, edges, kp, road) of a run WITHOUT the key; returns what the run WITH the key must equal, bit for bit: the
    nodes and edges of that run with its masks cleaned before the point extraction, and the cleaned masks."""
    with cleaned_before_extraction(plan):
        results = run()
    return [(n, e) + clean_pair(plan, kp, road) for n, e, kp, road in results]
