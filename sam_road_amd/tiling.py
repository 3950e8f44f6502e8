"""Sliding-window tile grid of the scene (reference dataset.py:56-67)."""
import numpy as np


def get_patch_info_one_img(image_index, image_size, sample_margin, patch_size, patches_per_edge):
    """List of (image_index, (x0, y0), (x1, y1)); x outer / y inner; origins are the python-rounded
    points of linspace(margin, size - (patch + margin), n)."""
    lo = sample_margin
    hi = image_size - (patch_size + sample_margin)
    origins = [round(v) for v in np.linspace(start=lo, stop=hi, num=patches_per_edge)]
    return [(image_index, (x, y), (x + patch_size, y + patch_size)) for x in origins for y in origins]


def patches_per_axis(patches_per_edge):
    """INFER_PATCHES_PER_EDGE -> (n_y, n_x).  An int is the same count on both axes (the reference's reading); a sequence of
    two ints is [n_y, n_x], in the order of img.shape.  Anything else raises ValueError."""
    def is_count(v):
        return isinstance(v, (int, np.integer)) and not isinstance(v, (bool, np.bool_)) and v >= 1
    n = patches_per_edge
    if is_count(n):
        return int(n), int(n)
    if isinstance(n, (list, tuple)) and len(n) == 2 and all(is_count(v) for v in n):
        return int(n[0]), int(n[1])
    raise ValueError(f"INFER_PATCHES_PER_EDGE must be a positive int or a pair of positive ints [n_y, n_x], got {n!r}")


def get_patch_info_hw(image_index, height, width, sample_margin, patch_size, patches_per_edge):
    """get_patch_info_one_img for a rectangular scene: the same rule on each axis on its own — x origins from `width` and
    n_x, y origins from `height` and n_y (patches_per_edge: see patches_per_axis), x outer / y inner.  For height == width
    and n_x == n_y this is get_patch_info_one_img's list, element for element."""
    n_y, n_x = patches_per_axis(patches_per_edge)
    lo = sample_margin
    xs = [round(v) for v in np.linspace(start=lo, stop=width - (patch_size + sample_margin), num=n_x)]
    ys = [round(v) for v in np.linspace(start=lo, stop=height - (patch_size + sample_margin), num=n_y)]
    return [(image_index, (x, y), (x + patch_size, y + patch_size)) for x in xs for y in ys]


def shard_tiles(n_tiles, world_size, rank):
    """Contiguous chunk of the tile list owned by `rank` (x-outer order makes each chunk a
    band of column strips).  Returns (begin, end)."""
    # balanced: chunk sizes differ by at most one and no rank is empty whenever n_tiles >= world_size
    return n_tiles * rank // world_size, n_tiles * (rank + 1) // world_size
