"""What the EDGE_SUPPORT tests share: the graphs of graph_raster_kit, an independent restatement of the statistics (per edge from the
brute-force raster of that edge alone, in exact rationals) and the CPU stand-in with the method the feature adds.  A plain module (not
collected); importing it does not touch the GPU."""
import numpy as np
import torch

import graph_raster_kit as gk
from graph_raster_kit import grid_graph, random_graph, star  # noqa: F401

from sam_road_amd.edge_support import edge_support_ref


def brute_stats(nodes, edges, mask, t, on_level, valid=None):
    """int64 [E, 4]: {n, s, n_on, n_invalid} of every edge from graph_raster_kit.brute_raster of that edge ALONE (every pixel of the image,
    its squared distance to the segment against t^2 / 4 in fractions.Fraction), then plain Python sums."""
    H, W = mask.shape
    out = np.zeros((len(edges), 4), np.int64)
    for k, e in enumerate(np.asarray(edges).tolist()):
        cov = gk.brute_raster(nodes, [e], (H, W), t) == 1
        vals = [int(v) for v in mask[cov].tolist()]
        out[k] = (len(vals), sum(vals), sum(v > on_level for v in vals), 0 if valid is None else sum(1 for v in np.asarray(valid)[cov].tolist() if not v))
    return out


class SupportStandIn(gk.RasterStandIn):
    """The stand-in with graph_edge_stats on the host statement of the rule.  Every call is logged: a run without the key must log none."""

    def graph_edge_stats(self, nodes, edges, mask, width=1, on_level=127, valid=None):
        mask = mask.numpy() if torch.is_tensor(mask) else np.asarray(mask)
        valid = valid.numpy() if torch.is_tensor(valid) else valid
        self.calls.append(("graph_edge_stats", tuple(mask.shape), int(width), int(on_level), valid is not None))
        return torch.from_numpy(edge_support_ref(nodes, edges, mask, width, on_level, valid))


def support_calls(net):
    return [c for c in net.calls if c[0] == "graph_edge_stats"]
