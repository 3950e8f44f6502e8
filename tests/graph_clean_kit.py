"""What the GRAPH_CLEAN tests share (tests/test_graph_clean_host.py, tests/test_gpu_graph_clean.py): the hand-built cases with their
answers worked out on paper, and the graph makers.  A plain module: no test in it.

Lengths are in sixteenths of a pixel: an axis-aligned edge of d pixels has len_q = 16 d; the edge (1, 1) has isqrt(512) = 22 and the
edge (7, 5) has isqrt(256 * 74) = 137, so the two in a row make 159 = 160 - 1: a length of 10 px less one sixteenth.  state is
4 * round + 1 (spur) + 2 (small component); DEAD is the out row of a dropped edge."""
import numpy as np
import torch

import road_width_kit as wk

from sam_road_amd.graph_clean import graph_clean_ref

DEAD = [-1, -1, 0, 0]
CLAMP = 2 ** 31 - 1


def case(name, nodes, edges, state, out, min_spur=None, min_component=None, rounds=1):
    key = {k: v for k, v in (("min_spur", min_spur), ("min_component", min_component)) if v is not None}
    key["rounds"] = rounds
    return dict(name=name, nodes=np.array(nodes, np.int32).reshape(-1, 2), edges=np.array(edges, np.int32).reshape(-1, 2), key=key,
                state=np.array(state, np.uint8), out=np.array(out, np.int32).reshape(-1, 4))


def _long_chain():
    """6000 edges of span 16383 on both axes (len_q 370 704 each, 2 224 224 000 > 2^31 in all) from a junction, node 0, which also
    carries two one-edge arms of 16383 px (len_q 262 128).  min_spur 2^20 px = 16 777 216 sixteenths: the arms are spurs and go; the
    chain is a dead end whose 64-bit length is far above the threshold and stays — a sum wrapped to 32 bits would be negative and drop
    it.  The final pass sees one path of 6000 edges: chain 0, component 0, both lengths clamped."""
    n = 6000
    k = np.arange(n + 1, dtype=np.int64) * 16383
    nodes = np.concatenate([np.stack([k, k], 1), [[-16383, 0], [0, -16383]]])
    edges = np.concatenate([np.stack([np.arange(n), np.arange(1, n + 1)], 1), [[0, n + 1], [0, n + 2]]])
    return case("chain of 6000 full-span edges", nodes, edges, [0] * n + [5, 5], [[0, 0, CLAMP, CLAMP]] * n + [DEAD, DEAD], min_spur=2 ** 20,
                min_component=2 ** 20)


def hand_cases():
    square = [[0, 0], [0, 5], [5, 5], [5, 0]]
    ring = [[0, 1], [1, 2], [2, 3], [3, 0]]
    star_n = [[0, 0], [0, 10], [1, 1], [8, 6], [0, -50]]                 # arm A 160, arm B 22 + 137 = 159, arm C 800
    star_e = [[0, 1], [0, 2], [2, 3], [0, 4]]
    two_n = [[0, 0], [0, 10], [20, 20], [21, 21], [28, 26]]              # a component of 160 and one of 159
    two_e = [[0, 1], [2, 3], [3, 4]]
    y_n = [[0, 0], [0, 3], [3, 0], [0, -10], [100, -10], [-100, -10]]    # tips 48, 48; stem 160; two arms of 1600 at the stem's far end
    y_e = [[0, 1], [0, 2], [0, 3], [3, 4], [3, 5]]
    return [
        case("single edge", [[0, 0], [0, 10]], [[0, 1]], [0], [[0, 0, 160, 160]], min_spur=20, min_component=10),
        case("single edge below c", [[0, 0], [0, 10]], [[0, 1]], [6], [DEAD], min_component=10.0625),
        case("self-loop alone", [[5, 5]], [[0, 0]], [0], [[0, 0, 0, 0]], min_spur=5),
        case("self-loop alone, small", [[5, 5]], [[0, 0]], [6], [DEAD], min_component=1),
        # the loop's two ends lie at a junction (degree 3): never a spur; the other edge is a dead end of exactly 10 px
        case("self-loop on a junction, s = 10", [[0, 0], [0, 10]], [[0, 0], [0, 1]], [0, 0], [[0, 0, 0, 160], [1, 0, 160, 160]], min_spur=10),
        case("self-loop on a junction, s = 11", [[0, 0], [0, 10]], [[0, 0], [0, 1]], [0, 5], [[0, 0, 0, 0], DEAD], min_spur=11),
        case("two parallel edges", [[0, 0], [0, 4]], [[0, 1], [1, 0]], [0, 0], [[0, 0, 128, 128]] * 2, min_spur=100),
        case("path of 3", [[0, 0], [0, 3], [0, 7], [0, 12]], [[0, 1], [1, 2], [2, 3]], [0] * 3, [[0, 0, 192, 192]] * 3, min_spur=1000, min_component=12),
        case("path of 3 below c", [[0, 0], [0, 3], [0, 7], [0, 12]], [[0, 1], [1, 2], [2, 3]], [6] * 3, [DEAD] * 3, min_spur=1000, min_component=12.01),
        case("ring", square, ring, [0] * 4, [[0, 0, 320, 320]] * 4, min_spur=1000, min_component=20),
        case("lollipop, tail of exactly s", square + [[10, 0]], ring + [[3, 4]], [0] * 5, [[0, 0, 320, 400]] * 4 + [[4, 0, 80, 400]], min_spur=5),
        case("lollipop, tail below s", square + [[10, 0]], ring + [[3, 4]], [0] * 4 + [5], [[0, 0, 320, 320]] * 4 + [DEAD], min_spur=6),
        # s = 10: the arm of exactly 160 stays, the arm of 159 goes; the centre then has degree 2 and arms A and C are one chain
        case("star, s = 10", star_n, star_e, [0, 5, 5, 0], [[0, 0, 960, 960], DEAD, DEAD, [0, 0, 960, 960]], min_spur=10),
        case("star, s = 10 - 1/16", star_n, star_e, [0] * 4, [[0, 0, 160, 1119], [1, 0, 159, 1119], [1, 0, 159, 1119], [3, 0, 800, 1119]], min_spur=9.9375),
        case("component exactly at c", two_n, two_e, [0, 6, 6], [[0, 0, 160, 160], DEAD, DEAD], min_component=10),
        case("spur and small at once", two_n[:2] + [[5, 0], [-5, 0]], [[0, 1], [0, 2], [0, 3]], [7] * 3, [DEAD] * 3, min_spur=11, min_component=100),
        case("Y, one round", y_n, y_e, [5, 5, 0, 0, 0], [DEAD, DEAD, [2, 0, 160, 3360], [3, 0, 1600, 3360], [4, 0, 1600, 3360]], min_spur=12),
        case("Y, two rounds", y_n, y_e, [5, 5, 9, 0, 0], [DEAD, DEAD, DEAD, [3, 3, 3200, 3200], [3, 3, 3200, 3200]], min_spur=12, rounds=2),
        case("attributes only", y_n, y_e, [0] * 5, [[0, 0, 48, 3456], [1, 0, 48, 3456], [2, 0, 160, 3456], [3, 0, 1600, 3456], [4, 0, 1600, 3456]], rounds=3),
        _long_chain(),
    ]


# ---- graph makers ------------------------------------------------------------------------------------------------------------------------------
def random_multigraph(rng, max_nodes=40, max_edges=60):
    """A small multigraph with self-loops and parallel edges: (nodes int32 [N, 2], edges int32 [E, 2])."""
    N = int(rng.integers(1, max_nodes + 1))
    E = int(rng.integers(1, max_edges + 1))
    nodes = rng.integers(0, 64, (N, 2)).astype(np.int32)
    edges = rng.integers(0, N, (E, 2)).astype(np.int32)
    loops = rng.random(E) < 0.05
    edges[loops, 1] = edges[loops, 0]
    dup = np.flatnonzero(rng.random(E) < 0.08)
    edges[dup] = edges[rng.integers(0, E, dup.size)][:, ::-1 if rng.random() < 0.5 else 1]
    return nodes, edges


def draw_thresholds(rng, nodes, edges):
    """Integer thresholds (spur_q, comp_q) at which a few per cent of this graph's edges drop: around the 40 % quantile of the lengths of
    its dead ends, and around the length of its smallest component when it has at least three different ones.  Either may be 0: not stated.
    The thresholds land on a length or one above it, so "exactly at the threshold" is drawn often."""
    from sam_road_amd import graph_clean as gc
    _, _, _, chain_len, comp_len, n_leaf, n_junc = gc.analyse(nodes.shape[0], edges, gc.edge_len_q(nodes, edges), np.ones(edges.shape[0], bool))
    dead_ends = chain_len[(n_leaf == 1) & (n_junc == 1)]
    spur_q = int(np.quantile(dead_ends, 0.4)) + int(rng.integers(0, 2)) if dead_ends.size and rng.random() < 0.8 else 0
    sizes = np.unique(comp_len)
    comp_q = int(sizes[0]) + int(rng.integers(0, 2)) if sizes.size >= 3 and rng.random() < 0.7 else 0
    return spur_q, comp_q


def sized_graph(rng, N, E):
    """Exactly N nodes and E edges, sparse enough for chains, spurs and several components."""
    nodes = rng.integers(0, 4096, (N, 2)).astype(np.int32)
    a = rng.integers(0, N, E)
    b = np.clip(a + rng.integers(-2, 3, E), 0, N - 1)                    # mostly neighbours in index: paths and small tangles
    far = rng.random(E) < 0.1
    b[far] = rng.integers(0, N, int(far.sum()))
    return nodes, np.stack([a, b], 1).astype(np.int32)


def shuffled_chain(rng, n_edges=5000):
    """One path of n_edges edges whose node and edge indices are shuffled: deep union-find trees, every sum on one root."""
    n = n_edges + 1
    perm = rng.permutation(n)
    pos = np.cumsum(rng.integers(1, 6, (n, 2)), axis=0)
    nodes = np.zeros((n, 2), np.int32)
    nodes[perm] = pos
    edges = np.stack([perm[:-1], perm[1:]], 1)
    flip = rng.random(n_edges) < 0.5
    edges[flip] = edges[flip][:, ::-1]
    return nodes, edges[rng.permutation(n_edges)].astype(np.int32)


def jittered_grid(rng, side=100, gap=0.04, stub=0.08, step=12):
    """A side x side street grid with jittered nodes, a fraction `gap` of its edges missing, a one-edge stub on a fraction `stub` of its
    nodes, two short tips on every fourth stub's end (a Y whose stem is a dead end only once the tips are gone) and side / 2 free-standing
    two-edge fragments: one large component of about 2 side^2 edges with junctions, chains, spurs and rings, and small components."""
    r, c = np.meshgrid(np.arange(side), np.arange(side), indexing="ij")
    nodes = np.stack([r, c], -1).reshape(-1, 2) * step + rng.integers(-3, 4, (side * side, 2))
    idx = np.arange(side * side).reshape(side, side)
    edges = np.concatenate([np.stack([idx[:, :-1].ravel(), idx[:, 1:].ravel()], 1), np.stack([idx[:-1].ravel(), idx[1:].ravel()], 1)])
    edges = edges[rng.random(edges.shape[0]) >= gap]
    at = np.flatnonzero(rng.random(side * side) < stub)
    tips = nodes[at] + rng.integers(-5, 6, (at.size, 2))
    first = side * side
    stubs = np.stack([at, first + np.arange(at.size)], 1)
    forked = first + np.arange(0, at.size, 4)                            # the stub ends that carry two tips
    first += at.size
    twigs = np.concatenate([nodes[at][::4] * 0 + tips[::4] + rng.integers(-2, 3, (forked.size, 2)) for _ in range(2)])
    twig_edges = np.stack([np.concatenate([forked, forked]), first + np.arange(2 * forked.size)], 1)
    first += 2 * forked.size
    n_frag = side // 2
    frag = rng.integers(0, side * step, (n_frag, 1, 2)) + rng.integers(-6, 7, (n_frag, 3, 2))
    f0 = first + 3 * np.arange(n_frag)
    frag_edges = np.concatenate([np.stack([f0, f0 + 1], 1), np.stack([f0 + 1, f0 + 2], 1)])
    nodes = np.concatenate([nodes, tips, twigs, frag.reshape(-1, 2)])
    edges = np.concatenate([edges, stubs, twig_edges, frag_edges])
    return nodes.astype(np.int32), edges[rng.permutation(edges.shape[0])].astype(np.int32)


# ---- the CPU stand-in ---------------------------------------------------------------------------------------------------------------------------
class CleanStandIn(wk.WidthStandIn):
    """The stand-in with graph_clean on the host statement of the rule.  Every call is logged: a run without the key must log none."""

    def graph_clean(self, nodes, edges, spur_q=0, comp_q=0, rounds=1):
        self.calls.append(("graph_clean", int(np.asarray(edges).reshape(-1, 2).shape[0]), int(spur_q), int(comp_q), int(rounds)))
        state, out = graph_clean_ref(nodes, edges, spur_q, comp_q, rounds)
        return torch.from_numpy(state), torch.from_numpy(out)


def clean_calls(net):
    return [c for c in net.calls if c[0] == "graph_clean"]
