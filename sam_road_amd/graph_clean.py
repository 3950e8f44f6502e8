"""GRAPH_CLEAN: the one statement of how a predicted road graph is cleaned — short dead-end spurs and small connected
components dropped, the remaining edges grouped into chains (road segments) and exported as one polyline per chain — on the host, in
integers.  numpy, scipy.sparse.csgraph and the stdlib only; the device (csrc/graph_clean.hip) must equal graph_clean_ref exactly, both
arrays.  The reference has no such step: its graph leaves as the votes produced it.

    GRAPH_CLEAN: {min_spur: s,          # optional, px, number 0 < s <= 2^20
                  min_component: c,     # optional, px, number 0 < c <= 2^20
                  rounds: r,            # int 1 .. 8, default 1
                  drop_isolated: bool}  # default false, edge_support.filter_graph's
    absent / None / {}: nothing is computed, nothing is launched.  A key without min_spur and min_component is valid: it yields
    attributes and polylines only (as ROAD_WIDTH's).

THE GRAPH is the multigraph that graph_raster.check_graph accepts, as it is: self-loops and parallel edges are allowed and count as they
stand.  All quantities are integers.

EDGE LENGTH.  len_q(e) = floor(16 sqrt(dr^2 + dc^2)) = isqrt(256 (dr^2 + dc^2)): sixteenths of a pixel.  An edge spans at most 16383
pixels per axis, so the argument is at most 256 * 2 * 16383^2 < 2^37 — a 64-bit integer square root — and len_q <= MAX_LEN_Q = 370 704.

DEGREE.  deg(v) = the number of ends of LIVE edges at v; a self-loop counts 2.

CHAIN.  The chains are the classes of the live edges under the transitive closure of "e and f share a node of degree exactly 2"; the
chain id is the smallest edge index of the class.  A chain is what a GIS user calls a road segment.  Its ends are the edge-ends (e, v)
of its edges with deg(v) != 2: none (a ring of degree-2 nodes) or two.  n_leaf = the number of ends with deg = 1, n_junc = the number
with deg >= 3, chain_len_q = the sum of len_q over the chain, in 64 bits (6000 edges of full span already pass 2^31).

COMPONENT.  A connected component of the nodes over the live edges; its id is the smallest node index in it; comp_len_q = the sum of
len_q of its edges, in 64 bits.

ONE ROUND.  All decisions of a round are taken on the same graph, at once.  A live edge is dropped if either test holds:
    its chain is a spur:      n_leaf == 1 and n_junc == 1 and chain_len_q < ceil(16 s)
    its component is small:   comp_len_q < ceil(16 c)
The thresholds are turned into the integers ceil(16 s), ceil(16 c) on the host, exactly, through Fraction (thresholds_q); the comparison
x < 16 s of an integer x is x < ceil(16 s).  So a dead end of length exactly s stays and one of s - 1/16 goes.  A free-standing path (two
leaf ends) is never a spur: only min_component removes it.  A test whose threshold is not stated never holds.

REPEAT.  The round is applied r times, each time on what the round before left: the two short tips of a Y go in round 1, the stem has
become a dead end that round 2 judges.  After the last round ONE MORE PASS analyses the kept graph and decides nothing; its numbers are
the attributes.  Rounds are not cut short when nothing was dropped: the work is the same whatever the graph holds.

THE OUTPUT, indexed by the edges that came in:
    state  uint8 [E]     0 kept, otherwise 4 * round + (1 if spur) + (2 if small component), round 1 .. 8: 5 .. 35
    out    int32 [E, 4]  {chain, component, min(chain_len_q, 2^31 - 1), min(comp_len_q, 2^31 - 1)} of the final pass, ids in the indices
                         that came in; {-1, -1, 0, 0} for a dropped edge.  Every element is defined.
The decisions use the 64-bit sums; only `out` saturates (a chain or component of more than 134 217 727 px reports that length).

THE KEPT GRAPH.  edge_support.filter_graph(nodes, edges, state == 0, drop_isolated).  The chain ids are renumbered to the new edge
indices — the smallest edge of a chain is itself kept, so this is a cumsum of the keep mask — and the component ids to the new node
indices (the smallest node of a component with an edge is not isolated).

THE ATTRIBUTES (clean_attrs), per kept edge: chain, chain_length_px = chain_len_q / 16, component, component_length_px = comp_len_q / 16.

THE POLYLINES (chains, polylines_geojson).  One node-index sequence per chain, in the order of the chain ids; consecutive nodes are
joined by the chain's edges, each exactly once, so a sequence has n_edges + 1 nodes and a ring's first node is also its last.
    a chain with two ends starts at the end whose node index is smaller;
    if both ends are the same node it starts along the smaller edge index;
    a ring starts at its smallest node index and goes along the smaller of that node's two incident edges.
polylines_geojson: one LineString per chain, coordinates and geotransform exactly graph_geojson's (edge_support.py), properties chain,
n_edges, length_px, component, component_length_px, deg_start, deg_end.

What this step does not do is listed in DESIGN.md §7: no gap bridging, no choice among the spurs of a junction, no node merging, no
geometric simplification, thresholds in pixels only."""
import collections
import json
import math
from fractions import Fraction

import numpy as np

from .edge_support import _geotransform, _is_int, _is_num, _ops, filter_graph
from .graph_raster import check_graph

MAX_THRESHOLD = 2 ** 20                                   # px
MAX_ROUNDS = 8
MAX_LEN_Q = 370704                                        # isqrt(256 * 2 * 16383^2)
MAX_ITEMS = 2 ** 26                                       # nodes, edges: 2^26 * MAX_LEN_Q < 2^45, far inside 64 bits
CLAMP = 2 ** 31 - 1
SPUR, SMALL = 1, 2                                        # the reason bits of state
assert MAX_LEN_Q == math.isqrt(256 * 2 * 16383 ** 2)
_KEYS = ("min_spur", "min_component", "rounds", "drop_isolated")

# min_spur / min_component: the number as given, or None; rounds: int; drop_isolated: bool
GraphClean = collections.namedtuple("GraphClean", "min_spur min_component rounds drop_isolated")


def _threshold(name, v):
    if v is None:
        return None
    if not _is_num(v) or not np.isfinite(v) or not 0 < v <= MAX_THRESHOLD:
        raise ValueError(f"GRAPH_CLEAN: {name} must be a number 0 < x <= 2^20 (px), got {v!r}")
    return v if _is_int(v) else float(v)


def check_rounds(r):
    if not _is_int(r) or not 1 <= r <= MAX_ROUNDS:
        raise ValueError(f"GRAPH_CLEAN: rounds must be an int 1 .. {MAX_ROUNDS}, got {r!r}")
    return int(r)


def graph_clean_key_of(v):
    """A GRAPH_CLEAN value (the mapping of the module's docstring) as a GraphClean tuple; None for None / {}.  ValueError for anything
    else: unknown keys, bools used as numbers, values outside their range."""
    if v is None or (isinstance(v, dict) and not v):
        return None
    if isinstance(v, GraphClean):
        return v
    if not isinstance(v, dict):
        raise ValueError(f"GRAPH_CLEAN must be a mapping with {', '.join(_KEYS)}, got {v!r}")
    unknown = sorted(set(v) - set(_KEYS), key=str)
    if unknown:
        raise ValueError(f"GRAPH_CLEAN: unknown key {unknown[0]!r} ({', '.join(_KEYS)})")
    s, c = _threshold("min_spur", v.get("min_spur")), _threshold("min_component", v.get("min_component"))
    r = check_rounds(1 if v.get("rounds") is None else v["rounds"])
    drop = v.get("drop_isolated", False)
    if not isinstance(drop, (bool, np.bool_)):
        raise ValueError(f"GRAPH_CLEAN: drop_isolated must be true or false, got {drop!r}")
    return GraphClean(s, c, r, bool(drop))


def graph_clean_key(config):
    """config.GRAPH_CLEAN as a GraphClean tuple, None without the key; ValueError before any device is touched."""
    return graph_clean_key_of(config.get("GRAPH_CLEAN"))


def filters(key):
    """Does the key state a threshold?"""
    return key is not None and (key.min_spur is not None or key.min_component is not None)


def graph_clean_override(config, enable=None, min_spur=None, min_component=None, rounds=None, drop_isolated=None):
    """The GRAPH_CLEAN mapping with the CLI's flags laid over the config's key: a flag that is given replaces that field, the others stay
    as the config has them; `enable` alone (--graph-polylines) turns an absent key into the attributes-only one, {rounds: 1}.  The
    result is validated."""
    base = config.get("GRAPH_CLEAN")
    graph_clean_key_of(base)
    out = dict(base) if isinstance(base, dict) else {}
    for field, val in (("min_spur", min_spur), ("min_component", min_component), ("rounds", rounds)):
        if val is not None:
            out[field] = val
    if drop_isolated and (out or enable):
        out["drop_isolated"] = True
    if enable and not out:
        out["rounds"] = 1
    graph_clean_key_of(out)
    return out


def threshold_q(v):
    """ceil(16 v) of a threshold, exactly (the number is taken as the rational it is); 0 for None: not stated."""
    return 0 if v is None else math.ceil(16 * Fraction(v))


def thresholds_q(key):
    """(ceil(16 min_spur), ceil(16 min_component)) as the device takes them, 0 where not stated."""
    return threshold_q(key.min_spur), threshold_q(key.min_component)


# ---- the rule --------------------------------------------------------------------------------------------------------------------------------
def edge_len_q(nodes, edges):
    """EDGE LENGTH: int64 [E]."""
    n, e = check_graph(nodes, edges)
    d = n[e[:, 1]].astype(np.int64) - n[e[:, 0]].astype(np.int64)
    return np.array([math.isqrt(v) for v in (256 * (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1])).tolist()], np.int64).reshape(-1)


def _labels_min(n_items, rows, cols):
    """For the graph on n_items items with the undirected links rows[k] -- cols[k]: int64 [n_items], the smallest index of every item's
    connected component."""
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    m = coo_matrix((np.ones(len(rows), np.int8), (rows, cols)), shape=(n_items, n_items))
    _, lab = connected_components(m, directed=False)
    _, first = np.unique(lab, return_index=True)          # per label, the first (smallest) item that carries it
    return first.astype(np.int64)[lab]


def analyse(N, edges, len_q, live):
    """One analysis of the live graph: (deg int64 [N], chain int64 [E], comp int64 [E], chain_len int64 [E], comp_len int64 [E], n_leaf
    [E], n_junc [E]); the per-edge arrays are defined on the live edges (0 / -1 elsewhere)."""
    E = edges.shape[0]
    idx = np.flatnonzero(live)
    a, b = edges[idx, 0].astype(np.int64), edges[idx, 1].astype(np.int64)
    deg = np.bincount(np.concatenate([a, b]), minlength=N).astype(np.int64)
    comp = np.full(E, -1, np.int64)
    chain = np.full(E, -1, np.int64)
    chain_len, comp_len, n_leaf, n_junc = (np.zeros(E, np.int64) for _ in range(4))
    if idx.size == 0:
        return deg, chain, comp, chain_len, comp_len, n_leaf, n_junc
    node_comp = _labels_min(N, a, b)
    comp[idx] = node_comp[a]
    # the two edge-ends of every node of degree 2, side by side: the links of the line graph
    end_node, end_edge = np.concatenate([a, b]), np.concatenate([idx, idx])
    at2 = deg[end_node] == 2
    order = np.argsort(end_node[at2], kind="stable")
    pairs = end_edge[at2][order].reshape(-1, 2)
    chain_all = _labels_min(E, pairs[:, 0], pairs[:, 1])
    chain[idx] = chain_all[idx]
    lq = len_q[idx]
    # integer sums (np.add.at on int64): no float weight enters
    for key, total in ((chain[idx], chain_len), (comp[idx], comp_len)):
        acc = np.zeros(max(N, E), np.int64)
        np.add.at(acc, key, lq)
        total[idx] = acc[key]
    leaf = (deg[a] == 1).astype(np.int64) + (deg[b] == 1)
    junc = (deg[a] >= 3).astype(np.int64) + (deg[b] >= 3)
    for val, total in ((leaf, n_leaf), (junc, n_junc)):
        acc = np.zeros(E, np.int64)
        np.add.at(acc, chain[idx], val)
        total[idx] = acc[chain[idx]]
    return deg, chain, comp, chain_len, comp_len, n_leaf, n_junc


def graph_clean_ref(nodes, edges, spur_q=0, comp_q=0, rounds=1):
    """THE RULE of the module's docstring on the host, vectorised: (state uint8 [E], out int32 [E, 4]).  spur_q / comp_q: the integer
    thresholds ceil(16 s) / ceil(16 c) (thresholds_q), 0 = not stated."""
    n, e = check_graph(nodes, edges)
    rounds = check_rounds(rounds)
    if not _is_int(spur_q) or not _is_int(comp_q) or spur_q < 0 or comp_q < 0:
        raise ValueError(f"GRAPH_CLEAN: the integer thresholds are >= 0, got {spur_q!r}, {comp_q!r}")
    N, E = n.shape[0], e.shape[0]
    if N > MAX_ITEMS or E > MAX_ITEMS:
        raise ValueError(f"GRAPH_CLEAN: at most 2^26 nodes and edges, got {N}, {E}")
    len_q = edge_len_q(n, e)
    state = np.zeros(E, np.uint8)
    live = np.ones(E, bool)
    for r in range(1, rounds + 1):
        _, _, _, chain_len, comp_len, n_leaf, n_junc = analyse(N, e, len_q, live)
        spur = live & (spur_q > 0) & (n_leaf == 1) & (n_junc == 1) & (chain_len < spur_q)
        small = live & (comp_q > 0) & (comp_len < comp_q)
        drop = spur | small
        state[drop] = (4 * r + SPUR * spur + SMALL * small)[drop]
        live &= ~drop
    _, chain, comp, chain_len, comp_len, _, _ = analyse(N, e, len_q, live)
    out = np.stack([chain, comp, np.minimum(chain_len, CLAMP), np.minimum(comp_len, CLAMP)], axis=1)
    out[~live] = (-1, -1, 0, 0)
    return state, np.ascontiguousarray(out.astype(np.int32)).reshape(E, 4)


# ---- the kept graph, its attributes and polylines -----------------------------------------------------------------------------------------------
def _result(state, out, E):
    s, o = np.asarray(state), np.asarray(out)
    if o.size == 0:
        o = np.zeros((0, 4), np.int32)
    if s.shape != (E,) or s.dtype != np.uint8 or o.shape != (E, 4) or o.dtype.kind not in "iu":
        raise ValueError(f"GRAPH_CLEAN: state must be uint8 [{E}] and out an integer [{E}, 4] array, got {s.dtype} {s.shape}, {o.dtype} {o.shape}")
    return s, o.astype(np.int64)


def kept_graph(nodes, edges, state, out, drop_isolated=False):
    """THE KEPT GRAPH: (nodes, edges, keep bool [E], table int64 [E', 4]) — the filtered graph, the keep mask over the edges that came in
    and, per kept edge, {chain, component, chain_len_q, comp_len_q} with the ids renumbered to the kept graph's indices."""
    E = np.asarray(edges).reshape(-1, 2).shape[0]
    s, o = _result(state, out, E)
    keep = s == 0
    new_nodes, new_edges, index = filter_graph(nodes, edges, keep, drop_isolated)
    table = o[keep]
    if table.shape[0]:
        table[:, 0] = (np.cumsum(keep) - 1)[table[:, 0]]
        if drop_isolated:
            new = np.full(np.asarray(nodes).reshape(-1, 2).shape[0], -1, np.int64)
            new[index] = np.arange(index.size)
            table[:, 1] = new[table[:, 1]]
    return new_nodes, new_edges, keep, table


def clean_attrs(table):
    """THE ATTRIBUTES: a list of {chain, chain_length_px, component, component_length_px}, one per kept edge (table: kept_graph's)."""
    t = np.asarray(table).reshape(-1, 4)
    ch, co = t[:, 0].astype(np.int64).tolist(), t[:, 1].astype(np.int64).tolist()
    cl, pl = (t[:, 2] / 16).tolist(), (t[:, 3] / 16).tolist()           # exact: integers below 2^53 over a power of two
    # column lists and dict displays of numbers only: no per-row list, and the collector does not track such a dict (35 000 tracked
    # containers per call cost the writer thread 100 ms of collections)
    return [{"chain": a, "chain_length_px": b, "component": c, "component_length_px": d} for a, b, c, d in zip(ch, cl, co, pl)]


def chains(nodes, edges, chain_ids):
    """THE POLYLINES: a list of (chain id, [node indices]) in the order of the chain ids, oriented as the module's docstring states.
    chain_ids: int [E], equal on two edges iff they belong to one chain (kept_graph's first column, or analyse's)."""
    n, e = check_graph(nodes, edges)
    ids = np.asarray(chain_ids).reshape(-1)
    E = e.shape[0]
    if ids.shape != (E,) or (E and ids.dtype.kind not in "iu"):
        raise ValueError(f"GRAPH_CLEAN: chain_ids must be an integer [{E}] array, got {ids.dtype} {ids.shape}")
    if E == 0:
        return []
    deg = np.bincount(e.reshape(-1), minlength=n.shape[0])
    # the edge-ends of every node, sorted by (node, edge): a node's incident edges in rising order
    end_node = np.concatenate([e[:, 0], e[:, 1]]).astype(np.int64)
    end_edge = np.concatenate([np.arange(E), np.arange(E)])
    order = np.lexsort((end_edge, end_node))
    inc_edge = end_edge[order].tolist()
    start = np.concatenate([[0], np.cumsum(deg)]).tolist()
    el, dl = e.tolist(), deg.tolist()
    by_chain = collections.defaultdict(list)
    for k, c in enumerate(ids.tolist()):
        by_chain[c].append(k)
    result = []
    for c in sorted(by_chain):
        members = by_chain[c]
        ends = sorted((v, k) for k in members for v in el[k] if dl[v] != 2)           # (node, edge): smaller node, then smaller edge
        if len(ends) not in (0, 2):
            raise ValueError(f"GRAPH_CLEAN: chain {c} has {len(ends)} ends: chain_ids are not the chains of this graph")
        if ends:
            v, k = ends[0]
        else:                                              # a ring: its smallest node, along that node's smaller incident edge
            v = min(min(el[k]) for k in members)
            k = inc_edge[start[v]]
        seq = [v]
        for _ in range(len(members)):
            a, b = el[k]
            v = a + b - v
            seq.append(v)
            if dl[v] != 2:
                break
            k0, k1 = inc_edge[start[v]], inc_edge[start[v] + 1]
            k = k1 if k0 == k else k0
        if len(seq) != len(members) + 1:
            raise ValueError(f"GRAPH_CLEAN: chain {c} is not one walk: chain_ids are not the chains of this graph")
        result.append((int(c), seq))
    return result


def polylines_geojson(nodes, edges, table, geotransform=None):
    """THE POLYLINES as a FeatureCollection dict, one LineString per chain in the order of the chain ids.  table: kept_graph's, int
    [E, 4] rows {chain, component, chain_len_q, comp_len_q} of the graph's own edges.  json.dump writes it."""
    n, e = check_graph(nodes, edges)
    t = np.asarray(table).reshape(-1, 4)
    if t.shape[0] != e.shape[0]:
        raise ValueError(f"GRAPH_CLEAN: {t.shape[0]} table rows for {e.shape[0]} edges")
    g = _geotransform(geotransform)
    deg = np.bincount(e.reshape(-1), minlength=n.shape[0]).tolist()
    row = {int(r[0]): r for r in t.tolist()}

    def point(i):
        x, y = float(n[i, 1]) + 0.5, float(n[i, 0]) + 0.5
        return [x, y] if g is None else [g[0] + x * g[1] + y * g[2], g[3] + x * g[4] + y * g[5]]

    feats = []
    for c, seq in chains(n, e, t[:, 0].astype(np.int64)):
        _, comp, cl, pl = row[c]
        feats.append({"type": "Feature", "geometry": {"type": "LineString", "coordinates": [point(i) for i in seq]},
                      "properties": dict(chain=c, n_edges=len(seq) - 1, length_px=cl / 16, component=int(comp), component_length_px=pl / 16,
                                         deg_start=deg[seq[0]], deg_end=deg[seq[-1]])})
    return {"type": "FeatureCollection", "features": feats}


def write_polylines(path, nodes, edges, table, geotransform=None):
    with open(path, "w") as f:
        json.dump(polylines_geojson(nodes, edges, table, geotransform), f)


# ---- the device ------------------------------------------------------------------------------------------------------------------------------
def clean(nodes, edges, key, device=None, net=None):
    """THE RULE on the device (srh_graph_clean): HOST arrays (state uint8 [E], out int32 [E, 4]) equal to graph_clean_ref.  key: a
    GraphClean tuple or its mapping.  net: the model whose device is used; without one the device `device` (default cuda).  Runs on
    torch's current stream and waits for that stream alone."""
    key = graph_clean_key_of(key)
    if key is None:
        raise ValueError("GRAPH_CLEAN: clean() needs a key")
    n, e = check_graph(nodes, edges)
    if e.shape[0] == 0:
        return np.zeros(0, np.uint8), np.zeros((0, 4), np.int32)
    spur_q, comp_q = thresholds_q(key)
    state, out = _ops(device, net).graph_clean(n, e, spur_q=spur_q, comp_q=comp_q, rounds=key.rounds)
    return state.cpu().numpy(), out.cpu().numpy()


def _finish(key, result, state, out):
    nodes, edges, kp_mask, road_mask = result
    new_nodes, new_edges, keep, table = kept_graph(nodes, edges, state, out, key.drop_isolated)
    return (new_nodes, new_edges, kp_mask, road_mask), clean_attrs(table), keep


def apply(key, result, net=None, device=None, return_keep=False):
    """The key applied to `result`, the 4-tuple (nodes, edges, kp_mask, road_mask) of infer_one_img:
    ((nodes, edges, kp_mask, road_mask), attrs) with the kept graph and the attributes of its edges.  key None returns the result
    object itself (and no attributes) and calls nothing.  return_keep: a third element, bool [E] over the edges that came in (None
    without a key), for a caller that carries other per-edge data along."""
    if key is None:
        return (result, None, None) if return_keep else (result, None)
    state, out = clean(result[0], result[1], key, device=device, net=net)
    res = _finish(key, result, state, out)
    return res if return_keep else res[:2]


def apply_ref(key, result, return_keep=False):
    """apply() on the host statement alone."""
    if key is None:
        return (result, None, None) if return_keep else (result, None)
    res = _finish(key, result, *graph_clean_ref(result[0], result[1], *thresholds_q(key), key.rounds))
    return res if return_keep else res[:2]


def table_of(attrs):
    """kept_graph's table back from the attributes of a kept graph (the CLI carries the attributes): int64 [E, 4]."""
    return np.array([[a["chain"], a["component"], round(a["chain_length_px"] * 16), round(a["component_length_px"] * 16)] for a in attrs],
                    np.int64).reshape(-1, 4)
