"""Pass-2 TopoNet cost against MAX_NEIGHBOR_QUERIES (K): srh_toponet_ragged on ~16 k rows of synthetic queries (40 tiles of ViT-B
embeddings, pairs inside their tile, 70 % valid) at every K, timed with HIP events (median of --iters calls after --warmup), plus the
fused trunk's TFLOP/s from the library's own profile rows (srh_profile_read, class "topo_fused": real key count, ABI 10).
One JSON line per K, then a summary line with pairs/s relative to K = 16.

    python tools/topo_k_bench.py [--ks 1,2,4,8,12,16,17,24,32,48,64 | --all] [--rows 16384] [--out FILE]"""
import argparse
import json
import os
import sys
import warnings

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ISSUE_KS = [1, 2, 4, 8, 12, 16, 17, 24, 32, 48, 64]


def make_net():
    from oracle.synth import synth_state_dict
    from sam_road_amd import Config, SAMRoad
    warnings.simplefilter("ignore")
    net = SAMRoad(Config(dict(SAM_VERSION="vit_b", PATCH_SIZE=512, TOPONET_VERSION="normal", SAM_CKPT_PATH="", ENCODER_DEPTH=1,
                              ENCODER_GLOBAL_ATTN_INDEXES=[])))
    net.load_state_dict(synth_state_dict(net, 1234), strict=True)
    return net.eval().to("cuda")


def queries(K, rows, n_tiles=40, seed=0):
    g = torch.Generator().manual_seed(seed)
    counts = torch.full((n_tiles,), rows // n_tiles, dtype=torch.int64)
    counts[: rows - int(counts.sum())] += 1
    off = np.concatenate([[0], np.cumsum(counts.numpy())]).astype(np.int64)
    R = int(off[-1])
    tile = torch.repeat_interleave(torch.arange(n_tiles, dtype=torch.int32), counts)
    points = (torch.rand(R, 2, generator=g) * 512).floor()
    first = torch.from_numpy(off[:-1])[tile.long()]
    tgt = first[:, None] + (torch.rand(R, K, generator=g) * counts[tile.long()][:, None]).long()
    pairs = torch.stack([torch.arange(R)[:, None].expand(R, K), tgt], -1).to(torch.int32)
    valid = (torch.rand(R, K, generator=g) < 0.7).to(torch.uint8)
    return [t.cuda() for t in (points, tile, pairs, valid)], off


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ks", default=",".join(map(str, ISSUE_KS)))
    ap.add_argument("--all", action="store_true", help="every K from 1 to 64")
    ap.add_argument("--rows", type=int, default=16384)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    a = ap.parse_args()
    ks = list(range(1, 65)) if a.all else [int(k) for k in a.ks.split(",")]
    net = make_net()
    emb = torch.randn(40, 256, 32, 32, generator=torch.Generator().manual_seed(1)).cuda()
    from sam_road_amd import _lib
    ctx = _lib.Context.get(0)
    out = open(a.out, "a") if a.out else None
    res = {}
    for K in ks:
        (points, tile, pairs, valid), off = queries(K, a.rows)
        R = points.shape[0]
        for _ in range(a.warmup):
            net.infer_toponet_ragged(emb, points, tile, pairs, valid, tile_offsets=off)
        torch.cuda.synchronize()
        ts = []
        for _ in range(a.iters):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            net.infer_toponet_ragged(emb, points, tile, pairs, valid, tile_offsets=off)
            e1.record()
            e1.synchronize()
            ts.append(e0.elapsed_time(e1) * 1e3)
        net.check_finite(synchronize=True)
        ctx.profile_enable(True)
        for _ in range(a.iters):
            net.infer_toponet_ragged(emb, points, tile, pairs, valid, tile_offsets=off)
        rows = {r["name"]: r for r in ctx.profile_read()}
        ctx.profile_enable(False)
        tf = rows.get("topo_fused")
        us = float(np.median(ts))
        rec = dict(K=K, rows=R, pairs=R * K, us_per_call=round(us, 1), pairs_per_s=R * K / (us * 1e-6),
                   topo_fused_us=round(tf["ms"] * 1e3 / a.iters, 1) if tf else None,
                   topo_fused_tflops=round(tf["flops"] / (tf["ms"] * 1e-3) / 1e12, 1) if tf and tf["ms"] > 0 else None)
        res[K] = rec
        line = json.dumps(rec)
        print(line, flush=True)
        if out:
            out.write(line + "\n")
    if 16 in res:
        base = res[16]["pairs_per_s"]
        worst = min(res, key=lambda k: res[k]["pairs_per_s"])
        summ = dict(summary=True, pairs_per_s_vs_k16={k: round(r["pairs_per_s"] / base, 3) for k, r in res.items()},
                    worst_k=worst, worst_ratio=round(res[worst]["pairs_per_s"] / base, 3))
        print(json.dumps(summ), flush=True)
        if out:
            out.write(json.dumps(summ) + "\n")


if __name__ == "__main__":
    main()
