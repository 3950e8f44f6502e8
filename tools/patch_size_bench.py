#!/usr/bin/env python
"""Timing of the PATCH_SIZE values other than 256 / 512 / 1024 (bench.py measures the shipped configs only).

  python tools/patch_size_bench.py attn  [--sizes 24,32,48] [--B 16] [--iters 20]
      global attention alone (srh_op_attention, win = S, ViT-B: 12 heads x 64) per size: ms per call and TFLOP/s.  Run it once more
      with SRH_LIB_PATH pointing at another build (e.g. the parent commit's, whose only kernel for S not in {16, 32, 64} is
      attn_generic_kernel) for the A/B on the same box.
  python tools/patch_size_bench.py model [--sizes 384,768] [--B 16] [--steps 10] [--warmup 3]
      full-depth ViT-B infer_masks_and_img_features (encoder + map_decoder) on synthetic weights: ms per step and tiles/s.
      Under `rocprofv3 --kernel-trace --stats -- python tools/patch_size_bench.py model --sizes 384 --steps 3` the kernel table
      shows which global attention kernel each size runs.
One JSON line per measurement."""
import argparse
import ctypes as C
import json
import os
import sys
import warnings

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sam_road_amd import _lib  # noqa: E402


def _p(t):
    return C.c_void_p(t.data_ptr())


def _time(fn, iters, warm):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def bench_attn(sizes, B, iters):
    ctx = _lib.Context.get(0)
    heads, hd = 12, 64
    D = heads * hd
    for S in sizes:
        g = torch.Generator().manual_seed(S)
        qkv = (torch.randn(B * S * S, 3 * D, generator=g) * 1.5).half().cuda()
        bias = (torch.randn(3 * D, generator=g) * 0.5).half().cuda()
        rel_h = (torch.randn(2 * S - 1, hd, generator=g) * 0.3).half().cuda()
        rel_w = (torch.randn(2 * S - 1, hd, generator=g) * 0.3).half().cuda()
        out = torch.empty((B * S * S, D), device="cuda", dtype=torch.half)

        def run():
            ctx.check(ctx.lib.srh_op_attention(ctx.handle, _p(qkv), _p(rel_h), _p(rel_w), _p(bias), B, S, heads, S, _p(out), None),
                      "srh_op_attention")
        ms = _time(run, iters, 3)
        flops = 4.0 * B * heads * S ** 4 * hd          # the two products over the real S^2 x S^2 scores (as api_model.hip attn_flops)
        print(json.dumps({"op": "global_attention", "patch": 16 * S, "S": S, "B": B, "heads": heads, "hd": hd, "ms": round(ms, 4),
                          "tflops": round(flops / (ms * 1e-3) / 1e12, 1), "lib": os.path.basename(os.path.dirname(_lib.LIB_PATH))}),
              flush=True)


def bench_model(sizes, B, steps, warmup):
    from oracle.synth import synth_state_dict, synth_tiles
    from sam_road_amd import Config, SAMRoad
    warnings.simplefilter("ignore")
    for S in sizes:
        patch = 16 * S
        net = SAMRoad(Config(dict(SAM_VERSION="vit_b", PATCH_SIZE=patch, TOPONET_VERSION="normal", SAM_CKPT_PATH="")))
        net.load_state_dict(synth_state_dict(net, 1234), strict=True)
        net.eval().to("cuda")
        rgb = synth_tiles(B, patch, seed=0).cuda()
        with torch.no_grad():
            ms = _time(lambda: net.infer_masks_and_img_features(rgb), steps, warmup)
        print(json.dumps({"workload": "vitb_encode_decode", "patch": patch, "B": B, "ms_per_step": round(ms, 3),
                          "tiles_per_s": round(B / (ms * 1e-3), 1)}), flush=True)
        del net
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["attn", "model"])
    ap.add_argument("--sizes", default=None, help="comma-separated S = PATCH_SIZE / 16 (attn) or PATCH_SIZE in px (model)")
    ap.add_argument("--B", type=int, default=16)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    if a.what == "attn":
        sizes = [int(s) for s in (a.sizes or "12,20,24,25,32,40,48,63,64").split(",")]
        bench_attn(sizes, a.B, a.iters)
    else:
        sizes = [int(s) // 16 for s in (a.sizes or "384,640,768").split(",")]
        bench_model(sizes, a.B, a.steps, a.warmup)


if __name__ == "__main__":
    main()
