#!/usr/bin/env python
"""Cost of TTA: the two permutation kernels at P = 512, B = 64 against what they are measured against IN THE SAME RUN, and
pass 1 of a 2048^2 / 256-tile scene with k orientations against k times the plain pass 1.

  * patch_im2col_oriented, each of the 7 codes, against the unchanged patch_im2col on the same tiles (library event times);
  * scores_unorient, each code, against a device-to-device copy of the same bytes (torch copy_, device events);
  * pass 1 (scene_pass1 + scene_normalise, wall time around a synchronise) for k = 1, 2, 4, 8.
Prints a table and, with --csv PATH, writes the kernel rows there (profiles/tta_kernel_stats.csv).

    python tools/tta_cost.py [--csv profiles/tta_kernel_stats.csv] [--no-scene]
"""
import argparse, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import warnings
import numpy as np, torch
warnings.simplefilter("ignore")
from sam_road_amd import Config, SAMRoad, _lib
from sam_road_amd.inferencer import TTA_NAMES

ap = argparse.ArgumentParser()
ap.add_argument("--csv", default=None)
ap.add_argument("--no-scene", action="store_true")
args = ap.parse_args()
dev = torch.device("cuda", 0)
P, B, N = 512, 64, 20
base = dict(SAM_VERSION="vit_b", PATCH_SIZE=P, TOPONET_VERSION="normal", SAM_CKPT_PATH="", DATASET="cityscale", INFER_BATCH_SIZE=B,
            SAMPLE_MARGIN=64, INFER_PATCHES_PER_EDGE=16)
net = SAMRoad(Config(base))
g = torch.Generator().manual_seed(1234)
sd = {k: (1.0 + 0.1 * torch.randn(v.shape, generator=g) if v.dim() == 1 and k.endswith("weight") else 0.02 * torch.randn(v.shape, generator=g))
      for k, v in net.state_dict().items()}
net.load_state_dict(sd, strict=True)
net.eval().to(dev)
H = W = 2048
rng = np.random.default_rng(0)
scene = torch.from_numpy(rng.integers(0, 256, size=(H, W, 3), dtype=np.uint8)).to(dev)
xs = [round(v) for v in np.linspace(64, W - P - 64, 16)]
xy_all = torch.tensor([[x, y] for x in xs for y in xs], dtype=torch.int32, device=dev)
xy = xy_all[:B].contiguous()
ctx = _lib.Context.get(0)
rows_out = []


def lib_us(fn, cls):
    """Mean library event time of class `cls` per launch over N calls of fn (after 3 warm-up calls), in us."""
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ctx.profile_read(); ctx.profile_enable(True)
    for _ in range(N):
        fn()
    torch.cuda.synchronize()
    rows = {r["name"]: r for r in ctx.profile_read()}
    ctx.profile_enable(False)
    r = rows[cls]
    assert r["launches"] == N, (cls, r)
    return 1e3 * r["ms"] / N


def event_us(fn):
    for _ in range(3):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(N):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return 1e3 * e0.elapsed_time(e1) / N


plain = lib_us(lambda: net.op_patch_im2col(scene, xy, orient=0), "patch_im2col")
print(f"P = {P}, B = {B}: patch_im2col (unchanged kernel) {plain:8.2f} us")
rows_out.append(("patch_im2col", "id", plain, 1.0))
for code in range(1, 8):
    us = lib_us(lambda: net.op_patch_im2col(scene, xy, orient=code), "patch_im2col_oriented")
    print(f"    patch_im2col_oriented {TTA_NAMES[code]:<15s} {us:8.2f} us   x {us / plain:.2f} of patch_im2col (expectation <= 3)")
    rows_out.append(("patch_im2col_oriented", TTA_NAMES[code], us, us / plain))
scores = torch.randn((B, P, P, 2), device=dev)
out = torch.empty_like(scores)
copy = event_us(lambda: out.copy_(scores))
print(f"device-to-device copy of {scores.numel() * 4 / 1e6:.1f} MB {copy:8.2f} us")
rows_out.append(("d2d_copy", "-", copy, 1.0))
for code in range(1, 8):
    us = lib_us(lambda: net.op_scores_unorient(scores, code), "scores_unorient")
    print(f"    scores_unorient {TTA_NAMES[code]:<15s} {us:8.2f} us   x {us / copy:.2f} of the copy (expectation <= 3)")
    rows_out.append(("scores_unorient", TTA_NAMES[code], us, us / copy))
if args.csv:
    with open(args.csv, "w") as f:
        f.write("kernel,orientation,us_per_launch_P512_B64,ratio_to_baseline_of_same_run\n")
        for r in rows_out:
            f.write(f"{r[0]},{r[1]},{r[2]:.2f},{r[3]:.3f}\n")
if args.no_scene:
    sys.exit(0)


def pass1(codes):
    kw = {} if len(codes) == 1 else dict(tta=codes)
    kp, road, _ = net.scene_pass1(scene, xy_all, B, **kw)
    net.scene_normalise(kp, road, xy_all if len(codes) == 1 else xy_all.repeat(len(codes), 1))


def wall_ms(fn, n=3):
    fn()
    torch.cuda.synchronize(); t0 = time.perf_counter()
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0) / n


t1 = wall_ms(lambda: pass1([0]))
print(f"pass 1 of a {H} x {W} scene, {len(xy_all)} tiles, plain: {t1:.2f} ms")
for codes in ([0, 5], [0, 1, 5, 6], list(range(8))):
    t = wall_ms(lambda: pass1(codes))
    k = len(codes)
    print(f"    k = {k}: {t:8.2f} ms = {t / (k * t1):.4f} x k x plain (expectation <= 1.03)")
