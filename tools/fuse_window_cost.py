#!/usr/bin/env python
"""Cost of FUSE_WINDOW on the 2048^2 / 256-tile CityScale config of tools/scene_bench.py: library event times of the canvas
kernel classes without and with a Hann window, then infer_one_img and the pipelined infer_imgs with and without it.  Under
`rocprofv3 --kernel-trace --stats --output-format csv -- python tools/fuse_window_cost.py --kernels-only` the kernel stats of the same
scenes are profiles/fuse_window_kernel_stats.csv.

    python tools/fuse_window_cost.py [--kernels-only]
"""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import warnings
import numpy as np, torch
warnings.simplefilter("ignore")
from sam_road_amd import Config, SAMRoad, _lib
from sam_road_amd.inferencer import infer_one_img, infer_imgs
dev = torch.device("cuda", 0)
base = dict(SAM_VERSION="vit_b", PATCH_SIZE=512, TOPONET_VERSION="normal", SAM_CKPT_PATH="", DATASET="cityscale", INFER_BATCH_SIZE=64,
            SAMPLE_MARGIN=64, INFER_PATCHES_PER_EDGE=16, ITSC_THRESHOLD=0.248, ROAD_THRESHOLD=0.364, TOPO_THRESHOLD=0.499,
            ITSC_NMS_RADIUS=8, ROAD_NMS_RADIUS=16, NEIGHBOR_RADIUS=64, MAX_NEIGHBOR_QUERIES=16)
cfgs = (("uniform", Config(base)), ("hann", Config(dict(base, FUSE_WINDOW="hann"))))
net = SAMRoad(cfgs[0][1])
g = torch.Generator().manual_seed(1234)
sd = {}
for k, v in net.state_dict().items():
    sd[k] = 1.0 + 0.1 * torch.randn(v.shape, generator=g) if v.dim() == 1 and k.endswith("weight") else 0.02 * torch.randn(v.shape, generator=g)
sd["map_decoder.7.weight"] = 16.0 * torch.randn(sd["map_decoder.7.weight"].shape, generator=g)
sd["map_decoder.7.bias"] = torch.full_like(sd["map_decoder.7.bias"], -2.2)
net.load_state_dict(sd, strict=True)
net.eval().to(dev)
H = W = 2048
rng = np.random.default_rng(0)
img = np.kron(rng.integers(0, 256, size=(H // 8, W // 8, 3)).astype(np.float32), np.ones((8, 8, 1), np.float32)).astype(np.uint8)
for _ in range(2):
    for _, cfg in cfgs:
        res = infer_one_img(net, img, cfg)
ctx = _lib.Context.get(0)
N = 5
for name, cfg in cfgs:
    ctx.profile_read(); ctx.profile_enable(True)
    for _ in range(N):
        res = infer_one_img(net, img, cfg)
    torch.cuda.synchronize()
    rows = ctx.profile_read(); ctx.profile_enable(False)
    print(f"--- {name}: library event times per class, mean of {N} scenes ({res[0].shape[0]} graph points, {res[1].shape[0]} edges)")
    for r in sorted(rows, key=lambda r: -r["ms"]):
        if r["name"].startswith("scene_"):
            print(f"    {r['name']:<20s} launches/scene {r['launches'] / N:5.1f}  ms/scene {r['ms'] / N:8.4f}  us/launch {1e3 * r['ms'] / max(1, r['launches']):8.2f}")
if "--kernels-only" in sys.argv:
    sys.exit(0)
for name, cfg in cfgs:
    torch.cuda.synchronize(); t0 = time.perf_counter()
    for _ in range(N):
        infer_one_img(net, img, cfg)
    torch.cuda.synchronize()
    print(f"infer_one_img {name}: {1e3 * (time.perf_counter() - t0) / N:.2f} ms per scene")
for name, cfg in cfgs:
    list(infer_imgs(net, (img for _ in range(3)), cfg))
    runs = []
    for _ in range(3):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        list(infer_imgs(net, (img for _ in range(12)), cfg))
        torch.cuda.synchronize(); runs.append(1e3 * (time.perf_counter() - t0) / 12)
    print(f"infer_imgs (12 scenes) {name}: {['%.2f' % r for r in runs]} ms per scene")
