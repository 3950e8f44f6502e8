#!/usr/bin/env python
"""Cost of the validity-mask path on the 2048^2 / 256-tile CityScale config of tools/scene_bench.py with a mask that drops
ONE tile: library event times of the scene kernel classes with and without the mask, the wall time of the selection step alone,
infer_one_img and infer_imgs with and without the mask, and (--laps) the SRH_PROFILE_HOST laps of one masked scene, serial and
pipelined.  Under `rocprofv3 --kernel-trace --stats --output-format csv -- python tools/valid_mask_cost.py` the kernel stats of the
same run are profiles/valid_mask_kernel_stats.csv.

    python tools/valid_mask_cost.py [--laps]
"""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import warnings
import numpy as np, torch
warnings.simplefilter("ignore")
from sam_road_amd import Config, SAMRoad, _lib
from sam_road_amd.inferencer import infer_one_img, infer_imgs, scene_tiles
dev = torch.device("cuda", 0)
cfg = Config(SAM_VERSION="vit_b", PATCH_SIZE=512, TOPONET_VERSION="normal", SAM_CKPT_PATH="", DATASET="cityscale", INFER_BATCH_SIZE=64,
             SAMPLE_MARGIN=64, INFER_PATCHES_PER_EDGE=16, ITSC_THRESHOLD=0.248, ROAD_THRESHOLD=0.364, TOPO_THRESHOLD=0.499,
             ITSC_NMS_RADIUS=8, ROAD_NMS_RADIUS=16, NEIGHBOR_RADIUS=64, MAX_NEIGHBOR_QUERIES=16)
net = SAMRoad(cfg)
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
valid = np.ones((H, W), bool)
valid[:64 + 512, :64 + 512] = False            # the first tile (origin 64, 64) holds no valid pixel; its neighbours keep some
kept = scene_tiles(img.shape, cfg, valid=valid, net=net)
print("tiles kept", len(kept), "of 256", flush=True)
for _ in range(2):
    infer_one_img(net, img, cfg); infer_one_img(net, img, cfg, valid=valid)
ctx = _lib.Context.get(0)
N = 5
for name, v in (("unmasked", None), ("masked", valid)):
    ctx.profile_read(); ctx.profile_enable(True)
    for _ in range(N):
        infer_one_img(net, img, cfg, valid=v)
    torch.cuda.synchronize()
    rows = ctx.profile_read(); ctx.profile_enable(False)
    tot = sum(r["ms"] for r in rows)
    print(f"--- {name}: library event times per class, mean of {N} scenes (ms per scene; total {tot / N:.3f})")
    for r in sorted(rows, key=lambda r: -r["ms"]):
        if r["name"] in ("tile_valid_count", "scene_fill_invalid", "scene_norm_valid", "scene_normalise", "scene_count", "scene_add"):
            gbs = r["bytes"] / (r["ms"] * 1e-3) / 1e9 if r["ms"] else 0
            print(f"    {r['name']:<20s} launches/scene {r['launches'] / N:5.1f}  ms/scene {r['ms'] / N:8.4f}  declared bytes/s {gbs:8.1f} GB/s")
# wall time of the selection step alone, as infer_one_img issues it (resident mask: upload excluded / included)
vd = torch.from_numpy(valid.view(np.uint8)).to(dev)
from sam_road_amd.inferencer import _tile_plan
xy = torch.as_tensor(_tile_plan(H, W, cfg)[1]).to(dev)
torch.cuda.synchronize()
ts = []
for _ in range(20):
    t0 = time.perf_counter(); c = net.scene_tile_valid(vd, xy).cpu().numpy(); ts.append(time.perf_counter() - t0)
print(f"count kernel + counts D2H + wait (device idle, mask resident): median {1e3 * np.median(ts):.3f} ms, min {1e3 * min(ts):.3f} ms")
ts = []
for _ in range(20):
    t0 = time.perf_counter(); vd2 = torch.from_numpy(valid.view(np.uint8)).to(dev); c = net.scene_tile_valid(vd2, xy).cpu().numpy(); ts.append(time.perf_counter() - t0)
print(f"mask upload (4 MB pageable) + count + D2H + wait: median {1e3 * np.median(ts):.3f} ms, min {1e3 * min(ts):.3f} ms")
# end to end
for name, v in (("unmasked", None), ("masked (255 of 256 tiles)", valid)):
    torch.cuda.synchronize(); t0 = time.perf_counter()
    for _ in range(N):
        infer_one_img(net, img, cfg, valid=v)
    torch.cuda.synchronize()
    print(f"infer_one_img {name}: {1e3 * (time.perf_counter() - t0) / N:.2f} ms per scene")
for name, v in (("unmasked", None), ("masked (255 of 256 tiles)", valid)):
    list(infer_imgs(net, (img for _ in range(3)), cfg, valids=(v for _ in range(3))))
    runs = []
    for _ in range(3):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        list(infer_imgs(net, (img for _ in range(12)), cfg, valids=(v for _ in range(12))))
        torch.cuda.synchronize(); runs.append(1e3 * (time.perf_counter() - t0) / 12)
    print(f"infer_imgs (12 scenes) {name}: {['%.2f' % r for r in runs]} ms per scene")
if "--laps" in sys.argv:
    os.environ["SRH_PROFILE_HOST"] = "1"
    print("--- host laps, masked scene"); infer_one_img(net, img, cfg, valid=valid)
    print("--- host laps, pipelined, 3 masked scenes"); list(infer_imgs(net, (img for _ in range(3)), cfg, valids=(valid for _ in range(3))))
