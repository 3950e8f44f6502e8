#!/usr/bin/env python
"""Scene-level timing (BASELINE configs[3], one GPU): one synthetic 2048x2048 u8 scene (2 km x 2 km at 1 m/px),
toponet_vitb_512_cityscale.yaml tiling (SAMPLE_MARGIN 64, 16x16 = 256 tiles of 512^2), seeded random weights.
Reports ms per scene for pass 1 alone (crop -> encoder -> decoder -> fused u8 masks, all on the GPU) and for the
whole infer_one_img (pass 1 + host NMS + pass-2 queries + TopoNet + edge vote) = the latency of one scene, and for a run of
scenes through infer_imgs (the CLI's loop: scene i's host stages overlap scene i+1's pass 1) = the throughput figure.
The final map_decoder bias is lowered so that the random network yields sparse masks (a few thousand graph points, as a trained one does).

    python tools/scene_bench.py [--bias -2.2] [--wscale 16] [--batch 64] [--iters 3]
    python tools/scene_bench.py --scene 2048 4096 --tiles 16 32     # a rectangular scene H W (or 2048x4096) with [n_y, n_x] tiles;
                                                                    # --scene 4096 --tiles 32 = the square a user had to pad it to
    python tools/scene_bench.py --scene 2048 4096 --tiles 16 32 --valid-frac 0.5    # a validity mask: a diagonal band covering that share
                                                                    # of the scene; only tiles that hold valid pixels run (kept / all is printed)
    python tools/scene_bench.py --fuse-window hann                  # overlapping tiles fused with a window (FUSE_WINDOW) instead of the uniform mean
    python tools/scene_bench.py --tta id,flip_h,rot90               # test-time augmentation (TTA): every tile runs once per orientation
    python tools/scene_bench.py --scene-pad 64 [--scene-pad-mode edge]    # SCENE_PAD: the scene is padded by 64 px on every side on the device
                                                                    # (reflect by default), the masks and the graph are those of the real scene
    python tools/scene_bench.py --scene 400 --tiles 1 --scene-pad 0 --scenes 256 --group 16    # a STREAM of 256 small scenes (chips) through
                                                                    # infer_imgs with SCENE_GROUP 16: scenes/s, tiles/s, device ms of pass 1 and
                                                                    # pass 2 per group, host ms per scene; --group 1 is the loop without the key
    python tools/scene_bench.py --patch 256 --margin 0 --scene 400 --tiles 4 --scenes 256 --group 16     # the spacenet_4x4 geometry: 16 tiles of 256 px
    python tools/scene_bench.py --bands 4 uint16 --stretch percentile 2 98    # SCENE_BANDS: the scene arrives as a raw uint16 scene of 4 bands;
                                                                    # band selection and the stretch run on the device in front of pass 1
                                                                    # (--stretch range LO HI: a fixed range; default: the whole range).  Adds
                                                                    # "scene_bands": the new stages and the numpy host step they replace
    python tools/scene_bench.py --scene 4096 --tiles 16 --scale 1 2    # SCENE_SCALE: a 4096^2 scene at 0.5 m/px runs in the 2048^2 model frame
                                                                    # (--tiles counts tiles of the MODEL frame); the resample steps are part of
                                                                    # every pass 1, and "scene_scale" reports their device time alone, forward
                                                                    # and back, in the separable LDS form and in the direct form
    python tools/scene_bench.py --mask-clean 200 0.6 [20 0.5]       # MASK_CLEAN: road min_area and min_peak [keypoint's]; the filter is part of
                                                                    # every timed run, and "mask_clean" reports its device time alone — on the
                                                                    # scene's own masks and on a random mask at density 0.5, per kernel — next to
                                                                    # pass 1's, the pipelined loop with and without the key in turn, and the host
                                                                    # time of mask_clean_ref on the same masks
    python tools/scene_bench.py --float 4 [--float-range LO HI] [--float-percentile P Q]    # SCENE_FLOAT: the scene arrives as float32 of 4 bands;
                                                                    # "scene_float": the three launches alone, the pipelined loop handed
                                                                    # float_scene_ref's outputs / keyed with a fixed range / with a percentile
    python tools/scene_bench.py --nodata 0 --nodata-tolerance 3 --nodata-min-area 50 --nodata-grow 2 [--bands 4 uint16]    # SCENE_NODATA: the scene
                                                                    # gets a collar, a fringe and interior specks of the value; "scene_nodata"
                                                                    # compares the derived mask with nodata_ref (the run ends if they differ) and
                                                                    # reports the device time of the nodata launches (match alone / the key as
                                                                    # given, per kernel), pass 1's, the pipelined loop unmasked / keyed / with the
                                                                    # identical mask passed as valid in turn, and the host time of nodata_ref
    python tools/scene_bench.py --edge-support [T] [--scene 4096 --tiles 32]     # EDGE_SUPPORT: the per-edge statistics against edge_support_ref, the whole
                                                                    # call, the kernel alone, the host reference, the pipelined loop without / with the filter
    python tools/scene_bench.py --road-width [R] [--scene 4096 --tiles 32]       # ROAD_WIDTH: the distance map and the per-edge statistics against their
                                                                    # references, the whole call, the three kernels alone, the same work on the host,
                                                                    # the pipelined loop without / with the key
    python tools/scene_bench.py --graph-clean [S C] [--scene 4096 --tiles 32]    # GRAPH_CLEAN: state and out of the device against graph_clean_ref on the
                                                                    # scene's own graph (the run ends if they differ), the kernels alone, the whole
                                                                    # call, the host reference, the pipelined loop without / with the key
    python tools/scene_bench.py --viz [--scene 4096 --tiles 32]     # GRAPH_RASTER: "graph_raster" compares the device class map with graph_raster_ref
                                                                    # (the run ends if they differ), reports the device time of raster, composite and
                                                                    # compare beside pass 1 and the host reference, and the pipelined loop with PNG
                                                                    # writers without renders / with viz / with diff, alternated
    python tools/scene_bench.py --aoi-frac 0.4 [--scene 4096 --no-pipelined]    # SCENE_AOI: a star polygon that covers about 0.4 of the scene;
                                                                    # "scene_aoi" compares the device mask with aoi_ref (the run ends if they
                                                                    # differ) for the star, a hexagon, a 1000-vertex circle and a ring at the
                                                                    # 16384-edge limit, and reports the device time of scene_aoi_fill alone for
                                                                    # each, pass 1's, the pipelined loop unmasked / keyed / with the identical
                                                                    # mask passed as valid in turn, and the host time of aoi_ref
    python tools/scene_bench.py --geotiff {none,deflate,lzw} ... [--tiled] [--planar] [--geotiff-cache DIR]    # GEOTIFF: the scene as a u8 RGB
                                                                    # and a 4-band uint16 GeoTIFF written with the test kit's writer; "geotiff" reports
                                                                    # host decompress, upload, srh_tiff_assemble alone beside srh_scene_bands_apply,
                                                                    # PIL and numpy on the same data, and the pipelined loop fed the TIFF with the
                                                                    # key / fed the .npy of the same scene, alternated
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 tools/scene_bench.py    # N GPUs:
        tiles sharded over the ranks (RCCL: packed-weight broadcast, banded canvas reduce, point broadcast, vote gather);
        rank 0 prints ms/scene (max over ranks) and the per-rank stage times
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def parse_scene(words):
    """['2048'] -> (2048, 2048); ['2048', '4096'] or ['2048x4096'] -> (2048, 4096): height first, as in img.shape."""
    parts = [p for w in words for p in str(w).lower().split("x")]
    if len(parts) not in (1, 2) or not all(p.isdigit() and int(p) > 0 for p in parts):
        raise SystemExit(f"--scene takes S, H W or HxW, got {words}")
    return int(parts[0]), int(parts[-1])


def stream(args, net, cfg, H, W):
    """--scenes M [--group N]: M scenes of H x W (eight different ones, in turn) through infer_imgs, three timed runs after a warm-up run.
    Prints one JSON line: scenes/s and tiles/s (median run), the device time of pass 1 and pass 2 per unit of the loop (a group, or a
    scene) from events, and the host time of one scene's points + queries on ONE thread, measured apart on the masks of the run."""
    import sam_road_amd.inferencer as inf
    from sam_road_amd.graph_points import extract_graph_points
    rng = np.random.default_rng(0)
    imgs = [np.kron(rng.integers(0, 256, size=(H // 8, W // 8, 3)).astype(np.float32), np.ones((8, 8, 1), np.float32)).astype(np.uint8) for _ in range(8)]
    n_tiles = len(inf.scene_tiles((H, W), cfg))
    group = {} if args.group == 1 else dict(group=args.group)
    scenes = lambda m: (imgs[i % 8] for i in range(m))
    outs = list(inf.infer_imgs(net, scenes(min(args.scenes, 2 * max(args.group, 8))), cfg, **group))       # warm-up: staging, workspaces
    runs = []
    inf._Lane.times = []
    for _ in range(3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        n_out = sum(1 for _ in inf.infer_imgs(net, scenes(args.scenes), cfg, **group))
        torch.cuda.synchronize()
        runs.append(time.perf_counter() - t0)
        assert n_out == args.scenes
    times, inf._Lane.times = inf._Lane.times, None
    full = [t for t in times if t[0] == max(u[0] for u in times)] if times else []
    host = []
    for nodes, _, kp, road in outs[:8]:
        t0 = time.perf_counter()
        pts = extract_graph_points(kp, road, cfg, n_threads=1)
        if pts.shape[0]:
            inf.build_all_patch_queries(pts, inf.scene_tiles((H, W), cfg), 0, n_tiles, cfg, flat=True, n_threads=1)
        host.append(1e3 * (time.perf_counter() - t0))
    sec = float(np.median(runs))
    med = lambda j: None if not full else round(float(np.median([t[j] for t in full])), 3)
    print(json.dumps({"stream": f"{args.scenes} synthetic {H}x{W} u8 scenes, {n_tiles} tiles of {args.patch}^2 each (margin {args.margin})",
                      "scene_group": args.group, "scene_pad": None if inf.scene_pad_key(cfg) is None else list(inf.scene_pad_plan((H, W), cfg)[:4]),
                      "infer_batch_size": args.batch, "scenes_per_s": round(args.scenes / sec, 1), "tiles_per_s": round(args.scenes * n_tiles / sec, 1),
                      "runs_scenes_per_s": [round(args.scenes / r, 1) for r in runs], "scenes_per_unit": full[0][0] if full else None,
                      "device_ms_pass1_per_unit": med(1), "device_ms_pass2_per_unit": med(2),
                      "host_ms_points_and_queries_per_scene_one_thread": round(float(np.median(host)), 3),
                      "host_pool_threads": inf._group_pool_threads(args.group) if args.group > 1 else None,
                      "graph_points_per_scene": round(float(np.mean([o[0].shape[0] for o in outs])), 1),
                      "edges_per_scene": round(float(np.mean([o[1].shape[0] for o in outs])), 1)}))


def bands_front(net, cfg, raw_d, valid_d=None):
    """The SCENE_BANDS front end as _pass1_front runs it, from the resident raw scene: [histogram -> host -> ranges ->] tables -> upload -> apply."""
    from sam_road_amd import radiometry as R
    key = R.scene_bands_key(cfg)
    levels = 256 if raw_d.dtype == torch.uint8 else 65536
    if key.percentile is not None:
        ranges = R.stretch_from_hist(net.scene_bands_hist(raw_d, key.select, valid_d).cpu().numpy(), *key.percentile)
    else:
        ranges = R.fixed_ranges(key, levels)
    return net.scene_bands_apply(raw_d, key.select, torch.from_numpy(R.band_luts(ranges, key.gamma, levels)).to(raw_d.device))


def bands_scene(args, net, cfg, img, dev, rng, iters=20):
    """--bands C DTYPE [--stretch ...]: sets cfg.SCENE_BANDS and returns (the raw scene, the report): device ms of the two kernels alone
    (events around `iters` launches after a warm-up) with the bytes they must move, host ms of the whole front end (with the percentile's
    round trip and the table build) and of the numpy step it replaces (np.percentile per band + rescale + cast), both on this box."""
    from sam_road_amd import radiometry as R
    C, dt = int(args.bands[0]), np.dtype(args.bands[1])
    if dt not in R.LEVELS or not 1 <= C <= R.MAX_BANDS:
        raise SystemExit("--bands takes C in 1..16 and uint8 or uint16")
    levels, (H, W) = R.LEVELS[dt], img.shape[:2]
    raw = rng.integers(0, levels, size=(H, W, C), dtype=dt)
    for b in range(min(3, C)):
        raw[..., b] = img[..., b].astype(dt) * (257 if levels > 256 else 1)
    key = {"select": [min(b, C - 1) for b in range(3)]}
    if args.stretch is not None:
        kind, a, b = args.stretch
        if kind not in ("range", "percentile"):
            raise SystemExit("--stretch takes 'range LO HI' or 'percentile PLO PHI'")
        key["stretch"] = [int(a), int(b)] if kind == "range" else {"percentile": [float(a), float(b)]}
    cfg.SCENE_BANDS = key
    k = R.scene_bands_key(cfg)
    raw_d = torch.from_numpy(raw).to(dev)
    lut_d = torch.from_numpy(R.band_luts(R.fixed_ranges(k, levels) if k.percentile is None else [(0, levels - 1)] * 3, k.gamma, levels)).to(dev)

    def device_ms(fn):
        fn()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / iters

    def wall_ms(fn, n=5):
        fn()
        ts = []
        for _ in range(n):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts.append(1e3 * (time.perf_counter() - t0))
        return float(np.median(ts))

    def numpy_step():
        out = np.empty((H, W, 3), np.uint8)
        for j, b in enumerate(k.select):
            x = raw[..., b]
            lo, hi = np.percentile(x, list(k.percentile)) if k.percentile is not None else R.fixed_ranges(k, levels)[j]
            t = np.clip((x.astype(np.float32) - lo) / max(float(hi - lo), 1.0), 0.0, 1.0)
            out[..., j] = (255.0 * (t if k.gamma == 1.0 else t ** (1.0 / k.gamma)) + 0.5).astype(np.uint8)
        return out

    e = dt.itemsize
    ms_hist = device_ms(lambda: net.scene_bands_hist(raw_d, k.select))
    const_d = torch.full_like(raw_d, levels // 3)
    ms_hist_const = device_ms(lambda: net.scene_bands_hist(const_d, k.select))
    del const_d
    ms_apply = device_ms(lambda: net.scene_bands_apply(raw_d, k.select, lut_d))
    gbs = lambda nbytes, ms: round(nbytes / ms * 1e-6, 1)
    report = {"bands": C, "dtype": dt.name, "key": key,
              "hist_ms": round(ms_hist, 4), "hist_ms_all_one_value": round(ms_hist_const, 4), "hist_must_read_bytes": 3 * e * H * W,
              "hist_GBps_of_must_read": gbs(3 * e * H * W, ms_hist),
              "apply_ms": round(ms_apply, 4), "apply_must_move_bytes": (3 * e + 3) * H * W, "apply_GBps_of_must_move": gbs((3 * e + 3) * H * W, ms_apply),
              "front_end_wall_ms": round(wall_ms(lambda: bands_front(net, cfg, raw_d)), 3),
              "numpy_host_step_wall_ms": round(wall_ms(numpy_step, 3), 2)}
    return raw, report


def scale_report(net, scale, scene_d, iters=20):
    """--scale P Q: device ms of the resample steps alone (events around `iters` launches after a warm-up) with the bytes they must move:
    the scene forward (p/q), the two masks back (q/p, to the scene's own size), each in the separable LDS form and in the direct form."""
    p, q = scale
    H, W = int(scene_d.shape[0]), int(scene_d.shape[1])

    def device_ms(fn):
        fn()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / iters

    small = net.scene_resample(scene_d, p, q)
    Hm, Wm = int(small.shape[0]), int(small.shape[1])
    masks = [small[..., c].contiguous() for c in (0, 1)]
    back = lambda direct: [net.scene_resample(m, q, p, out_shape=(H, W), direct=direct) for m in masks]
    assert torch.equal(net.scene_resample(scene_d, p, q, direct=True), small) and all(torch.equal(a, b) for a, b in zip(back(False), back(True)))
    fwd_bytes, back_bytes = 3 * (H * W + Hm * Wm), 2 * (H * W + Hm * Wm)
    rep = {"scale": [p, q], "scene": [H, W], "model_frame": [Hm, Wm], "forward_must_move_bytes": fwd_bytes, "back_must_move_bytes": back_bytes}
    for name, direct in (("lds", False), ("direct", True)):
        f, b = device_ms(lambda: net.scene_resample(scene_d, p, q, direct=direct)), device_ms(lambda: back(direct))
        rep.update({f"forward_ms_{name}": round(f, 4), f"back_two_masks_ms_{name}": round(b, 4),
                    f"forward_GBps_{name}": round(fwd_bytes / f * 1e-6, 1), f"back_GBps_{name}": round(back_bytes / b * 1e-6, 1)})
    return rep


def mask_clean_report(net, cfg, img, valid, pass1, iters=10):
    """--mask-clean: device ms of the filter alone (events around each of `iters` calls on a fresh copy of the masks, after a warm-up) on
    the scene's own two masks, on two random masks at density 0.5 and on two all-foreground masks (one component each), with the per-kernel rows of one profiled call; device ms of this
    scene's pass 1; ms per scene of the pipelined loop without / with / without / with the key; host ms of mask_clean_ref."""
    import sam_road_amd.inferencer as inf
    from sam_road_amd import Config, _lib
    from sam_road_amd.mask_clean import mask_clean_ref, mask_clean_stats, mask_clean_table
    plan = inf.mask_clean_plan(cfg)
    plain = Config({k: v for k, v in cfg.items() if k != "MASK_CLEAN"})
    _, _, kp, road = inf.infer_one_img(net, img, plain, valid=valid)
    H, W = kp.shape
    dev = next(net.parameters()).device
    ctx = _lib.Context.get(dev.index)
    table = mask_clean_table([(0, H, W, plan.keypoint), (H * W, H, W, plan.road)])
    table_d = torch.from_numpy(table).to(dev)
    rng = np.random.default_rng(7)

    def random_mask(rule):
        fg = rng.random((H, W)) < 0.5
        return np.where(fg, rng.integers(rule.t_on, 256, size=(H, W)), rng.integers(0, max(1, rule.t_on), size=(H, W))).astype(np.uint8)

    def measure(pair):
        src = torch.from_numpy(np.stack(pair)).to(dev)
        work = torch.empty_like(src)
        run = lambda: net.mask_clean(work.copy_(src).view(-1), table, table_dev=table_d, connectivity=plan.connectivity)
        run()
        want = [mask_clean_ref(m, *rule, plan.connectivity) for m, rule in zip(pair, (plan.keypoint, plan.road))]
        got = work.cpu().numpy()
        if not np.array_equal(got, np.stack(want)):
            for k in range(2):
                bad = got[k] != want[k]
                print(f"mask {k}: {int(bad.sum())} px differ, kept wrongly {int((bad & (got[k] != 0)).sum())}, rows {np.unique(np.nonzero(bad)[0])[:8].tolist()} "
                      f"cols {np.unique(np.nonzero(bad)[1])[:8].tolist()} levels {pair[k][bad][:8].tolist()}", file=sys.stderr, flush=True)
            raise SystemExit("the device filter differs from mask_clean_ref")
        evs = []
        for _ in range(iters):
            work.copy_(src)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            net.mask_clean(work.view(-1), table, table_dev=table_d, connectivity=plan.connectivity)
            e1.record()
            evs.append((e0, e1))
        torch.cuda.synchronize()
        ms = sorted(a.elapsed_time(b) for a, b in evs)
        ctx.profile_read()
        ctx.profile_enable(True)
        run()
        torch.cuda.synchronize()
        rows = {r["name"]: round(r["ms"], 4) for r in ctx.profile_read() if r["name"].startswith("mask_clean")}
        ctx.profile_enable(False)
        t0 = time.perf_counter()
        for m, rule in zip(pair, (plan.keypoint, plan.road)):
            mask_clean_ref(m, *rule, plan.connectivity)
        host = 1e3 * (time.perf_counter() - t0)
        comps = [int(mask_clean_stats(m, rule.t_on, plan.connectivity)[0].size) for m, rule in zip(pair, (plan.keypoint, plan.road))]
        return {"device_ms_median": round(ms[len(ms) // 2], 4), "device_ms_min_max": [round(ms[0], 4), round(ms[-1], 4)], "kernel_ms_one_call": rows,
                "host_ms_mask_clean_ref_both_masks": round(host, 1), "components": comps,
                "foreground_frac": [round(float((m >= rule.t_on).mean()), 4) for m, rule in zip(pair, (plan.keypoint, plan.road))],
                "pixels_dropped": [int((w != m).sum()) for w, m in zip(want, pair)]}

    rep = {"key": cfg.MASK_CLEAN, "rules": [list(plan.keypoint), list(plan.road)], "connectivity": plan.connectivity, "masks": [H, W],
           "own_masks": measure((kp, road)), "random_0.5": measure((random_mask(plan.keypoint), random_mask(plan.road))),
           "all_foreground": measure(tuple(rng.integers(max(1, rule.t_on), 256, size=(H, W)).astype(np.uint8) for rule in (plan.keypoint, plan.road)))}
    evs = []
    for _ in range(3):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        pass1()
        e1.record()
        evs.append((e0, e1))
    torch.cuda.synchronize()
    rep["pass1_device_ms"] = [round(a.elapsed_time(b), 2) for a, b in evs]

    def piped(c, n=12):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in inf.infer_imgs(net, (img for _ in range(n)), c, valids=(valid for _ in range(n))):
            pass
        torch.cuda.synchronize()
        return round(1e3 * (time.perf_counter() - t0) / n, 2)

    piped(plain, 3), piped(cfg, 3)
    rep["pipelined_ms_per_scene_runs_of_12"] = {"without_a": [piped(plain) for _ in range(3)], "with_a": [piped(cfg) for _ in range(3)],
                                                "without_b": [piped(plain) for _ in range(3)], "with_b": [piped(cfg) for _ in range(3)]}
    return rep


def nodata_paint(raw, value, rng):
    """The synthetic scene of --nodata, IN PLACE: a triangular collar of the value at the origin (about 6 % of the scene), a 3 px fringe of
    the three levels next to it, 200 isolated pixels and 40 blobs of 5..40 pixels of the value in the interior."""
    H, W, C = raw.shape
    levels = 256 if raw.dtype == np.uint8 else 65536
    yy, xx = np.mgrid[0:H, 0:W]
    collar = yy * W + xx * H < 0.35 * H * W
    fringe = ((yy - 3) * W + (xx - 3) * H < 0.35 * H * W) & ~collar
    near = np.array([value + d if value + 3 < levels else value - d for d in (1, 2, 3)])
    keep = raw == value                                      # natural pixels of the value itself move one level away
    raw[keep] = value + 1 if value + 1 < levels else value - 1
    raw[collar] = value
    raw[fringe] = near[rng.integers(0, 3, size=(int(fringe.sum()), C))]
    for k in range(240):
        h, w = (1, 1) if k < 200 else (int(rng.integers(1, 6)), int(rng.integers(5, 9)))
        y, x = int(rng.integers(H // 2, H - 8)), int(rng.integers(8, W - 16))
        raw[y:y + h, x:x + w] = value
    return raw


def nodata_report(args, net, cfg, raw, iters=20):
    """--nodata: the derived mask against nodata_ref on this scene (the run ends if they differ); device ms of the nodata launches alone
    (events around each of `iters` runs after a warm-up) for the value-only key and for the key as given, with the per-kernel rows of one
    profiled run; device ms of pass 1 of the same scene (from the lane's events); ms per scene of the pipelined loop without a mask / with
    the key / with the identical mask passed as `valid`, alternated; host ms of nodata_ref, the work the key takes off the feeding thread."""
    import sam_road_amd.inferencer as inf
    from sam_road_amd import Config, _lib
    from sam_road_amd.nodata import nodata_ref, nodata_table, scene_nodata_check, scene_nodata_key
    dev = next(net.parameters()).device
    ctx = _lib.Context.get(dev.index)
    key = scene_nodata_key(cfg)
    H, W = raw.shape[:2]
    lo, hi = scene_nodata_check(raw, key)
    raw_d = torch.from_numpy(raw).to(dev)
    table = nodata_table([(0, H, W)], key)
    table_d = torch.from_numpy(table).to(dev)
    t0 = time.perf_counter()
    want = nodata_ref(raw, key)
    host_ms = 1e3 * (time.perf_counter() - t0)
    rep = {"key": dict(cfg.SCENE_NODATA), "raw": [str(raw.dtype), list(raw.shape)], "valid_frac": round(float(want.mean()), 4),
           "host_ms_nodata_ref": round(host_ms, 1)}

    def measure(k):
        run = lambda: inf._scene_nodata_mask(net, k, raw_d, lo, hi, None, table, table_d)
        got = run().view(H, W).cpu().numpy()
        ref = nodata_ref(raw, k)
        if not np.array_equal(got, ref):
            bad = got != ref
            raise SystemExit(f"the derived mask differs from nodata_ref on {int(bad.sum())} px, rows {np.unique(np.nonzero(bad)[0])[:8].tolist()}")
        evs = []
        for _ in range(iters):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            run()
            e1.record()
            evs.append((e0, e1))
        torch.cuda.synchronize()
        ms = sorted(a.elapsed_time(b) for a, b in evs)
        ctx.profile_read()
        ctx.profile_enable(True)
        run()
        torch.cuda.synchronize()
        rows = {r["name"]: round(r["ms"], 4) for r in ctx.profile_read() if r["name"].startswith(("scene_nodata", "mask_clean"))}
        ctx.profile_enable(False)
        return {"device_ms_median": round(ms[len(ms) // 2], 4), "device_ms_min_max": [round(ms[0], 4), round(ms[-1], 4)], "kernel_ms_one_call": rows,
                "equals_nodata_ref": True}

    rep["match_alone"] = measure(key._replace(min_area=1, grow=0))
    rep["key_as_given"] = measure(key)
    plain = Config({k: v for k, v in cfg.items() if k != "SCENE_NODATA"})
    inf._Lane.times = []

    def piped(c, valid, n=12):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in inf.infer_imgs(net, (raw for _ in range(n)), c, **({} if valid is None else dict(valids=(valid for _ in range(n))))):
            pass
        torch.cuda.synchronize()
        return round(1e3 * (time.perf_counter() - t0) / n, 2)

    piped(plain, None, 3), piped(cfg, None, 3), piped(plain, want, 3)
    inf._Lane.times.clear()
    runs = {"unmasked": [], "keyed": [], "mask_passed_as_valid": []}
    for _ in range(3):
        runs["unmasked"].append(piped(plain, None))
        runs["keyed"].append(piped(cfg, None))
        runs["mask_passed_as_valid"].append(piped(plain, want))
    rep["pipelined_ms_per_scene_runs_of_12_alternated"] = runs
    p1 = sorted(t[1] for t in inf._Lane.times)
    rep["pass1_device_ms_median_of_all_scenes_above"] = round(p1[len(p1) // 2], 2) if p1 else None
    inf._Lane.times = None
    a = inf.infer_one_img(net, raw, cfg)
    b = inf.infer_one_img(net, raw, plain, valid=want)
    rep["keyed_equals_mask_passed"] = all(np.array_equal(x, y) for x, y in zip(a, b))
    rep["graph_points"], rep["edges"] = int(a[0].shape[0]), int(a[1].shape[0])
    return rep


def aoi_star(H, W, frac, points=7):
    """The polygon of --aoi-frac: a star around the scene's centre, 2 * points vertices of alternating radii R and R / 2 (fractions of the half
    axes), R such that its area n sin(pi / n) R (R / 2) (H / 2) (W / 2) is frac H W; tips that leave the scene are cut by it."""
    n = points
    R = np.sqrt(frac * 8.0 / (n * np.sin(np.pi / n)))
    return [[[float(H / 2 * (1 + (R if i % 2 == 0 else R / 2) * np.sin(np.pi * i / n))), float(W / 2 * (1 + (R if i % 2 == 0 else R / 2) * np.cos(np.pi * i / n)))]
             for i in range(2 * n)]]


def aoi_report(args, net, cfg, img, iters=20):
    """--aoi-frac: scene_aoi_fill against aoi_ref on this scene size (the run ends if they differ) and its device ms alone (events around each
    of `iters` runs after a warm-up) for the star, a hexagon, a 1000-vertex circle and a zigzag ring of 16384 edges; device ms of pass 1 of
    the same scene (from the lane's events); ms per scene of the pipelined loop without a mask / with the key / with the identical mask
    passed as `valid`, alternated; host ms of aoi_ref for the star, the work the key takes off the feeding thread."""
    import sam_road_amd.inferencer as inf
    from sam_road_amd import Config
    from sam_road_amd.aoi import aoi_edges, aoi_key_of, aoi_pack, aoi_ref, scene_aoi_key
    dev = next(net.parameters()).device
    H, W = img.shape[:2]
    key = scene_aoi_key(cfg)
    t0 = time.perf_counter()
    want = aoi_ref((H, W), key)
    host_ms = 1e3 * (time.perf_counter() - t0)
    rep = {"aoi_frac_asked": args.aoi_frac, "valid_frac": round(float(want.mean()), 4), "host_ms_aoi_ref": round(host_ms, 1)}
    n = 16384
    polygons = {"star_14_vertices": cfg.SCENE_AOI["include"],
                "hexagon_6_vertices": [[[[float(H / 2 * (1 + 0.8 * np.sin(np.pi * i / 3))), float(W / 2 * (1 + 0.8 * np.cos(np.pi * i / 3)))] for i in range(6)]]],
                "circle_1000_vertices": [[[[float(H / 2 + 0.4 * H * np.sin(2 * np.pi * i / 1000)), float(W / 2 + 0.4 * W * np.cos(2 * np.pi * i / 1000))] for i in range(1000)]]],
                "zigzag_16384_edges": [[[[(0.05 if i % 2 == 0 else 0.6) * H + (i % 7) / 256.0, (i + 0.5) * W / (n - 1)] for i in range(n - 1)] + [[0.9 * H, float(W)], [0.9 * H, 0.0]]]]}
    fills = {}
    for name, include in polygons.items():
        k = aoi_key_of({"include": include})
        tab = aoi_edges(k, H, W)
        tab_d = torch.from_numpy(aoi_pack(*tab[:2])).to(dev)
        run = lambda: net.scene_aoi_fill((H, W), *tab, table_dev=tab_d)
        got, ref = run().cpu().numpy(), aoi_ref((H, W), k)
        if not np.array_equal(got, ref):
            bad = got != ref
            raise SystemExit(f"{name}: the device mask differs from aoi_ref on {int(bad.sum())} px, rows {np.unique(np.nonzero(bad)[0])[:8].tolist()}")
        evs = []
        for _ in range(iters):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            run()
            e1.record()
            evs.append((e0, e1))
        torch.cuda.synchronize()
        ms = sorted(a.elapsed_time(b) for a, b in evs)
        fills[name] = {"edges_in_table": int(tab[0].shape[0]), "inside_frac": round(float(ref.mean()), 4), "device_ms_median": round(ms[len(ms) // 2], 4),
                       "device_ms_min_max": [round(ms[0], 4), round(ms[-1], 4)], "equals_aoi_ref": True}
    rep["scene_aoi_fill_alone"] = fills
    if args.no_pipelined:
        return rep
    plain = Config({k: v for k, v in cfg.items() if k != "SCENE_AOI"})
    inf._Lane.times = []

    def piped(c, valid, n=12):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in inf.infer_imgs(net, (img for _ in range(n)), c, **({} if valid is None else dict(valids=(valid for _ in range(n))))):
            pass
        torch.cuda.synchronize()
        return round(1e3 * (time.perf_counter() - t0) / n, 2)

    piped(plain, None, 3), piped(cfg, None, 3), piped(plain, want, 3)
    inf._Lane.times.clear()
    runs = {"unmasked": [], "keyed": [], "mask_passed_as_valid": []}
    for _ in range(3):
        runs["unmasked"].append(piped(plain, None))
        runs["keyed"].append(piped(cfg, None))
        runs["mask_passed_as_valid"].append(piped(plain, want))
    rep["pipelined_ms_per_scene_runs_of_12_alternated"] = runs
    p1 = sorted(t[1] for t in inf._Lane.times)
    rep["pass1_device_ms_median_of_all_scenes_above"] = round(p1[len(p1) // 2], 2) if p1 else None
    inf._Lane.times = None
    rep["tiles_run_of_planned"] = [len(inf.scene_tiles(img.shape, cfg, net=net)), len(inf.scene_tiles(img.shape, plain))]
    a = inf.infer_one_img(net, img, cfg)
    b = inf.infer_one_img(net, img, plain, valid=want)
    rep["keyed_equals_mask_passed"] = all(np.array_equal(x, y) for x, y in zip(a, b))
    rep["graph_points"], rep["edges"] = int(a[0].shape[0]), int(a[1].shape[0])
    return rep


def road_grid(H, W, step, seed):
    """A synthetic road-grid graph: nodes on a lattice of `step` pixels with a jitter of a quarter step, edges to the right and the lower neighbour."""
    rng = np.random.default_rng(seed)
    rr, cc = np.meshgrid(np.arange(step // 2, H, step), np.arange(step // 2, W, step), indexing="ij")
    j = step // 4
    nodes = np.stack([rr + rng.integers(-j, j + 1, rr.shape), cc + rng.integers(-j, j + 1, cc.shape)], axis=-1).reshape(-1, 2)
    idx = np.arange(nodes.shape[0]).reshape(rr.shape)
    edges = np.concatenate([np.stack([idx[:, :-1].ravel(), idx[:, 1:].ravel()], axis=1), np.stack([idx[:-1].ravel(), idx[1:].ravel()], axis=1)])
    return nodes.astype(np.int64), edges.astype(np.int64)


def graph_report(args, net, cfg, img, iters=20):
    """--viz / --diff (GRAPH_RASTER): the class map against graph_raster_ref on this scene size (the run ends if they differ); device ms (events
    around each of `iters` runs after a warm-up) of the raster at the viz style and at the diff's four styles, of the composite and of the
    compare; host ms of graph_raster_ref; device ms of pass 1 of the same scene; and ms per scene of the pipelined loop as the CLI runs it —
    mask PNGs on writer threads — without renders, with viz and with diff, alternated.  The graph is the scene's own if the stand-in weights
    yield at least 1000 edges, else a synthetic road grid of 32-px cells; the ground truth is another grid."""
    import sam_road_amd.inferencer as inf
    from concurrent.futures import ThreadPoolExecutor
    from PIL import Image
    import io
    from sam_road_amd import graph_raster as gr
    dev = next(net.parameters()).device
    H, W = img.shape[:2]
    nodes, edges, _, _ = inf.infer_one_img(net, img, cfg)
    own = edges.shape[0] >= 1000
    if not own:
        nodes, edges = road_grid(H, W, 32, 1)
    gt = road_grid(H, W, 32, 2)
    rep = {"graph": "the scene's own" if own else "synthetic road grid, 32-px cells", "nodes": int(nodes.shape[0]), "edges": int(edges.shape[0])}
    t0 = time.perf_counter()
    want = gr.graph_raster_ref(nodes, edges, (H, W), 4, "disc", 4)
    rep["host_ms_graph_raster_ref"] = round(1e3 * (time.perf_counter() - t0), 1)
    got = net.graph_raster((H, W), nodes, edges, 4, "disc", 4)
    if not np.array_equal(got.cpu().numpy(), want):
        raise SystemExit(f"the device class map differs from graph_raster_ref on {int((got.cpu().numpy() != want).sum())} px")
    rep["equals_graph_raster_ref"], rep["covered_frac"] = True, round(float((want != 0).mean()), 4)
    img_d = torch.from_numpy(img).to(dev)
    maps = [net.graph_raster((H, W), *g, 2 * r, "square", r, values=(255, 255)) for g, r in (((nodes, edges), 1), ((nodes, edges), 5), (gt, 1), (gt, 5))]
    m_dev, _ = gr.compare_graphs((nodes, edges), gt, (H, W), 1, 5, net=net)
    t0 = time.perf_counter()
    m_ref, _ = gr.compare_ref((nodes, edges), gt, (H, W), 1, 5, diff=False)
    rep["host_ms_compare_ref"] = round(1e3 * (time.perf_counter() - t0), 1)
    if m_dev != m_ref:
        raise SystemExit(f"the device counts {m_dev} differ from compare_ref's {m_ref}")
    rep["metrics"] = m_dev

    def device_ms(fn):
        fn()
        evs = []
        for _ in range(iters):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            evs.append((e0, e1))
        torch.cuda.synchronize()
        ms = sorted(a.elapsed_time(b) for a, b in evs)
        return {"median": round(ms[len(ms) // 2], 4), "min_max": [round(ms[0], 4), round(ms[-1], 4)]}

    out3 = torch.empty((H, W, 3), dtype=torch.uint8, device=dev)
    rep["device_ms"] = {"raster_viz_style_with_table_upload": device_ms(lambda: net.graph_raster((H, W), nodes, edges, 4, "disc", 4, out=got)),
                        "raster_width_10_squares_5": device_ms(lambda: net.graph_raster((H, W), nodes, edges, 10, "square", 5, out=got)),
                        "composite": device_ms(lambda: net.graph_composite(got, img_d, out=out3)),
                        "compare_with_diff_image": device_ms(lambda: net.graph_compare(*maps, img=img_d, diff=True)),
                        "compare_counts_only": device_ms(lambda: net.graph_compare(*maps))}
    ctx, _ = net._weights(dev)
    ctx.profile_read()
    ctx.profile_enable(True)
    for _ in range(iters):
        net.graph_raster((H, W), nodes, edges, 4, "disc", 4, out=got)
    torch.cuda.synchronize()
    rep["raster_kernels_ms_per_call"] = {r["name"]: round(r["ms"] / r["launches"], 4) for r in ctx.profile_read() if r["launches"]}
    ctx.profile_enable(False)
    if args.no_pipelined:
        return rep
    inf._Lane.times = []
    stream = torch.cuda.Stream(dev)

    def png(a):
        Image.fromarray(a).save(io.BytesIO(), format="PNG", compress_level=1)

    stages = {}                                            # per product: (ms until the product is on the host, ms of its PNG encoding) per scene

    def render(key, res):
        t0 = time.perf_counter()
        with torch.cuda.stream(stream):
            prod = gr.render(key, res[0], res[1], (H, W), img=img, gt=gt, net=net)
        t1 = time.perf_counter()
        for k in ("viz", "mask", "diff"):
            if k in prod:
                png(prod[k])
        stages.setdefault("viz" if key.viz is not None else "diff", []).append((1e3 * (t1 - t0), 1e3 * (time.perf_counter() - t1)))

    def piped(key, n=12):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        waits = 0.0
        with ThreadPoolExecutor(2 + (0 if key is None else 1)) as pool:
            futs = []
            for res in inf.infer_imgs(net, (img for _ in range(n)), cfg):
                futs += [pool.submit(png, res[2]), pool.submit(png, res[3])]
                if key is not None:
                    futs.append(pool.submit(render, key, res))
            t1 = time.perf_counter()
            for f in futs:
                f.result()
            waits = time.perf_counter() - t1
        torch.cuda.synchronize()
        return round(1e3 * (time.perf_counter() - t0) / n, 2), round(1e3 * waits / n, 2)

    keys = {"without": None, "viz": gr.graph_raster_key_of({"viz": True}), "diff": gr.graph_raster_key_of({"diff": True})}
    for k in keys.values():
        piped(k, 3)
    inf._Lane.times.clear()
    stages.clear()
    runs = {k: [] for k in keys}
    for _ in range(3):
        for name, k in keys.items():
            runs[name].append(piped(k))
    rep["pipelined_ms_per_scene_and_writer_drain_ms_runs_of_12_alternated"] = runs
    med = lambda v: round(sorted(v)[len(v) // 2], 2)
    rep["writer_thread_ms_per_scene_median"] = {k: {"upload_launch_wait_download": med([a for a, _ in v]), "png_encode": med([b for _, b in v])} for k, v in stages.items()}
    p1 = sorted(t[1] for t in inf._Lane.times)
    rep["pass1_device_ms_median_of_all_scenes_above"] = round(p1[len(p1) // 2], 2) if p1 else None
    inf._Lane.times = None
    return rep


def edge_support_report(args, net, cfg, img, iters=20):
    """--edge-support [T] (EDGE_SUPPORT): the device statistics against edge_support_ref on this scene size (the run ends if they differ);
    ms of the whole call from host arrays (table upload, mask upload, kernel, 16 E-byte download; wall clock around a synchronised call),
    device ms of the kernel alone (the profiler row), host ms of edge_support_ref; and ms per scene of the pipelined loop as the CLI runs
    it — mask PNGs on writer threads — without the key and with it (filter on a writer thread, on a stream of its own), alternated.  The
    graph is the scene's own if the stand-in weights yield at least 1000 edges, else a synthetic road grid of 32-px cells."""
    import sam_road_amd.inferencer as inf
    from concurrent.futures import ThreadPoolExecutor
    from PIL import Image
    import io
    from sam_road_amd import edge_support as es
    dev = next(net.parameters()).device
    H, W = img.shape[:2]
    t = args.edge_support
    nodes, edges, _, road = inf.infer_one_img(net, img, cfg)
    own = edges.shape[0] >= 1000
    if not own:
        nodes, edges = road_grid(H, W, 32, 1)
    level = es.on_level_of(cfg.ROAD_THRESHOLD)
    rep = {"graph": "the scene's own" if own else "synthetic road grid, 32-px cells", "nodes": int(nodes.shape[0]), "edges": int(edges.shape[0]), "width": t,
           "on_level": level}
    t0 = time.perf_counter()
    want = es.edge_support_ref(nodes, edges, road, t, level)
    rep["host_ms_edge_support_ref"] = round(1e3 * (time.perf_counter() - t0), 1)
    got = es.edge_stats(nodes, edges, road, t, level, net=net)
    if not np.array_equal(got, want):
        raise SystemExit(f"the device statistics differ from edge_support_ref on {int((got != want).any(axis=1).sum())} edges")
    rep["equals_edge_support_ref"], rep["covered_px_per_edge_mean"] = True, round(float(want[:, 0].mean()), 2)

    def wall_ms(fn):
        fn()
        ms = []
        for _ in range(iters):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            ms.append(1e3 * (time.perf_counter() - t0))
        ms.sort()
        return {"median": round(ms[len(ms) // 2], 4), "min_max": [round(ms[0], 4), round(ms[-1], 4)]}

    road_d = torch.from_numpy(road).to(dev)
    rep["whole_call_ms_from_host_arrays"] = wall_ms(lambda: es.edge_stats(nodes, edges, road, t, level, net=net))
    rep["whole_call_ms_mask_on_the_device"] = wall_ms(lambda: net.graph_edge_stats(nodes, edges, road_d, t, level).cpu())
    ctx, _ = net._weights(dev)
    per_call = []
    for _ in range(3):                                     # three groups of `iters` calls: the run-to-run span of the kernel time
        ctx.profile_read()
        ctx.profile_enable(True)
        for _ in range(iters):
            net.graph_edge_stats(nodes, edges, road_d, t, level)
        torch.cuda.synchronize()
        per_call.append({r["name"]: round(r["ms"] / r["launches"], 4) for r in ctx.profile_read() if r["launches"]}["graph_edge_stats"])
        ctx.profile_enable(False)
    rep["kernel_ms_per_call_three_groups"] = per_call
    if args.no_pipelined:
        return rep
    stream = torch.cuda.Stream(dev)
    key = es.edge_support_key_of({"width": t, "min_on": 0.5, "drop_isolated": True}, cfg.ROAD_THRESHOLD)

    def png(a):
        Image.fromarray(a).save(io.BytesIO(), format="PNG", compress_level=1)

    stage = []

    def finish(res):
        t0 = time.perf_counter()
        with torch.cuda.stream(stream):
            es.apply(key, res, net=net)
        stage.append(1e3 * (time.perf_counter() - t0))

    def piped(on, n=12, writers=3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        with ThreadPoolExecutor(writers) as pool:
            futs = []
            for res in inf.infer_imgs(net, (img for _ in range(n)), cfg):
                futs += [pool.submit(png, res[2]), pool.submit(png, res[3])]
                if on:
                    futs.append(pool.submit(finish, res))
            for f in futs:
                f.result()
        torch.cuda.synchronize()
        return round(1e3 * (time.perf_counter() - t0) / n, 2)

    for on in (False, True):
        piped(on, 3)
    stage.clear()
    runs = {"without_2_writers": [], "without": [], "with": []}      # the CLI adds a writer thread with the key: both pools, so the thread is not mistaken for the key
    for _ in range(3):
        for name, on, writers in (("without_2_writers", False, 2), ("without", False, 3), ("with", True, 3)):
            runs[name].append(piped(on, writers=writers))
    rep["pipelined_ms_per_scene_runs_of_12_alternated"] = runs
    rep["writer_thread_ms_per_scene_median_filter"] = round(sorted(stage)[len(stage) // 2], 2)
    return rep


def graph_clean_report(args, net, cfg, img, iters=20):
    """--graph-clean [S C] (GRAPH_CLEAN; min_spur S and min_component C in px, default 12 and 60, 2 rounds): state and out of the device
    against graph_clean_ref on this scene's own graph (the run ends if they differ); device ms of the 15 launches of a call (the profiler
    rows, three groups) and of each kernel, ms of the whole call from host arrays (table upload, launches, the 17 E-byte download; wall
    clock around a synchronised call) and of apply (that plus the kept graph and the attributes on the host), host ms of graph_clean_ref;
    and ms per scene of the pipelined loop as the CLI runs it — mask PNGs on writer threads — without the key and with it (on a writer
    thread, on a stream of its own), alternated.  The graph is the scene's own if the stand-in weights yield at least 1000 edges, else a
    synthetic road grid of 32-px cells."""
    import sam_road_amd.inferencer as inf
    from concurrent.futures import ThreadPoolExecutor
    from PIL import Image
    import io
    from sam_road_amd import graph_clean as gc
    dev = next(net.parameters()).device
    H, W = img.shape[:2]
    s_px, c_px = args.graph_clean if args.graph_clean else (12.0, 60.0)
    key = gc.graph_clean_key_of({"min_spur": s_px, "min_component": c_px, "rounds": 2, "drop_isolated": True})
    spur_q, comp_q = gc.thresholds_q(key)
    nodes, edges, _, _ = inf.infer_one_img(net, img, cfg)
    own = edges.shape[0] >= 1000
    if not own:
        nodes, edges = road_grid(H, W, 32, 1)
    rep = {"graph": "the scene's own" if own else "synthetic road grid, 32-px cells", "nodes": int(nodes.shape[0]), "edges": int(edges.shape[0]),
           "min_spur_px": s_px, "min_component_px": c_px, "rounds": key.rounds, "launches_per_call": 5 * (key.rounds + 1)}
    host = []
    for _ in range(3):
        t0 = time.perf_counter()
        want = gc.graph_clean_ref(nodes, edges, spur_q, comp_q, key.rounds)
        host.append(round(1e3 * (time.perf_counter() - t0), 1))
    rep["host_ms_graph_clean_ref_three_runs"] = host
    got = gc.clean(nodes, edges, key, net=net)
    if not (np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])):
        raise SystemExit(f"the device differs from graph_clean_ref on {int(((got[0] != want[0]) | (got[1] != want[1]).any(axis=1)).sum())} edges")
    kept = want[1][want[0] == 0]
    rep.update(equals_graph_clean_ref=True, dropped=int((want[0] != 0).sum()), dropped_as_spur=int(((want[0] & 1) == 1).sum()),
               dropped_as_small=int(((want[0] & 2) == 2).sum()), chains_kept=int(np.unique(kept[:, 0]).size), components_kept=int(np.unique(kept[:, 1]).size),
               edges_of_the_largest_component=int(np.bincount(kept[:, 1]).max()) if kept.size else 0)

    def wall_ms(fn):
        fn()
        ms = []
        for _ in range(iters):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            ms.append(1e3 * (time.perf_counter() - t0))
        ms.sort()
        return {"median": round(ms[len(ms) // 2], 4), "min_max": [round(ms[0], 4), round(ms[-1], 4)]}

    result = (nodes, edges, np.zeros((1, 1), np.uint8), np.zeros((1, 1), np.uint8))
    rep["whole_call_ms_from_host_arrays"] = wall_ms(lambda: gc.clean(nodes, edges, key, net=net))
    rep["apply_ms_from_host_arrays"] = wall_ms(lambda: gc.apply(key, result, net=net))
    t0 = time.perf_counter()
    (n1, e1, _, _), attrs = gc.apply_ref(key, result)
    table = gc.table_of(attrs)
    t1 = time.perf_counter()
    doc = gc.polylines_geojson(n1, e1, table)
    rep["host_ms_polylines_geojson"] = round(1e3 * (time.perf_counter() - t1), 1)
    rep["polylines"] = len(doc["features"])
    ctx, _ = net._weights(dev)
    groups, kernels = [], {}
    for _ in range(3):                                     # three groups of `iters` calls: the run-to-run span of the kernel time
        ctx.profile_read()
        ctx.profile_enable(True)
        for _ in range(iters):
            net.graph_clean(nodes, edges, spur_q=spur_q, comp_q=comp_q, rounds=key.rounds)
        torch.cuda.synchronize()
        rows = {r["name"]: r["ms"] / iters for r in ctx.profile_read() if r["launches"] and r["name"].startswith("graph_clean_")}
        ctx.profile_enable(False)
        groups.append(round(sum(rows.values()), 4))
        kernels = {k: round(v, 4) for k, v in rows.items()}
    rep["kernel_ms_per_call_three_groups"] = groups
    rep["kernel_ms_per_call_by_kernel_last_group"] = kernels
    if args.no_pipelined:
        return rep
    stream = torch.cuda.Stream(dev)

    def png(a):
        Image.fromarray(a).save(io.BytesIO(), format="PNG", compress_level=1)

    stage = []

    def finish(res):
        t0 = time.perf_counter()
        with torch.cuda.stream(stream):
            gc.apply(key, res, net=net)
        stage.append(1e3 * (time.perf_counter() - t0))

    def piped(on, n=12, writers=3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        with ThreadPoolExecutor(writers) as pool:
            futs = []
            for res in inf.infer_imgs(net, (img for _ in range(n)), cfg):
                futs += [pool.submit(png, res[2]), pool.submit(png, res[3])]
                if on:
                    futs.append(pool.submit(finish, res))
            for f in futs:
                f.result()
        torch.cuda.synchronize()
        return round(1e3 * (time.perf_counter() - t0) / n, 2)

    for on in (False, True):
        piped(on, 3)
    stage.clear()
    runs = {"without_2_writers": [], "without": [], "with": []}      # the CLI adds a writer thread with the key: both pools, so the thread is not mistaken for the key
    for _ in range(3):
        for name, on, writers in (("without_2_writers", False, 2), ("without", False, 3), ("with", True, 3)):
            runs[name].append(piped(on, writers=writers))
    rep["pipelined_ms_per_scene_runs_of_12_alternated"] = runs
    rep["writer_thread_ms_per_scene_median_apply"] = round(sorted(stage)[len(stage) // 2], 2)
    return rep


def road_width_report(args, net, cfg, img, iters=20):
    """--road-width [R] (ROAD_WIDTH): the device distance map against road_dist_ref and the device statistics against road_width_ref on
    this scene size (the run ends if they differ); ms of the whole apply call from host arrays (mask and table upload, three kernels, the
    32 E-byte download, keep rule and attributes; wall clock around a synchronised call) and of the device part alone, device ms of each
    of the three kernels (the profiler rows), host ms of the same work (scipy's distance_transform_edt where it is installed, road_dist_ref,
    the per-edge loop of road_width_ref); and ms per scene of the pipelined loop as the CLI runs it — mask PNGs on writer threads —
    without the key and with it (on a writer thread, on a stream of its own), alternated.  The graph is the scene's own if the stand-in
    weights yield at least 1000 edges, else a synthetic road grid of 32-px cells."""
    import sam_road_amd.inferencer as inf
    from concurrent.futures import ThreadPoolExecutor
    from PIL import Image
    import io
    from sam_road_amd import edge_support as es
    from sam_road_amd import road_width as rw
    dev = next(net.parameters()).device
    H, W = img.shape[:2]
    R = args.road_width
    nodes, edges, _, road = inf.infer_one_img(net, img, cfg)
    own = edges.shape[0] >= 1000
    if not own:
        nodes, edges = road_grid(H, W, 32, 1)
    level = es.on_level_of(cfg.ROAD_THRESHOLD)
    rep = {"graph": "the scene's own" if own else "synthetic road grid, 32-px cells", "nodes": int(nodes.shape[0]), "edges": int(edges.shape[0]), "max_radius": R,
           "on_level": level}
    try:
        from scipy.ndimage import distance_transform_edt
        t0 = time.perf_counter()
        distance_transform_edt(road > level)
        rep["host_ms_scipy_distance_transform_edt"] = round(1e3 * (time.perf_counter() - t0), 1)
    except ImportError:
        rep["host_ms_scipy_distance_transform_edt"] = None
    t0 = time.perf_counter()
    d2 = rw.road_dist_ref(road, level, R)
    rep["host_ms_road_dist_ref"] = round(1e3 * (time.perf_counter() - t0), 1)
    t0 = time.perf_counter()
    want = rw.road_width_ref(nodes, edges, road, level, R, d2=d2)
    rep["host_ms_road_width_ref_edge_loop"] = round(1e3 * (time.perf_counter() - t0), 1)
    road_d = torch.from_numpy(road).to(dev)
    d2_d = net.road_dist(road_d, level, R)
    if not np.array_equal(d2_d.cpu().numpy(), d2):
        raise SystemExit(f"the device distance map differs from road_dist_ref on {int((d2_d.cpu().numpy() != d2).sum())} pixels")
    got = rw.edge_widths(nodes, edges, road, level, R, net=net)
    if not np.array_equal(got, want):
        raise SystemExit(f"the device statistics differ from road_width_ref on {int((got != want).any(axis=1).sum())} edges")
    rep["equals_road_dist_ref"] = rep["equals_road_width_ref"] = True
    rep["road_fraction"], rep["capped_fraction_of_road"] = round(float((d2 > 0).mean()), 4), round(float((d2 == R * R).sum() / max(1, (d2 > 0).sum())), 4)
    rep["covered_px_per_edge_mean"], rep["in_road_px_per_edge_mean"] = round(float(want[:, 0].mean()), 2), round(float(want[:, 1].mean()), 2)

    def wall_ms(fn):
        fn()
        ms = []
        for _ in range(iters):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            ms.append(1e3 * (time.perf_counter() - t0))
        ms.sort()
        return {"median": round(ms[len(ms) // 2], 4), "min_max": [round(ms[0], 4), round(ms[-1], 4)]}

    key = rw.road_width_key_of({"max_radius": R}, cfg.ROAD_THRESHOLD)
    result = (nodes, edges, road, road)
    rep["whole_apply_ms_from_host_arrays"] = wall_ms(lambda: rw.apply(key, result, net=net))
    rep["edge_widths_ms_from_host_arrays"] = wall_ms(lambda: rw.edge_widths(nodes, edges, road, level, R, net=net))
    rep["device_part_ms_mask_on_the_device"] = wall_ms(lambda: net.graph_edge_widths(nodes, edges, net.road_dist(road_d, level, R), R).cpu())
    ctx, _ = net._weights(dev)
    per_call = []
    for _ in range(3):                                     # three groups of `iters` calls: the run-to-run span of the kernel times
        ctx.profile_read()
        ctx.profile_enable(True)
        for _ in range(iters):
            net.graph_edge_widths(nodes, edges, net.road_dist(road_d, level, R), R)
        torch.cuda.synchronize()
        rows = {r["name"]: round(r["ms"] / r["launches"], 4) for r in ctx.profile_read() if r["launches"]}
        per_call.append({k: rows[k] for k in ("road_dist_cols", "road_dist_rows", "graph_edge_widths")})
        ctx.profile_enable(False)
    rep["kernel_ms_per_call_three_groups"] = per_call
    if args.no_pipelined:
        return rep
    stream = torch.cuda.Stream(dev)

    def png(a):
        Image.fromarray(a).save(io.BytesIO(), format="PNG", compress_level=1)

    stage = []

    def finish(res):
        t0 = time.perf_counter()
        with torch.cuda.stream(stream):
            rw.apply(key, res, net=net)
        stage.append(1e3 * (time.perf_counter() - t0))

    def piped(on, n=12, writers=3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        with ThreadPoolExecutor(writers) as pool:
            futs = []
            for res in inf.infer_imgs(net, (img for _ in range(n)), cfg):
                futs += [pool.submit(png, res[2]), pool.submit(png, res[3])]
                if on:
                    futs.append(pool.submit(finish, res))
            for f in futs:
                f.result()
        torch.cuda.synchronize()
        return round(1e3 * (time.perf_counter() - t0) / n, 2)

    for on in (False, True):
        piped(on, 3)
    stage.clear()
    runs = {"without_2_writers": [], "without": [], "with": []}      # the CLI adds a writer thread with the key: both pools, so the thread is not mistaken for the key
    for _ in range(3):
        for name, on, writers in (("without_2_writers", False, 2), ("without", False, 3), ("with", True, 3)):
            runs[name].append(piped(on, writers=writers))
    rep["pipelined_ms_per_scene_runs_of_12_alternated"] = runs
    rep["writer_thread_ms_per_scene_median_width_step"] = round(sorted(stage)[len(stage) // 2], 2)
    return rep


def float_report(args, net, cfg, img, rng, iters=20):
    """--float C [--float-range LO HI] [--float-percentile P Q]: the scene as a C-band float32 scene (bands 0..2 hold the synthetic RGB / 255,
    the rest noise).  The device result against float_scene_ref for both keys (the run ends if they differ); device ms of each SCENE_FLOAT
    launch alone (events around each of `iters` runs after a warm-up) with the bytes it moves; ms per scene of the pipelined loop handed
    float_scene_ref's uint8 scene and mask / with the fixed-range key / with the percentile key, alternated; host ms of float_scene_ref,
    the work the key takes off the feeding thread."""
    import sam_road_amd.inferencer as inf
    from sam_road_amd import Config
    from sam_road_amd import float_scene as fs
    dev = next(net.parameters()).device
    H, W = img.shape[:2]
    C = int(args.float)
    if not 3 <= C <= 16:
        raise SystemExit("--float takes C in 3..16")
    raw = rng.normal(size=(H, W, C)).astype(np.float32)
    raw[..., :3] = img.astype(np.float32) / np.float32(255)
    lo, hi = args.float_range or (0.0, 1.0)
    keys = {"fixed": {"select": [0, 1, 2], "stretch": [lo, hi]}, "percentile": {"select": [0, 1, 2], "stretch": {"percentile": list(args.float_percentile or (2.0, 98.0))}}}
    n = H * W
    rep = {"bands": C, "keys": keys, "upload_bytes": {"float_scene": int(raw.nbytes), "uint8_scene_and_mask": 4 * n}}
    refs = {}
    for name, key in keys.items():
        t0 = time.perf_counter()
        refs[name] = fs.float_scene_ref(raw, key)
        rep[f"host_ms_float_scene_ref_{name}"] = round(1e3 * (time.perf_counter() - t0), 1)
    raw_d = torch.from_numpy(raw).to(dev)
    k = fs.as_key(keys["percentile"])

    def device_ms(fn):
        fn()
        evs = []
        for _ in range(iters):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            evs.append((e0, e1))
        torch.cuda.synchronize()
        ms = sorted(a.elapsed_time(b) for a, b in evs)
        return ms[len(ms) // 2], ms[0], ms[-1]

    def row(ms, nbytes):
        return {"device_us_median": round(1e3 * ms[0], 1), "device_us_min_max": [round(1e3 * ms[1], 1), round(1e3 * ms[2], 1)], "bytes": int(nbytes),
                "GB_per_s_at_median": round(nbytes / ms[0] / 1e6, 1)}

    valid_d = net.scene_float_valid(raw_d, k.select)
    hist1 = net.scene_float_hist(raw_d, k.select, valid_d).cpu().numpy()
    targets, picks = fs.float_hist_targets(hist1, k)
    hist2 = net.scene_float_hist(raw_d, k.select, valid_d, targets).cpu().numpy()
    ranges = fs.float_ranges_from_hists(targets, picks, hist2, k)
    if [(a.tobytes(), b.tobytes()) for a, b in ranges] != [(a.tobytes(), b.tobytes()) for a, b in fs.float_ranges_ref(raw, k)]:
        raise SystemExit("the ranges of the two device histograms differ from float_ranges_ref")
    thr_d = torch.from_numpy(fs.threshold_keys(fs.float_thresholds(ranges, k))).to(dev)
    got = net.scene_float_apply(raw_d, k.select, valid_d, thr_d).cpu().numpy()
    if not np.array_equal(got, refs["percentile"][0]) or not np.array_equal(valid_d.cpu().numpy(), refs["percentile"][1]):
        raise SystemExit("the device scene or mask differs from float_scene_ref")
    line = 4 * C * n                                   # C <= 16: every 64-byte line of the source holds a selected band
    const_d = torch.full_like(raw_d, 0.5)
    rep["launches_alone"] = {
        "scene_float_valid": row(device_ms(lambda: net.scene_float_valid(raw_d, k.select)), line + n),
        "scene_float_hist_pass1": row(device_ms(lambda: net.scene_float_hist(raw_d, k.select, valid_d)), line + n + 3 * 65536 * 4),
        "scene_float_hist_pass1_constant_scene": row(device_ms(lambda: net.scene_float_hist(const_d, k.select, valid_d)), line + n + 3 * 65536 * 4),
        "scene_float_hist_pass2": dict(row(device_ms(lambda: net.scene_float_hist(raw_d, k.select, valid_d, targets)), line + n + len(targets) * 65536 * 4), targets=len(targets)),
        "scene_float_apply": row(device_ms(lambda: net.scene_float_apply(raw_d, k.select, valid_d, thr_d)), line + n + 3 * n)}
    rep["source_bytes_counted_as"] = "all C bands (whole cache lines), not only the 3 selected"
    del const_d
    if args.no_pipelined:
        return rep
    plain = Config({kk: v for kk, v in cfg.items() if kk != "SCENE_FLOAT"})
    cfgs = {name: Config(dict(plain, SCENE_FLOAT=key)) for name, key in keys.items()}
    u8, ok = refs["fixed"]
    inf._Lane.times = []

    def piped(c, scene, valid, n=12):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in inf.infer_imgs(net, (scene for _ in range(n)), c, **({} if valid is None else dict(valids=(valid for _ in range(n))))):
            pass
        torch.cuda.synchronize()
        return round(1e3 * (time.perf_counter() - t0) / n, 2)

    piped(plain, u8, ok, 3), piped(cfgs["fixed"], raw, None, 3), piped(cfgs["percentile"], raw, None, 3)
    inf._Lane.times.clear()
    runs = {"a_uint8_scene_and_mask_passed": [], "b_keyed_fixed_range": [], "c_keyed_percentile": []}
    for _ in range(3):
        runs["a_uint8_scene_and_mask_passed"].append(piped(plain, u8, ok))
        runs["b_keyed_fixed_range"].append(piped(cfgs["fixed"], raw, None))
        runs["c_keyed_percentile"].append(piped(cfgs["percentile"], raw, None))
    rep["pipelined_ms_per_scene_runs_of_12_alternated"] = runs
    p1 = sorted(t[1] for t in inf._Lane.times)
    rep["pass1_device_ms_median_of_all_scenes_above"] = round(p1[len(p1) // 2], 2) if p1 else None
    inf._Lane.times = None
    for name in keys:
        a = inf.infer_one_img(net, raw, cfgs[name])
        b = inf.infer_one_img(net, refs[name][0], plain, valid=refs[name][1])
        rep[f"keyed_equals_reference_passed_{name}"] = all(np.array_equal(x, y) for x, y in zip(a, b))
    rep["graph_points"], rep["edges"] = int(a[0].shape[0]), int(a[1].shape[0])
    return rep


def geotiff_report(args, net, cfg, img, rng, iters=20):
    """--geotiff {none,deflate,lzw} ... [--tiled] [--planar] [--geotiff-cache DIR]: the scene as a u8 RGB and as a 4-band uint16 GeoTIFF
    (bands 0..2 the synthetic RGB x 257, band 3 another blocky band; predictor 2 where compressed), written with the test kit's writer into
    a temporary directory (or kept in DIR from one run to the next: the kit's LZW coder is plain Python).  Per file: host ms of open_scene +
    segments() at the loader's thread count, upload ms of the flat array, device ms of srh_tiff_assemble alone with the bytes it moves, and
    srh_scene_bands_apply on the same raster as the yardstick of a bandwidth-bound pass; the same file through PIL where PIL reads it and
    the numpy steps of tiff_read_ref (cumsum, planar -> interleaved); the device raster against tiff_read_ref (the run ends if they
    differ); ms per scene of the pipelined loop fed the TIFF with the key and fed the .npy of the same scene, both through the CLI's
    three loader threads, three runs of 12 scenes each, alternated."""
    import tempfile
    from concurrent.futures import ThreadPoolExecutor
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
    import geotiff_kit as gk
    import sam_road_amd.inferencer as inf
    from sam_road_amd import Config
    from sam_road_amd import geotiff as gt
    from sam_road_amd.hostcpu import fill_threads
    dev = next(net.parameters()).device
    H, W = img.shape[:2]
    u16 = np.empty((H, W, 4), np.uint16)
    u16[..., :3] = img.astype(np.uint16) * 257
    u16[..., 3] = np.kron(rng.integers(0, 65536, size=(H // 8, W // 8)), np.ones((8, 8))).astype(np.uint16)
    rasters = {"u8_rgb": (img, {}), "u16_4band": (u16, dict(SCENE_BANDS={"select": [0, 1, 2], "stretch": [0, 65535]}))}
    work = args.geotiff_cache or tempfile.mkdtemp(prefix="scene_bench_tif_")
    os.makedirs(work, exist_ok=True)
    threads = fill_threads()
    report = {"loader_threads": 3, "decompress_threads": threads, "layout": ("tiles 512x512" if args.tiled else "strips") + (", planar" if args.planar else ""), "files": {}}

    def device_ms(fn):
        fn()
        evs = []
        for _ in range(iters):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            evs.append((e0, e1))
        torch.cuda.synchronize()
        ms = sorted(a.elapsed_time(b) for a, b in evs)
        return ms[len(ms) // 2], ms[0], ms[-1]

    def row(ms, nbytes):
        return {"device_us_median": round(1e3 * ms[0], 1), "device_us_min_max": [round(1e3 * ms[1], 1), round(1e3 * ms[2], 1)], "bytes": int(nbytes),
                "GB_per_s_at_median": round(nbytes / ms[0] / 1e6, 1)}

    def wall_ms(fn, n=3):
        best = None
        for _ in range(n):
            t0 = time.perf_counter()
            out = fn()
            t = 1e3 * (time.perf_counter() - t0)
            best = t if best is None or t < best else best
        return round(best, 2), out

    def fed(load, paths, c):                               # the CLI's loader: three threads decode ahead of the scene's turn
        def gen():
            with ThreadPoolExecutor(3) as ex:
                futs = {}
                for j in range(len(paths)):
                    for k in range(j, min(j + 3, len(paths))):
                        if k not in futs:
                            futs[k] = ex.submit(load, paths[k])
                    yield futs.pop(j).result()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in inf.infer_imgs(net, gen(), c):
            pass
        torch.cuda.synchronize()
        return round(1e3 * (time.perf_counter() - t0) / len(paths), 2)

    for rname, (raster, keys) in rasters.items():
        npy = os.path.join(work, f"{rname}.npy")
        np.save(npy, raster)
        t_cumsum, _ = wall_ms(lambda: np.cumsum(raster, axis=1, dtype=raster.dtype))
        planes = np.ascontiguousarray(raster.transpose(2, 0, 1))
        t_inter, _ = wall_ms(lambda: np.ascontiguousarray(planes.transpose(1, 2, 0)))
        report[f"{rname}_numpy_ms"] = {"cumsum": t_cumsum, "planar_to_interleaved": t_inter, "np_load": wall_ms(lambda: np.load(npy))[0]}
        raster_d = torch.from_numpy(raster).to(dev)
        lut = torch.zeros((3, 256 if raster.dtype == np.uint8 else 65536), dtype=torch.uint8, device=dev)
        report[f"{rname}_yardstick_scene_bands_apply"] = row(device_ms(lambda: net.scene_bands_apply(raster_d, [0, 1, 2], lut)), raster.nbytes + 3 * H * W)
        del raster_d
        base = Config(dict(cfg, **keys))
        keyed = Config(dict(base, GEOTIFF=True))
        for comp in args.geotiff:
            name = f"{rname}_{comp}_{'tiled' if args.tiled else 'strips'}{'_planar' if args.planar else ''}"
            path = os.path.join(work, name + ".tif")
            if not os.path.exists(path):
                gk.write_tiff(path, raster, compression=comp, predictor=1 if comp == "none" else 2, planar=2 if args.planar else 1,
                              tile=(512, 512) if args.tiled else None, rows_per_strip=None if args.tiled else 64, geo=gk.GEO)
            sc = gt.open_scene(path)
            rep = {"file_bytes": os.path.getsize(path), "segments": len(sc.offsets), "is_raster": bool(sc.is_raster)}
            rep["host_ms_open_and_segments"], (flat, table) = wall_ms(lambda: gt.open_scene(path).segments(threads))
            rep["host_ms_segments_one_thread"] = wall_ms(lambda: gt.open_scene(path).segments(1), 1)[0]
            if raster.dtype == np.uint8 and not args.planar:
                from PIL import Image
                try:
                    rep["host_ms_PIL_read"] = wall_ms(lambda: np.array(Image.open(path)))[0]
                except Exception as e:
                    rep["host_ms_PIL_read"] = f"PIL does not read it: {type(e).__name__}"

            def upload():
                t = torch.from_numpy(flat).to(dev)
                torch.cuda.synchronize()
                return t
            rep["upload_ms_pageable"], flat_d = wall_ms(upload)
            rep["flat_bytes"] = int(flat.size)
            if not sc.is_raster:
                table_d = torch.from_numpy(table).to(dev)
                got = net.tiff_assemble(sc, flat_d, table, table_d)
                if not gk.same_bits(got.cpu().numpy(), raster):
                    raise SystemExit(f"{name}: the device raster differs from the source")
                rep["tiff_assemble"] = row(device_ms(lambda: net.tiff_assemble(sc, flat_d, table, table_d)), flat.size + raster.nbytes)
            del flat_d
            report["files"][name] = rep
            if args.no_pipelined:
                continue
            load_tif = lambda p: gt.open_scene(p).load(threads)
            fed(load_tif, [path] * 3, keyed), fed(np.load, [npy] * 3, base)
            runs = {"tiff_with_the_key": [], "npy_of_the_same_scene": []}
            for _ in range(3):
                runs["tiff_with_the_key"].append(fed(load_tif, [path] * 12, keyed))
                runs["npy_of_the_same_scene"].append(fed(np.load, [npy] * 12, base))
            rep["pipelined_ms_per_scene_runs_of_12_alternated"] = runs
            a = inf.infer_one_img(net, gt.open_scene(path), keyed)
            b = inf.infer_one_img(net, raster, base)
            rep["keyed_equals_the_array_run"] = all(np.array_equal(x, y) for x, y in zip(a, b))
            rep["graph_points"], rep["edges"] = int(a[0].shape[0]), int(a[1].shape[0])
    return report


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bias", type=float, default=-2.2)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--wscale", type=float, default=16.0)   # spread of the final layer: with 16 the random net yields ~4k graph points
    ap.add_argument("--scene", nargs="+", default=["2048"], metavar="PX", help="scene size: S (square), H W or HxW; multiples of 8")
    ap.add_argument("--tiles", nargs="+", type=int, default=[16], metavar="N", help="INFER_PATCHES_PER_EDGE: N or N_Y N_X")
    ap.add_argument("--valid-frac", type=float, default=None, metavar="F",
                    help="run the scene with a validity mask: a diagonal band that covers the share F (0 < F <= 1) of its pixels")
    ap.add_argument("--fuse-window", default=None, metavar="NAME", choices=("uniform", "hann", "triangle"),
                    help="FUSE_WINDOW: how overlapping tiles are fused (default: the key is absent, the reference's uniform mean)")
    ap.add_argument("--tta", default=None, metavar="NAMES",
                    help="TTA: orientation names separated by commas, the first one id (default: the key is absent, one run per tile)")
    ap.add_argument("--scene-pad", type=int, default=None, metavar="B",
                    help="SCENE_PAD: pad the scene by B px on every side on the device (default: the key is absent)")
    ap.add_argument("--scene-pad-mode", default=None, metavar="MODE", choices=("reflect", "edge", "constant"),
                    help="SCENE_PAD's mode (default reflect)")
    ap.add_argument("--bands", nargs=2, default=None, metavar=("C", "DTYPE"),
                    help="SCENE_BANDS: the scene is a raw C-band scene of DTYPE uint8 / uint16 (bands 0..2 hold the synthetic RGB, the rest noise)")
    ap.add_argument("--stretch", nargs=3, default=None, metavar=("KIND", "A", "B"),
                    help="with --bands: 'range LO HI' (ints) or 'percentile PLO PHI' (default: the whole range of the dtype)")
    ap.add_argument("--scale", nargs=2, type=int, default=None, metavar=("P", "Q"),
                    help="SCENE_SCALE: the scene is at P/Q model pixels per scene pixel and is resampled on the device (default: the key is absent)")
    ap.add_argument("--mask-clean", nargs="+", default=None, metavar="V",
                    help="MASK_CLEAN: ROAD_MIN_AREA ROAD_MIN_PEAK [KEYPOINT_MIN_AREA KEYPOINT_MIN_PEAK] (default: the key is absent)")
    ap.add_argument("--nodata", nargs="+", type=int, default=None, metavar="V",
                    help="SCENE_NODATA: the value (one, or one per band); the synthetic scene gets a collar, a fringe and interior specks of it, the "
                         "derived mask is compared with nodata_ref, and the nodata launches, pass 1 and the pipelined loop are timed (one GPU; with "
                         "--bands C DTYPE the raw scene has C bands of that dtype)")
    ap.add_argument("--nodata-tolerance", type=int, default=None, metavar="T")
    ap.add_argument("--nodata-grow", type=int, default=None, metavar="R")
    ap.add_argument("--nodata-min-area", type=int, default=None, metavar="A")
    ap.add_argument("--aoi-frac", type=float, default=None, metavar="F",
                    help="SCENE_AOI: a star polygon that covers about F of the scene; the device mask is compared with aoi_ref, and scene_aoi_fill, pass 1 "
                         "and the pipelined loop are timed (one GPU; --no-pipelined: the fill alone)")
    ap.add_argument("--viz", action="store_true", help="GRAPH_RASTER: time the graph's renders (raster, composite, compare) on this scene and the pipelined "
                                                       "loop with and without them (the same leg as --diff)")
    ap.add_argument("--diff", action="store_true", help="GRAPH_RASTER: the same leg as --viz")
    ap.add_argument("--edge-support", type=int, nargs="?", const=1, default=None, metavar="T",
                    help="EDGE_SUPPORT: time the per-edge statistics at width T (default 1) on this scene and the pipelined loop without / with the filter, alternated")
    ap.add_argument("--road-width", type=int, nargs="?", const=32, default=None, metavar="R",
                    help="ROAD_WIDTH: time the distance map at max_radius R (default 32) and the per-edge statistics on this scene and the pipelined loop "
                         "without / with the key, alternated")
    ap.add_argument("--graph-clean", type=float, nargs="*", default=None, metavar="PX",
                    help="GRAPH_CLEAN: compare the device with graph_clean_ref on this scene's own graph and time the kernels, the whole call, the host "
                         "reference and the pipelined loop without / with the key; optional: min_spur and min_component in px (default 12 60)")
    ap.add_argument("--float", type=int, default=None, metavar="C",
                    help="SCENE_FLOAT: the scene arrives as a float32 scene of C bands (bands 0..2 hold the synthetic RGB / 255, the rest noise); "
                         "the three launches, the pipelined loop with a fixed range and with a percentile stretch and the host reference are timed")
    ap.add_argument("--float-range", nargs=2, type=float, default=None, metavar=("LO", "HI"), help="with --float: the fixed range (default 0 1)")
    ap.add_argument("--float-percentile", nargs=2, type=float, default=None, metavar=("P", "Q"), help="with --float: the percentiles (default 2 98)")
    ap.add_argument("--geotiff", nargs="+", default=None, choices=("none", "deflate", "lzw"), metavar="COMP",
                    help="GEOTIFF: write the scene to temporary TIFFs (u8 RGB and 4-band uint16) with the test kit's writer, time the decode on host and "
                         "device and run the pipelined loop on them against the .npy of the same scenes")
    ap.add_argument("--tiled", action="store_true", help="with --geotiff: 512 x 512 tiles instead of strips of 64 rows")
    ap.add_argument("--planar", action="store_true", help="with --geotiff: PlanarConfiguration 2")
    ap.add_argument("--geotiff-cache", default=None, metavar="DIR", help="with --geotiff: keep the files in DIR and reuse those that are there")
    ap.add_argument("--no-pipelined", action="store_true", help="skip the infer_imgs runs (12- and 48-scene streams)")
    ap.add_argument("--patch", type=int, default=512, metavar="P", help="PATCH_SIZE (default 512)")
    ap.add_argument("--margin", type=int, default=64, metavar="M", help="SAMPLE_MARGIN (default 64)")
    ap.add_argument("--scenes", type=int, default=None, metavar="M",
                    help="time a STREAM of M scenes of the given size through infer_imgs instead of one scene (one GPU)")
    ap.add_argument("--group", type=int, default=1, metavar="N", help="with --scenes: SCENE_GROUP, N consecutive scenes run as one (default 1: the key is absent)")
    args = ap.parse_args()
    H, W = parse_scene(args.scene)
    if len(args.tiles) not in (1, 2) or H % 8 or W % 8:
        ap.error("--tiles takes one or two counts; the synthetic scene is made of 8-px blocks")
    per_edge = args.tiles[0] if len(args.tiles) == 1 else list(args.tiles)
    from sam_road_amd import Config, SAMRoad
    from sam_road_amd.inferencer import infer_one_img
    from sam_road_amd.inferencer import _scene_plan
    from sam_road_amd.tiling import shard_tiles
    rank, local_rank, world = (int(os.environ.get(k, d)) for k, d in (("RANK", "0"), ("LOCAL_RANK", "0"), ("WORLD_SIZE", "1")))
    if world > 1:
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        torch.cuda.set_device(local_rank)
        dist.init_process_group("nccl", device_id=torch.device("cuda", local_rank))
    dev = torch.device("cuda", local_rank)
    torch.cuda.set_device(dev)
    from sam_road_amd.hostcpu import usable_cpus
    torch.set_num_threads(max(1, min(torch.get_num_threads(), usable_cpus() // world)))      # as the CLI does: respect the container's CPU quota
    cfg = Config(SAM_VERSION="vit_b", PATCH_SIZE=args.patch, TOPONET_VERSION="normal", SAM_CKPT_PATH="", DATASET="cityscale",
                 INFER_BATCH_SIZE=args.batch, SAMPLE_MARGIN=args.margin, INFER_PATCHES_PER_EDGE=per_edge, ITSC_THRESHOLD=0.248,
                 ROAD_THRESHOLD=0.364, TOPO_THRESHOLD=0.499, ITSC_NMS_RADIUS=8, ROAD_NMS_RADIUS=16, NEIGHBOR_RADIUS=64,
                 MAX_NEIGHBOR_QUERIES=16)
    if args.fuse_window is not None:
        cfg.FUSE_WINDOW = args.fuse_window
    if args.tta is not None:
        cfg.TTA = [t.strip() for t in args.tta.split(",")]
    if args.scene_pad is not None or args.scene_pad_mode is not None:
        cfg.SCENE_PAD = {"border": args.scene_pad or 0, "mode": args.scene_pad_mode or "reflect"}
    if args.scale is not None:
        if args.valid_frac is not None or args.scenes is not None:
            ap.error("--scale times one unmasked scene (not with --valid-frac or --scenes)")
        cfg.SCENE_SCALE = list(args.scale)
    if args.mask_clean is not None:
        if len(args.mask_clean) not in (2, 4) or args.scenes is not None or world > 1:
            ap.error("--mask-clean takes ROAD_MIN_AREA ROAD_MIN_PEAK [KEYPOINT_MIN_AREA KEYPOINT_MIN_PEAK]; one GPU, not with --scenes")
        v = args.mask_clean
        cfg.MASK_CLEAN = {"road": {"min_area": int(v[0]), "min_peak": float(v[1])}}
        if len(v) == 4:
            cfg.MASK_CLEAN["keypoint"] = {"min_area": int(v[2]), "min_peak": float(v[3])}
    from sam_road_amd.inferencer import fuse_window, mask_clean_plan, scene_pad_plan, tta_plan
    clean = mask_clean_plan(cfg)
    from sam_road_amd.resample import model_shape, scene_scale_key
    window = fuse_window(cfg)
    tta_names, tta = tta_plan(cfg)
    scale = scene_scale_key(cfg)
    Hm, Wm = model_shape((H, W), scale)                # the frame pass 1 runs in (the scene's own without --scale)
    pad = scene_pad_plan((Hm, Wm), cfg)
    pads = pad[:4] if pad is not None and any(pad[:4]) else None      # all four 0: the run of a scene without the key
    net = SAMRoad(cfg)
    g = torch.Generator().manual_seed(1234)
    sd = {}
    for k, v in net.state_dict().items():
        if v.dim() == 1 and k.endswith("weight"):
            sd[k] = 1.0 + 0.1 * torch.randn(v.shape, generator=g)
        else:
            sd[k] = 0.02 * torch.randn(v.shape, generator=g)
    sd["map_decoder.7.weight"] = args.wscale * torch.randn(sd["map_decoder.7.weight"].shape, generator=g)
    sd["map_decoder.7.bias"] = torch.full_like(sd["map_decoder.7.bias"], args.bias)
    if rank == 0:
        net.load_state_dict(sd, strict=True)
    net.eval().to(dev)
    t_w = time.perf_counter()
    net.share_packed_weights(src=0)          # N > 1: rank 0 packs once, the packed fp16 arena is broadcast over RCCL / xGMI
    torch.cuda.synchronize()
    t_w = time.perf_counter() - t_w
    rng = np.random.default_rng(0)
    coarse = rng.integers(0, 256, size=(H // 8, W // 8, 3)).astype(np.float32)
    img = np.kron(coarse, np.ones((8, 8, 1), np.float32)).astype(np.uint8)

    if args.nodata is not None:
        if world > 1 or args.scenes is not None or args.valid_frac is not None or args.scale is not None:
            ap.error("--nodata times one unmasked scene on one GPU (not with --scenes, --valid-frac or --scale)")
        from sam_road_amd.nodata import scene_nodata_override
        cfg.SCENE_NODATA = scene_nodata_override(cfg, args.nodata, args.nodata_tolerance, None, args.nodata_min_area, args.nodata_grow)
        raw = img
        if args.bands is not None:                         # bands 0..2 hold the synthetic RGB spread over the dtype's range, the rest noise
            C, dtype = int(args.bands[0]), np.dtype(args.bands[1])
            mul = 257 if dtype == np.uint16 else 1
            raw = rng.integers(0, 256 * mul, size=(H, W, C)).astype(dtype)
            raw[..., :3] = img.astype(dtype) * mul
            cfg.SCENE_BANDS = {"select": [0, 1, 2]}
        raw = np.ascontiguousarray(nodata_paint(raw, args.nodata[0], rng))
        print(json.dumps({"scene": f"synthetic {H}x{W} {raw.dtype} x {raw.shape[2]} with a collar, a fringe and specks of {args.nodata[0]}",
                          "infer_batch_size": args.batch, "scene_nodata": nodata_report(args, net, cfg, raw)}))
        return
    if args.aoi_frac is not None:
        if world > 1 or args.scenes is not None or args.valid_frac is not None or args.scale is not None or args.bands is not None or not 0.0 < args.aoi_frac <= 1.0:
            ap.error("--aoi-frac F, 0 < F <= 1, times one unmasked u8 scene on one GPU (not with --scenes, --valid-frac, --scale or --bands)")
        cfg.SCENE_AOI = {"include": [aoi_star(H, W, args.aoi_frac)]}
        print(json.dumps({"scene": f"synthetic {H}x{W} under a star polygon", "infer_batch_size": args.batch, "scene_aoi": aoi_report(args, net, cfg, img)}))
        return
    if args.viz or args.diff:
        if world > 1 or args.scenes is not None or args.valid_frac is not None or args.scale is not None or args.bands is not None:
            ap.error("--viz / --diff time one unmasked u8 scene on one GPU (not with --scenes, --valid-frac, --scale or --bands)")
        print(json.dumps({"scene": f"synthetic {H}x{W}", "infer_batch_size": args.batch, "graph_raster": graph_report(args, net, cfg, img)}))
        return
    if args.edge_support is not None:
        if world > 1 or args.scenes is not None or args.valid_frac is not None or args.scale is not None or args.bands is not None:
            ap.error("--edge-support times one unmasked u8 scene on one GPU (not with --scenes, --valid-frac, --scale or --bands)")
        print(json.dumps({"scene": f"synthetic {H}x{W}", "infer_batch_size": args.batch, "edge_support": edge_support_report(args, net, cfg, img)}))
        return
    if args.road_width is not None:
        if world > 1 or args.scenes is not None or args.valid_frac is not None or args.scale is not None or args.bands is not None:
            ap.error("--road-width times one unmasked u8 scene on one GPU (not with --scenes, --valid-frac, --scale or --bands)")
        print(json.dumps({"scene": f"synthetic {H}x{W}", "infer_batch_size": args.batch, "road_width": road_width_report(args, net, cfg, img)}))
        return
    if args.graph_clean is not None:
        if world > 1 or args.scenes is not None or args.valid_frac is not None or args.scale is not None or args.bands is not None or len(args.graph_clean) not in (0, 2):
            ap.error("--graph-clean [S C] times one unmasked u8 scene on one GPU (not with --scenes, --valid-frac, --scale or --bands)")
        print(json.dumps({"scene": f"synthetic {H}x{W}", "infer_batch_size": args.batch, "graph_clean": graph_clean_report(args, net, cfg, img)}))
        return
    if args.float is not None:
        if world > 1 or args.scenes is not None or args.valid_frac is not None or args.scale is not None or args.bands is not None:
            ap.error("--float C times one unmasked float32 scene on one GPU (not with --scenes, --valid-frac, --scale or --bands)")
        print(json.dumps({"scene": f"synthetic {H}x{W} float32 x {args.float}", "infer_batch_size": args.batch, "scene_float": float_report(args, net, cfg, img, rng)}))
        return
    if args.geotiff is not None:
        if world > 1 or args.scenes is not None or args.valid_frac is not None or args.scale is not None or args.bands is not None:
            ap.error("--geotiff times unmasked scenes on one GPU (not with --scenes, --valid-frac, --scale or --bands)")
        print(json.dumps({"scene": f"synthetic {H}x{W} as GeoTIFFs", "infer_batch_size": args.batch, "geotiff": geotiff_report(args, net, cfg, img, rng)}))
        return
    bands_report = None
    if args.bands is not None:
        if args.scenes is not None:
            ap.error("--bands times one scene (not with --scenes)")
        img, bands_report = bands_scene(args, net, cfg, img, dev, rng)
    elif args.stretch is not None:
        ap.error("--stretch goes with --bands")
    if args.scenes is not None:
        if world > 1 or args.scenes < 1 or args.group < 1:
            ap.error("--scenes M --group N take M, N >= 1 and one GPU")
        return stream(args, net, cfg, H, W)
    img, infos, all_xy = _scene_plan(img, cfg)         # the product's own validation and tile list (SCENE_PAD: of the padded scene)
    n_all = len(infos)
    valid = None
    if args.valid_frac is not None:
        if not 0.0 < args.valid_frac <= 1.0:
            ap.error("--valid-frac takes a share in (0, 1]")
        # |y / H - x / W| < w covers 1 - (1 - w)^2 of the rectangle
        yy, xx = np.mgrid[0:H, 0:W]
        valid = np.abs(yy / H - xx / W) < 1.0 - np.sqrt(1.0 - args.valid_frac)
        from sam_road_amd.inferencer import scene_tiles
        infos = scene_tiles(img.shape, cfg, valid=valid, net=net)
        all_xy = np.array([[p[1][0], p[1][1]] for p in infos], dtype=np.int32).reshape(-1, 2)
        if pads is not None:                           # scene_tiles speaks of the real scene's frame, the canvases are the padded scene's
            all_xy = all_xy + np.array([[pads[2], pads[0]]], dtype=np.int32)
    xy = torch.as_tensor(all_xy).to(dev)
    scene = torch.as_tensor(img).to(dev)
    valid_d = None if valid is None else torch.as_tensor(valid).to(dev)
    lo, hi = shard_tiles(len(infos), world, rank)
    wkw = {} if window is None else dict(window=torch.from_numpy(window).to(dev))
    tkw = {} if len(tta) == 1 else dict(tta=tta)                      # TTA: pass 1 runs the list once per orientation,
    xy_norm = xy if len(tta) == 1 else xy.repeat(len(tta), 1)         # the normalise gets the k-fold list

    def cleaned(kpu, ru):     # SCENE_PAD: the real scene's window of the masks of the padded scene, cut out on the device; MASK_CLEAN: the
        kpu, ru = (m if pads is None else m[pads[0]:pads[0] + Hm, pads[2]:pads[2] + Wm].contiguous() for m in (kpu, ru))      # filter on them
        return (kpu, ru) if clean is None else net.mask_clean_pair(kpu, ru, clean)

    def crop(m):              # SCENE_SCALE: the way back
        return m if scale is None else net.scene_resample(m, scale[1], scale[0], out_shape=(H, W))

    def pass1():              # this rank's share of the tiles (no collective: tile throughput)
        sc, vd = scene, valid_d
        if bands_report is not None:   # from the resident RAW scene: histogram + round trip (percentile), tables, apply are part of every pass 1
            sc = bands_front(net, cfg, scene, valid_d)
        if scale is not None:      # from the resident scene at its own resolution: the resample is part of every pass 1
            sc = net.scene_resample(sc, *scale)
        if pads is not None:       # from the resident real scene: the pad is part of every pass 1
            sc = net.scene_pad(sc, pads, pad[4], pad[5])
            vd = None if valid_d is None else net.scene_pad(valid_d, pads, pad[4], (0, 0, 0))
        if vd is not None:         # the masked pass 1 from the resident scene: count, fill (of a copy), kept tiles, masked normalise
            net.scene_tile_valid(vd, torch.as_tensor(_scene_plan(img, cfg)[2]).to(dev)).cpu()
            filled = net.scene_fill_invalid(sc.clone(), vd, (124, 116, 104))
            kp, road, emb = net.scene_pass1(filled, xy[lo:hi], args.batch, **wkw, **tkw)
            kpu, ru = cleaned(*net.scene_normalise(kp, road, xy_norm, valid=vd, **wkw))
            return crop(kpu).cpu(), crop(ru).cpu()
        kp, road, emb = net.scene_pass1(sc, xy[lo:hi], args.batch, **wkw, **tkw)
        kpu, ru = cleaned(*net.scene_normalise(kp, road, xy_norm, **wkw))
        return crop(kpu).cpu(), crop(ru).cpu()

    pass1()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.iters):
        pass1()
    torch.cuda.synchronize()
    p1 = (time.perf_counter() - t0) / args.iters
    # host-stage split: wrap the two host-side stages with timers
    import sam_road_amd.inferencer as inf
    acc = {"extract_graph_points": 0.0, "edge_votes": 0.0}
    def timed(name, fn):
        def w(*a, **k):
            torch.cuda.synchronize(); t = time.perf_counter(); r = fn(*a, **k); torch.cuda.synchronize()
            acc[name] += time.perf_counter() - t
            return r
        return w
    plain = inf.extract_graph_points, inf.edge_votes
    inf.extract_graph_points = timed("extract_graph_points", inf.extract_graph_points)
    inf.edge_votes = timed("edge_votes", inf.edge_votes)
    res = infer_one_img(net, img, cfg, valid=valid)
    for k in acc: acc[k] = 0.0
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.iters):
        res = infer_one_img(net, img, cfg, valid=valid)
    torch.cuda.synchronize()
    full = (time.perf_counter() - t0) / args.iters
    # throughput of the CLI's scene loop: the same scenes through the software-pipelined generator (one GPU only; the timed
    # region of a run covers 12 scenes from the first upload to the last edge list, so the pipeline's fill and drain are included;
    # the median of the runs is reported next to every run)
    piped, piped_runs, same, piped48 = None, None, None, None
    inf.extract_graph_points, inf.edge_votes = plain            # the timing wrappers synchronise the device
    if world == 1 and not args.no_pipelined:
        n, piped_runs, same = 12, [], True
        list(inf.infer_imgs(net, (img for _ in range(3)), cfg, valids=(valid for _ in range(3))))
        for _ in range(max(args.iters, 3)):                     # several runs: the rate varies in phases of a second or two
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            outs = list(inf.infer_imgs(net, (img for _ in range(n)), cfg, valids=(valid for _ in range(n))))
            torch.cuda.synchronize()
            piped_runs.append(round(1e3 * (time.perf_counter() - t0) / n, 2))
            same = same and all(all(np.array_equal(a, b) for a, b in zip(o, res)) for o in outs)
        piped = float(np.median(piped_runs)) * 1e-3
        torch.cuda.synchronize()                                 # one long run: fill + drain (~one scene) amortised over 48 scenes
        t0 = time.perf_counter()
        for o in inf.infer_imgs(net, (img for _ in range(48)), cfg, valids=(valid for _ in range(48))):
            pass
        torch.cuda.synchronize()
        piped48 = (time.perf_counter() - t0) / 48
    per_rank = None
    if world > 1:
        # per-rank stage times (ms): pass 1 of the rank's tile chunk, its pass-2 share, the whole call — gathered on rank 0
        mine = torch.tensor([1e3 * p1, 1e3 * acc["edge_votes"] / args.iters, 1e3 * acc["extract_graph_points"] / args.iters, 1e3 * full,
                             float(hi - lo)], dtype=torch.float64, device=dev)
        allr = [torch.zeros_like(mine) for _ in range(world)]
        dist.all_gather(allr, mine)
        per_rank = [dict(zip(("ms_pass1_own_tiles", "ms_edge_votes", "ms_extract_graph_points", "ms_full", "tiles"),
                             [round(v, 2) for v in a.tolist()])) for a in allr]
        t = torch.tensor([p1, full], dtype=torch.float64, device=dev)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        p1, full = t.tolist()
    if rank != 0:
        if world > 1:
            dist.destroy_process_group()
        return
    nodes, edges, kp, road = res
    print(json.dumps({"scene": f"synthetic {H}x{W} u8, {n_all} tiles of {args.patch}^2 ({per_edge} per edge, margin {args.margin})", "n_gpus": world,
                      "fuse_window": args.fuse_window or "uniform",
                      "tta": tta_names,
                      "scene_pad": None if pad is None else {"pads": list(pad[:4]), "mode": pad[4]},
                      "scene_bands": bands_report,
                      "scene_scale": None if scale is None else scale_report(net, scale, scene if bands_report is None else bands_front(net, cfg, scene)),
                      "mask_clean": None if clean is None else mask_clean_report(net, cfg, img, valid, pass1),
                      "valid_frac": None if valid is None else round(float(valid.mean()), 4), "tiles_kept": len(infos), "tiles_all": n_all,
                      "ms_weight_share": round(1e3 * t_w, 2) if world > 1 else None, "per_rank": per_rank,
                      "infer_batch_size": args.batch, "ms_per_scene_pass1": round(1e3 * p1, 2),
                      "tiles_per_s_pass1": round(len(infos) / p1, 1), "ms_per_scene_full": round(1e3 * full, 2),
                      "ms_per_scene_pipelined": None if piped is None else round(1e3 * piped, 2), "pipelined_runs_of_12_scenes": piped_runs,
                      "ms_per_scene_pipelined_run_of_48": None if piped48 is None else round(1e3 * piped48, 2),
                      "pipelined_equals_serial": same,
                      "ms_extract_graph_points": round(1e3 * acc["extract_graph_points"] / args.iters, 2),
                      "ms_edge_votes": round(1e3 * acc["edge_votes"] / args.iters, 2), "graph_points": int(nodes.shape[0]), "edges": int(edges.shape[0]),
                      "kp_mask_frac": float((kp > cfg.ITSC_THRESHOLD * 255).mean()),
                      "road_mask_frac": float((road > cfg.ROAD_THRESHOLD * 255).mean())}))
    if world > 1:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
