"""world_size-2 gloo tests of the N>1 exchange steps (sam_road_amd/distributed.py) on CPU."""
import os

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from scene_kit import E2E_CFG as _E2E_CFG       # bench.py --plumbing-cpu takes _E2E_CFG and _CpuStandIn from this module
from scene_kit import E2E_SCENE as _E2E_SCENE
from scene_kit import SceneStandIn as _CpuStandIn
from scene_kit import free_port as _free_port
from scene_kit import make_fake_dataset, run_worlds


def _worker(rank, world, port, out):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from sam_road_amd import distributed as D
    from sam_road_amd.tiling import shard_tiles
    try:
        # weights: one flat broadcast
        g = torch.Generator().manual_seed(3)
        ref = {"a.weight": torch.randn(5, 7, generator=g), "b.bias": torch.randn(11, generator=g)}
        sd = ref if rank == 0 else {k: torch.empty_like(v) for k, v in ref.items()}
        got = D.broadcast_state_dict(sd, src=0)
        assert all(torch.equal(got[k], ref[k]) for k in ref)
        # canvases: each rank adds its own tiles, reduce == single-process sum
        S, P = 96, 32
        tiles = [(x, y) for x in (0, 21, 43, 64) for y in (0, 21, 43, 64)]
        rng = np.random.default_rng(0)
        patches = rng.random((len(tiles), P, P, 2)).astype(np.float32)
        full_kp = np.zeros((S, S), np.float32); full_rd = np.zeros((S, S), np.float32)
        for (x, y), pch in zip(tiles, patches):
            full_kp[y:y + P, x:x + P] += pch[..., 0]; full_rd[y:y + P, x:x + P] += pch[..., 1]
        lo, hi = shard_tiles(len(tiles), world, rank)
        kp = torch.zeros((S, S)); rd = torch.zeros((S, S))
        for (x, y), pch in zip(tiles[lo:hi], patches[lo:hi]):
            kp[y:y + P, x:x + P] += torch.tensor(pch[..., 0]); rd[y:y + P, x:x + P] += torch.tensor(pch[..., 1])
        kp_dense, rd_dense = kp.clone(), rd.clone()
        D.reduce_canvases(kp_dense, rd_dense, dst=0)                     # dense form: one reduce of both full canvases
        # band form: every rank ships only the columns its tile chunk touches (x-outer tile order => vertical bands)
        bands = D.tile_bands(np.array(tiles), P, world)
        assert bands == [(0, 21 + P), (43, 64 + P)] if world == 2 else True
        for r_, (x0, x1) in enumerate(bands):                            # a rank's canvas is zero outside its band
            if r_ == rank:
                assert float(kp[:, :x0].abs().sum() + kp[:, x1:].abs().sum()) == 0.0
        D.reduce_canvases(kp, rd, dst=0, bands=bands)
        if rank == 0:
            np.testing.assert_allclose(kp.numpy(), full_kp, atol=1e-5)
            np.testing.assert_allclose(rd.numpy(), full_rd, atol=1e-5)
            np.testing.assert_allclose(kp_dense.numpy(), full_kp, atol=1e-5)
            assert torch.equal(kp, kp_dense) and torch.equal(rd, rd_dense)   # two ranks: one addition per pixel either way
        # packed weights: a byte buffer held by rank 0 only
        blob = torch.arange(1000, dtype=torch.int64).to(torch.uint8) if rank == 0 else None
        got_blob = D.broadcast_bytes(blob, src=0)
        assert got_blob.dtype == torch.uint8 and torch.equal(got_blob, torch.arange(1000, dtype=torch.int64).to(torch.uint8))
        # raw votes: rank-major concatenation == the one-process visiting order, so ONE accumulation is exact
        rngv = np.random.default_rng(5)
        all_k = rngv.integers(0, 50, size=400).astype(np.int64)
        all_s = rngv.random(400)
        cut = 170
        kk, ss = (all_k[:cut], all_s[:cut]) if rank == 0 else (all_k[cut:], all_s[cut:])
        gk, gs = D.gather_raw_votes(kk, ss, dst=0)
        if rank == 0:
            np.testing.assert_array_equal(gk, all_k)
            np.testing.assert_array_equal(gs, all_s)
        else:
            assert gk is None and gs is None
        # points broadcast (incl. empty)
        pts = np.array([[3, 4], [50, 60], [7, 7]], dtype=np.int64)
        np.testing.assert_array_equal(D.broadcast_points(pts if rank == 0 else None, src=0), pts)
        assert D.broadcast_points(np.zeros((0, 2), np.int64) if rank == 0 else None, src=0).shape == (0, 2)
        # edge votes: overlapping keys across ranks are summed
        n_pts = 100
        if rank == 0:
            k, s, c = np.array([5, 17, 230], np.int64), np.array([0.5, 1.5, 0.25]), np.array([1.0, 2.0, 1.0])
            f = np.array([7, 0, 3], np.int64)
        else:
            k, s, c = np.array([17, 999], np.int64), np.array([0.5, 0.75]), np.array([1.0, 1.0])
            f = np.array([1, 0], np.int64)
        uk, us, uc, uf = D.gather_edge_votes(k, s, c, n_pts, dst=0, first=f)
        if rank == 0:
            np.testing.assert_array_equal(uk, [5, 17, 230, 999])
            np.testing.assert_allclose(us, [0.5, 2.0, 0.25, 0.75])
            np.testing.assert_allclose(uc, [1.0, 3.0, 1.0, 1.0])
            # first-vote order: rank-major, then the rank's local position => 17 (rank 0, pos 0), 230, 5, 999 (rank 1)
            np.testing.assert_array_equal(uk[np.argsort(uf)], [17, 230, 5, 999])
        else:
            assert uk is None
        out.put((rank, "ok"))
    except Exception as e:  # pragma: no cover
        out.put((rank, repr(e)))
    finally:
        dist.destroy_process_group()


def test_exchange_steps_world2_gloo():
    world = 2
    port = _free_port()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = [q.get(timeout=120) for _ in range(world)]
    for p in procs:
        p.join(timeout=60)
    assert sorted(res) == [(0, "ok"), (1, "ok")], res


# ---------------------------------------------------------------------------------------------------------------------------------
# The whole N > 1 data flow of infer_one_img (tile sharding, canvas reduce, point broadcast, per-rank pass 2, vote gather with
# first-vote order) on gloo, world 3, against the single-process run.  The GPU model is replaced by the CPU stand-in of
# tests/scene_kit.py, built on the oracle (test infrastructure) — what is under test is the orchestration in
# sam_road_amd/inferencer.py and sam_road_amd/distributed.py, which is exactly the code the 8-GPU run executes.
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scene_size,overrides,must_be_identical", [
    (_E2E_SCENE, None, False),                                               # overlapping tiles (the shipped tilings)
    (512, dict(SAMPLE_MARGIN=0, INFER_PATCHES_PER_EDGE=2), True),            # disjoint tiles: every canvas pixel has ONE addend
    (512, dict(SAMPLE_MARGIN=0, INFER_PATCHES_PER_EDGE=2, EXACT_VOTE_MERGE=True), True),   # raw votes merged on rank 0 (exact sums)
])
def test_infer_one_img_world3_matches_single_process(scene_size, overrides, must_be_identical):
    results = run_worlds((1, 3), dict(base="e2e", overrides=overrides, shapes=[(scene_size, scene_size)], seeds=[6], mode="serial"))
    (n1, e1, k1, r1), (n3, e3, k3, r3) = results[1][0], results[3][0]
    assert n1.shape[0] > 30 and e1.shape[0] > 100
    # canvases are summed in a different association order across ranks: the f32 sums may differ in the last bit, which the
    # u8 truncation can turn into one level on a few pixels
    assert np.abs(k1.astype(int) - k3.astype(int)).max() <= 1 and np.abs(r1.astype(int) - r3.astype(int)).max() <= 1
    same_masks = np.array_equal(k1, k3) and np.array_equal(r1, r3)
    print("world-3 masks identical to single process:", same_masks, "| nodes", n1.shape[0], "edges", e1.shape[0])
    assert same_masks or not must_be_identical
    if same_masks:
        np.testing.assert_array_equal(n1, n3)
        np.testing.assert_array_equal(e1, e3)                                # same edges in the same (insertion) order
    else:
        assert abs(n1.shape[0] - n3.shape[0]) <= 2


def test_infer_imgs_pipeline_matches_infer_one_img():
    """The software-pipelined scene generator (infer_imgs: pass 1 of scene i+1 queued before scene i's host stages, staging pools
    reused every second scene) yields exactly infer_one_img's tuples, in order — checked on the CPU stand-in with three different
    scenes (the third reuses the first one's staging pool), and once more with thresholds no pixel can pass (no graph points: the early-out path of every stage)."""
    import warnings
    warnings.simplefilter("ignore")
    from oracle.synth import synth_scene
    from sam_road_amd import Config
    from sam_road_amd.inferencer import infer_imgs, infer_one_img
    torch.set_num_threads(4)
    cfg = dict(_E2E_CFG)
    net = _CpuStandIn(cfg)
    imgs = [synth_scene(_E2E_SCENE, seed=6), np.zeros((_E2E_SCENE, _E2E_SCENE, 3), np.uint8), synth_scene(_E2E_SCENE, seed=9)]
    want = [infer_one_img(net, im, Config(cfg), device="cpu") for im in imgs]
    got = list(infer_imgs(net, iter(imgs), Config(cfg), device="cpu"))
    assert len(got) == len(want) == 3
    n_pts = [w[0].shape[0] for w in want]
    print("graph points per scene:", n_pts, "edges:", [w[1].shape[0] for w in want])
    assert max(n_pts) > 30
    for w, g in zip(want, got):
        for a, b in zip(w, g):
            np.testing.assert_array_equal(np.asarray(a), np.asarray(b))
            assert np.asarray(a).dtype == np.asarray(b).dtype
    assert list(infer_imgs(net, iter([]), Config(cfg), device="cpu")) == []
    none = Config(dict(cfg, ITSC_THRESHOLD=1.0, ROAD_THRESHOLD=1.0))
    want = [infer_one_img(net, im, none, device="cpu") for im in imgs[:2]]
    got = list(infer_imgs(net, iter(imgs[:2]), none, device="cpu"))
    for w, g in zip(want, got):
        assert w[0].shape[0] == 0 and w[1].shape == (0, 2)
        for a, b in zip(w, g):
            np.testing.assert_array_equal(np.asarray(a), np.asarray(b))
            assert np.asarray(a).dtype == np.asarray(b).dtype


def _cli_rank(world, rank, port, work, out):
    """One rank of `torchrun ... -m sam_road_amd.inferencer --shard scenes` (gloo, CPU): the model is replaced by a function of
    the image, so this checks the multi-process plumbing of the CLI only."""
    try:
        os.environ.update(RANK=str(rank), LOCAL_RANK=str(rank), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        os.chdir(work)
        from sam_road_amd import cli, inferencer as inf
        seen = []

        def fake_infer_imgs(net, imgs, config, device=None, tile_sharded=None, pipelined=None):
            assert tile_sharded is False                      # scene sharding: no collective on the data path
            for im in imgs:
                seen.append(int(im[:8, :8].astype(np.int64).sum()))
                nodes = np.array([[1, 2], [3, 4], [int(im[0, 0, 0]), 7]], dtype=np.int64)
                yield nodes, np.array([[0, 1], [1, 2]], dtype=np.int64), im[:, :, 0].copy(), im[:, :, 1].copy()
        inf.infer_imgs = fake_infer_imgs
        cli._build_net = lambda config, checkpoint, device: None
        inf.main(["--config", "cfg.yaml", "--checkpoint", "ckpt.ckpt", "--output_dir", "run2", "--device", "cpu"])
        out.put((rank, seen))
    except Exception:  # pragma: no cover
        import traceback
        out.put((rank, "ERR " + traceback.format_exc()))
    finally:
        if dist.is_initialized():
            dist.destroy_process_group()


def test_cli_scene_sharding_world2(tmp_path, golden_dir):
    """The CLI under a 2-process launch, `--shard scenes` (default): ranks take the test scenes round-robin, write into ONE output
    directory, rank 0 writes config.yaml and inference_time.txt (max over ranks); every scene's files exist exactly once."""
    import pickle
    from PIL import Image
    work = tmp_path / "cityscale"
    ids = [int(i) for i in np.load(f"{golden_dir}/refrun_cli.npz")["cityscale_ids"]]      # the test split the CLI reads
    make_fake_dataset(work, "cityscale", ids, dict(_E2E_CFG, INFER_PATCHES_PER_EDGE=2), 288)
    ctx = mp.get_context("spawn")
    q, port = ctx.Queue(), _free_port()
    procs = [ctx.Process(target=_cli_rank, args=(2, r, port, str(work), q)) for r in range(2)]
    for p in procs:
        p.start()
    got = dict(q.get(timeout=300) for _ in range(2))
    for p in procs:
        p.join(timeout=60)
    for r, v in got.items():
        assert not isinstance(v, str), v
    assert len(got[0]) == len(ids[0::2]) and len(got[1]) == len(ids[1::2])
    outdir = work / "save" / "run2"
    files = sorted(os.path.relpath(os.path.join(d, f), outdir) for d, _, fs in os.walk(outdir) for f in fs)
    want = sorted(["config.yaml", "inference_time.txt"] + [f"mask/{i}_road.png" for i in ids] + [f"mask/{i}_itsc.png" for i in ids]
                  + [f"graph/{i}.p" for i in ids])
    assert files == want
    for j, i in enumerate(ids):                                   # each scene was processed by the rank that owns it, from ITS image
        src = np.array(Image.open(work / "cityscale" / "20cities" / f"region_{i}_sat.png").convert("RGB"))
        np.testing.assert_array_equal(np.array(Image.open(outdir / "mask" / f"{i}_itsc.png")), src[:, :, 0])
        np.testing.assert_array_equal(np.array(Image.open(outdir / "mask" / f"{i}_road.png")), src[:, :, 1])
        assert int(src[:8, :8].astype(np.int64).sum()) == got[j % 2][j // 2]
        gr = pickle.load(open(outdir / "graph" / f"{i}.p", "rb"))
        assert (int(src[0, 0, 0]), 7) in gr
    assert open(outdir / "inference_time.txt").read().startswith("Inference completed for cfg.yaml in ")


# ---------------------------------------------------------------------------------------------------------------------------------
# Tile-sharded scenes, software-pipelined (inferencer._infer_imgs_tile_sharded: pass 1 of scene i+1 is queued before the host
# stages of scene i; the band receives are posted at once): world 8 on gloo against the single-process results.
# ---------------------------------------------------------------------------------------------------------------------------------
def test_pipelined_tile_sharded_scenes_world8_match_single_process():
    """Three scenes (one of them all-zero pixels) through the pipelined tile-sharded generator on 8 ranks — more ranks than
    tiles, so half of them own an empty shard and an empty band — with disjoint tiles (every canvas pixel has one addend: the
    results must be IDENTICAL to the single-process run, edges in the same order)."""
    # in the ranks: the generator itself, infer_imgs' serial tile-sharded loop (the default under torch.distributed) and the pipelined one
    # by config key give the same graphs
    spec = dict(base="e2e", overrides=dict(SAMPLE_MARGIN=0, INFER_PATCHES_PER_EDGE=2), shapes=[(512, 512)] * 3, seeds=[6, -1, 9],
                mode="pipelined", threads=1, checks=("serial_loop", "sharded_generator"))
    stats = {}
    results = run_worlds((1, 8), spec, stats=stats)
    one, eight = results[1], results[8]
    assert len(one) == len(eight) == 3 and one[0][0].shape[0] > 30 and one[2][1].shape[0] > 100
    for a, b in zip(one, eight):
        for x, y in zip(a, b):
            np.testing.assert_array_equal(x, y)
            assert x.dtype == y.dtype
    assert stats["scenes"] == 3 and stats["canvas_bytes"] > 0 and stats["points_bytes"] > 0 and stats["votes_bytes"] >= 0


def test_bench_launch_contract_two_ranks_on_cpu():
    """`python -m torch.distributed.run --nproc-per-node 2 ... bench.py --gpus 2 --plumbing-cpu`: the driver's multi-GPU launch
    line on gloo / CPU with the oracle stand-in — rank / world / master address from the environment, collectives connect both
    ranks, rank 0 prints ONE JSON line; the tile-sharded scenes equal the one-process run.  The BARE form `python bench.py --gpus 2
    ...` (no launcher environment) re-execs itself under the launcher and prints the same 2-rank line — it can never report a
    one-rank run as the 2-GPU point; a launcher whose WORLD_SIZE contradicts --gpus is refused."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env["OMP_NUM_THREADS"] = "1"
    lines = {}
    for form, n in (("plain", 1), ("launcher", 2), ("bare", 2)):
        cmd = [sys.executable, os.path.join(root, "bench.py"), "--gpus", str(n), "--plumbing-cpu"]
        if form == "launcher":
            cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(n), "--master-addr", "127.0.0.1",
                   "--master-port", str(_free_port())] + cmd[1:]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=900, env=env, cwd=root)
        assert r.returncode == 0, r.stderr[-2000:]
        js = [json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")]
        assert len(js) == 1, r.stdout
        lines[form] = js[0]
    for form in ("launcher", "bare"):
        two = lines[form]
        assert two["collective_ranks"] == 2 and two["n_gpus"] == 2 and two["plumbing_only"] and two["value"] is None
        assert lines["plain"]["graph_points"] == two["graph_points"] and lines["plain"]["edges"] == two["edges"]
        assert len(two["per_rank"]) == 2 and two["per_rank"][1][1] > 0        # rank 1 shipped canvas bytes
        # the N > 1 line carries EVERY rank's roofline figures (bench.gather_per_rank: one all_gather after the timed region), not rank 0's alone
        prr = two["per_rank_roofline"]
        assert [e["rank"] for e in prr] == [0, 1]
        assert all(set(e) == {"rank", "dominant_kernel_frac", "gemm_frac", "dominant_avg_launch_ms", "sustained_tiles_per_s",
                              "smi_sclk_mhz_under_load"} for e in prr)
    # a launcher environment that contradicts --gpus: refused with the launch line, nothing printed as a result
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "4", "--plumbing-cpu"], capture_output=True, text=True,
                       timeout=120, env=dict(env, WORLD_SIZE="1", RANK="0"), cwd=root)
    assert r.returncode != 0 and "torch.distributed.run" in r.stderr and not [l for l in r.stdout.splitlines() if l.startswith("{")]
