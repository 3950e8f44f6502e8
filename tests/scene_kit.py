"""What the scene tests share, once: configurations, scene / mask builders, comparison helpers, the (oracle, net) pair, the CPU
stand-in model, the gloo harness, the CLI harness, the oracle's pass 1 with every scene option, and the oracle-parity check.

A plain module (not collected; tests/test_scene_kit.py is its CPU self-test).  Importing it does not touch the GPU: torch.cuda is used
inside functions only.  The oracle side (oracle_scene, the stand-in's orientation table) uses nothing of sam_road_amd."""
import contextlib
import os
import pickle
import re
import socket
import warnings

import numpy as np
import pytest
import torch

import tolerances
from oracle import scene as oscene
from oracle.samroad import AttrDict, SAMRoadOracle
from oracle.synth import synth_scene, synth_state_dict

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# ---- configurations ---------------------------------------------------------------------------------------------------------------
# the GPU scene tests: 256-px tiles, a two-block encoder (windowed + global)
CFG = dict(SAM_VERSION="vit_b", PATCH_SIZE=256, TOPONET_VERSION="normal", SAM_CKPT_PATH="",
           ENCODER_DEPTH=2, ENCODER_GLOBAL_ATTN_INDEXES=[1],
           INFER_BATCH_SIZE=5, SAMPLE_MARGIN=16, INFER_PATCHES_PER_EDGE=4,
           ITSC_THRESHOLD=0.5, ROAD_THRESHOLD=0.5, TOPO_THRESHOLD=0.5,
           ITSC_NMS_RADIUS=8, ROAD_NMS_RADIUS=16, NEIGHBOR_RADIUS=64, MAX_NEIGHBOR_QUERIES=16)
# the host tests on the stand-in: 128-px tiles keep the oracle at seconds, and 384 x 640 = 3 x 5 such tiles exactly, so a disjoint tiling
# exists: every canvas pixel then has ONE addend and a multi-rank result must be IDENTICAL to the single-process one
HOST_CFG = dict(SAM_VERSION="vit_b", PATCH_SIZE=128, TOPONET_VERSION="normal", SAM_CKPT_PATH="", ENCODER_DEPTH=1,
                ENCODER_GLOBAL_ATTN_INDEXES=[], INFER_BATCH_SIZE=3, SAMPLE_MARGIN=16, INFER_PATCHES_PER_EDGE=5,
                ITSC_THRESHOLD=0.5, ROAD_THRESHOLD=0.5, TOPO_THRESHOLD=0.5, ITSC_NMS_RADIUS=8, ROAD_NMS_RADIUS=16,
                NEIGHBOR_RADIUS=64, MAX_NEIGHBOR_QUERIES=16)
# the square 256-px scenes of tests/test_distributed_cpu.py and tests/test_scene_pad_host.py
E2E_CFG = dict(HOST_CFG, PATCH_SIZE=256, INFER_PATCHES_PER_EDGE=3)
E2E_SCENE = 352
FILL = (124, 116, 104)
# (H, W, INFER_PATCHES_PER_EDGE, scene seed): 15 tiles in 5 columns, and the odd row pitch whose rows are not aligned against each
# other (tile origins 16, 94, 173, 251 / 16, 54, 91, 129: none divisible by 16)
SCENES = {"384x640": (384, 640, [3, 5], 41), "401x523": (401, 523, 4, 43)}
PARITY_SCENES = dict(SCENES, **{"523x701": (523, 701, [4, 5], 44)})      # a larger odd pitch: half of 401 x 523 is too small a graph
KP_PERCENTILE, ROAD_PERCENTILE = 99.5, 98.0
NAMES = ("id", "flip_h", "flip_v", "rot180", "transpose", "rot90", "rot270", "anti_transpose")      # index = orientation code
# the orientation table of DESIGN.md §6f, restated: these expressions ARE the definition
ORIENT = {
    "id": lambda T: T,
    "flip_h": lambda T: T[:, ::-1],
    "flip_v": lambda T: T[::-1, :],
    "rot180": lambda T: T[::-1, ::-1],
    "transpose": lambda T: T.swapaxes(0, 1),
    "rot90": lambda T: np.rot90(T, 1, axes=(0, 1)),
    "rot270": lambda T: np.rot90(T, 3, axes=(0, 1)),
    "anti_transpose": lambda T: T[::-1, ::-1].swapaxes(0, 1),
}
UNORIENT = dict(ORIENT, rot90=ORIENT["rot270"], rot270=ORIENT["rot90"])     # the others are their own inverse


# ---- scene and mask builders ------------------------------------------------------------------------------------------------------
def rect_scene(H, W, seed):
    """oracle.synth.synth_scene is square: a contiguous rectangle cut out of a larger square."""
    return np.ascontiguousarray(synth_scene(max(H, W), seed=seed)[:H, :W])


def rect_grid(H, W, margin, P, per_edge):
    """The reference's tile rule (dataset.py:56-67) per axis, restated independently of sam_road_amd/tiling.py: x origins from W and
    n_x, y origins from H and n_y, x outer / y inner.  per_edge: int or [n_y, n_x]."""
    n_y, n_x = (per_edge, per_edge) if isinstance(per_edge, int) else per_edge
    xs = [round(v) for v in np.linspace(start=margin, stop=W - (P + margin), num=n_x)]
    ys = [round(v) for v in np.linspace(start=margin, stop=H - (P + margin), num=n_y)]
    return [(0, (x, y), (x + P, y + P)) for x in xs for y in ys]


def make_mask(kind, H, W):
    """bool [H, W]."""
    yy, xx = np.mgrid[0:H, 0:W]
    if kind == "all":
        return np.ones((H, W), bool)
    if kind == "none":
        return np.zeros((H, W), bool)
    if kind == "band":                                    # |distance from the main diagonal| below a quarter: about half the pixels
        return np.abs(yy / H - xx / W) < 0.29
    if kind == "hole":                                    # nodata strictly inside: kept tiles straddle its edge
        m = np.ones((H, W), bool)
        m[H // 3:H // 3 + 130, W // 3:W // 3 + 150] = False
        return m
    if kind in ("pixel", "pixel_mid"):                    # two different inputs: the GPU tests' pixel lies near the left edge (only the
        m = np.zeros((H, W), bool)                        # first tile column holds it), the host tests' in the middle
        m[H // 2 + 3, 21 if kind == "pixel" else W // 2 + 5] = True
        return m
    if kind == "left":
        return xx < 300
    raise KeyError(kind)


def np_counts(valid, infos):
    return np.array([int(valid[y0:y1, x0:x1].sum()) for _, (x0, y0), (x1, y1) in infos], dtype=np.int64)


def np_kept(valid, infos, P, frac=0.0):
    c = np_counts(valid, infos)
    return np.flatnonzero((c > 0) & (c >= frac * P * P))


def np_pad(arr, pads, mode, fill=FILL):
    """numpy.pad is the reference of the three SCENE_PAD modes; a constant colour goes channel by channel."""
    top, bottom, left, right = pads
    width = ((top, bottom), (left, right))
    if mode != "constant":
        return np.ascontiguousarray(np.pad(arr, width + ((0, 0),) * (arr.ndim - 2), mode=mode))
    if arr.ndim == 2:
        return np.ascontiguousarray(np.pad(arr, width, mode="constant", constant_values=arr.dtype.type(fill[0])))
    return np.ascontiguousarray(np.stack([np.pad(arr[..., c], width, mode="constant", constant_values=fill[c]) for c in range(arr.shape[2])], -1))


def shift_infos(infos, pads):
    """Tiles of the padded scene in the frame of the real one."""
    top, _, left, _ = pads
    return [(k, (x0 - left, y0 - top), (x1 - left, y1 - top)) for k, (x0, y0), (x1, y1) in infos]


def crop_pads(m, pads, shape):
    return np.ascontiguousarray(m[pads[0]:pads[0] + shape[0], pads[2]:pads[2] + shape[1]])


# ---- comparison helpers -----------------------------------------------------------------------------------------------------------
def same_bits(a, b):
    """Equal dtype, shape and bit patterns (floats compared as bytes); tensors or arrays."""
    a, b = (np.ascontiguousarray(t.detach().cpu().numpy() if torch.is_tensor(t) else t) for t in (a, b))      # (embeddings arrive as a permuted view)
    assert a.dtype == b.dtype and a.shape == b.shape, (a.dtype, b.dtype, a.shape, b.shape)
    np.testing.assert_array_equal(a.view(np.uint8) if a.dtype.kind == "f" else a, b.view(np.uint8) if b.dtype.kind == "f" else b)


def same_tuple(a, b):
    for x, y in zip(a, b):
        assert np.asarray(x).dtype == np.asarray(y).dtype
        np.testing.assert_array_equal(np.asarray(x), np.asarray(y))


def thresholds(kp_m, road_m):
    return dict(ITSC_THRESHOLD=float(np.percentile(kp_m[kp_m > 0], KP_PERCENTILE)) / 255.0,
                ROAD_THRESHOLD=float(np.percentile(road_m[road_m > 0], ROAD_PERCENTILE)) / 255.0)


def xy_of(infos):
    return torch.tensor([[p[1][0], p[1][1]] for p in infos], dtype=torch.int32).reshape(-1, 2).cuda()


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ---- model builders ---------------------------------------------------------------------------------------------------------------
def build_oracle(cfg, seed=77, decoder_bias=(-0.3, 0.2)):
    """(oracle, state dict) with synthetic weights; the decoder bias gives denser masks than the default -3."""
    warnings.simplefilter("ignore")
    oracle = SAMRoadOracle(AttrDict(cfg)).eval()
    sd = synth_state_dict(oracle, seed)
    sd["map_decoder.7.bias"] = torch.tensor(decoder_bias)
    oracle.load_state_dict(sd, strict=True)
    return oracle, sd


def build_pair(cfg, seed=77, decoder_bias=(-0.3, 0.2)):
    """(oracle on the CPU, SAMRoad on the GPU) with the same weights."""
    from sam_road_amd import Config, SAMRoad
    oracle, sd = build_oracle(cfg, seed, decoder_bias)
    net = SAMRoad(Config(cfg))
    net.load_state_dict(sd, strict=True)
    net.eval().to("cuda")
    return oracle, net


@pytest.fixture(scope="module")
def pair():
    return build_pair(CFG)


_NETS = {}


def net_for(P):
    """A model object per PATCH_SIZE (the shim reads the tile size from it); one encoder block keeps the weight packing short."""
    from sam_road_amd import Config, SAMRoad
    if P not in _NETS:
        warnings.simplefilter("ignore")
        _NETS[P] = SAMRoad(Config(dict(CFG, PATCH_SIZE=P, ENCODER_DEPTH=1, ENCODER_GLOBAL_ATTN_INDEXES=[]))).eval().to("cuda")
    return _NETS[P]


# ---- the CPU stand-in -------------------------------------------------------------------------------------------------------------
def _tile_valid(self, valid, tile_xy):
    self.calls.append(("tile_valid", int(tile_xy.shape[0])))
    v = valid.numpy() != 0
    return torch.tensor([int(v[y0:y0 + self.P, x0:x0 + self.P].sum()) for x0, y0 in tile_xy.tolist()], dtype=torch.int32)


class SceneStandIn(torch.nn.Module):
    """SAMRoad's scene-level interface (scene_pass1 / scene_normalise / infer_toponet) on the CPU oracle, for [H, W] scenes, in CPU
    torch, logging its calls.  features, a subset of {"valid", "window", "tta", "pad"}, switches on what the scene features added to
    that interface — valid: scene_tile_valid, scene_fill_invalid, scene_normalise(valid=); window: window= on both passes (the rule of
    DESIGN.md §6e in f32, tile by tile in list order); tta: scene_pass1(tta=) (§6f: for every orientation the whole list, the crop
    oriented, the scores brought back, then the add) and a ("normalise", n) log entry; pad: scene_pad from numpy.pad.  The gate is strict:
    a method of a feature that is off does not exist and its keyword is a TypeError, so a library that passes an option in the case
    where it must make the calls it always made fails on the stand-in without the feature."""
    FEATURES = ("valid", "window", "tta", "pad")

    def __init__(self, cfg, features=()):
        super().__init__()
        assert set(features) <= set(self.FEATURES), features
        self.oracle, _ = build_oracle(cfg)
        self.P, self.features, self.calls = cfg["PATCH_SIZE"], frozenset(features), []
        if "valid" in self.features:
            self.scene_tile_valid, self.scene_fill_invalid = self._tile_valid, self._fill_invalid
        if "pad" in self.features:
            self.scene_pad = self._pad

    def _options(self, where, kw, *names):
        for k in kw:
            if k not in names or k not in self.features:
                raise TypeError(f"{where}() got an unexpected keyword argument '{k}'")
        return [kw.get(k) for k in names]

    def scene_pass1(self, scene, tile_xy, bs, **kw):
        window, tta = self._options("scene_pass1", kw, "window", "tta")
        n, (H, W), P = int(tile_xy.shape[0]), scene.shape[:2], self.P
        if tta is not None:
            self.calls.append(("pass1_tta", n, tuple(tta), window is not None))
            assert tta[0] == 0 and len(set(tta)) == len(tta) > 1
        else:
            self.calls.append(("pass1", n) if window is None else ("pass1_window", n))
        if window is not None:
            assert window.dtype == torch.float32 and tuple(window.shape) == (P,)
            w2 = window[:, None] * window[None, :]
        kp, road = torch.zeros((H, W)), torch.zeros((H, W))
        embs = []
        for code in tta or [0]:
            for x0, y0 in tile_xy.tolist():
                crop = scene[y0:y0 + P, x0:x0 + P]
                if tta is None:
                    s, e = self.oracle.infer_masks_and_img_features(crop.float()[None])
                    s = s[0]
                else:
                    crop = np.ascontiguousarray(ORIENT[NAMES[code]](crop.numpy()))
                    s, e = self.oracle.infer_masks_and_img_features(torch.from_numpy(crop).float()[None])
                    s = torch.from_numpy(np.ascontiguousarray(UNORIENT[NAMES[code]](s[0].detach().numpy())))
                kp[y0:y0 + P, x0:x0 + P] += s[:, :, 0] if window is None else w2 * s[:, :, 0]
                road[y0:y0 + P, x0:x0 + P] += s[:, :, 1] if window is None else w2 * s[:, :, 1]
                if code == 0:
                    embs.append(e)
        emb = torch.cat(embs) if embs else torch.zeros((0, 256, P // 16, P // 16))
        return kp, road, emb

    def scene_normalise(self, kp, road, tile_xy, **kw):
        valid, window = self._options("scene_normalise", kw, "valid", "window")
        if "tta" in self.features:
            self.calls.append(("normalise", int(tile_xy.shape[0])))
        if window is not None:
            self.calls.append(("normalise_window", int(tile_xy.shape[0])))
        w2 = 1.0 if window is None else window[:, None] * window[None, :]
        wsum = torch.zeros_like(kp)                          # the coverage count without a window
        for x0, y0 in tile_xy.tolist():
            wsum[y0:y0 + self.P, x0:x0 + self.P] += w2
        u8 = lambda t: torch.nan_to_num(t / wsum * 255, nan=0.0).to(torch.uint8)
        kp_u8, road_u8 = u8(kp), u8(road)
        if valid is not None:
            kp_u8[valid == 0] = 0
            road_u8[valid == 0] = 0
        return kp_u8, road_u8

    def infer_toponet(self, emb, points, pairs, valid):
        return self.oracle.infer_toponet(emb, points, pairs.long(), valid.bool())

    _tile_valid = _tile_valid

    def _fill_invalid(self, scene, valid, fill):
        self.calls.append(("fill", tuple(fill)))
        scene[valid == 0] = torch.tensor(fill, dtype=torch.uint8)
        return scene

    def _pad(self, t, pads, mode="reflect", fill=(0, 0, 0)):
        self.calls.append(("pad", tuple(pads), mode))
        return torch.from_numpy(np_pad(t.numpy(), pads, mode, fill))


class _CountOnly(torch.nn.Module):
    """A model object that can count and nothing else: whatever else is called raises AttributeError."""

    def __init__(self, P):
        super().__init__()
        self.P, self.w, self.calls = P, torch.nn.Parameter(torch.zeros(1)), []

    scene_tile_valid = _tile_valid


# ---- the gloo harness -------------------------------------------------------------------------------------------------------------
def free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def rank_worker(world, rank, port, out, spec):
    """One rank of a tile-sharded run on gloo / CPU (world 1: the single-process run).  spec, a plain dict:
      base "host" | "e2e", overrides       the config
      features                             of the SceneStandIn
      shapes, seeds, kinds                 the scenes (seed 60 + i by default, a negative seed is an all-zero scene) and their masks
      mode "serial" | "pipelined"          which loop's results are returned (world 1: always infer_one_img's)
      threads                              torch threads per rank
      checks                               in-rank assertions by name, see below
    Puts (rank, [tuple or None per scene], stats)."""
    import torch.distributed as dist
    warnings.simplefilter("ignore")
    if world > 1:
        os.environ["MASTER_ADDR"] = "127.0.0.1"
        os.environ["MASTER_PORT"] = str(port)
        dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from sam_road_amd import Config
        from sam_road_amd import distributed as D
        from sam_road_amd.inferencer import _infer_imgs_tile_sharded, infer_imgs, infer_one_img
        torch.set_num_threads(spec.get("threads", 2))
        D._CHECK_BANDS[0] = True                  # every sender asserts that its canvas is zero outside the band it ships
        cfg = dict(E2E_CFG if spec.get("base") == "e2e" else HOST_CFG, **(spec.get("overrides") or {}))
        net = SceneStandIn(cfg, spec.get("features", ()))
        shapes, checks, stats = spec["shapes"], spec.get("checks", ()), {}
        seeds = spec.get("seeds") or [60 + i for i in range(len(shapes))]
        imgs = [rect_scene(h, w, s) if s >= 0 else np.zeros((h, w, 3), np.uint8) for (h, w), s in zip(shapes, seeds)]
        kinds = spec.get("kinds")
        valids = [None] * len(imgs) if kinds is None else [None if k is None else make_mask(k, h, w) for k, (h, w) in zip(kinds, shapes)]
        vkw = (lambda v: {}) if kinds is None else (lambda v: dict(valids=v))

        def equal(got, want):
            for a, b in zip(got, want):
                assert (a is None) == (b is None) == (rank != 0)
                if a is not None:
                    same_tuple(a, b)

        net.calls.clear()
        serial = [infer_one_img(net, im, Config(cfg), device="cpu", **({} if kinds is None else dict(valid=v))) for im, v in zip(imgs, valids)]
        if "window_calls" in checks:
            assert not [c for c in net.calls if c[0] in ("pass1", "normalise")]          # every pass 1 was the weighted one
            assert ("normalise_window" in [c[0] for c in net.calls]) == (rank == 0)    # rank 0 alone normalises, with the full list
        got = serial
        if spec.get("mode") == "pipelined" and world > 1:
            # same world size: same summation orders, so the pipelined and the serial tile-sharded loop agree exactly
            got = list(infer_imgs(net, iter(imgs), Config(dict(cfg, TILE_SHARD_PIPELINE=True)), device="cpu", **vkw(valids)))
            equal(got, serial)
            if "serial_loop" in checks:           # infer_imgs without the key: the serial tile-sharded loop
                equal(list(infer_imgs(net, iter(imgs), Config(cfg), device="cpu", **vkw(iter(valids)))), serial)
            if "sharded_generator" in checks:     # the generator itself, with its traffic statistics; an empty list of scenes
                equal(list(_infer_imgs_tile_sharded(net, iter(imgs), Config(cfg), device="cpu", stats=stats)), serial)
                assert list(infer_imgs(net, iter([]), Config(cfg), device="cpu", tile_sharded=True)) == []
        out.put((rank, [None if r is None else [np.asarray(a) for a in r] for r in got], stats))
    except Exception:  # pragma: no cover
        import traceback
        out.put((rank, "ERR " + traceback.format_exc(), None))
    finally:
        if world > 1:
            dist.destroy_process_group()


def run_worlds(worlds, spec, stats=None):
    """rank_worker at every world size: {world: rank 0's results}.  stats, a dict, receives rank 0's traffic statistics."""
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    results = {}
    for world in worlds:
        port, q = free_port(), ctx.Queue()
        procs = [ctx.Process(target=rank_worker, args=(world, r, port, q, spec)) for r in range(world)]
        for p in procs:
            p.start()
        got = dict((r, (v, st)) for r, v, st in (q.get(timeout=900) for _ in range(world)))
        for p in procs:
            p.join(timeout=60)
        for r, (v, _) in got.items():
            assert not isinstance(v, str), v
            assert all((x is None) == (r != 0) for x in v)                     # only rank 0 returns the graphs
        results[world] = got[0][0]
        if stats is not None:
            stats.update(got[0][1])
    return results


def compare_worlds(one, many, shapes, kinds, must_be_identical):
    """A disjoint tiling gives every canvas pixel one addend, so the multi-rank result is IDENTICAL; with overlapping tiles the f32
    canvas sums are associated differently across ranks and the u8 truncation may turn the last bit into one level on a few pixels."""
    kinds = kinds or [None] * len(shapes)
    assert len(one) == len(many) == len(shapes)
    for (n1, e1, k1, r1), (nw, ew, kw, rw), hw, kind in zip(one, many, shapes, kinds):
        assert k1.shape == r1.shape == kw.shape == rw.shape == tuple(hw)
        valid = make_mask(kind, *hw) if kind is not None else np.ones(hw, bool)
        if kind == "none":
            assert n1.shape == nw.shape == (0, 2) and e1.shape == ew.shape == (0, 2) and not k1.any() and not kw.any() and not rw.any()
            continue
        assert n1.shape[0] > 30 and e1.shape[0] > 100
        assert n1[:, 0].max() < hw[0] and n1[:, 1].max() < hw[1]               # (row, col)
        assert valid[n1[:, 0], n1[:, 1]].all() and valid[nw[:, 0], nw[:, 1]].all()
        assert not kw[~valid].any() and not rw[~valid].any()
        assert np.abs(k1.astype(int) - kw.astype(int)).max() <= 1 and np.abs(r1.astype(int) - rw.astype(int)).max() <= 1
        same_masks = np.array_equal(k1, kw) and np.array_equal(r1, rw)
        print(hw, kind, "masks identical to single process:", same_masks, "| nodes", n1.shape[0], "edges", e1.shape[0])
        assert same_masks or not must_be_identical
        if same_masks:
            np.testing.assert_array_equal(n1, nw)
            np.testing.assert_array_equal(e1, ew)                              # same edges in the same (insertion) order
        else:
            assert abs(n1.shape[0] - nw.shape[0]) <= 2


# ---- the CLI harness --------------------------------------------------------------------------------------------------------------
def run_cli(cli, net, tmp_path, monkeypatch, name, cfg, images, *argv):
    """cli.main (sam_road_amd.cli, the module whose _build_net it replaces) in tmp_path with the model replaced by net: writes cfg as {name}.yaml, runs --output_dir name on the image files, reads
    the results back: {image stem: (itsc mask, road mask, graph, the saved config)}."""
    import yaml
    from PIL import Image
    monkeypatch.chdir(tmp_path)
    monkeypatch.setattr(cli, "_build_net", lambda config, checkpoint, device: net)
    with open(f"{name}.yaml", "w") as f:
        yaml.safe_dump(dict(cfg, DATASET="cityscale"), f)
    cli.main(["--config", f"{name}.yaml", "--checkpoint", "none", "--device", "cpu", "--output_dir", name, *argv, "--images", *images])
    saved = yaml.safe_load(open(f"save/{name}/config.yaml"))
    out = {}
    for stem in [os.path.splitext(os.path.basename(p))[0] for p in images]:
        with open(f"save/{name}/graph/{stem}.p", "rb") as f:
            g = pickle.load(f)
        out[stem] = (np.array(Image.open(f"save/{name}/mask/{stem}_itsc.png")), np.array(Image.open(f"save/{name}/mask/{stem}_road.png")), g, saved)
    return out


def make_fake_dataset(work, dataset, ids, cfg, size):
    """The directory the CLI reads without --images: work/cfg.yaml and one synthetic size x size scene per id in the dataset's layout."""
    import json
    import yaml
    from PIL import Image
    os.makedirs(work)
    with open(work / "cfg.yaml", "w") as f:
        yaml.safe_dump(dict(cfg, DATASET=dataset), f)
    if dataset == "spacenet":
        os.makedirs(work / "spacenet" / "RGB_1.0_meter")
        with open(work / "spacenet" / "data_split.json", "w") as f:
            json.dump({"train": ["x"], "validation": ["y"], "test": ids}, f)
        pat = "spacenet/RGB_1.0_meter/{}__rgb.png"
    else:
        os.makedirs(work / "cityscale" / "20cities")
        pat = "cityscale/20cities/region_{}_sat.png"
    for j, i in enumerate(ids):
        Image.fromarray(synth_scene(size, seed=100 + j)).save(work / pat.format(i))


@contextlib.contextmanager
def kernel_rows(ctx):
    """Profile capture on the library context: yields a function that returns the set of kernel names launched since its last call."""
    def read():
        torch.cuda.synchronize()
        return {r["name"] for r in ctx.profile_read() if r["launches"]}
    ctx.profile_read()                                       # reading clears the rows
    ctx.profile_enable(True)
    try:
        yield read
    finally:
        ctx.profile_enable(False)


def assert_abi_11(names_with_arg_counts):
    """The symbol table equals the header, the entries exist with their argument counts, and the ABI stays 11: (header text, lib)."""
    from sam_road_amd import _lib
    header = open(os.path.join(ROOT, "include", "samroad_hip.h")).read()
    declared = set(re.findall(r"^[A-Za-z_][\w \*]*?\b(srh_\w+)\(", header, flags=re.M))
    assert declared == set(_lib.SYMBOLS), (declared ^ set(_lib.SYMBOLS))
    lib = _lib.load()
    assert lib.srh_abi_version() == _lib.ABI_VERSION == int(re.search(r"#define SRH_ABI_VERSION (\d+)", header).group(1)) == 11
    for name, n_args in names_with_arg_counts:
        assert hasattr(lib, name) and len(_lib.SYMBOLS[name][1]) == n_args
        decl = re.search(r"\bint %s\(([^;]*)\);" % name, header).group(1)
        assert len(decl.split(",")) == n_args
    return header, lib


# ---- the oracle's side ------------------------------------------------------------------------------------------------------------
def fuse_f64(shape, xy, scores, w1_f32, prior=None):
    """The weighted rule of FUSE_WINDOW in float64: (kp, road, Wsum, cover count) for tile origins xy [n,2] (x0, y0) and scores
    [n,P,P,2]; the weights are the exact products of the f32 profile values."""
    H, W = shape
    P = w1_f32.shape[0]
    w2 = np.outer(w1_f32.astype(np.float64), w1_f32.astype(np.float64))       # [ly, lx]
    kp = np.zeros((H, W)) if prior is None else prior[0].astype(np.float64)
    road = np.zeros((H, W)) if prior is None else prior[1].astype(np.float64)
    ws, cnt = np.zeros((H, W)), np.zeros((H, W), np.int64)
    for (x0, y0), s in zip(np.asarray(xy).tolist(), scores):
        kp[y0:y0 + P, x0:x0 + P] += w2 * s[:, :, 0]
        road[y0:y0 + P, x0:x0 + P] += w2 * s[:, :, 1]
        ws[y0:y0 + P, x0:x0 + P] += w2
        cnt[y0:y0 + P, x0:x0 + P] += 1
    return kp, road, ws, cnt


def oracle_scene(oracle, img, per_edge, cfg=CFG, valid=None, window=None, orientations=None, pads=None):
    """The oracle's pass 1 from oracle.scene's public pieces: (infos, feats, kp u8, road u8).  With no option, get_batch_img_patches ->
    infer_masks_and_img_features -> fuse_masks on the tiles of rect_grid.  valid: bool [H, W] — the kept tiles on the filled scene, the
    masks zeroed on nodata.  window: the f32 profile — the per-tile scores fused by fuse_f64, 0 where no tile covers the pixel.
    orientations: names — every tile once per orientation, un-oriented and fused over the k-fold list; feats are those of id.  pads:
    (top, bottom, left, right) — the scene reflected by numpy.pad, the masks cropped, the tiles in the real scene's frame."""
    P, bs = cfg["PATCH_SIZE"], cfg["INFER_BATCH_SIZE"]
    shape = img.shape[:2]
    if pads is not None:
        assert valid is None
        img = np_pad(img, pads, "reflect")
    H, W = img.shape[:2]
    infos = rect_grid(H, W, cfg["SAMPLE_MARGIN"], P, per_edge)
    if valid is not None:
        infos = [infos[i] for i in np_kept(valid, infos, P)]
        img = np.ascontiguousarray(np.where(valid[..., None], img, np.array(FILL, np.uint8)))
    names = ["id"] if orientations is None else list(orientations)
    feats, scores = [], []
    for name in names:
        for i in range(0, len(infos), bs):
            batch = oscene.get_batch_img_patches(img, infos[i:i + bs])
            if name != "id":
                batch = torch.from_numpy(np.stack([np.ascontiguousarray(ORIENT[name](t)) for t in batch.numpy()]))
            s, f = oracle.infer_masks_and_img_features(batch)
            if name != "id":
                s = torch.from_numpy(np.stack([np.ascontiguousarray(UNORIENT[name](t)) for t in s.detach().numpy()]))
            scores.append(s)
            if name == "id":
                feats.append(f)
    if window is None:
        kp, road = (m.copy() for m in oscene.fuse_masks((H, W), infos * len(names), scores))
    else:
        s64 = np.concatenate([s.detach().numpy().astype(np.float64) for s in scores])
        kp, road, ws, _ = fuse_f64((H, W), [p[1] for p in infos] * len(names), s64, window)
        kp, road = (np.where(ws > 0, np.floor(c / np.where(ws > 0, ws, 1.0) * 255.0), 0.0).astype(np.uint8) for c in (kp, road))
    if valid is not None:
        kp[~valid] = 0
        road[~valid] = 0
    if pads is not None:
        infos, kp, road = shift_infos(infos, pads), crop_pads(kp, pads, shape), crop_pads(road, pads, shape)
    return infos, feats, kp, road


def check_scene_parity(tag, result, oracle_result, cfg, oracle, valid=None, min_voted=50, min_oracle_edges=None):
    """infer_one_img's (nodes, edges, kp, road) against oracle_scene's (infos, feats, kp, road), stage-wise on IDENTICAL intermediate
    inputs — greedy NMS on the u8 masks is chaotic w.r.t. +-1-level differences, one different pick cascades.  Masks: within one level
    on U8_WITHIN1 of the pixels, at most two anywhere.  Points: the product's host stage equals the oracle's on the product's masks, and
    they are the nodes.  Edges: pass 2 of the oracle (its own fp32 features) on the same points — every oracle decision farther than
    TOPO_SCORE from the threshold is reproduced, and the symmetric difference is at most max(2, 2 %) of the oracle's edges.  The scene
    must give a graph that makes these conditions: more than 20 points, more than min_voted voted edges (or at least min_oracle_edges
    oracle edges), at most 5 % of them left out by the firm filter.  With a tag the measurements are recorded (tolerances.check); the
    tests that predate the record pass None.  Returns the (x, y) points."""
    from sam_road_amd import Config
    from sam_road_amd.graph_points import extract_graph_points
    nodes, edges, kp, road = result
    infos, feats, kp_r, road_r = oracle_result
    assert kp.shape == road.shape == kp_r.shape and kp.dtype == road.dtype == np.uint8
    assert kp_r.max() > 0 and road_r.max() > 0

    def check(name, value, bound, at_least=False):
        if tag is not None:
            tolerances.check(f"{tag}_{name}", value, bound, at_least)
        assert value >= bound if at_least else value < bound, (name, value, bound)

    for name, got, ref in (("kp", kp, kp_r), ("road", road, road_r)):
        d = np.abs(got.astype(int) - ref.astype(int))
        print(f"[parity] {tag}_{name}_u8_max_diff: {d.max()} levels (bound <= 2)")
        check(f"{name}_u8_within1", (d <= 1).mean(), tolerances.U8_WITHIN1, at_least=True)
        check(f"{name}_u8_max_diff", d.max(), 3)                                 # integers: < 3 is <= 2 levels
        assert d.max() <= 2
        if valid is not None:
            assert not got[~valid].any() and got[valid].any()
    pts = extract_graph_points(kp, road, Config(cfg))
    np.testing.assert_array_equal(pts, oscene.extract_graph_points(kp, road, AttrDict(cfg)))
    np.testing.assert_array_equal(nodes, pts[:, ::-1])
    assert pts.shape[0] > 20, "the scene produced too few points to be a meaningful test"
    assert pts.min() >= 0 and pts[:, 0].max() < kp.shape[1] and pts[:, 1].max() < kp.shape[0]      # (x, y)
    if valid is not None:
        assert valid[pts[:, 1], pts[:, 0]].all()                                 # no node on nodata
    edges_r, sums_r, cnts_r = oscene.infer_pass2(oracle, feats, pts, infos, AttrDict(cfg))
    got = {(int(a), int(b)) for a, b in edges.tolist()}
    ref = {(int(a), int(b)) for a, b in edges_r.tolist()}
    firm = {e for e, s in sums_r.items() if abs(s / cnts_r[e] - cfg["TOPO_THRESHOLD"]) > tolerances.TOPO_SCORE}
    if min_oracle_edges is not None:
        assert len(ref) >= min_oracle_edges, f"the scene must give the oracle at least {min_oracle_edges} edges for the 2 % cap to be a condition"
    else:
        assert len(sums_r) > min_voted
    left_out = 1.0 - len(firm) / len(sums_r)
    print(f"[parity] {tag}: {len(infos)} tiles, {pts.shape[0]} points, {len(sums_r)} voted edges, {len(ref)} oracle edges, "
          f"firm filter leaves out {left_out:.4f}, symmetric difference {len(got ^ ref)}")
    assert left_out <= 0.05
    assert {e for e in ref if e in firm} == {e for e in got if e in firm}
    check("edge_symdiff", len(got ^ ref), int(max(2, 0.02 * len(ref))) + 1)      # integers: < floor(b) + 1 is <= b
    assert len(got ^ ref) <= max(2, 0.02 * len(ref))
    return pts
