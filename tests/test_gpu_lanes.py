"""Lanes: encode_batch runs the encoder of a batch as two half-batch chains on two streams (include/samroad_hip.h srh_ctx_set_lanes,
sam_road_amd/csrc/api_model.hip EncLane).  Tiles never interact in the encoder and a lane runs the kernels the whole call would run, on
half the rows, so every comparison here is torch.equal: forced lanes against two one-lane calls on the halves, auto at its smallest
eligible shape against one lane, the scene loop, the stream semantics the caller sees, the sentinel, and the context's memory.
Shapes: ViT-B with two blocks, one windowed and one global; 128-px tiles (8 x 8 tokens: a padded 14-window, lanes of one tile, the
generic GEMMs with split-K in fc2 at two tiles per lane) and 512-px tiles at B = 16 (half a batch = 8192 tokens = 128 z192 tiles, the
bound of auto).  Run on an MI355X: pytest -m gpu."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle.synth import synth_scene, synth_tiles

from scene_kit import build_pair, kernel_rows

CFG = dict(SAM_VERSION="vit_b", TOPONET_VERSION="normal", SAM_CKPT_PATH="", ENCODER_DEPTH=2, ENCODER_GLOBAL_ATTN_INDEXES=[1])


@pytest.fixture(scope="module")
def pair128():
    return build_pair(dict(CFG, PATCH_SIZE=128))


@pytest.fixture(scope="module")
def pair512():
    return build_pair(dict(CFG, PATCH_SIZE=512))


@pytest.fixture
def lanes():
    """set(mode) on the process's one library context; auto again afterwards, whatever the test did."""
    from sam_road_amd import _lib
    ctx = _lib.Context.get(torch.cuda.current_device())
    try:
        yield ctx
    finally:
        ctx.set_lanes(0)


def run(net, rgb):
    s, e = net.infer_masks_and_img_features(rgb)
    torch.cuda.synchronize()
    return s, e


@pytest.mark.parametrize("B", [4, 2])
def test_forced_lanes_equal_two_half_calls(pair128, lanes, B):
    net = pair128[1]
    rgb = synth_tiles(B, 128, seed=5).cuda()
    lanes.set_lanes(2)
    s2, e2 = run(net, rgb)
    assert lanes.last_lanes() == 2
    lanes.set_lanes(1)
    halves = [run(net, rgb[:B // 2]), run(net, rgb[B // 2:])]
    assert lanes.last_lanes() == 1
    assert torch.equal(s2, torch.cat([h[0] for h in halves])) and torch.equal(e2, torch.cat([h[1] for h in halves]))
    # (not against ONE call on the whole batch: at these sizes fc2's split-K factor follows the row count — 4 slices at 128 rows, none
    # at 64 — so a call's bits depend on its own batch size, lanes or not; auto only pairs shapes that dispatch alike)
    assert torch.isfinite(e2).all() and e2.abs().max() > 0


def test_odd_batch_stays_one_lane(pair128, lanes):
    net = pair128[1]
    rgb = synth_tiles(3, 128, seed=6).cuda()
    lanes.set_lanes(2)
    s2, e2 = run(net, rgb)
    assert lanes.last_lanes() == 1
    lanes.set_lanes(1)
    s1, e1 = run(net, rgb)
    assert torch.equal(s2, s1) and torch.equal(e2, e1)


def test_bad_mode_is_refused(lanes):
    from sam_road_amd import _lib
    with pytest.raises(_lib.SrhError, match="srh_ctx_set_lanes"):
        lanes.set_lanes(3)


@pytest.fixture(scope="module")
def one_lane_512(pair512):
    """The one-lane outputs at auto's smallest eligible shape, computed once."""
    from sam_road_amd import _lib
    ctx = _lib.Context.get(torch.cuda.current_device())
    rgb = synth_tiles(16, 512, seed=7).cuda()
    ctx.set_lanes(1)
    try:
        s, e = run(pair512[1], rgb)
        assert ctx.last_lanes() == 1
    finally:
        ctx.set_lanes(0)
    return rgb, s, e


def test_auto_at_the_smallest_eligible_shape(pair512, one_lane_512, lanes):
    net = pair512[1]
    rgb, s1, e1 = one_lane_512
    s, e = run(net, rgb)                                     # auto is the default
    assert lanes.last_lanes() == 2
    assert torch.equal(s, s1) and torch.equal(e, e1)
    run(net, rgb[:14])                                       # half a batch is 7168 tokens: 112 z192 tiles, below the 128 that occupy the chip
    assert lanes.last_lanes() == 1


def test_profiling_runs_one_lane(pair512, one_lane_512, lanes):
    net = pair512[1]
    rgb, s1, e1 = one_lane_512
    with kernel_rows(lanes) as read:
        s, e = run(net, rgb)
        assert lanes.last_lanes() == 1
        rows = read()
    assert {"patch_im2col", "gemm_patch_embed", "layernorm", "gemm_qkv", "attn_window", "attn_global", "gemm_proj", "gemm_fc1", "gemm_fc2",
            "gemm_neck", "map_decoder"} <= rows
    assert torch.equal(s, s1) and torch.equal(e, e1)
    run(net, rgb)
    assert lanes.last_lanes() == 2


def test_caller_stream_sees_one_stream(pair512, one_lane_512, lanes):
    """Outputs are ordered on the caller's stream and the input may be overwritten on it right after the call: a reduction of the
    outputs and an in-place overwrite of the input are queued behind the call on a side stream with no synchronisation in between."""
    net = pair512[1]
    rgb, s1, e1 = one_lane_512
    want = (s1.sum(dim=(1, 2, 3)), e1.sum(dim=(1, 2, 3)))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        mine = rgb.clone()
        s, e = net.infer_masks_and_img_features(mine)
        got = (s.sum(dim=(1, 2, 3)), e.sum(dim=(1, 2, 3)))
        mine.fill_(255.0)
    assert lanes.last_lanes() == 2
    side.synchronize()
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    assert torch.equal(s, s1) and torch.equal(e, e1)         # lane 1 read its tiles before the overwrite


@pytest.mark.parametrize("which,P,B,mode", [("image_encoder.blocks.0.mlp.lin2.weight", 512, 16, 0),      # auto: the z192 path, fp16 branch outputs
                                           ("image_encoder.blocks.1.attn.qkv.weight", 128, 2, 2)])     # forced: the generic epilogues
def test_overflow_is_still_reported_with_lanes_on(pair128, pair512, lanes, which, P, B, mode):
    """Weights scaled as in test_gpu_model.py::test_fp16_overflow_is_reported_not_returned_as_masks: both lanes write the same
    set-only flags, and the message still names the block."""
    from sam_road_amd import Config, SAMRoad, _lib
    oracle, good = pair512 if P == 512 else pair128
    sd = {k: v.clone() for k, v in oracle.state_dict().items()}
    sd[which] = sd[which] * 3.0e6
    bad = SAMRoad(Config(dict(CFG, PATCH_SIZE=P)))
    bad.load_state_dict(sd, strict=True)
    bad.eval().to("cuda")
    rgb = synth_tiles(B, P, seed=3).cuda()
    lanes.set_lanes(mode)
    good.check_finite()
    bad.infer_masks_and_img_features(rgb)
    assert lanes.last_lanes() == 2
    with pytest.raises(_lib.SrhError, match=r"status -6.*non-finite.*encoder block 1"):
        bad.check_finite()
    good.check_finite()                                      # reported once, then clear
    s, e = run(good, rgb)
    assert lanes.last_lanes() == 2
    good.check_finite()
    assert torch.isfinite(e).all() and torch.isfinite(s).all()


def test_scene_pass1_with_lanes(pair128, lanes):
    """The scene loop gets lanes through the same call: batches of 4 run two lanes, the last batch of one tile runs one; the canvas adds
    come after the join, in tile order."""
    net = pair128[1]
    scene = torch.from_numpy(synth_scene(256, seed=11)).cuda()
    xy = torch.tensor([[x, y] for y in (0, 64, 128) for x in (0, 64, 128)], dtype=torch.int32).cuda()
    out = {}
    for mode in (1, 2):
        lanes.set_lanes(mode)
        kp, road, emb = net.scene_pass1(scene, xy[:8], 4)
        torch.cuda.synchronize()
        assert lanes.last_lanes() == mode
        kp, road, emb9 = net.scene_pass1(scene, xy, 4, canvas_kp=kp, canvas_road=road)       # 4 + 4 + 1 tiles
        torch.cuda.synchronize()
        assert lanes.last_lanes() == 1
        out[mode] = (kp, road, emb, emb9)
    for a, b in zip(out[1], out[2]):
        assert torch.equal(a, b)
    assert out[1][0].abs().max() > 0


def test_lanes_allocate_nothing(pair128, lanes):
    net = pair128[1]
    rgb = synth_tiles(4, 128, seed=8).cuda()
    lanes.set_lanes(1)
    run(net, rgb)
    before = lanes.lib.srh_ctx_device_bytes(lanes.handle)
    lanes.set_lanes(2)
    run(net, rgb)
    assert lanes.last_lanes() == 2
    assert lanes.lib.srh_ctx_device_bytes(lanes.handle) == before
