"""The units of the command line (sam_road_amd/cli.py) on their own: the run plan without files or a model, the scene records under a
scene-sharded launch, the decode-ahead loader.  The whole runs through main() are in the feature tests (scene_kit.run_cli)."""
import dataclasses
import threading

import pytest
import yaml

from sam_road_amd import Config, cli
from sam_road_amd import inferencer as inf

from scene_kit import HOST_CFG

CFG = dict(HOST_CFG, DATASET="cityscale")


def _resolve(*argv, cfg=CFG, world=1):
    ap = cli.build_parser()
    args = ap.parse_args(list(argv))
    config = Config(cfg)
    return args, config, cli.resolve_run(ap, args, config, world)


def test_valid_masks_count_fails_before_the_model_is_built(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    with open("a.yaml", "w") as f:
        yaml.safe_dump(CFG, f)
    monkeypatch.setattr(cli, "_build_net", lambda *a, **k: (_ for _ in ()).throw(AssertionError("the model was built")))
    base = ["--config", "a.yaml", "--checkpoint", "none", "--device", "cpu", "--output_dir", "e"]
    with pytest.raises(SystemExit):
        inf.main(base + ["--images", "a.png", "b.png", "--valid-masks", "m.png"])
    with pytest.raises(SystemExit):
        inf.main(base + ["--valid-masks", "m.png"])                        # and without --images there is nothing to be parallel to
    assert not (tmp_path / "save").exists()


def test_resolve_run_without_an_extension_flag_changes_nothing():
    args, config, plan = _resolve("--images", "a.png")
    assert dict(config) == CFG
    assert plan.support is None and plan.width is None and plan.raster is None and plan.job_aois is None
    assert plan.tiff is None and plan.tiff_heads == {} and plan.export_gt is None
    assert plan.geojson is False and plan.tiff_masks is False and not plan.post and not plan.keeps_inputs


def test_drop_isolated_nodes_goes_to_the_keys_in_use():
    """--drop-isolated-nodes is shared: alone it is EDGE_SUPPORT's as it always was; next to ROAD_WIDTH it is that key's only, and
    EDGE_SUPPORT's as well once that key is in use too."""
    with pytest.raises(ValueError, match="EDGE_SUPPORT: the key states none of"):      # it landed there, where a key must filter ...
        _resolve("--drop-isolated-nodes")
    _, config, plan = _resolve("--drop-isolated-nodes", "--graph-geojson")              # ... or serve the export's attributes
    assert config["EDGE_SUPPORT"] == {"drop_isolated": True} and "ROAD_WIDTH" not in config
    assert plan.support is not None and plan.support.drop_isolated and plan.width is None and plan.geojson and plan.post
    _, config, plan = _resolve("--drop-isolated-nodes", "--road-width")
    assert "EDGE_SUPPORT" not in config and config["ROAD_WIDTH"]["drop_isolated"] is True
    assert plan.support is None and plan.width is not None and plan.width.drop_isolated
    _, config, plan = _resolve("--drop-isolated-nodes", "--road-width", "--edge-min-on", "0.5")
    assert config["EDGE_SUPPORT"] == {"min_on": 0.5, "drop_isolated": True} and config["ROAD_WIDTH"]["drop_isolated"] is True
    assert plan.support.drop_isolated and plan.width.drop_isolated


def test_scene_records_stay_aligned_under_one_slice():
    images = [f"dir/s{k}.png" for k in range(5)]
    masks = ["m0.png", "-", "m2.npy", "-", "m4.png"]
    gts = ["g0.p", "g1.p", "-", "g3.p", "-"]
    args, config, plan = _resolve("--images", *images, "--valid-masks", *masks, "--diff", "--gt-graphs", *gts)
    aois = [{"include": [k]} if k != 3 else None for k in range(5)]
    plan = dataclasses.replace(plan, job_aois=aois)
    whole = cli.scene_records(args, config, plan)
    assert [(r.img_id, r.path, r.mask_path, r.gt_path, r.aoi) for r in whole] == [
        ("s0", "dir/s0.png", "m0.png", "g0.p", {"include": [0]}), ("s1", "dir/s1.png", None, "g1.p", {"include": [1]}),
        ("s2", "dir/s2.png", "m2.npy", None, {"include": [2]}), ("s3", "dir/s3.png", None, "g3.p", None),
        ("s4", "dir/s4.png", "m4.png", None, {"include": [4]})]
    assert cli.scene_records(args, config, plan, 0, 2) == whole[0::2]
    assert cli.scene_records(args, config, plan, 1, 2) == whole[1::2] == [whole[1], whole[3]]
    args.shard = "tiles"                                                   # a tile-sharded launch: every rank sees every scene
    assert cli.scene_records(args, config, plan, 1, 2) == whole


@pytest.mark.parametrize("keep", (False, True))
def test_loader_hands_out_scenes_in_order_with_their_masks(keep):
    """The first scene finishes decoding LAST (the other two of the first window are done before it returns): the scenes still come out
    in order, and a scene's mask is in the mask iterator at the moment the scene is yielded, which is when infer_imgs reads it."""
    records = [cli.Scene(k, f"s{k}") for k in range(5)]
    done = {1: threading.Event(), 2: threading.Event()}
    order = []

    def load(record):
        k = record.img_id
        if k == 0:
            assert done[1].wait(60) and done[2].wait(60)
        order.append(k)
        if k in done:
            done[k].set()
        return f"img{k}", (f"valid{k}" if k % 2 == 0 else None)

    loader = cli.SceneLoader(records, load, keep=keep)
    valids = loader.valids()
    for k, img in enumerate(loader.scenes()):
        assert img == f"img{k}"
        assert next(valids) == (f"valid{k}" if k % 2 == 0 else None)
        assert (loader.kept.popleft() == (img, f"valid{k}" if k % 2 == 0 else None)) if keep else not loader.kept
    assert k == 4 and order.index(0) == 2 and sorted(order) == list(range(5))
