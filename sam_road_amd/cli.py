"""Drop-in for `python inferencer.py --config ... --checkpoint ... [--output_dir ...] [--device cuda]` (reference
inferencer.py:24-35,239-349), run from a sam_road checkout: enumerates the test split of config.DATASET
(./cityscale/20cities/region_{}_sat.png or ./spacenet/RGB_1.0_meter/{}__rgb.png), runs the scenes through infer_imgs, writes
save/<output_dir>/{config.yaml, mask/{id}_road.png, mask/{id}_itsc.png, graph/{id}.p, inference_time.txt} with the
reference's formats (8-bit grayscale PNG masks, sat2graph pickle, SpaceNet (400 - r, c) flip).  The reference's `viz/` renderings
(inferencer.py:324-329) and the pred-against-gt comparison it carries commented out (inferencer.py:283-322) are opt-in here and are
NOT cv2's bytes: `--viz` writes viz/{id}.png, `--graph-mask RHO` graph_mask/{id}.png, `--diff [THIN WIDE]` diff/{id}.png and
diff/metrics.json (per-scene counts, relaxed pixel precision and recall, and the totals) against the ground-truth graphs —
the dataset's own sat2graph pickles, or `--gt-graphs g0.p g1.p ...` parallel to `--images` ('-' = none for that scene).  They lay
over the config's GRAPH_RASTER; the rule is sam_road_amd/graph_raster.py's, rasterised on the device on a stream of its own, encoded
on the writer threads.  Without them the run writes the files and bytes it always wrote.
`--edge-min-mean M`, `--edge-min-on F`, `--edge-max-invalid K` (with `--edge-support-width T`, `--edge-on T`, `--drop-isolated-nodes`)
lay over the config's EDGE_SUPPORT (sam_road_amd/edge_support.py): the road mask under every edge is counted on the device and the
edges it does not support are dropped before the pickle, the renders and diff/metrics.json are written; `--graph-geojson` writes
graph_geojson/{id}.geojson, one LineString per edge with its evidence as properties, through `--geotransform G0 .. G5` into map
coordinates.  Without them nothing of this runs.
`--road-width` (with `--road-width-radius R`, `--road-width-on T`, `--road-min-width W`, `--road-max-width W`, `--road-min-in F`,
`--drop-isolated-nodes`) lay over the config's ROAD_WIDTH (sam_road_amd/road_width.py): an exact distance map of the thresholded road
mask is built on the device and every edge gets its road width from it along its centre line; edges outside the stated widths are
dropped, behind EDGE_SUPPORT's filter and before the files are written, and the GeoJSON's features carry the width attributes.
`--graph-min-spur S`, `--graph-min-component C`, `--graph-clean-rounds R`, `--graph-polylines` (with `--drop-isolated-nodes`) lay over
the config's GRAPH_CLEAN (sam_road_amd/graph_clean.py): dead-end spurs shorter than S px and connected components shorter than C px are
dropped on the device, behind the two filters above and before the files are written; every kept edge gets its chain (road segment) and
component with their lengths, and `--graph-polylines` writes graph_polylines/{id}.geojson, one LineString per chain.
Extras: `--images a.png b.npy ...` runs explicit scene files instead of the dataset split; under torchrun
(one process per GPU) the scenes are dealt round-robin to the ranks (`--shard scenes`, default) or every scene's tiles are split
over the ranks (`--shard tiles`; `tiles-pipelined` for the software-pipelined loop), all ranks writing into the one output directory.
`--valid-masks m0.png m1.npy ...` (parallel to `--images`; `-` = no mask for that scene) gives every scene a validity mask
(infer_one_img's `valid`); without it an RGBA `--images` file uses its alpha > 0.  Output formats do not change.

The units: build_parser(); resolve_run(), which lays the flags over the config and validates every key without a model, a device or a
directory; scene_records(); SceneLoader, the decode-ahead loader; SceneWriter, the files of a scene; main(), which strings them together
around inferencer.infer_imgs (inferencer.main delegates here).  The pipeline module is read through `scene`, so a replaced
inferencer.infer_imgs / *_data_partition takes effect here; every other collaborator (_build_net, the feature modules' functions) is a
global of THIS module, and this is where a test replaces it."""
import argparse
import collections
import contextlib
import dataclasses
import json
import os
import pickle
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch
from PIL import Image

from . import distributed as D
from . import inferencer as scene
from .aoi import aoi_key_of, read_geojson, scene_aoi_key, scene_aoi_override
from .config import load_config
from .edge_support import apply as apply_edge_support, edge_support_key, edge_support_override, write_geojson
from .float_scene import scene_float_override
from .formats import convert_to_sat2graph_format
from .geotiff import TiffScene, geotiff_key, geotiff_override, is_tiff_path, open_scene, write_geotiff
from .graph_raster import graph_raster_key, graph_raster_override, read_gt_graph, render as render_graph, total_metrics
from .hostcpu import fill_threads, usable_cpus
from .mask_clean import mask_clean_override
from .nodata import scene_nodata_key, scene_nodata_override
from .radiometry import scene_bands_key, scene_bands_override
from .resample import scene_scale_key, scene_scale_override
from .graph_clean import apply as apply_graph_clean, graph_clean_key, graph_clean_override, table_of as clean_table_of, write_polylines
from .road_width import apply as apply_road_width, road_width_key, road_width_override


def _nodata_from_files(heads):
    """GEOTIFF nodata: file — the ONE nodata value (tag 42113) the run's GeoTIFF scenes state, as (value, whether the files are float):
    an int for integer files.  ValueError for a run without such scenes, a file without the tag, two files that differ (both are named),
    integer and float files side by side, or a value an integer file cannot hold."""
    if not heads:
        raise ValueError("GEOTIFF: nodata 'file' (--nodata-from-file) needs --images with .tif / .tiff scenes")
    items = list(heads.items())
    p0, h0 = items[0]
    same = lambda a, b: a == b or (a != a and b != b)
    for p, h in items:
        if h.nodata is None:
            raise ValueError(f"{p}: the file states no nodata value (tag 42113), which GEOTIFF nodata 'file' (--nodata-from-file) asks for")
        if not same(h.nodata, h0.nodata):
            raise ValueError(f"GEOTIFF: nodata 'file': {p0} states {h0.nodata!r} and {p} states {h.nodata!r}; all scenes of a run must state one value")
        if (h.dtype.kind == "f") != (h0.dtype.kind == "f"):
            raise ValueError(f"GEOTIFF: nodata 'file': {p0} is {h0.dtype} and {p} is {h.dtype}; run integer and float scenes apart")
    if h0.dtype.kind == "f":
        return float(h0.nodata), True
    if h0.nodata != int(h0.nodata) or not 0 <= h0.nodata < 2 ** (8 * h0.dtype.itemsize):
        raise ValueError(f"{p0}: the nodata value {h0.nodata!r} (tag 42113) is no level of a {h0.dtype} scene")
    return int(h0.nodata), False


def create_output_dir_and_save_config(output_dir_prefix, config, specified_dir=None):
    """utils.py:11-29."""
    import yaml
    from datetime import datetime
    out = specified_dir if specified_dir else f"{output_dir_prefix}_{datetime.now().strftime('%Y%m%d_%H%M%S')}"
    os.makedirs(out, exist_ok=True)
    with open(os.path.join(out, "config.yaml"), "w") as f:
        yaml.dump(config.to_dict(), f)
    return out


def _build_net(config, checkpoint, device):
    """inferencer.py:246-254.  Under torchrun only rank 0 reads the checkpoint: it packs the weights once and the packed arena
    is broadcast device-to-device over RCCL (SAMRoad.share_packed_weights); the other ranks never touch the file."""
    from .model import SAMRoad
    net = SAMRoad(config)
    shared = D.is_distributed() and device.type == "cuda"
    if not shared or torch.distributed.get_rank() == 0:
        ckpt = torch.load(checkpoint, map_location="cpu")
        print(f"##### Loading Trained CKPT {checkpoint} #####")
        net.load_state_dict(ckpt["state_dict"], strict=True)
    net.eval()
    net.to(device)
    if shared:
        net.share_packed_weights(src=0)
    return net


def build_parser():
    ap = argparse.ArgumentParser()
    ap.add_argument("--checkpoint", default=None, help="checkpoint of the model to test.")
    ap.add_argument("--config", default=None, help="model config.")
    ap.add_argument("--output_dir", default=None, help="Name of the output dir, if not specified will use timestamp")
    ap.add_argument("--device", default="cuda", help="device to use (an MI355X: there is no CPU path)")
    ap.add_argument("--images", nargs="*", default=None, help="(extension) explicit scene images instead of the dataset split")
    ap.add_argument("--valid-masks", nargs="*", default=None, metavar="MASK",
                    help="(extension) one validity mask per --images entry (.npy bool / uint8 [H,W], or an image: non-zero = valid; "
                         "'-' = none): nodata tiles are skipped and nothing is predicted on nodata.  Default: alpha > 0 of an RGBA image")
    ap.add_argument("--shard", choices=("scenes", "tiles", "tiles-pipelined"), default="scenes",
                    help="(extension, multi-GPU runs under torchrun) scenes: every rank takes whole scenes, no data-path collective "
                         "(throughput); tiles: the tiles of every scene are split over the ranks, scene by scene (latency of one scene); "
                         "tiles-pipelined: the same with scene i+1's pass 1 queued before scene i's host stages (opt-in: exercised on gloo only)")
    ap.add_argument("--fuse-window", default=None, metavar="NAME", choices=scene.FUSE_WINDOW_NAMES,
                    help="(extension) how overlapping tiles are fused, overriding the config's FUSE_WINDOW: uniform (the reference's mean), "
                         "hann or triangle (centre-weighted: tile borders count less)")
    ap.add_argument("--tta", default=None, metavar="NAMES",
                    help="(extension) test-time augmentation, overriding the config's TTA: orientation names separated by commas, the first "
                         "one id (id,flip_h,flip_v,rot180,transpose,rot90,rot270,anti_transpose); every tile is run once per name and "
                         "the masks are averaged")
    ap.add_argument("--scene-pad", default=None, type=int, metavar="B",
                    help="(extension) pad every scene by B >= 0 pixels on all four sides on the device before it is tiled, overriding the "
                         "border of the config's SCENE_PAD; the masks and the graph are those of the unpadded scene.  With the key (any B) "
                         "a scene smaller than a tile is padded up to one instead of being refused")
    ap.add_argument("--scene-pad-mode", default=None, metavar="MODE", choices=scene.SCENE_PAD_MODES,
                    help="(extension) how the padding is filled, overriding the mode of the config's SCENE_PAD: reflect (default), edge "
                         "or constant (the colour NODATA_FILL)")
    ap.add_argument("--scene-scale", default=None, nargs=2, type=int, metavar=("P", "Q"),
                    help="(extension) the scenes' ground resolution as the fraction P/Q, model pixels per scene pixel (a 0.5 m/px scene for a "
                         "1 m/px model: 1 2), overriding the config's SCENE_SCALE: the scene is resampled on the device in front of pass 1, the "
                         "masks and the graph come back in the scene's own pixels.  1 <= P, Q <= 16, 1/8 <= P/Q <= 4; not with --scene-group")
    ap.add_argument("--scene-gsd", default=None, type=float, metavar="A",
                    help="(extension) the same as metres per scene pixel: the scale is A / B with --model-gsd B, which must be such a fraction")
    ap.add_argument("--model-gsd", default=None, type=float, metavar="B", help="(extension) metres per pixel the model was trained at (default 1.0)")
    ap.add_argument("--mask-min-area", default=None, nargs="+", type=int, metavar="N",
                    help="(extension) ROAD [KEYPOINT]: drop the connected components of the thresholded road (keypoint) mask that have fewer than "
                         "N pixels before the graph points are extracted, on the device, overriding min_area of the config's MASK_CLEAN")
    ap.add_argument("--mask-min-peak", default=None, nargs="+", type=float, metavar="P",
                    help="(extension) ROAD [KEYPOINT]: drop the components whose highest score is not above P (in [0, 1)), overriding min_peak "
                         "of the config's MASK_CLEAN")
    ap.add_argument("--mask-connectivity", default=None, type=int, metavar="N",
                    help="(extension) 8 (default) or 4: which neighbours connect two mask pixels, overriding connectivity of the config's MASK_CLEAN")
    ap.add_argument("--scene-group", default=None, type=int, metavar="N",
                    help="(extension) run up to N consecutive scenes as one — one upload, one pass 1 over all their tiles in full batches, "
                         "one TopoNet launch sequence — overriding the config's SCENE_GROUP; for streams of small scenes (chips).  1: scene "
                         "by scene.  Not with --shard tiles / tiles-pipelined")
    ap.add_argument("--bands", default=None, metavar="I,J,K",
                    help="(extension) the three bands of a multi-band scene (.npy, uint8 / uint16 [H,W,C]) that become R, G, B, overriding "
                         "select of the config's SCENE_BANDS; repeats allowed (0,0,0: a panchromatic scene as grey)")
    ap.add_argument("--stretch-range", default=None, nargs=2, type=int, metavar=("LO", "HI"),
                    help="(extension) the input levels that map to 0 and 255, overriding stretch of the config's SCENE_BANDS")
    ap.add_argument("--stretch-percentile", default=None, nargs=2, type=float, metavar=("PLO", "PHI"),
                    help="(extension) stretch every selected band between these two percentiles of its valid pixels, per scene "
                         "(numpy.percentile, method lower), overriding stretch of the config's SCENE_BANDS; not with --scene-group")
    ap.add_argument("--gamma", default=None, type=float, metavar="G",
                    help="(extension) gamma of the stretch (out = 255 t^(1/G)), overriding gamma of the config's SCENE_BANDS")
    ap.add_argument("--float-bands", default=None, metavar="I,J,K",
                    help="(extension) the three bands of a float32 scene (.npy, float32 [H,W,C]) that become R, G, B, overriding select of the "
                         "config's SCENE_FLOAT; repeats allowed")
    ap.add_argument("--float-range", default=None, nargs=2, type=float, metavar=("LO", "HI"),
                    help="(extension) the values that map to 0 and 255, overriding stretch of the config's SCENE_FLOAT")
    ap.add_argument("--float-percentile", default=None, nargs=2, type=float, metavar=("PLO", "PHI"),
                    help="(extension) stretch every selected band between these two percentiles of its valid pixels, per scene (the value at "
                         "sorted index floor(p / 100 (N - 1))), overriding stretch of the config's SCENE_FLOAT")
    ap.add_argument("--float-gamma", default=None, type=float, metavar="G",
                    help="(extension) gamma of the stretch (out = 255 t^(1/G)), overriding gamma of the config's SCENE_FLOAT")
    ap.add_argument("--float-transfer", default=None, choices=("linear", "log"),
                    help="(extension) linear (default) or log (a stretch of log x; x <= 0 is nodata), overriding transfer of the config's SCENE_FLOAT")
    ap.add_argument("--float-nodata", default=None, nargs="+", type=float, metavar="V",
                    help="(extension) up to 4 values that mark nodata in a float32 scene (NaN and +-inf always do), overriding nodata of the "
                         "config's SCENE_FLOAT; not with --scene-group")
    ap.add_argument("--nodata", default=None, nargs="+", type=int, metavar="V",
                    help="(extension) the nodata level of the raw scene, one for every band or one per band, overriding value of the config's "
                         "SCENE_NODATA: the validity mask is derived from it on the device (and ANDed with --valid-masks / alpha)")
    ap.add_argument("--nodata-tolerance", default=None, type=int, metavar="T",
                    help="(extension) a band hits within T levels of the value, overriding tolerance of the config's SCENE_NODATA")
    ap.add_argument("--nodata-match", default=None, choices=("all", "any"),
                    help="(extension) all (default): every band must hit; any: one is enough — overriding match of the config's SCENE_NODATA")
    ap.add_argument("--nodata-min-area", default=None, type=int, metavar="A",
                    help="(extension) a connected set of fewer than A hit pixels is not nodata, overriding min_area of the config's SCENE_NODATA")
    ap.add_argument("--nodata-grow", default=None, type=int, metavar="R",
                    help="(extension) grow nodata by R pixels (0..16), overriding grow of the config's SCENE_NODATA")
    ap.add_argument("--aoi", default=None, nargs="+", metavar="FILE",
                    help="(extension) the area of interest as GeoJSON (Polygon, MultiPolygon, Feature, FeatureCollection, GeometryCollection), [x, y] "
                         "pixel coordinates unless --aoi-geotransform is given: one file for every scene, or one per --images entry ('-' for a scene "
                         "without one), overriding include of the config's SCENE_AOI; rasterised on the device and ANDed with the other masks")
    ap.add_argument("--aoi-exclude", default=None, nargs="+", metavar="FILE",
                    help="(extension) GeoJSON files whose polygons are cut out of every scene's area, overriding exclude of the config's SCENE_AOI")
    ap.add_argument("--aoi-geotransform", default=None, nargs=6, type=float, metavar="G",
                    help="(extension) the six numbers that map (col, row) to the polygons' map coordinates: X = G0 + col G1 + row G2, Y = G3 + col G4 + "
                         "row G5, overriding geotransform of the config's SCENE_AOI")
    ap.add_argument("--aoi-buffer", default=None, type=int, metavar="B",
                    help="(extension) grow (B > 0) or shrink (B < 0) the area by |B| pixels (-16..16), overriding buffer of the config's SCENE_AOI")
    ap.add_argument("--viz", action="store_true", default=None,
                    help="(extension) write viz/{id}.png, the graph drawn over the scene (the reference's viz/, by the exact rule of "
                         "GRAPH_RASTER, not cv2's bytes), switching on viz of the config's GRAPH_RASTER")
    ap.add_argument("--graph-mask", default=None, type=int, metavar="RHO",
                    help="(extension) write graph_mask/{id}.png, the graph as a 0 / 255 mask: edges of width 2 RHO, nodes as squares of half-side "
                         "RHO (the reference's rasterize_graph), overriding mask of the config's GRAPH_RASTER")
    ap.add_argument("--diff", default=None, nargs="*", type=int, metavar="N",
                    help="(extension) [THIN WIDE] (default 1 5): write diff/{id}.png (false positives blue, missed ground truth red) and "
                         "diff/metrics.json (n_pred, n_fp, n_gt, n_missed, precision, recall per scene and in total) against the ground-truth "
                         "graphs, overriding diff of the config's GRAPH_RASTER")
    ap.add_argument("--gt-graphs", default=None, nargs="*", metavar="FILE",
                    help="(extension) one sat2graph pickle per --images entry ('-' = none) for --diff; without --images the dataset's own")
    ap.add_argument("--edge-support-width", default=None, type=int, metavar="T",
                    help="(extension) the width 1..255 of the line under which an edge's road-mask evidence is counted (default 1: the "
                         "8-connected centre line), overriding width of the config's EDGE_SUPPORT")
    ap.add_argument("--edge-on", default=None, type=float, metavar="T",
                    help="(extension) a pixel of the road mask is 'on' above floor(T * 255) (default ROAD_THRESHOLD), overriding on of the config's EDGE_SUPPORT")
    ap.add_argument("--edge-min-mean", default=None, type=float, metavar="M",
                    help="(extension) drop the edges whose mean road-mask value under the line is not above M (0..1), overriding min_mean of the "
                         "config's EDGE_SUPPORT; the pickle, the renders, diff/metrics.json and the GeoJSON show the filtered graph")
    ap.add_argument("--edge-min-on", default=None, type=float, metavar="F",
                    help="(extension) drop the edges with less than the fraction F (0..1) of their pixels 'on', overriding min_on of the config's EDGE_SUPPORT")
    ap.add_argument("--edge-max-invalid", default=None, type=int, metavar="K",
                    help="(extension) drop the edges with more than K pixels on nodata or outside the area of interest (the scene's validity mask), "
                         "overriding max_invalid of the config's EDGE_SUPPORT")
    ap.add_argument("--drop-isolated-nodes", action="store_true", default=None,
                    help="(extension) after the edge filter, drop the nodes without an edge (drop_isolated of the config's EDGE_SUPPORT)")
    ap.add_argument("--road-width", action="store_true", default=None,
                    help="(extension) measure the road width under every edge from an exact distance map of the thresholded road mask "
                         "(ROAD_WIDTH with its defaults; --graph-geojson writes the widths as properties)")
    ap.add_argument("--road-width-radius", default=None, type=int, metavar="R",
                    help="(extension) distances are exact up to R px (1..254, default 32) and capped there, overriding max_radius of the config's ROAD_WIDTH")
    ap.add_argument("--road-width-on", default=None, type=float, metavar="T",
                    help="(extension) a pixel is road above floor(T * 255) (default ROAD_THRESHOLD), overriding on of the config's ROAD_WIDTH")
    ap.add_argument("--road-min-width", default=None, type=float, metavar="W",
                    help="(extension) drop the edges whose mean road width is below W px, overriding min_width of the config's ROAD_WIDTH")
    ap.add_argument("--road-max-width", default=None, type=float, metavar="W",
                    help="(extension) drop the edges whose mean road width is above W px, overriding max_width of the config's ROAD_WIDTH")
    ap.add_argument("--road-min-in", default=None, type=float, metavar="F",
                    help="(extension) drop the edges with less than the fraction F (0..1) of their centre line on the road, overriding min_in of "
                         "the config's ROAD_WIDTH")
    ap.add_argument("--graph-min-spur", default=None, type=float, metavar="S",
                    help="(extension) drop the dead-end chains (one end of degree 1, one at a junction) shorter than S px, overriding min_spur of "
                         "the config's GRAPH_CLEAN")
    ap.add_argument("--graph-min-component", default=None, type=float, metavar="C",
                    help="(extension) drop the connected components whose edges add up to less than C px, overriding min_component of the config's GRAPH_CLEAN")
    ap.add_argument("--graph-clean-rounds", default=None, type=int, metavar="R",
                    help="(extension) apply the two tests R times (1..8, default 1), each time on what the round before left, overriding rounds of "
                         "the config's GRAPH_CLEAN")
    ap.add_argument("--graph-polylines", action="store_true", default=None,
                    help="(extension) write graph_polylines/{id}.geojson: one LineString per chain of the graph (a road segment between junctions "
                         "or dead ends), with --geotransform as --graph-geojson; alone it turns on a GRAPH_CLEAN that filters nothing")
    ap.add_argument("--graph-geojson", action="store_true", default=None,
                    help="(extension) write graph_geojson/{id}.geojson: one LineString per edge, [x, y] = [col + 1/2, row + 1/2], with the "
                         "edge's attributes of EDGE_SUPPORT as properties where the key is given")
    ap.add_argument("--geotransform", default=None, nargs=6, type=float, metavar="G",
                    help="(extension) G0 .. G5 of the GeoJSON export: X = G0 + x G1 + y G2, Y = G3 + x G4 + y G5 (the forward of --aoi-geotransform, "
                         "whose value it takes when only that one is given)")
    ap.add_argument("--geotiff", action="store_true", default=None,
                    help="(extension) read .tif / .tiff scenes as GeoTIFFs (GEOTIFF with its defaults): strips or tiles, 1..16 bands of uint8 / uint16 / "
                         "float32, LZW or deflate, predictors, both byte orders, BigTIFF; decompressed on host threads, assembled on the device.  The "
                         "scene's own geotransform becomes the default of --geotransform and --aoi-geotransform")
    ap.add_argument("--nodata-from-file", action="store_true", default=None,
                    help="(extension) take the files' nodata value (tag 42113) as the value of SCENE_NODATA, or as nodata of SCENE_FLOAT for float "
                         "files (nodata: file of the config's GEOTIFF); every scene of the run must state the same value")
    ap.add_argument("--mask-geotiff", action="store_true", default=None,
                    help="(extension) also write mask_tif/{id}_road.tif and mask_tif/{id}_itsc.tif with the scene's geo tags (masks of the config's GEOTIFF)")
    return ap


@dataclasses.dataclass(frozen=True)
class RunPlan:
    """What resolve_run leaves for the steps behind it; the config carries the rest."""
    tiff: object                    # the GEOTIFF key, or None
    tiff_heads: dict                # path -> header of the --images that are read as GeoTIFFs
    support: object                 # the EDGE_SUPPORT key, or None
    width: object                   # the ROAD_WIDTH key, or None
    clean: object                   # the GRAPH_CLEAN key, or None
    raster: object                  # the GRAPH_RASTER key, or None
    export_gt: object               # the geotransform of the GeoJSON export that was given, or None
    job_aois: object                # one SCENE_AOI value per --images entry where the scenes have their own, or None
    geojson: bool                   # graph_geojson/ is written
    polylines: bool                 # graph_polylines/ is written
    tiff_masks: bool                # mask_tif/ is written
    spacenet_gt: bool               # the ground-truth graphs are the SpaceNet dataset's own (flipped rows)

    @property
    def post(self):
        """A step between a scene's result and its files."""
        return self.support is not None or self.width is not None or self.clean is not None or self.geojson

    @property
    def keeps_inputs(self):
        """The writers read the scene and its mask again."""
        return self.raster is not None or self.post or self.tiff_masks

    def as_tiff(self, path):
        """GEOTIFF: such a scene's bands are bands, none is an alpha."""
        return self.tiff is not None and is_tiff_path(path)


def _one_per_image(ap, entries, images, message):
    if entries is not None and (images is None or len(entries) != len(images)):
        ap.error(message)


def resolve_run(ap, args, config, world=1):
    """Lays the flags over the config (which is mutated: the saved config.yaml shows the overrides) and validates every key, in a fixed
    order.  No model, no device, no directory, no process group: a key that cannot be used fails here, before any of them exists."""
    if args.geotiff or args.nodata_from_file or args.mask_geotiff:
        config.GEOTIFF = geotiff_override(config, args.geotiff, args.nodata_from_file, args.mask_geotiff)
    tiff = geotiff_key(config)                   # a GEOTIFF that cannot be used fails here, and so does a file that cannot be read:
    tiff_heads = {p: open_scene(p) for p in (args.images or []) if is_tiff_path(p)} if tiff is not None else {}      # headers only
    road_flags = (args.road_width, args.road_width_on, args.road_width_radius, args.road_min_width, args.road_max_width, args.road_min_in)
    road_on = any(v is not None for v in road_flags) or bool(config.get("ROAD_WIDTH"))
    edge_flags = (args.edge_support_width, args.edge_on, args.edge_min_mean, args.edge_min_on, args.edge_max_invalid)
    clean_flags = (args.graph_polylines, args.graph_min_spur, args.graph_min_component, args.graph_clean_rounds)
    clean_on = any(v is not None for v in clean_flags) or bool(config.get("GRAPH_CLEAN"))
    # --drop-isolated-nodes is shared: it goes to every key that is in use, and to EDGE_SUPPORT as before where neither ROAD_WIDTH nor
    # GRAPH_CLEAN is
    edge_drop = args.drop_isolated_nodes if any(v is not None for v in edge_flags) or config.get("EDGE_SUPPORT") or not (road_on or clean_on) else None
    if any(v is not None for v in edge_flags + (edge_drop,)):
        config.EDGE_SUPPORT = edge_support_override(config, args.edge_support_width, args.edge_on, args.edge_min_mean, args.edge_min_on,
                                                    args.edge_max_invalid, edge_drop, attributes_only=bool(args.graph_geojson))
    support = edge_support_key(config, attributes_only=bool(args.graph_geojson))      # an EDGE_SUPPORT that cannot be used fails here
    if any(v is not None for v in road_flags):
        config.ROAD_WIDTH = road_width_override(config, *road_flags, drop_isolated=args.drop_isolated_nodes)
    width = road_width_key(config)               # and a ROAD_WIDTH
    if any(v is not None for v in clean_flags):
        config.GRAPH_CLEAN = graph_clean_override(config, *clean_flags, drop_isolated=args.drop_isolated_nodes)
    clean = graph_clean_key(config)              # and a GRAPH_CLEAN
    export_gt = args.geotransform if args.geotransform is not None else args.aoi_geotransform
    if args.viz or args.graph_mask is not None or args.diff is not None:
        config.GRAPH_RASTER = graph_raster_override(config, args.viz, args.graph_mask, True if args.diff == [] else args.diff)
    raster = graph_raster_key(config)            # and a GRAPH_RASTER
    _one_per_image(ap, args.gt_graphs, args.images, "--gt-graphs takes exactly one entry per --images entry ('-' for a scene without a ground-truth graph)")
    if raster is not None and raster.diff is not None and args.images is not None and args.gt_graphs is None:
        raise ValueError("GRAPH_RASTER: diff needs ground-truth graphs: pass --gt-graphs with --images")
    job_aois = None
    if any(v is not None for v in (args.aoi, args.aoi_exclude, args.aoi_geotransform, args.aoi_buffer)):
        own_aois = args.aoi is not None and len(args.aoi) > 1        # a scene's own file takes the place of include for that scene
        _one_per_image(ap, args.aoi if own_aois else None, args.images,
                       "--aoi takes one file for all scenes or exactly one entry per --images entry ('-' for a scene without one)")
        exclude = None if args.aoi_exclude is None else [poly for path in args.aoi_exclude for poly in read_geojson(path)]
        shared = read_geojson(args.aoi[0]) if args.aoi is not None and len(args.aoi) == 1 and args.aoi[0] != "-" else None
        config.SCENE_AOI = scene_aoi_override(config, shared, exclude, args.aoi_geotransform, args.aoi_buffer)
        if own_aois:
            job_aois = [None if path == "-" else scene_aoi_override(config, read_geojson(path)) for path in args.aoi]
            for a in job_aois:
                aoi_key_of(a)
    if tiff is not None and tiff.georef and tiff_heads and config.get("SCENE_AOI"):
        # GEOTIFF: a scene's own geotransform is the default of the area of interest's, scene by scene; one that is given wins
        base = config.SCENE_AOI if isinstance(config.SCENE_AOI, dict) else {"include": list(config.SCENE_AOI)}
        if "geotransform" not in base:
            mine = lambda k: job_aois[k] if job_aois is not None and job_aois[k] is not None else base
            own = [dict(mine(k), geotransform=list(tiff_heads[p].geotransform)) if p in tiff_heads and tiff_heads[p].geotransform is not None else mine(k)
                   for k, p in enumerate(args.images)]
            stated = [a["geotransform"] for a in own if "geotransform" in a]
            if stated:                       # every scene brings its own key; the config's (saved with the run) says the first scene's transform
                for a in own:
                    aoi_key_of(a)
                job_aois, config.SCENE_AOI = own, dict(base, geotransform=stated[0])
    if tiff is not None and tiff.nodata == "file":
        value, is_float = _nodata_from_files(tiff_heads)
        if is_float and value == value:      # NaN is nodata under SCENE_FLOAT whatever the key says
            config.SCENE_FLOAT = scene_float_override(config, nodata=[value])
        elif not is_float:
            config.SCENE_NODATA = scene_nodata_override(config, [value])
    if any(v is not None for v in (args.nodata, args.nodata_tolerance, args.nodata_match, args.nodata_min_area, args.nodata_grow)):
        config.SCENE_NODATA = scene_nodata_override(config, args.nodata, args.nodata_tolerance, args.nodata_match, args.nodata_min_area, args.nodata_grow)
    if args.bands is not None or args.stretch_range is not None or args.stretch_percentile is not None or args.gamma is not None:
        config.SCENE_BANDS = scene_bands_override(config, None if args.bands is None else [int(b) for b in args.bands.split(",")],
                                                  args.stretch_range, args.stretch_percentile, args.gamma)
    if any(v is not None for v in (args.float_bands, args.float_range, args.float_percentile, args.float_gamma, args.float_transfer, args.float_nodata)):
        config.SCENE_FLOAT = scene_float_override(config, None if args.float_bands is None else [int(b) for b in args.float_bands.split(",")],
                                                  args.float_range, args.float_percentile, args.float_gamma, args.float_transfer, args.float_nodata)
    if args.scene_group is not None:
        config.SCENE_GROUP = args.scene_group
    if args.scene_scale is not None or args.scene_gsd is not None or args.model_gsd is not None:
        config.SCENE_SCALE = scene_scale_override(config, args.scene_scale, args.scene_gsd, args.model_gsd)
    if args.mask_min_area is not None or args.mask_min_peak is not None or args.mask_connectivity is not None:
        config.MASK_CLEAN = mask_clean_override(config, args.mask_min_area, args.mask_min_peak, args.mask_connectivity)
    if args.scene_pad is not None or args.scene_pad_mode is not None:
        config.SCENE_PAD = scene.scene_pad_override(config, args.scene_pad, args.scene_pad_mode)
    if args.fuse_window is not None:
        config.FUSE_WINDOW = args.fuse_window
    if args.tta is not None:
        config.TTA = [t.strip() for t in args.tta.split(",")]
    scene.neighbor_queries(config)               # a K the TopoNet trunk cannot run fails here, not after the first scene's pass 1
    scene.fuse_window(config)                    # and so does a FUSE_WINDOW that cannot be used
    scene.tta_plan(config)                       # and a TTA list that cannot be run
    scene.scene_pad_plan((1, 1), config)         # and a SCENE_PAD (or the NODATA_FILL it uses) that cannot be used
    bands = scene_bands_key(config)              # and a SCENE_BANDS that cannot be used
    scene_scale_key(config)                      # and a SCENE_SCALE that cannot be used (or that meets a SCENE_GROUP)
    scene.mask_clean_plan(config)                # and a MASK_CLEAN that cannot be used
    nodata = scene_nodata_key(config)            # and a SCENE_NODATA that cannot be used
    if scene.scene_float_plan(config) is not None and scene.scene_group_key(config) > 1:                                        # and a SCENE_FLOAT
        raise ValueError("SCENE_FLOAT does not combine with SCENE_GROUP (float scenes run one by one)")
    if (scene_aoi_key(config) is not None or job_aois is not None) and scene.scene_group_key(config) > 1:                       # and a SCENE_AOI
        raise ValueError("SCENE_AOI does not combine with SCENE_GROUP (the polygons are in the pixel frame of ONE scene)")
    if nodata is not None and nodata.min_area > 1 and scene.scene_group_key(config) > scene.MASK_CLEAN_MAX_IMAGES:
        raise ValueError(f"SCENE_NODATA: min_area does not combine with a SCENE_GROUP above {scene.MASK_CLEAN_MAX_IMAGES}")
    if bands is not None and bands.percentile is not None and scene.scene_group_key(config) > 1:
        raise ValueError("SCENE_BANDS: a percentile stretch does not combine with SCENE_GROUP (every scene needs its own tables); use a fixed range")
    if scene.scene_group_key(config) > 1 and args.shard != "scenes" and world > 1:                                              # and a SCENE_GROUP
        raise ValueError("SCENE_GROUP applies to --shard scenes (every rank runs whole scenes); a tile-sharded mode runs its scenes one by one")
    _one_per_image(ap, args.valid_masks, args.images, "--valid-masks takes exactly one entry per --images entry ('-' for a scene without a mask)")
    return RunPlan(tiff=tiff, tiff_heads=tiff_heads, support=support, width=width, clean=clean, raster=raster, export_gt=export_gt, job_aois=job_aois,
                   geojson=bool(args.graph_geojson), polylines=bool(args.graph_polylines), tiff_masks=bool(tiff is not None and tiff.masks),
                   spacenet_gt=args.images is None and config.DATASET == "spacenet")


@dataclasses.dataclass(frozen=True)
class Scene:
    """One scene of the run: its id, its file, and the files and the key that go with it (None: it has none)."""
    img_id: object
    path: str
    mask_path: object = None
    gt_path: object = None          # the ground-truth graph, for GRAPH_RASTER's diff
    aoi: object = None


def scene_records(args, config, plan, rank=0, world=1):
    """The scenes of the run — --images, or the test split of config.DATASET — and under `--shard scenes` this rank's share of them:
    independent scenes, dealt round-robin over the ranks, nothing to exchange."""
    if args.images is not None:
        jobs = [(os.path.splitext(os.path.basename(p))[0], p) for p in args.images]
    elif config.DATASET == "cityscale":
        _, _, test_img_indices = scene.cityscale_data_partition()
        jobs = [(i, "./cityscale/20cities/region_{}_sat.png".format(i)) for i in test_img_indices]
    elif config.DATASET == "spacenet":
        _, _, test_img_indices = scene.spacenet_data_partition()
        jobs = [(i, "./spacenet/RGB_1.0_meter/{}__rgb.png".format(i)) for i in test_img_indices]
    else:
        raise ValueError(f"config.DATASET must be 'cityscale' or 'spacenet' (got {config.DATASET!r}), or pass --images")
    masks = [None if m == "-" else m for m in args.valid_masks] if args.valid_masks is not None else [None] * len(jobs)
    gts = [None] * len(jobs)
    if plan.raster is not None and plan.raster.diff is not None:
        if args.images is not None:
            gts = [None if g == "-" else g for g in args.gt_graphs]
        else:                                    # the reference's gt_graph_pattern (inferencer.py:259,263)
            pat = "cityscale/20cities/region_{}_graph_gt.pickle" if config.DATASET == "cityscale" else "./spacenet/RGB_1.0_meter/{}__gt_graph.p"
            gts = [pat.format(i) for i, _ in jobs]
    aois = plan.job_aois if plan.job_aois is not None else [None] * len(jobs)
    records = [Scene(i, p, m, g, a) for (i, p), m, g, a in zip(jobs, masks, gts, aois)]
    return records[rank::world] if world > 1 and args.shard == "scenes" else records


def load_scene(record, plan, use_alpha):
    """(scene, validity mask or None) of one record, as infer_imgs takes them."""
    path = record.path
    if plan.as_tiff(path):                       # header, then the segments decompressed on host threads: the pixels are assembled on the device
        img = open_scene(path).load(fill_threads())
    else:
        img = np.load(path) if str(path).endswith(".npy") else scene.read_rgb_img(path)
    if record.mask_path is not None:
        return img, scene.read_valid_mask(record.mask_path)
    return img, (scene.read_alpha_valid(path) if use_alpha and not plan.as_tiff(path) else None)


class SceneLoader:
    """Decodes ahead on worker threads: a 2048^2 RGB PNG takes ~100 ms to decode, more than the GPU needs for the scene.  scenes() and
    valids() are the two iterators infer_imgs reads, a scene, then its mask; with `keep`, kept holds (scene, mask) of every scene handed
    out, in the same order, until the writers take them."""

    def __init__(self, records, load, keep=False, depth=3):
        self.records, self.load, self.keep, self.depth = records, load, keep, depth
        self._valids = collections.deque()
        self.kept = collections.deque()

    def scenes(self):
        n = len(self.records)
        with ThreadPoolExecutor(self.depth) as ex:
            futs = {}
            for j in range(n):
                for k in range(j, min(j + self.depth, n)):
                    if k not in futs:
                        futs[k] = ex.submit(self.load, self.records[k])
                img, valid = futs.pop(j).result()
                self._valids.append(valid)
                if self.keep:
                    self.kept.append((img, valid))
                yield img

    def valids(self):
        while True:
            yield self._valids.popleft()


def _merge_attrs(attrs, keep, more):
    """The attributes of the steps so far, subset by the keep mask of the step that just ran, with that step's own laid over them."""
    if more is None:
        return attrs
    if attrs is None:
        return more
    return [dict(attrs[k], **m) for k, m in zip(np.flatnonzero(keep).tolist(), more)]


class SceneWriter:
    """The files of a scene: mask/{id}_road.png, mask/{id}_itsc.png, graph/{id}.p, and what the plan adds to them.  PNG encoding and
    pickling (tens of ms per 2048^2 scene) run on writer threads so that the scene loop goes straight back to the GPU.

    GRAPH_RASTER: a scene's renders run on a writer thread, on a stream of their own — upload of the graph (and of the scene, once),
    the launches, the download, the PNG encoding — so the feeding thread hands the graph over and goes straight back to the GPU, and the
    wait for scene i's render does not queue behind scene i+1's pass 1.  The entries touch no workspace of the library context."""

    def __init__(self, output_dir, config, plan, net, device):
        self.output_dir, self.config, self.plan, self.net = output_dir, config, plan, net
        raster = plan.raster
        self.mask_dir, self.graph_dir = os.path.join(output_dir, "mask"), os.path.join(output_dir, "graph")
        self.render_dirs = {} if raster is None else {k: os.path.join(output_dir, d) for k, d, on in (
            ("viz", "viz", raster.viz), ("mask", "graph_mask", raster.mask), ("diff", "diff", raster.diff)) if on is not None}
        self.geojson_dir = os.path.join(output_dir, "graph_geojson") if plan.geojson else None
        self.polylines_dir = os.path.join(output_dir, "graph_polylines") if plan.polylines else None
        extra = ([os.path.join(output_dir, "mask_tif")] if plan.tiff_masks else []) + ([self.geojson_dir] if plan.geojson else []) + \
            ([self.polylines_dir] if plan.polylines else [])
        for d in [self.mask_dir, self.graph_dir, *self.render_dirs.values(), *extra]:
            os.makedirs(d, exist_ok=True)
        on_device = (raster is not None or plan.support is not None or plan.width is not None or plan.clean is not None) and device.type == "cuda"
        self.render_stream = torch.cuda.Stream(device) if on_device else None
        self.threads = 2 + len(self.render_dirs) + int(plan.post)

    def _on_render_stream(self):
        return torch.cuda.stream(self.render_stream) if self.render_stream is not None else contextlib.nullcontext()

    def write_mask_tifs(self, img_id, img, road_mask, itsc_mask):               # GEOTIFF masks: the PNGs' pixels with the scene's geo tags
        write_geotiff(os.path.join(self.output_dir, "mask_tif", f"{img_id}_road.tif"), road_mask, like=img)
        write_geotiff(os.path.join(self.output_dir, "mask_tif", f"{img_id}_itsc.tif"), itsc_mask, like=img)

    def write_png(self, mask, name):
        # zlib level 1 = cv2.imwrite's default for PNG (the reference, inferencer.py:303-304); PIL's default level 6 takes ~50 ms per
        # 2048^2 mask — two masks per scene would make the encoder, not the GPU, the bottleneck of the loop.  Same pixels either way.
        Image.fromarray(mask).save(os.path.join(self.mask_dir, name), compress_level=1)

    def write_graph(self, img_id, pred_nodes, pred_edges):                      # inferencer.py:330-343
        if self.config.DATASET == "spacenet":
            pred_nodes = np.stack([400 - pred_nodes[:, 0], pred_nodes[:, 1]], axis=1)   # inferencer.py:332-334
        with open(os.path.join(self.graph_dir, f"{img_id}.p"), "wb") as f:
            pickle.dump(convert_to_sat2graph_format(pred_nodes, pred_edges), f)
        print(f"Done for {img_id}.")

    def render_scene(self, img_id, img, valid, pred_nodes, pred_edges, shape, gt_path):
        gt = None if gt_path is None else read_gt_graph(gt_path, spacenet=self.plan.spacenet_gt)
        with self._on_render_stream():
            prod = render_graph(self.plan.raster, pred_nodes, pred_edges, shape, img=img, gt=gt, valid=valid, net=self.net)
        for k, d in self.render_dirs.items():
            if k in prod:
                Image.fromarray(prod[k]).save(os.path.join(d, f"{img_id}.png"), compress_level=1)
        return img_id, prod.get("metrics")

    def finish_scene(self, img_id, img, valid, res, gt_path):
        """EDGE_SUPPORT: a scene's filter runs on a writer thread, on the render stream, IN FRONT of write_graph and
        render_scene, so the pickle, the renders, diff/metrics.json and the GeoJSON all show the filtered graph.  It is applied to a
        result: infer_imgs does not read the key."""
        plan = self.plan
        with self._on_render_stream():
            kept, attrs = apply_edge_support(plan.support, res, valid=valid, net=self.net)
            # ROAD_WIDTH runs behind EDGE_SUPPORT, on the graph it kept; the attributes of the edges both keep are merged
            measured, widths, keep = apply_road_width(plan.width, kept, net=self.net, return_keep=True)
            attrs = _merge_attrs(attrs, keep, widths)
            # GRAPH_CLEAN runs behind both, on the graph they kept, and the attributes are carried along in the same way
            (pred_nodes, pred_edges, itsc_mask, _), chains, keep = apply_graph_clean(plan.clean, measured, net=self.net, return_keep=True)
            attrs = _merge_attrs(attrs, keep, chains)
        self.write_graph(img_id, pred_nodes, pred_edges)
        own_gt = img.geotransform if plan.tiff is not None and plan.tiff.georef and isinstance(img, TiffScene) else None          # GEOTIFF: the default
        export_gt = plan.export_gt if plan.export_gt is not None else own_gt
        if self.geojson_dir is not None:
            write_geojson(os.path.join(self.geojson_dir, f"{img_id}.geojson"), pred_nodes, pred_edges, attrs, export_gt)
        if self.polylines_dir is not None:
            write_polylines(os.path.join(self.polylines_dir, f"{img_id}.geojson"), pred_nodes, pred_edges, clean_table_of(chains), export_gt)
        return self.render_scene(img_id, img, valid, pred_nodes, pred_edges, itsc_mask.shape, gt_path) if plan.raster is not None else (img_id, None)

    def submit(self, pool, record, img, valid, res):
        """Hands one scene's result to the pool: (the futures of its files, the future of its (id, metrics) or None)."""
        plan, img_id = self.plan, record.img_id
        pred_nodes, pred_edges, itsc_mask, road_mask = res
        files, rendered = [], None
        if plan.tiff_masks and isinstance(img, TiffScene):
            files.append(pool.submit(self.write_mask_tifs, img_id, img, road_mask, itsc_mask))
        if plan.post:                            # the graph's files follow the filter; the masks are what they were
            rendered = pool.submit(self.finish_scene, img_id, img, valid, res, record.gt_path)
            files += [pool.submit(self.write_png, road_mask, f"{img_id}_road.png"), pool.submit(self.write_png, itsc_mask, f"{img_id}_itsc.png")]
            return files, rendered
        if plan.raster is not None:              # rank 0 of a tile-sharded run, or this rank's own scene
            rendered = pool.submit(self.render_scene, img_id, img, valid, pred_nodes, pred_edges, itsc_mask.shape, record.gt_path)
        files += [pool.submit(self.write_png, road_mask, f"{img_id}_road.png"), pool.submit(self.write_png, itsc_mask, f"{img_id}_itsc.png"),
                  pool.submit(self.write_graph, img_id, pred_nodes, pred_edges)]
        return files, rendered

    def write_metrics(self, scene_metrics):
        diff = self.plan.raster.diff
        with open(os.path.join(self.render_dirs["diff"], "metrics.json"), "w") as f:
            json.dump({"thin": diff[0], "wide": diff[1], "scenes": dict(scene_metrics), "total": total_metrics([m for _, m in scene_metrics])}, f, indent=1)


def main(argv=None):
    """Parse, resolve, process group, model, output directory, scene loop, metrics and time over the ranks: see the module's docstring."""
    ap = build_parser()
    args = ap.parse_args(argv)
    config = load_config(args.config)
    rank, local_rank, world = (int(os.environ.get(k, d)) for k, d in (("RANK", "0"), ("LOCAL_RANK", "0"), ("WORLD_SIZE", "1")))
    plan = resolve_run(ap, args, config, world)
    device = torch.device("cuda") if args.device == "cuda" else torch.device(args.device)
    torch.set_num_threads(max(1, min(torch.get_num_threads(), usable_cpus() // max(1, world))))   # this rank's share of the container's CPU quota (hostcpu.py)
    scene._numpy_hugepages(False)                # for the whole run: image decoding and output encoding allocate beside the GPU too (_host_quiet)
    dist = torch.distributed
    if world > 1:                                # one process per GPU (torchrun); the reference is single-process (inferencer.py:243)
        if device.type == "cuda":
            torch.cuda.set_device(local_rank)
            device = torch.device("cuda", local_rank)
        if not dist.is_initialized():
            os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
            if device.type == "cuda":
                dist.init_process_group("nccl", device_id=device)
            else:
                dist.init_process_group("gloo")
    by_scene = world > 1 and args.shard == "scenes"
    net = _build_net(config, args.checkpoint, device)

    records = scene_records(args, config, plan, rank, world)
    use_alpha = args.valid_masks is None and any(scene.has_alpha(r.path) for r in records if not plan.as_tiff(r.path))      # headers only; mask files take precedence
    masked = args.valid_masks is not None or use_alpha
    loader = SceneLoader(records, lambda record: load_scene(record, plan, use_alpha), keep=plan.keeps_inputs)

    name = [None]                                # one directory for all ranks: rank 0 creates it (and its timestamp), the others wait
    if rank == 0:
        name[0] = create_output_dir_and_save_config("./save/infer_", config, specified_dir=f"./save/{args.output_dir}" if args.output_dir else None)
    if world > 1:
        dist.broadcast_object_list(name, src=0)
    output_dir = name[0]
    writer = SceneWriter(output_dir, config, plan, net, device)

    # the reference times infer_one_img per image (inferencer.py:292-296); the scenes are software-pipelined here (infer_imgs), so
    # the time reported is what the loop spends waiting for results — its sum over the images is the wall time of inference
    total_inference_seconds = 0.0
    results = scene.infer_imgs(net, loader.scenes(), config, device=device, tile_sharded=world > 1 and not by_scene,
                               pipelined=True if args.shard == "tiles-pipelined" else None, **(dict(valids=loader.valids()) if masked else {}),
                               **(dict(aois=[r.aoi for r in records]) if plan.job_aois is not None else {}))
    pending, rendered = [], []
    with ThreadPoolExecutor(writer.threads) as pool:
        for record in records:
            print(f"Processing {record.img_id}")
            start_seconds = time.time()
            res = next(results)
            total_inference_seconds += time.time() - start_seconds
            img, valid = loader.kept.popleft() if plan.keeps_inputs else (None, None)
            if res is None:                      # non-zero rank of a tile-sharded run
                continue
            files, metrics = writer.submit(pool, record, img, valid, res)
            pending += files
            if metrics is not None:
                rendered.append(metrics)
        for f in pending:
            f.result()
        scene_metrics = [(str(i), m) for i, m in (f.result() for f in rendered) if m is not None]

    if plan.raster is not None and plan.raster.diff is not None:
        if by_scene:                             # every rank rendered its own scenes: rank 0 writes the one file
            parts = [None] * world
            dist.all_gather_object(parts, scene_metrics)
            scene_metrics = [x for part in parts for x in part]
        if rank == 0:
            writer.write_metrics(scene_metrics)

    if world > 1:                                # the slowest rank is the wall time of the run
        t = torch.tensor([total_inference_seconds], dtype=torch.float64, device=device)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        total_inference_seconds = float(t.item())
    time_txt = f"Inference completed for {args.config} in {total_inference_seconds} seconds."
    print(time_txt)
    if rank == 0:
        with open(os.path.join(output_dir, "inference_time.txt"), "w") as f:
            f.write(time_txt)
    if world > 1:
        dist.barrier()
