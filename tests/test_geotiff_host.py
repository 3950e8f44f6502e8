"""GEOTIFF (GeoTIFF scenes decoded on the device): everything that runs without a GPU.  pytest -m "not gpu".

The reader is pinned from two sides: PIL / libtiff WRITES files that tiff_read_ref and segments() + the CPU restatement of the kernel
(geotiff.assemble_ref) must decode exactly, and PIL READS what the kit's writer writes, which pins the writer for the variants only it can
make.  The kit's writer and the reader share no code."""
import json
import os
import re
import shutil
import subprocess
import warnings

import numpy as np
import pytest
import torch
from PIL import Image

from sam_road_amd import Config
from sam_road_amd import geotiff as gt
from sam_road_amd import cli
from sam_road_amd import inferencer as inf
from sam_road_amd.edge_support import graph_geojson
from sam_road_amd.inferencer import infer_imgs, infer_one_img

import geotiff_kit as gk
from scene_kit import E2E_CFG, E2E_SCENE, assert_abi_11, run_cli
from scene_nodata_kit import NodataStandIn
from test_scene_bands_host import SELECT, BandsStandIn, raw_scene
from test_scene_float_host import FloatStandIn, reflectance

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCENE_SEED = 6


def _decodes_to(path, want):
    sc = gt.open_scene(path)
    want = want[:, :, None] if want.ndim == 2 else want
    assert sc.shape == want.shape and sc.dtype == want.dtype
    assert gk.same_bits(gt.tiff_read_ref(path), want)
    flat, table = sc.segments(3)
    assert table.dtype == np.int64 and table.shape[1] == 7 and (sc.is_raster or not (table[:, 0] % 16).any())
    gt.check_table(sc, flat.size, table) if not sc.is_raster else None
    assert gk.same_bits(gt.assemble_ref(sc, flat, table), want)
    assert gk.same_bits(np.asarray(sc), want)                 # __array__
    return sc


# ---- 1. PIL / libtiff writes, the project reads ----------------------------------------------------------------------------------------------
PIL_RASTERS = {"u8rgb": ((37, 53, 3), "uint8"), "u16": ((37, 53, 1), "uint16"), "f32": ((37, 53, 1), "float32"),
               "u8rgb_tall": ((500, 53, 3), "uint8"), "u16_tall": ((700, 53, 1), "uint16"), "f32_tall": ((400, 53, 1), "float32")}
PIL_FORMS = [("raw", 1), ("tiff_lzw", 1), ("tiff_lzw", "p"), ("tiff_adobe_deflate", 1), ("tiff_adobe_deflate", "p")]


@pytest.mark.parametrize("form", PIL_FORMS, ids=lambda f: f"{f[0]}-{f[1]}")
@pytest.mark.parametrize("name", sorted(PIL_RASTERS))
def test_files_written_by_libtiff_decode_exactly(tmp_path, name, form):
    shape, dtype = PIL_RASTERS[name]
    a = gk.sample(shape, dtype, 11)
    a = a if shape[2] == 3 else a[:, :, 0]
    comp, pred = form
    pred = (3 if dtype == "float32" else 2) if pred == "p" else 1
    p = str(tmp_path / "w.tif")
    Image.fromarray(a).save(p, compression=comp, tiffinfo={317: pred} if pred != 1 else {})
    sc = _decodes_to(p, a)
    assert sc.predictor == pred and sc.compression == {"raw": 1, "tiff_lzw": 5, "tiff_adobe_deflate": 8}[comp]
    if name.endswith("_tall") and comp != "raw":
        assert len(sc.offsets) > 1                            # several strips, the last one short


# ---- 2. the kit writes, PIL reads (where it can) and the project reads ------------------------------------------------------------------------
KIT_PIL = {"tiled_rgb": ("uint8", 3, dict(tile=(16, 16))), "tiled_rgb_32x16_lzw": ("uint8", 3, dict(tile=(32, 16), compression="lzw", predictor=2)),
           "big_endian_u16": ("uint16", 1, dict(big_endian=True, compression="lzw", predictor=2)), "planar_rgb": ("uint8", 3, dict(planar=2, rows_per_strip=5)),
           "bigtiff_rgb": ("uint8", 3, dict(bigtiff=True, compression="deflate")), "strips_of_5_deflate": ("uint8", 3, dict(rows_per_strip=5, compression="deflate", predictor=2)),
           "f32_lzw_pred3": ("float32", 1, dict(compression="lzw", predictor=3)), "f32_big_endian": ("float32", 1, dict(big_endian=True, rows_per_strip=5))}
# what only the kit can write (no PIL mode holds them): checked against the source array alone
# (a big-endian float file that is compressed is among them: PIL takes libtiff's native-order floats for big-endian ones)
KIT_ONLY = {"f32_big_endian_pred3": ("float32", 1, dict(big_endian=True, compression="deflate", predictor=3)),
            "u16_4band_tiled_lzw": ("uint16", 4, dict(tile=(16, 32), compression="lzw", predictor=2)),
            "u16_4band_planar_big_endian": ("uint16", 4, dict(planar=2, big_endian=True, compression="deflate", predictor=2, rows_per_strip=7)),
            "u16_16band_bigtiff": ("uint16", 16, dict(bigtiff=True, tile=(16, 16))),
            "f32_3band_pred3_tiled": ("float32", 3, dict(tile=(32, 16), compression="deflate", predictor=3)),
            "f32_4band_planar_pred3_big_endian": ("float32", 4, dict(planar=2, big_endian=True, predictor=3, compression="lzw", rows_per_strip=5)),
            "u8_16band_planar_tiled": ("uint8", 16, dict(planar=2, tile=(16, 16), compression="lzw", predictor=2)),
            "deflate_old_code": ("uint16", 4, dict(compression="deflate-old"))}


@pytest.mark.parametrize("name", sorted(KIT_PIL))
def test_pil_reads_the_kit_files(tmp_path, name):
    dtype, C, kw = KIT_PIL[name]
    a = gk.sample((37, 53, C), dtype, 3)
    p = gk.write_tiff(str(tmp_path / "k.tif"), a, **kw)
    _decodes_to(p, a)
    if name == "bigtiff_rgb":
        try:
            back = np.array(Image.open(p))
        except Exception:                                    # a PIL whose libtiff has no BigTIFF: the reader's own check above stands
            return
    else:
        back = np.array(Image.open(p))
    back = back.astype(back.dtype.newbyteorder("="))           # PIL hands a big-endian file's samples out in the file's byte order
    assert gk.same_bits(back if C > 1 else back[:, :, None] if back.ndim == 2 else back, a), name


@pytest.mark.parametrize("name", sorted(KIT_ONLY))
def test_variants_only_the_kit_writes(tmp_path, name):
    dtype, C, kw = KIT_ONLY[name]
    a = gk.sample((37, 53, C), dtype, 4)
    _decodes_to(gk.write_tiff(str(tmp_path / "k.tif"), a, **kw), a)


def test_the_fast_path_is_the_raster(tmp_path):
    a = gk.sample((37, 53, 4), "uint16", 8)
    sc = gt.open_scene(gk.write_tiff(str(tmp_path / "k.tif"), a, rows_per_strip=5))
    assert sc.is_raster
    flat, table = sc.segments()
    assert flat.size == a.nbytes and np.array_equal(flat.view(np.uint16).reshape(a.shape), a)
    for kw in (dict(big_endian=True), dict(planar=2), dict(tile=(16, 16)), dict(compression="deflate"), dict(predictor=2)):
        assert not gt.open_scene(gk.write_tiff(str(tmp_path / "k.tif"), a, **kw)).is_raster, kw
    assert gt.open_scene(gk.write_tiff(str(tmp_path / "k.tif"), a[:, :, :1], planar=2)).is_raster      # one band: planar is chunky


# ---- 3. the LZW entry ---------------------------------------------------------------------------------------------------------------------------
def test_lzw_entry_equals_the_python_decoder(tmp_path):
    rng = np.random.default_rng(5)
    datas = [rng.integers(0, 256, 24000, dtype=np.uint8).tobytes(),          # incompressible: every code width and several table resets
             bytes(30000), bytes([7]), (np.arange(9000) // 3 % 11).astype(np.uint8).tobytes(), rng.integers(0, 4, 5000, dtype=np.uint8).tobytes()]
    streams = [gk.lzw_encode(d) for d in datas]
    assert len(streams[0]) * 8 // 12 > 3 * 3836             # more 12-bit codes than three full tables: at least three resets
    a = gk.sample((500, 53, 3), "uint8", 2)
    Image.fromarray(a).save(str(tmp_path / "w.tif"), compression="tiff_lzw")
    sc = gt.open_scene(str(tmp_path / "w.tif"))
    with open(sc.path, "rb") as fh:
        for k in range(len(sc.offsets)):
            streams.append(sc._read_segment(fh, k))
            datas.append(gt.lzw_decode_ref(streams[-1], sc.seg_geometry(k)[5]))
    assert b"".join(datas[5:]) == a.tobytes()
    for d, s in zip(datas, streams):
        assert gt.lzw_decode_ref(s, len(d)) == d
    for threads in (1, 4):
        sizes = np.array([len(d) for d in datas], np.int64)
        offs = np.concatenate([[0], np.cumsum((sizes + 15) // 16 * 16)[:-1]]).astype(np.int64)
        flat = np.full(int(offs[-1] + sizes[-1]), 0xCD, np.uint8)
        gt.lzw_decode_into(streams, flat, offs, sizes, threads)
        for d, o in zip(datas, offs):
            assert flat[o:o + len(d)].tobytes() == d
        gaps = np.ones(flat.size, bool)
        for d, o in zip(datas, offs):
            gaps[o:o + len(d)] = False
        assert (flat[gaps] == 0xCD).all()                     # nothing between the slots is written
    # a damaged, a short and a long stream are errors that name the segment
    for bad, size in ((streams[0][:100], len(datas[0])), (streams[3], len(datas[3]) + 1), (streams[3], len(datas[3]) - 1), (b"\xff\xff\xff\xff", 10)):
        flat = np.zeros(len(datas[0]) + 16, np.uint8)
        with pytest.raises(ValueError, match="segment 1"):
            gt.lzw_decode_into([streams[2], bad], flat, np.array([0, 16]), np.array([1, size]), 2)
        with pytest.raises(ValueError):
            gt.lzw_decode_ref(bad, size)


# ---- 4. tags --------------------------------------------------------------------------------------------------------------------------------------
def test_geotransform_nodata_and_geo_tags(tmp_path):
    a = gk.sample((20, 30, 3), "uint8", 1)
    p = str(tmp_path / "g.tif")
    sc = gt.open_scene(gk.write_tiff(p, a, geo=gk.GEO, nodata=-9999))
    assert sc.geotransform == gk.GEO_TRANSFORM and sc.nodata == -9999.0
    assert {t: v[2] for t, v in sc.geo_tags.items()} == {t: v[1] for t, v in gk.GEO.items()}
    # a tiepoint at another pixel
    geo = {**gk.GEO, 33922: (12, (10.0, 4.0, 0.0, 431005.0, 5511999.0, 0.0))}
    assert gt.open_scene(gk.write_tiff(p, a, geo=geo)).geotransform == gk.GEO_TRANSFORM
    # PixelIsPoint: the tags speak of pixel centres
    point = {**gk.GEO, 34735: (3, (1, 1, 0, 2, 1024, 0, 1, 1, 1025, 0, 1, 2))}
    assert gt.open_scene(gk.write_tiff(p, a, geo=point)).geotransform == (431000.0 - 0.25, 0.5, 0.0, 5512000.0 + 0.125, 0.0, -0.25)
    # a 4 x 4 matrix, with rotation
    m = (0.5, 0.1, 0.0, 100.0, -0.2, -0.25, 0.0, 200.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0)
    assert gt.open_scene(gk.write_tiff(p, a, geo={34264: (12, m)})).geotransform == (100.0, 0.5, 0.1, 200.0, -0.2, -0.25)
    assert gt.open_scene(gk.write_tiff(p, a, geo={34264: (12, m), 34735: point[34735]})).geotransform == (100.0 - 0.3, 0.5, 0.1, 200.0 + 0.225, -0.2, -0.25)
    plain = gt.open_scene(gk.write_tiff(p, a))
    assert plain.geotransform is None and plain.nodata is None and plain.geo_tags == {}
    for text, want in (("0", 0.0), ("65535", 65535.0), ("-3.4e+38", -3.4e38), ("1.5 ", 1.5)):
        assert gt.open_scene(gk.write_tiff(p, a, nodata=text)).nodata == want
    assert np.isnan(gt.open_scene(gk.write_tiff(p, a, nodata="nan")).nodata)
    assert gt.open_scene(gk.write_tiff(p, a, nodata="none of it")).nodata is None
    # write_geotiff: PIL reads the pixels, the geo tags come back verbatim, from a scene or from six numbers
    for arr in (gk.sample((33, 41, 1), "uint8", 2)[:, :, 0], gk.sample((33, 41, 4), "uint16", 2), gk.sample((300, 500, 1), "uint8", 3)[:, :, 0]):
        gt.write_geotiff(p, arr, like=sc, nodata=0)
        back = gt.open_scene(p)
        assert back.geo_tags == sc.geo_tags and back.geotransform == gk.GEO_TRANSFORM and back.nodata == 0.0
        assert back.compression == 8 and back.predictor == 2 and not back.tiled and gk.same_bits(gt.tiff_read_ref(back), arr.reshape(back.shape))
        if arr.ndim == 2:
            im = Image.open(p)
            assert np.array_equal(np.array(im), arr) and tuple(im.tag_v2[33550]) == gk.GEO[33550][1] and tuple(im.tag_v2[34735]) == gk.GEO[34735][1]
    gt.write_geotiff(p, a, geotransform=(1, 2, 3, 4, 5, 6))
    assert gt.open_scene(p).geotransform == (1.0, 2.0, 3.0, 4.0, 5.0, 6.0) and np.array_equal(np.array(Image.open(p)), a)
    with pytest.raises(ValueError):
        gt.write_geotiff(p, a.astype(np.float32))
    with pytest.raises(ValueError):
        gt.write_geotiff(p, a, like=sc, geotransform=(1, 2, 3, 4, 5, 6))


REFUSED = {"jpeg": (dict(override={259: (3, (7,))}), "Compression"), "old_jpeg": (dict(override={259: (3, (6,))}), "Compression"),
           "packbits": (dict(override={259: (3, (32773,))}), "PackBits"), "palette": (dict(override={262: (3, (3,))}), "palette"),
           "min_is_white": (dict(override={262: (3, (0,))}), "PhotometricInterpretation"),
           "1bit": (dict(override={258: (3, (1, 1, 1))}), "BitsPerSample"), "4bit": (dict(override={258: (3, (4, 4, 4))}), "BitsPerSample"),
           "12bit": (dict(override={258: (3, (12, 12, 12))}), "BitsPerSample"), "32bit_int": (dict(override={258: (3, (32, 32, 32))}), "BitsPerSample"),
           "mixed_bits": (dict(override={258: (3, (8, 8, 16))}), "BitsPerSample"),
           "signed": (dict(override={339: (3, (2, 2, 2))}), "SampleFormat"), "float64": (dict(override={258: (3, (64, 64, 64)), 339: (3, (3, 3, 3))}), "BitsPerSample"),
           "float16": (dict(override={258: (3, (16, 16, 16)), 339: (3, (3, 3, 3))}), "BitsPerSample"),
           "fill_order": (dict(override={266: (3, (2,))}), "FillOrder"), "predictor_3_on_ints": (dict(override={317: (3, (3,))}), "Predictor"),
           "predictor_9": (dict(override={317: (3, (9,))}), "Predictor"), "tile_of_20": (dict(tile=(16, 16), override={322: (3, (20,))}), "TileWidth"),
           "no_width": (dict(drop=(256,)), "ImageWidth"), "no_offsets": (dict(drop=(273,)), "StripOffsets"),
           "too_few_counts": (dict(rows_per_strip=5, override={279: (4, (10, 10))}), "StripByteCounts"),
           "offset_past_the_end": (dict(override={273: (4, (10 ** 6,))}), "StripOffsets"),
           "count_past_the_end": (dict(override={279: (4, (10 ** 6,))}), "StripOffsets"),
           "short_raw_strip": (dict(override={279: (4, (100,))}), "StripByteCounts")}


@pytest.mark.parametrize("name", sorted(REFUSED))
def test_every_refusal_is_a_value_error_before_anything_is_decoded(tmp_path, name, monkeypatch):
    kw, word = REFUSED[name]
    a = gk.sample((37, 53, 3), "uint8", 1)
    p = gk.write_tiff(str(tmp_path / f"{name}.tif"), a, **kw)
    for fn in ("decompressobj",):
        monkeypatch.setattr(gt.zlib, fn, lambda *a, **k: (_ for _ in ()).throw(AssertionError("decoded")))
    monkeypatch.setattr(gt, "lzw_decode_ref", lambda *a, **k: (_ for _ in ()).throw(AssertionError("decoded")))
    with pytest.raises(ValueError) as e:
        gt.open_scene(p)
    assert name + ".tif" in str(e.value) and word in str(e.value), str(e.value)
    with pytest.raises(ValueError):
        gt.tiff_read_ref(p)


def test_other_refusals_and_truncated_files(tmp_path):
    a = gk.sample((37, 53, 3), "uint8", 1)
    p = gk.write_tiff(str(tmp_path / "ok.tif"), a, compression="lzw", geo=gk.GEO)
    data = open(p, "rb").read()
    assert gt.open_scene(p).shape == (37, 53, 3)
    for n in (0, 3, 7, 9, 20, 100, len(data) - 200, len(data) - 1):          # every truncation is refused, by the header, the IFD or an offset
        t = str(tmp_path / "cut.tif")
        open(t, "wb").write(data[:n])
        with pytest.raises(ValueError, match="cut.tif"):
            gt.open_scene(t)
    open(str(tmp_path / "png.tif"), "wb").write(b"\x89PNG\r\n\x1a\n" + bytes(64))
    with pytest.raises(ValueError, match="not a TIFF"):
        gt.open_scene(str(tmp_path / "png.tif"))
    with pytest.raises(ValueError, match="SamplesPerPixel"):
        gt.open_scene(gk.write_tiff(str(tmp_path / "c17.tif"), gk.sample((5, 5, 17), "uint8", 1)))
    with pytest.raises(ValueError, match="2\\^31"):
        gt.open_scene(gk.write_tiff(str(tmp_path / "huge.tif"), a, override={256: (4, (65536,)), 257: (4, (65536,))}))
    # old-style LZW: the clear code stored low bit first
    old = gk.write_tiff(str(tmp_path / "old.tif"), a, compression="lzw")
    sc = gt.open_scene(old)
    blob = bytearray(open(old, "rb").read())
    blob[sc.offsets[0]:sc.offsets[0] + 2] = b"\x00\x01"
    open(old, "wb").write(blob)
    with pytest.raises(ValueError, match="old-style LZW"):
        gt.open_scene(old)
    # a second IFD (an overview) is ignored: next-IFD offset pointing at garbage
    assert gt.open_scene(p).geotransform == gk.GEO_TRANSFORM


# ---- 5. key and CLI -----------------------------------------------------------------------------------------------------------------------------
def test_key_every_accepted_form_and_the_flags():
    K = gt.GeoTiffKey
    for v in (None, False):
        assert gt.geotiff_key_of(v) is None
    assert gt.geotiff_key(Config(E2E_CFG)) is None
    assert gt.geotiff_key_of(True) == gt.geotiff_key_of({}) == K(True, "ignore", False)
    assert gt.geotiff_key_of({"georef": False}) == K(False, "ignore", False)
    assert gt.geotiff_key_of({"nodata": "file", "masks": True}) == K(True, "file", True)
    assert gt.geotiff_key(Config(E2E_CFG, GEOTIFF={"nodata": "ignore", "georef": True, "masks": False})) == K(True, "ignore", False)
    for bad in (1, "yes", [True], {"georef": 1}, {"masks": "yes"}, {"nodata": "value"}, {"nodata": None}, {"overviews": True}):
        with pytest.raises(ValueError, match="GEOTIFF"):
            gt.geotiff_key_of(bad)
    # the flags lie over the key
    assert gt.geotiff_override(Config(E2E_CFG), True) is True
    assert gt.geotiff_override(Config(E2E_CFG), None, True, None) == {"nodata": "file"}
    assert gt.geotiff_override(Config(E2E_CFG), None, None, True) == {"masks": True}
    assert gt.geotiff_override(Config(E2E_CFG, GEOTIFF={"georef": False, "nodata": "file"}), True, None, True) == {"georef": False, "nodata": "file", "masks": True}
    assert gt.geotiff_override(Config(E2E_CFG, GEOTIFF={"masks": True}), None, True) == {"nodata": "file", "masks": True}


def test_nodata_from_files(tmp_path):
    a = gk.sample((20, 30, 4), "uint16", 1)
    f = gk.sample((20, 30, 2), "float32", 1)
    mk = lambda name, arr, nd: (lambda p: (p, gt.open_scene(p)))(gk.write_tiff(str(tmp_path / name), arr, nodata=nd))
    assert cli._nodata_from_files(dict([mk("a.tif", a, 0), mk("b.tif", a, "0.0")])) == (0, False)
    assert cli._nodata_from_files(dict([mk("a.tif", f, -9999), mk("b.tif", f, "-9999.0")])) == (-9999.0, True)
    v, is_float = cli._nodata_from_files(dict([mk("a.tif", f, "nan"), mk("b.tif", f, "nan")]))
    assert is_float and v != v
    with pytest.raises(ValueError, match=r"a\.tif states 0\.0 and .*b\.tif states 65535\.0"):
        cli._nodata_from_files(dict([mk("a.tif", a, 0), mk("b.tif", a, 65535)]))
    with pytest.raises(ValueError, match=r"b\.tif.*no nodata"):
        cli._nodata_from_files(dict([mk("a.tif", a, 0), mk("b.tif", a, None)]))
    with pytest.raises(ValueError, match="integer and float"):
        cli._nodata_from_files(dict([mk("a.tif", a, 0), mk("b.tif", f, 0)]))
    for nd in (-1, 65536, 0.5):
        with pytest.raises(ValueError, match="no level"):
            cli._nodata_from_files(dict([mk("a.tif", a, nd)]))
    with pytest.raises(ValueError, match="--images"):
        cli._nodata_from_files({})


# ---- 6. the whole loop on the CPU stand-in ----------------------------------------------------------------------------------------------------------
class TiffBands(gk.TiffAssembleMixin, BandsStandIn):
    pass


class TiffFloat(gk.TiffAssembleMixin, FloatStandIn):
    pass


class TiffNodata(gk.TiffAssembleMixin, NodataStandIn):
    pass


@pytest.fixture(scope="module")
def u8_scene():
    from oracle.synth import synth_scene
    return synth_scene(E2E_SCENE, seed=SCENE_SEED)


def _same(a, b):
    assert len(a) == len(b) == 4
    for x, y in zip(a, b):
        assert x.dtype == y.dtype and np.array_equal(x, y)


def _run(net, img, cfg, **kw):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return infer_one_img(net, img, Config(cfg), device="cpu", **kw)


def test_runs_on_a_tiff_equal_the_runs_on_its_array(tmp_path, u8_scene):
    torch.set_num_threads(4)
    bands, flt = TiffBands(dict(E2E_CFG), ("valid",)), TiffFloat(dict(E2E_CFG), ("valid",))
    cases = [("u8", bands, u8_scene, dict(compression="deflate", predictor=2, tile=(64, 48)), {}),
             ("u16", bands, raw_scene(u8_scene), dict(compression="lzw", predictor=2, planar=2, big_endian=True, rows_per_strip=37),
              dict(SCENE_BANDS={"select": SELECT, "stretch": {"percentile": [2, 98]}})),
             ("f32", flt, reflectance(u8_scene), dict(compression="deflate", predictor=3, tile=(32, 64)), dict(SCENE_FLOAT={"select": SELECT, "stretch": [0.0, 1.0]}))]
    for name, net, arr, kw, keys in cases:
        p = gk.write_tiff(str(tmp_path / f"{name}.tif"), arr, geo=gk.GEO, **kw)
        ref = gt.tiff_read_ref(p)
        assert gk.same_bits(ref, arr)
        cfg = dict(E2E_CFG, **keys)
        want = _run(net, ref, cfg)
        assert want[0].shape[0] >= 30 and want[1].shape[0] >= 1
        net.calls.clear()
        got = _run(net, gt.open_scene(p), dict(cfg, GEOTIFF=True))
        _same(got, want)
        assert gk.tiff_calls(net) == [("tiff_assemble", arr.shape, str(arr.dtype), len(gt.open_scene(p).offsets))]
        # the pipelined loop, a scene that was loaded ahead (the CLI's loader) and one that was not
        net.calls.clear()
        for got in infer_imgs(net, [gt.open_scene(p).load(2), gt.open_scene(p)], Config(dict(cfg, GEOTIFF=True)), device="cpu"):
            _same(got, want)
        assert len(gk.tiff_calls(net)) == 2
    # the fast path launches nothing, and an array still makes the calls it made
    p = gk.write_tiff(str(tmp_path / "raster.tif"), u8_scene, rows_per_strip=64)
    want = _run(bands, u8_scene, E2E_CFG)
    bands.calls.clear()
    _same(_run(bands, gt.open_scene(p), dict(E2E_CFG, GEOTIFF=True)), want)
    assert not gk.tiff_calls(bands)
    # SCENE_GROUP: a ValueError before the model is touched
    bands.calls.clear()
    with pytest.raises(ValueError, match="SCENE_GROUP"):
        list(infer_imgs(bands, [gt.open_scene(p), gt.open_scene(p)], Config(dict(E2E_CFG, INFER_PATCHES_PER_EDGE=2)), device="cpu", group=2))
    assert not bands.calls
    # the dtype rules are unchanged
    with pytest.raises(ValueError, match="uint8"):
        _run(bands, gt.open_scene(str(tmp_path / "u16.tif")), dict(E2E_CFG, GEOTIFF=True))
    with pytest.raises(ValueError, match="SCENE_FLOAT|float32|uint8"):
        _run(flt, gt.open_scene(str(tmp_path / "f32.tif")), dict(E2E_CFG, GEOTIFF=True))


def _files(root):
    return sorted(os.path.relpath(os.path.join(d, f), root) for d, _, fs in os.walk(root) for f in fs)


def test_cli(tmp_path, monkeypatch, u8_scene):
    warnings.simplefilter("ignore")
    torch.set_num_threads(4)
    net = TiffNodata(dict(E2E_CFG), ("valid",))
    monkeypatch.chdir(tmp_path)
    Image.fromarray(u8_scene).save("p.tif")                   # an 8-bit RGB TIFF, as PIL writes it
    # without the key the .tif goes through PIL as before, and the new code is out of the way: the same files, byte for byte
    plain = run_cli(cli, net, tmp_path, monkeypatch, "plain", E2E_CFG, ["p.tif"], "--graph-geojson")
    assert not gk.tiff_calls(net) and "GEOTIFF" not in plain["p"][3]
    with monkeypatch.context() as mp:
        def never(*a, **k):
            raise AssertionError("the new code ran")
        for fn in ("open_scene", "write_geotiff", "_nodata_from_files"):
            mp.setattr(cli, fn, never)
        run_cli(cli, net, tmp_path, mp, "bypassed", E2E_CFG, ["p.tif"], "--graph-geojson")
    assert _files("save/plain") == _files("save/bypassed") == ["config.yaml", "graph/p.p", "graph_geojson/p.geojson", "inference_time.txt", "mask/p_itsc.png", "mask/p_road.png"]
    for f in _files("save/plain"):
        if f != "inference_time.txt":
            assert open(f"save/plain/{f}", "rb").read() == open(f"save/bypassed/{f}", "rb").read(), f

    # the issue's command: a 4-band 16-bit LZW tiled GeoTIFF end to end with no other georeferencing flag
    raw = raw_scene(u8_scene)
    raw[:40, :50] = 0                                        # a nodata corner, all four bands
    gk.write_tiff("a.tif", raw, compression="lzw", predictor=2, tile=(64, 64), geo=gk.GEO, nodata=0)
    argv = ["--geotiff", "--bands", ",".join(str(b) for b in SELECT), "--stretch-percentile", "2", "98", "--nodata-from-file", "--graph-geojson", "--mask-geotiff"]
    net.calls.clear()
    got = run_cli(cli, net, tmp_path, monkeypatch, "geo", E2E_CFG, ["a.tif"], *argv)["a"]
    assert got[3]["GEOTIFF"] == {"nodata": "file", "masks": True} and got[3]["SCENE_NODATA"] == {"value": 0} and len(gk.tiff_calls(net)) == 1
    assert _files("save/geo") == ["config.yaml", "graph/a.p", "graph_geojson/a.geojson", "inference_time.txt", "mask/a_itsc.png", "mask/a_road.png",
                                  "mask_tif/a_itsc.tif", "mask_tif/a_road.tif"]
    cfg = dict(E2E_CFG, SCENE_BANDS=got[3]["SCENE_BANDS"], SCENE_NODATA=got[3]["SCENE_NODATA"])
    nodes, edges, itsc, road = _run(net, gt.tiff_read_ref("a.tif"), cfg)
    assert nodes.shape[0] >= 30 and edges.shape[0] >= 1 and not road[:40, :50].any()
    assert np.array_equal(got[0], itsc) and np.array_equal(got[1], road)
    from sam_road_amd.formats import convert_to_sat2graph_format
    assert got[2] == convert_to_sat2graph_format(nodes, edges)                                  # the graph of the run on tiff_read_ref(a.tif)
    # the GeoJSON is in map coordinates: the file's transform
    doc = json.load(open("save/geo/graph_geojson/a.geojson"))
    assert doc == json.loads(json.dumps(graph_geojson(nodes, edges, None, gk.GEO_TRANSFORM)))
    xs = [c[0] for f in doc["features"] for c in f["geometry"]["coordinates"]]
    assert min(xs) >= 431000.0 and max(xs) <= 431000.0 + 0.5 * E2E_SCENE
    # the mask TIFFs: PIL reads the PNGs' pixels, the geo tags are the input's, verbatim
    src = gt.open_scene("a.tif")
    for kind, mask in (("itsc", got[0]), ("road", got[1])):
        im = Image.open(f"save/geo/mask_tif/a_{kind}.tif")
        assert np.array_equal(np.array(im), mask)
        back = gt.open_scene(f"save/geo/mask_tif/a_{kind}.tif")
        assert back.geo_tags == src.geo_tags and back.geotransform == gk.GEO_TRANSFORM
    # an explicit --geotransform wins; georef: false switches the default off
    run_cli(cli, net, tmp_path, monkeypatch, "explicit", E2E_CFG, ["a.tif"], *argv[:-1], "--geotransform", "1", "2", "0", "3", "0", "4")
    assert json.load(open("save/explicit/graph_geojson/a.geojson")) == json.loads(json.dumps(graph_geojson(nodes, edges, None, (1.0, 2.0, 0.0, 3.0, 0.0, 4.0))))
    assert "mask_tif/a_road.tif" not in _files("save/explicit")
    run_cli(cli, net, tmp_path, monkeypatch, "pixels", dict(E2E_CFG, GEOTIFF={"georef": False}), ["a.tif"], *argv[1:-1])
    assert json.load(open("save/pixels/graph_geojson/a.geojson")) == json.loads(json.dumps(graph_geojson(nodes, edges)))
    # scenes that state different nodata values: refused before the model is built
    gk.write_tiff("b.tif", raw, geo=gk.GEO, nodata=65535)
    monkeypatch.setattr(cli, "_build_net", lambda *a, **k: (_ for _ in ()).throw(AssertionError("the model was built")))
    with open("geo.yaml") as f:
        assert f.read()
    with pytest.raises(ValueError, match=r"a\.tif states 0\.0 and b\.tif states 65535\.0"):
        inf.main(["--config", "geo.yaml", "--checkpoint", "none", "--device", "cpu", "--output_dir", "differ", *argv, "--images", "a.tif", "b.tif"])
    # and a file that cannot be read
    gk.write_tiff("j.tif", raw, override={259: (3, (7,))})
    with pytest.raises(ValueError, match=r"j\.tif.*JPEG"):
        inf.main(["--config", "geo.yaml", "--checkpoint", "none", "--device", "cpu", "--output_dir", "jpeg", "--geotiff", "--images", "j.tif"])


def test_cli_area_of_interest_takes_the_scene_transform(tmp_path, monkeypatch, u8_scene):
    """--aoi polygons in map coordinates and no --aoi-geotransform: the scene's own transform is the default, scene by scene."""
    warnings.simplefilter("ignore")
    torch.set_num_threads(4)
    net = TiffFloat(dict(E2E_CFG), ("valid",))                # the stand-in with the area-of-interest entries
    monkeypatch.chdir(tmp_path)
    gk.write_tiff("a.tif", u8_scene, compression="deflate", predictor=2, geo=gk.GEO)
    g = gk.GEO_TRANSFORM
    xy = lambda c, r: [g[0] + c * g[1] + r * g[2], g[3] + c * g[4] + r * g[5]]
    with open("aoi.geojson", "w") as f:
        json.dump({"type": "Polygon", "coordinates": [[xy(20, 30), xy(330, 30), xy(330, 300), xy(20, 300), xy(20, 30)]]}, f)
    own = run_cli(cli, net, tmp_path, monkeypatch, "own", E2E_CFG, ["a.tif"], "--geotiff", "--aoi", "aoi.geojson")["a"]
    stated = run_cli(cli, net, tmp_path, monkeypatch, "stated", E2E_CFG, ["a.tif"], "--geotiff", "--aoi", "aoi.geojson", "--aoi-geotransform", *[repr(v) for v in g])["a"]
    assert np.array_equal(own[0], stated[0]) and np.array_equal(own[1], stated[1]) and own[2] == stated[2]
    assert own[1][30:300, 20:330].any() and not own[1][:30].any() and not own[1][:, 330:].any()
    assert own[3]["SCENE_AOI"]["geotransform"] == list(g)
    with pytest.raises(ValueError, match="SCENE_AOI"):        # georef off: the polygons are pixels again, and these are far outside
        run_cli(cli, net, tmp_path, monkeypatch, "off", dict(E2E_CFG, GEOTIFF={"georef": False}), ["a.tif"], "--aoi", "aoi.geojson")


# ---- 7. the kernel's own code, on the CPU ---------------------------------------------------------------------------------------------------------
def test_kernel_addressing_and_lzw_on_the_cpu(tmp_path):
    """tests/geotiff_check.cpp runs whole launches of the assemble kernel through its own per-thread code (csrc/geotiff_piece.hpp) and the
    LZW decoder over valid, truncated, bit-flipped and over-long streams, as a stand-alone host program built with the address and
    undefined-behaviour sanitizers; every block has its exact size, so a byte read or written outside one ends it."""
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    cxx = next((c for c in (os.path.join(rocm, "llvm", "bin", "clang++"), os.path.join(rocm, "lib", "llvm", "bin", "clang++")) if os.path.exists(c)), None)
    if cxx is None:
        pytest.skip("no ROCm clang++")
    exe = str(tmp_path / "geotiff_check")
    csrc = os.path.join(ROOT, "sam_road_amd", "csrc")
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", csrc,
                        os.path.join(ROOT, "tests", "geotiff_check.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    assert "geotiff OK" in r.stdout
    piece = open(os.path.join(csrc, "geotiff_piece.hpp")).read()
    assert int(re.search(r"TIF_CHUNK = (\d+)", piece).group(1)) == gk.CHUNK and int(re.search(r"TIF_ALIGN = (\d+)", piece).group(1)) == gt.ALIGN
    assert int(re.search(r"TIF_TABLE_COLS = (\d+)", piece).group(1)) == gt.TABLE_COLS


# ---- 8. the cross-compile and the C ABI -----------------------------------------------------------------------------------------------------------
def test_kernel_compiles_for_gfx950_without_a_gpu():
    hipcc = next((c for c in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", shutil.which("hipcc")) if c and os.path.exists(c)), None)
    if hipcc is None:
        pytest.skip("hipcc not found")
    from sam_road_amd import build
    assert "scene_tiff.hip" in build.SOURCES and "scene_tiff.hip" in os.listdir(build.CSRC)      # in the library and in its build id
    r = subprocess.run([hipcc, *build.FLAGS, "-S", "--cuda-device-only", os.path.join(build.CSRC, "scene_tiff.hip"), "-o", "-"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    names = set(re.findall(r"^(_Z\w*tiff_assemble_kernel\w*):", r.stdout, re.M))
    assert len(names) == 1, names
    name = names.pop()
    meta = r.stdout[r.stdout.index(".amdhsa_kernel " + name):]
    meta = meta[:meta.index(".end_amdhsa_kernel")]
    assert int(re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", meta).group(1)) == 0           # no scratch: the carries are registers
    assert int(re.search(r"\.amdhsa_uses_dynamic_stack (\d+)", meta).group(1)) == 0
    assert int(re.search(r"\.amdhsa_group_segment_fixed_size (\d+)", meta).group(1)) == 4 * (gk.CHUNK + gk.CHUNK // 32) + 4 * 16 * 4      # whatever W is
    body = r.stdout[r.stdout.index(name + ":"):r.stdout.index(".amdhsa_kernel " + name)]
    assert "atomic" not in body and "s_barrier" in body and "global_store_dwordx4" in body and "global_store_byte" in body
    assert "ds_bpermute" in body or "dpp" in body                                                      # the shuffle scan


def test_abi_has_the_entries_and_stays_11():
    header, lib = assert_abi_11((("srh_tiff_assemble", 14), ("srh_tiff_lzw_decode", 10)))
    assert "GEOTIFF" in header
    out = torch.zeros(64, dtype=torch.uint8)
    assert lib.srh_tiff_assemble(None, None, 0, None, None, 0, out.data_ptr(), 2, 2, 1, 2, 1, 0, None) == -1      # refused without a context
    assert lib.srh_tiff_lzw_decode(None, 0, None, None, 1, out.data_ptr(), 64, None, None, 1) == -1
    assert lib.srh_tiff_lzw_decode(None, 0, None, None, 0, None, 0, None, None, 1) == 0                           # no segment: nothing to do
    assert not out.any()
