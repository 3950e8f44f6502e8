"""GeoTIFF scenes (config key GEOTIFF): the one statement of which files are read and what their bytes mean.  The stdlib and
numpy only.  open_scene parses the header and the first IFD and decodes nothing; TiffScene.segments decompresses the file's strips or tiles
on host threads and hands them on AS THEY ARE — predictor, byte order, planes and tiles still in place — for the device to assemble
(csrc/scene_tiff.hip, srh_tiff_assemble); tiff_read_ref is the reference decoder in plain numpy that the device must equal bit for bit,
and assemble_ref restates the device step from the same flat array and table.  write_geotiff writes masks back with a scene's geo tags.

WHAT IS READ.  Classic TIFF and BigTIFF, both byte orders, the first IFD only (overviews and further pages are ignored).  Strips or tiles,
PlanarConfiguration 1 or 2, 1 <= C <= 16 samples per pixel (extra samples are just bands), 8- or 16-bit unsigned or 32-bit IEEE float, all
samples alike; Compression 1 (none), 5 (LZW, MSB first, early change), 8 / 32946 (deflate); Predictor 1, 2 (8 / 16 bit) or 3 (float);
Photometric 1 or 2.  Everything else is a ValueError that names the file and the tag, raised by open_scene, before a segment is decoded;
every offset and byte count is checked against the file size there as well.

THE SEGMENT TABLE.  segments() returns (flat uint8, table int64 [n, 7]): flat holds the decompressed segments, each at a 16-byte aligned
offset; row k of the table is {offset, bytes, first row, first column, rows, columns, band or -1}.  A strip has `columns` = W and the
rows it really holds; a tile has its full size, padding included (the padding of right and bottom edge tiles is dropped by whoever places
it).  A segment of a chunky file (band -1) holds rows x columns x C samples, one of a planar file rows x columns of band `band`.

PREDICTORS.  2: within a row of a segment every sample is the wrapping difference to the sample C places before it (1 place in a planar
file), in the sample's own width, after the byte swap.  3 (TIFF Technical Note 3, as libtiff applies it): the row's columns x C floats are
split into four byte planes, most significant first WHATEVER the file's byte order, and the row of columns x C x 4 bytes is differenced
with stride C across the plane boundaries; undoing it is a running byte sum with stride C over the WHOLE row, then the regrouping.  Float
results are bit patterns: a NaN's payload comes through.

THE GEOTRANSFORM is the project's: X = g0 + x g1 + y g2, Y = g3 + x g4 + y g5 with (x, y) = (column, row) in the pixel-corner frame.  It
comes from ModelPixelScale (33550) + ModelTiepoint (33922) or from ModelTransformation (34264); with GTRasterTypeGeoKey = RasterPixelIsPoint
in 34735 the tags speak of pixel centres and the transform is shifted by half a pixel.  None when the file has none of them.  No CRS is
interpreted: geo_tags holds the raw values of 33550 / 33922 / 34264 / 34735 / 34736 / 34737, to be copied out verbatim."""
import collections
import os
import struct
import zlib

import numpy as np

MAX_BANDS = 16
MAX_PIXELS = 2 ** 31 - 1
ALIGN = 16                                                     # every segment of the flat array starts on a multiple of it
GEO_TAGS = (33550, 33922, 34264, 34735, 34736, 34737)
NODATA_TAG = 42113
TABLE_COLS = 7                                                 # offset, bytes, row0, col0, rows, cols, band

_TYPES = {1: ("B", 1), 2: ("c", 1), 3: ("H", 2), 4: ("I", 4), 5: ("II", 8), 6: ("b", 1), 7: ("B", 1), 8: ("h", 2), 9: ("i", 4), 10: ("ii", 8),
          11: ("f", 4), 12: ("d", 8), 13: ("I", 4), 16: ("Q", 8), 17: ("q", 8), 18: ("Q", 8)}
_NAMES = {256: "ImageWidth", 257: "ImageLength", 258: "BitsPerSample", 259: "Compression", 262: "PhotometricInterpretation", 266: "FillOrder",
          273: "StripOffsets", 277: "SamplesPerPixel", 278: "RowsPerStrip", 279: "StripByteCounts", 284: "PlanarConfiguration", 317: "Predictor",
          322: "TileWidth", 323: "TileLength", 324: "TileOffsets", 325: "TileByteCounts", 339: "SampleFormat"}
_COMPRESSIONS = {2: "CCITT RLE", 3: "CCITT T.4", 4: "CCITT T.6", 6: "old-style JPEG", 7: "JPEG", 32773: "PackBits", 34712: "JPEG 2000", 34925: "LZMA",
                 50000: "ZSTD", 50001: "WebP"}

GeoTiffKey = collections.namedtuple("GeoTiffKey", "georef nodata masks")


# ---- the key -------------------------------------------------------------------------------------------------------------------------------
def geotiff_key_of(v):
    """GEOTIFF parsed: None (absent, None, False: nothing changes) or a GeoTiffKey.  True = the defaults; a mapping may hold georef (bool,
    default true: a scene's own geotransform is the default of the GeoJSON export and of the area of interest), nodata ("file": the files'
    tag 42113 is the nodata value of SCENE_NODATA / SCENE_FLOAT, "ignore", the default) and masks (bool, default false: the masks are
    also written as GeoTIFFs with the scene's geo tags).  ValueError for anything else."""
    if v is None or v is False:
        return None
    if v is True:
        return GeoTiffKey(True, "ignore", False)
    if not isinstance(v, dict):
        raise ValueError(f"GEOTIFF must be true or a mapping {{georef, nodata, masks}}, got {v!r}")
    unknown = set(v) - {"georef", "nodata", "masks"}
    if unknown:
        raise ValueError(f"GEOTIFF: unknown entries {sorted(unknown)} (georef, nodata, masks)")
    georef, nodata, masks = v.get("georef", True), v.get("nodata", "ignore"), v.get("masks", False)
    if not isinstance(georef, bool) or not isinstance(masks, bool):
        raise ValueError(f"GEOTIFF: georef and masks are booleans, got {georef!r} and {masks!r}")
    if nodata not in ("file", "ignore"):
        raise ValueError(f"GEOTIFF: nodata is 'file' or 'ignore', got {nodata!r}")
    return GeoTiffKey(georef, nodata, masks)


def geotiff_key(config):
    return geotiff_key_of(config.get("GEOTIFF"))


def geotiff_override(config, enable=None, nodata_from_file=None, masks=None):
    """The config's GEOTIFF with the CLI's flags laid over it (--geotiff, --nodata-from-file, --mask-geotiff; any of them switches the key
    on): the value to store in the config, in the shortest form that says it."""
    base = config.get("GEOTIFF")
    key = geotiff_key_of(base) or GeoTiffKey(True, "ignore", False)
    if nodata_from_file:
        key = key._replace(nodata="file")
    if masks:
        key = key._replace(masks=True)
    out = {k: v for k, v, d in (("georef", key.georef, True), ("nodata", key.nodata, "ignore"), ("masks", key.masks, False)) if v != d}
    return out or True


def is_tiff_path(path):
    return str(path).lower().endswith((".tif", ".tiff"))


# ---- the file ------------------------------------------------------------------------------------------------------------------------------
class TiffScene:
    """A GeoTIFF scene that has been opened and not decoded (open_scene).  It stands where an array stands in infer_one_img / infer_imgs:
    shape (H, W, C), dtype and ndim are those of the raster; numpy.asarray(scene) decodes it on the host (tiff_read_ref: slowly)."""
    ndim = 3

    def __init__(self, path):
        self.path = str(path)

    def _bad(self, tag, what):
        name = f"{_NAMES[tag]} ({tag})" if tag in _NAMES else f"tag {tag}"
        return ValueError(f"{self.path}: {name}: {what}")

    def __array__(self, dtype=None, copy=None):
        a = tiff_read_ref(self)
        return a if dtype is None else a.astype(dtype, copy=False)

    def __repr__(self):
        return f"TiffScene({self.path!r}, shape={self.shape}, dtype={self.dtype})"

    @property
    def is_raster(self):
        """The fast path: a little-endian, uncompressed, predictor-1, chunky strip file IS the raster; segments() then lays the strips
        end to end and nothing has to be launched."""
        return self.little and self.compression == 1 and self.predictor == 1 and self.planar == 1 and not self.tiled

    def load(self, threads=1):
        """segments() now, kept for the scene's upload: what the CLI's loader thread calls ahead of the scene's turn.  Returns self."""
        self._loaded = self.segments(threads)
        return self

    def loaded(self, threads=1):
        """The (flat, table) of load(), handed out once, or of segments(threads) now."""
        got, self._loaded = getattr(self, "_loaded", None), None
        return got if got is not None else self.segments(threads)

    def seg_geometry(self, k):
        """(first row, first column, rows, columns, band or -1, decompressed bytes) of segment k."""
        H, W, C = self.shape
        per_band = len(self.offsets) // (C if self.planar == 2 else 1)
        band, j = (k // per_band, k % per_band) if self.planar == 2 else (-1, k)
        S = 1 if self.planar == 2 else C
        if self.tiled:
            across = (W + self.tile_w - 1) // self.tile_w
            r0, c0, rows, cols = (j // across) * self.tile_h, (j % across) * self.tile_w, self.tile_h, self.tile_w
        else:
            r0, c0, cols = j * self.rows_per_strip, 0, W
            rows = min(self.rows_per_strip, H - r0)
        return r0, c0, rows, cols, band, rows * cols * S * self.dtype.itemsize

    def _read_segment(self, fh, k):
        fh.seek(self.offsets[k])
        data = fh.read(self.counts[k])
        if len(data) != self.counts[k]:
            raise ValueError(f"{self.path}: segment {k} ends behind the end of the file")
        return data

    def segments(self, threads=1, aligned=False):
        """(flat uint8 [n], table int64 [segments, 7]) — the module's docstring has the layout.  Deflate runs in zlib on `threads` threads
        (zlib releases the interpreter lock), LZW in the library's host code on as many (srh_tiff_lzw_decode), uncompressed segments are
        read straight from the file into their place.  A file that is the raster (is_raster) gets its strips end to end, the raster itself,
        unless `aligned` asks for the 16-byte layout all the same."""
        n = len(self.offsets)
        table = np.zeros((n, TABLE_COLS), np.int64)
        pos = 0
        for k in range(n):
            r0, c0, rows, cols, band, nbytes = self.seg_geometry(k)
            table[k] = (pos, nbytes, r0, c0, rows, cols, band)
            pos += nbytes if self.is_raster and not aligned else (nbytes + ALIGN - 1) // ALIGN * ALIGN
        flat = np.zeros(pos, np.uint8)
        with open(self.path, "rb") as fh:
            if self.compression == 1:
                for k in range(n):
                    fh.seek(self.offsets[k])
                    if fh.readinto(memoryview(flat)[table[k, 0]:table[k, 0] + table[k, 1]]) != table[k, 1]:
                        raise ValueError(f"{self.path}: segment {k} ends behind the end of the file")
                return flat, table
            raw = [self._read_segment(fh, k) for k in range(n)]
        if self.compression == 5:
            lzw_decode_into(raw, flat, table[:, 0], table[:, 1], threads, self.path)
            return flat, table

        def inflate(k):
            data = _inflate(raw[k], int(table[k, 1]), self.path, k)
            flat[table[k, 0]:table[k, 0] + table[k, 1]] = np.frombuffer(data, np.uint8, int(table[k, 1]))
        if threads > 1 and n > 1:
            from concurrent.futures import ThreadPoolExecutor
            with ThreadPoolExecutor(min(int(threads), n)) as ex:
                list(ex.map(inflate, range(n)))
        else:
            for k in range(n):
                inflate(k)
        return flat, table


def _inflate(data, nbytes, path, k):
    try:
        out = zlib.decompressobj().decompress(data, nbytes)
    except zlib.error as e:
        raise ValueError(f"{path}: segment {k}: {e}") from None
    if len(out) != nbytes:
        raise ValueError(f"{path}: segment {k} inflates to {len(out)} bytes, {nbytes} expected")
    return out


def lzw_decode_into(raw, flat, offsets, nbytes, threads, path="<memory>"):
    """The LZW segments `raw` (a list of bytes) decoded into flat[offsets[k] : offsets[k] + nbytes[k]] by srh_tiff_lzw_decode, on `threads`
    host threads.  ValueError for a stream that does not hold exactly nbytes[k] bytes."""
    from . import _lib
    lib = _lib.load()
    n = len(raw)
    src = np.frombuffer(b"".join(raw), np.uint8)
    in_bytes = np.array([len(r) for r in raw], np.int64)
    in_off = np.concatenate([[0], np.cumsum(in_bytes)[:-1]]).astype(np.int64) if n else np.zeros(0, np.int64)
    out_off, out_bytes = np.ascontiguousarray(offsets, np.int64), np.ascontiguousarray(nbytes, np.int64)
    src_keep = src if src.size else np.zeros(1, np.uint8)
    rc = lib.srh_tiff_lzw_decode(src_keep.ctypes.data, int(src.size), in_off.ctypes.data, in_bytes.ctypes.data, n, flat.ctypes.data, int(flat.size),
                                 out_off.ctypes.data, out_bytes.ctypes.data, max(1, int(threads)))
    if rc > 0:
        raise ValueError(f"{path}: segment {rc - 1}: the LZW stream is damaged or does not hold the {int(out_bytes[rc - 1])} bytes of the segment")
    if rc != 0:
        raise ValueError(f"{path}: srh_tiff_lzw_decode refused its arguments (status {rc})")


def _values(buf, bo, typ, count, tag, scene):
    if typ not in _TYPES:
        raise scene._bad(tag, f"unknown field type {typ}")
    fmt, size = _TYPES[typ]
    if len(buf) < size * count:
        raise scene._bad(tag, "its values end behind the end of the file")
    if typ in (2, 7):
        return bytes(buf[:count])
    vals = struct.unpack(bo + fmt * count, buf[:size * count])
    return vals


def open_scene(path):
    """Header and first IFD of a TIFF -> TiffScene.  Nothing is decoded; everything that cannot be read is a ValueError here."""
    sc = TiffScene(path)
    size = os.path.getsize(sc.path)
    with open(sc.path, "rb") as fh:
        head = fh.read(16)
        if len(head) < 8 or head[:2] not in (b"II", b"MM"):
            raise ValueError(f"{sc.path}: not a TIFF file (byte order mark)")
        bo = "<" if head[:2] == b"II" else ">"
        magic = struct.unpack(bo + "H", head[2:4])[0]
        if magic == 42:
            big, ifd = False, struct.unpack(bo + "I", head[4:8])[0]
        elif magic == 43:
            if len(head) < 16 or struct.unpack(bo + "HH", head[4:8]) != (8, 0):
                raise ValueError(f"{sc.path}: a BigTIFF header with offsets of another size than 8 bytes")
            big, ifd = True, struct.unpack(bo + "Q", head[8:16])[0]
        else:
            raise ValueError(f"{sc.path}: not a TIFF file (magic number {magic})")
        cnt_fmt, cnt_size, ent_size, val_size = ("Q", 8, 20, 8) if big else ("H", 2, 12, 4)
        if ifd < 8 or ifd + cnt_size > size:
            raise ValueError(f"{sc.path}: the first IFD lies outside the file (offset {ifd}, {size} bytes)")
        fh.seek(ifd)
        n_ent = struct.unpack(bo + cnt_fmt, fh.read(cnt_size))[0]
        if n_ent < 1 or n_ent > 4096 or ifd + cnt_size + n_ent * ent_size > size:
            raise ValueError(f"{sc.path}: the first IFD ends behind the end of the file ({n_ent} entries)")
        body = fh.read(n_ent * ent_size)
        tags = {}
        for e in range(n_ent):
            ent = body[e * ent_size:(e + 1) * ent_size]
            tag, typ = struct.unpack(bo + "HH", ent[:4])
            count = struct.unpack(bo + ("Q" if big else "I"), ent[4:4 + val_size])[0]
            if typ not in _TYPES:
                continue                                       # a field of a type nobody knows is skipped, as the specification asks
            nbytes = _TYPES[typ][1] * count
            inline = ent[4 + val_size:]
            if nbytes <= val_size:
                buf = inline
            else:
                off = struct.unpack(bo + ("Q" if big else "I"), inline)[0]
                if off + nbytes > size:
                    raise sc._bad(tag, f"its {nbytes} bytes at offset {off} end behind the end of the file ({size} bytes)")
                if tag not in _NAMES and tag not in GEO_TAGS and tag != NODATA_TAG:
                    continue
                fh.seek(off)
                buf = fh.read(nbytes)
            tags[tag] = (typ, count, _values(buf, bo, typ, count, tag, sc))

        def one(tag, default=None):
            if tag not in tags:
                if default is None:
                    raise sc._bad(tag, "the tag is missing")
                return default
            v = tags[tag][2]
            if isinstance(v, bytes) or len(v) < 1:
                raise sc._bad(tag, "not a number")
            return int(v[0])

        W, H, C = one(256), one(257), one(277, 1)
        if W < 1 or H < 1:
            raise sc._bad(256, f"an image of {W} x {H} pixels")
        if H * W > MAX_PIXELS:
            raise sc._bad(257, f"{H} x {W} pixels are more than 2^31 - 1")
        if not 1 <= C <= MAX_BANDS:
            raise sc._bad(277, f"{C} samples per pixel (1 to {MAX_BANDS} are read)")
        bits = tuple(int(b) for b in tags[258][2]) if 258 in tags else (1,)
        if len(bits) not in (1, C) or len(set(bits)) != 1:
            raise sc._bad(258, f"{bits}: all samples must share one format")
        fmts = tuple(int(b) for b in tags[339][2]) if 339 in tags else (1,)
        if len(set(fmts)) != 1:
            raise sc._bad(339, f"{fmts}: all samples must share one format")
        bits, fmt = bits[0], fmts[0]
        if fmt == 4:                                           # "undefined": treated as unsigned, as libtiff does
            fmt = 1
        if fmt == 2:
            raise sc._bad(339, "signed integers are not read (8- or 16-bit unsigned, or 32-bit float)")
        if fmt == 1 and bits in (8, 16):
            dtype = np.dtype(np.uint8 if bits == 8 else np.uint16)
        elif fmt == 3 and bits == 32:
            dtype = np.dtype(np.float32)
        elif fmt == 3:
            raise sc._bad(258, f"{bits}-bit floats are not read (float32 only)")
        elif fmt == 1:
            raise sc._bad(258, f"{bits}-bit integers are not read (8 or 16 bits)")
        else:
            raise sc._bad(339, f"sample format {fmt} is not read")
        comp = one(259, 1)
        if comp not in (1, 5, 8, 32946):
            raise sc._bad(259, f"{_COMPRESSIONS.get(comp, 'compression ' + str(comp))} is not read (none, LZW and deflate are)")
        photo = one(262, 1 if C < 3 else 2)
        if photo not in (1, 2):
            raise sc._bad(262, f"{'a palette' if photo == 3 else 'photometric interpretation ' + str(photo)} is not read (BlackIsZero and RGB are)")
        if one(266, 1) != 1:
            raise sc._bad(266, "bit-reversed bytes are not read")
        planar = one(284, 1)
        if planar not in (1, 2):
            raise sc._bad(284, f"planar configuration {planar}")
        if C == 1:
            planar = 1                                         # one band: the two layouts are the same bytes
        pred = one(317, 1)
        if pred not in (1, 2, 3) or (pred == 2 and fmt != 1) or (pred == 3 and fmt != 3):
            raise sc._bad(317, f"predictor {pred} with {dtype} samples (1; 2 with integers; 3 with floats)")
        sc.shape, sc.dtype, sc.little, sc.big = (H, W, C), dtype, bo == "<", big
        sc.compression, sc.predictor, sc.planar = (8 if comp == 32946 else comp), pred, planar
        sc.tiled = 322 in tags or 324 in tags
        planes = C if planar == 2 else 1
        if sc.tiled:
            sc.tile_w, sc.tile_h = one(322), one(323)
            if sc.tile_w < 16 or sc.tile_h < 16 or sc.tile_w % 16 or sc.tile_h % 16 or sc.tile_w > 2 ** 20 or sc.tile_h > 2 ** 20:
                raise sc._bad(322, f"tiles of {sc.tile_w} x {sc.tile_h} (multiples of 16)")
            n_seg = planes * ((W + sc.tile_w - 1) // sc.tile_w) * ((H + sc.tile_h - 1) // sc.tile_h)
            t_off, t_cnt = 324, 325
        else:
            rps = one(278, 2 ** 32 - 1)
            sc.rows_per_strip = H if rps < 1 or rps > H else rps
            n_seg = planes * ((H + sc.rows_per_strip - 1) // sc.rows_per_strip)
            t_off, t_cnt = 273, 279
        for t in (t_off, t_cnt):
            if t not in tags or isinstance(tags[t][2], bytes):
                raise sc._bad(t, "the tag is missing")
            if len(tags[t][2]) != n_seg:
                raise sc._bad(t, f"{len(tags[t][2])} entries for {n_seg} segments")
        sc.offsets, sc.counts = [int(v) for v in tags[t_off][2]], [int(v) for v in tags[t_cnt][2]]
        for k in range(n_seg):
            if sc.offsets[k] < 8 or sc.counts[k] < 0 or sc.offsets[k] + sc.counts[k] > size:
                raise sc._bad(t_off, f"segment {k} (offset {sc.offsets[k]}, {sc.counts[k]} bytes) leaves the file ({size} bytes)")
            need = sc.seg_geometry(k)[5]
            if comp == 1 and sc.counts[k] < need:
                raise sc._bad(t_cnt, f"segment {k} holds {sc.counts[k]} bytes, {need} are needed")
            if comp != 1 and sc.counts[k] < 2:
                raise sc._bad(t_cnt, f"segment {k} holds {sc.counts[k]} bytes: not a compressed stream")
        if comp == 5:                                          # the bit-reversed LZW of very old writers starts with the clear code, low bits first
            fh.seek(sc.offsets[0])
            b = fh.read(2)
            if b[0] == 0 and b[1] & 1:
                raise sc._bad(259, "old-style LZW (codes stored low bit first) is not read")
    sc.geo_tags = {t: tags[t] for t in GEO_TAGS if t in tags}
    sc.nodata = _nodata_of(tags.get(NODATA_TAG))
    sc.geotransform = _geotransform_of(sc.geo_tags)
    return sc


def _nodata_of(entry):
    if entry is None or not isinstance(entry[2], bytes):
        return None
    try:
        return float(entry[2].split(b"\0")[0].decode("ascii").strip())
    except (ValueError, UnicodeDecodeError):
        return None


def _geotransform_of(geo):
    point = False
    if 34735 in geo:
        d = geo[34735][2]
        if not isinstance(d, bytes) and len(d) >= 4:
            for k in range(min(int(d[3]), (len(d) - 4) // 4)):
                key, loc, _, value = d[4 + 4 * k:8 + 4 * k]
                if key == 1025 and loc == 0 and value == 2:
                    point = True
    g = None
    if 34264 in geo and len(geo[34264][2]) == 16:
        m = [float(v) for v in geo[34264][2]]
        g = [m[3], m[0], m[1], m[7], m[4], m[5]]
    elif 33550 in geo and 33922 in geo and len(geo[33550][2]) >= 2 and len(geo[33922][2]) >= 6:
        sx, sy = float(geo[33550][2][0]), float(geo[33550][2][1])
        i, j, _, x, y = (float(v) for v in geo[33922][2][:5])
        g = [x - i * sx, sx, 0.0, y + j * sy, 0.0, -sy]
    if g is not None and point:
        g[0] -= 0.5 * g[1] + 0.5 * g[2]
        g[3] -= 0.5 * g[4] + 0.5 * g[5]
    return None if g is None else tuple(g)


# ---- the reference decoder -----------------------------------------------------------------------------------------------------------------
def lzw_decode_ref(data, nbytes):
    """TIFF LZW (MSB first, early change) in plain Python: exactly nbytes bytes or a ValueError.  Slow; for the tests."""
    out = bytearray()
    table = [bytes([i]) for i in range(256)] + [b"", b""]
    width, prev, pos, nbits_total = 9, None, 0, 8 * len(data)
    while len(out) < nbytes:
        if pos + width > nbits_total:
            raise ValueError("the LZW stream ends early")
        byte, shift = pos >> 3, pos & 7
        word = int.from_bytes(data[byte:byte + 4].ljust(4, b"\0"), "big")
        code = (word >> (32 - shift - width)) & ((1 << width) - 1)
        pos += width
        if code == 257:
            break
        if code == 256:
            table, width, prev = table[:258], 9, None
            continue
        if prev is None:
            if code > 255:
                raise ValueError("the LZW stream is damaged")
            entry = table[code]
        else:
            if code < len(table):
                entry = table[code]
            elif code == len(table):
                entry = prev + prev[:1]
            else:
                raise ValueError("the LZW stream is damaged")
            if len(table) < 4096:
                table.append(prev + entry[:1])
        out += entry
        prev = entry
        if len(table) >= (1 << width) - 1 and width < 12:
            width += 1
    if len(out) != nbytes:
        raise ValueError(f"the LZW stream holds {len(out)} bytes, {nbytes} expected")
    return bytes(out)


def _undo(scene, seg, rows, cols, S):
    """One decompressed segment -> its samples [rows, cols, S] in the native byte order: byte swap, then the predictor."""
    dt = scene.dtype
    if scene.predictor == 3:
        b = np.frombuffer(seg, np.uint8, rows * cols * S * 4).reshape(rows, cols * 4, S)
        b = np.cumsum(b, axis=1, dtype=np.uint8).reshape(rows, 4, cols * S).astype(np.uint32)
        bits = (b[:, 0] << 24) | (b[:, 1] << 16) | (b[:, 2] << 8) | b[:, 3]
        return bits.view(np.float32).reshape(rows, cols, S)
    a = np.frombuffer(seg, dt.newbyteorder("<" if scene.little else ">"), rows * cols * S).astype(dt).reshape(rows, cols, S)
    if scene.predictor == 2:
        a = np.cumsum(a, axis=1, dtype=dt)
    return a


def _place(scene, out, a, r0, c0, band):
    H, W, _ = scene.shape
    rr, cc = min(a.shape[0], H - r0), min(a.shape[1], W - c0)
    if band < 0:
        out[r0:r0 + rr, c0:c0 + cc, :] = a[:rr, :cc]
    else:
        out[r0:r0 + rr, c0:c0 + cc, band] = a[:rr, :cc, 0]


def tiff_read_ref(path):
    """The reference decoder: a path or a TiffScene -> the raster [H, W, C] in the file's sample type.  zlib, the Python LZW above and
    numpy.cumsum in the sample's own dtype; what srh_tiff_assemble must equal bit for bit (floats as uint32 bit patterns)."""
    sc = path if isinstance(path, TiffScene) else open_scene(path)
    out = np.zeros(sc.shape, sc.dtype)
    with open(sc.path, "rb") as fh:
        for k in range(len(sc.offsets)):
            r0, c0, rows, cols, band, nbytes = sc.seg_geometry(k)
            data = sc._read_segment(fh, k)
            if sc.compression == 8:
                data = _inflate(data, nbytes, sc.path, k)
            elif sc.compression == 5:
                try:
                    data = lzw_decode_ref(data, nbytes)
                except ValueError as e:
                    raise ValueError(f"{sc.path}: segment {k}: {e}") from None
            _place(sc, out, _undo(sc, data, rows, cols, 1 if band >= 0 else sc.shape[2]), r0, c0, band)
    return out


def assemble_ref(scene, flat, table):
    """What the device step does with segments()' output, restated in numpy: the raster [H, W, C]."""
    out = np.zeros(scene.shape, scene.dtype)
    for off, nbytes, r0, c0, rows, cols, band in np.asarray(table).tolist():
        _place(scene, out, _undo(scene, flat[off:off + nbytes].tobytes(), rows, cols, 1 if band >= 0 else scene.shape[2]), r0, c0, band)
    return out


def check_table(scene, flat_bytes, table):
    """The invariants srh_tiff_assemble relies on, for a table that did not come from segments(): ValueError otherwise."""
    H, W, C = scene.shape
    t = np.asarray(table)
    if t.ndim != 2 or t.shape[1] != TABLE_COLS or t.dtype != np.int64 or t.shape[0] < 1:
        raise ValueError(f"the segment table is int64 [n, {TABLE_COLS}], got {t.dtype} {t.shape}")
    for off, nbytes, r0, c0, rows, cols, band in t.tolist():
        S = 1 if band >= 0 else C
        if off < 0 or off % ALIGN or off + nbytes > flat_bytes or nbytes != rows * cols * S * scene.dtype.itemsize:
            raise ValueError("a segment leaves the flat array, is misaligned or has another size than its rows and columns")
        if not (0 <= r0 < H and 0 <= c0 < W and rows >= 1 and cols >= 1 and -1 <= band < C):
            raise ValueError("a segment lies outside the raster")
    return t


# ---- the writer ----------------------------------------------------------------------------------------------------------------------------
def geo_tags_from(geotransform):
    """Six numbers -> the geo tags that say them: ModelTransformation and a GeoKeyDirectory that names RasterPixelIsArea."""
    g = [float(v) for v in geotransform]
    if len(g) != 6:
        raise ValueError(f"a geotransform is six numbers, got {len(g)}")
    m = (g[1], g[2], 0.0, g[0], g[4], g[5], 0.0, g[3], 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0)
    return {34264: (12, 16, m), 34735: (3, 8, (1, 1, 0, 1, 1025, 0, 1, 1))}


def write_geotiff(path, arr, like=None, geotransform=None, nodata=None):
    """uint8 / uint16 [H, W] or [H, W, C] -> a little-endian classic TIFF: strips, deflate level 1, predictor 2.  The geo tags are copied
    verbatim from `like` (a TiffScene), or built from the six numbers of `geotransform`; nodata becomes tag 42113."""
    a = np.asarray(arr)
    if a.ndim == 2:
        a = a[:, :, None]
    if a.ndim != 3 or a.dtype not in (np.dtype(np.uint8), np.dtype(np.uint16)) or not 1 <= a.shape[2] <= MAX_BANDS or a.shape[0] < 1 or a.shape[1] < 1:
        raise ValueError(f"write_geotiff writes uint8 / uint16 [H, W] or [H, W, C <= {MAX_BANDS}], got {a.dtype} {a.shape}")
    if like is not None and geotransform is not None:
        raise ValueError("write_geotiff takes like or geotransform, not both")
    H, W, C = a.shape
    a = np.ascontiguousarray(a).astype(a.dtype.newbyteorder("<"), copy=False)
    rps = max(1, min(H, (1 << 18) // (W * C * a.dtype.itemsize)))
    diff = a.copy()
    diff[:, 1:] -= a[:, :-1]                                   # wrapping, in the sample's own width
    strips = [zlib.compress(diff[r:r + rps].tobytes(), 1) for r in range(0, H, rps)]
    geo = dict(like.geo_tags) if like is not None else geo_tags_from(geotransform) if geotransform is not None else {}
    ents = {256: (4, 1, (W,)), 257: (4, 1, (H,)), 258: (3, C, (8 * a.dtype.itemsize,) * C), 259: (3, 1, (8,)), 262: (3, 1, (2 if C >= 3 else 1,)),
            277: (3, 1, (C,)), 278: (4, 1, (rps,)), 279: (4, len(strips), tuple(len(s) for s in strips)), 284: (3, 1, (1,)), 317: (3, 1, (2,)),
            339: (3, C, (1,) * C)}
    extra = C - 3 if C >= 3 else C - 1
    if extra:
        ents[338] = (3, extra, (0,) * extra)
    ents.update(geo)
    if nodata is not None:
        s = (repr(int(nodata)) if float(nodata).is_integer() else repr(float(nodata))).encode("ascii") + b"\0"
        ents[NODATA_TAG] = (2, len(s), s)
    ents[273] = (4, len(strips), (0,) * len(strips))           # placeholder: the layout below fixes the offsets
    n = len(ents)
    ifd_off, pos = 8, 8 + 2 + 12 * n + 4
    blobs, where = [], {}
    for tag in sorted(ents):
        typ, count, vals = ents[tag]
        size = _TYPES[typ][1] * count
        if size > 4:
            pos += pos & 1
            where[tag] = pos
            pos += size
    pos += pos & 1
    offs = []
    for s in strips:
        offs.append(pos)
        pos += len(s) + (len(s) & 1)
    if pos > 2 ** 32 - 1:
        raise ValueError("write_geotiff writes classic TIFF files: the image does not fit 4 GiB")
    ents[273] = (4, len(strips), tuple(offs))

    def pack(typ, count, vals):
        if typ in (2, 7):
            return bytes(vals)
        flat = [x for v in vals for x in (v if isinstance(v, tuple) else (v,))] if typ in (5, 10) else list(vals)
        return struct.pack("<" + _TYPES[typ][0][0] * len(flat), *flat)
    out = bytearray(b"II" + struct.pack("<HI", 42, ifd_off) + struct.pack("<H", n))
    for tag in sorted(ents):
        typ, count, vals = ents[tag]
        data = pack(typ, count, vals)
        if tag in where:
            out += struct.pack("<HHII", tag, typ, count, where[tag])
            blobs.append((where[tag], data))
        else:
            out += struct.pack("<HHI", tag, typ, count) + data.ljust(4, b"\0")
    out += struct.pack("<I", 0)
    for off, data in blobs:
        out += b"\0" * (off - len(out)) + data
    for off, s in zip(offs, strips):
        out += b"\0" * (off - len(out)) + s
    with open(path, "wb") as fh:
        fh.write(out)
