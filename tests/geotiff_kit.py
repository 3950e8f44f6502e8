"""Shared by the GEOTIFF tests: a small TIFF WRITER that covers everything sam_road_amd/geotiff.py reads — strips with any
rows-per-strip, tiles in multiples of 16, both planar configurations, both byte orders, classic TIFF and BigTIFF, no compression / LZW /
deflate, predictors 1 / 2 / 3, geo tags and tag 42113 — sample rasters, and the scene-level stand-in of the device step.  The writer shares
no code with the reader: it imports nothing of sam_road_amd.geotiff and states the predictors and the LZW coder on its own."""
import struct
import zlib

import numpy as np
import torch

CHUNK = 4096            # = TIF_CHUNK of csrc/geotiff_piece.hpp: the elements of a row a workgroup scans at a time
PAD_BYTE = 0xA5         # what the padding of edge tiles holds: it must never reach the raster

GEO = {33550: (12, (0.5, 0.25, 0.0)), 33922: (12, (0.0, 0.0, 0.0, 431000.0, 5512000.0, 0.0)),
       34735: (3, (1, 1, 0, 3, 1024, 0, 1, 1, 1025, 0, 1, 1, 3072, 0, 1, 32632)), 34737: (2, b"WGS 84 / UTM zone 32N|\0")}
GEO_TRANSFORM = (431000.0, 0.5, 0.0, 5512000.0, 0.0, -0.25)

_FMT = {1: "B", 3: "H", 4: "I", 11: "f", 12: "d", 16: "Q"}
_SIZE = {1: 1, 2: 1, 3: 2, 4: 4, 7: 1, 11: 4, 12: 8, 16: 8}


def lzw_encode(data):
    """TIFF LZW, MSB first, early change, as libtiff writes it: a clear code first, a clear when entry 4093 has been made, the end code.
    The table is keyed by (code of the prefix) * 256 + next byte."""
    out, acc, nacc = bytearray(), 0, 0
    width, nxt, table = 9, 258, {}
    acc, nacc = 256, 9                                        # the clear code
    w = -1
    for b in bytes(data):
        if w < 0:
            w = b
            continue
        key = (w << 8) | b
        code = table.get(key)
        if code is not None:
            w = code
            continue
        acc, nacc = (acc << width) | w, nacc + width
        table[key] = nxt
        nxt += 1
        if nxt == 4094:
            acc, nacc = (acc << width) | 256, nacc + width
            width, nxt, table = 9, 258, {}
        elif nxt > (1 << width) - 1:
            width += 1
        while nacc >= 8:
            nacc -= 8
            out.append((acc >> nacc) & 0xFF)
        acc &= (1 << nacc) - 1
        w = b
    if w >= 0:
        acc, nacc = (acc << width) | w, nacc + width
        nxt += 1
        if nxt == 4094:
            acc, nacc = (acc << width) | 256, nacc + width
            width = 9
        elif nxt > (1 << width) - 1:
            width += 1
    acc, nacc = (acc << width) | 257, nacc + width
    while nacc >= 8:
        nacc -= 8
        out.append((acc >> nacc) & 0xFF)
    if nacc:
        out.append((acc << (8 - nacc)) & 0xFF)
    return bytes(out)


def _encode_block(block, predictor, big_endian):
    """[rows, cols, S] samples -> the bytes a TIFF stores for them, before compression."""
    rows, cols, S = block.shape
    if predictor == 3:
        be = block.astype(">f4").view(np.uint8).reshape(rows, cols * S, 4)             # most significant byte first, whatever the file's order
        planes = np.ascontiguousarray(be.transpose(0, 2, 1)).reshape(rows, 4 * cols * S)
        d = planes.copy()
        d[:, S:] = planes[:, S:] - planes[:, :-S]
        return d.tobytes()
    if predictor == 2:
        d = block.copy()
        d[:, 1:] = block[:, 1:] - block[:, :-1]
        block = d
    return block.astype(block.dtype.newbyteorder(">" if big_endian else "<")).tobytes()


def write_tiff(path, arr, compression="none", predictor=1, planar=1, big_endian=False, bigtiff=False, rows_per_strip=None, tile=None, geo=None,
               nodata=None, override=None, drop=()):
    """arr uint8 / uint16 / float32 [H, W] or [H, W, C] -> a TIFF.  tile = (rows, cols); geo = {tag: (type, values)}; override = {tag:
    (type, values)} replaces or adds raw tags (to write files the reader must refuse); drop = tags to leave out."""
    a = np.asarray(arr)
    a = a[:, :, None] if a.ndim == 2 else a
    H, W, C = a.shape
    bands = [a[:, :, b:b + 1] for b in range(C)] if planar == 2 and C > 1 else [a]
    segs = []
    for img in bands:
        if tile is not None:
            th, tw = tile
            for r in range(0, H, th):
                for c in range(0, W, tw):
                    blk = np.frombuffer(bytes([PAD_BYTE]) * (th * tw * img.shape[2] * a.dtype.itemsize), a.dtype).reshape(th, tw, img.shape[2]).copy()
                    part = img[r:r + th, c:c + tw]
                    blk[:part.shape[0], :part.shape[1]] = part
                    segs.append(blk)
        else:
            rps = H if rows_per_strip is None else rows_per_strip
            segs += [np.ascontiguousarray(img[r:r + rps]) for r in range(0, H, rps)]
    raw = [_encode_block(s, predictor, big_endian) for s in segs]
    packed = [r if compression == "none" else lzw_encode(r) if compression == "lzw" else zlib.compress(r, 6) for r in raw]
    code = {"none": 1, "lzw": 5, "deflate": 8, "deflate-old": 32946}[compression]
    bo = ">" if big_endian else "<"
    off_t = 16 if bigtiff else 4
    bits = 8 * a.dtype.itemsize
    tags = {256: (4, (W,)), 257: (4, (H,)), 258: (3, (bits,) * C), 259: (3, (code,)), 262: (3, (2 if C >= 3 else 1,)), 277: (3, (C,)),
            284: (3, (planar,)), 339: (3, (3 if a.dtype.kind == "f" else 1,) * C)}
    if predictor != 1:
        tags[317] = (3, (predictor,))
    extra = C - 3 if C >= 3 else C - 1
    if extra:
        tags[338] = (3, (0,) * extra)
    if tile is not None:
        tags.update({322: (3, (tile[1],)), 323: (3, (tile[0],)), 324: (off_t, (0,) * len(packed)), 325: (off_t, tuple(len(p) for p in packed))})
    else:
        tags.update({278: (4, (H if rows_per_strip is None else rows_per_strip,)), 273: (off_t, (0,) * len(packed)), 279: (off_t, tuple(len(p) for p in packed))})
    tags.update(geo or {})
    if nodata is not None:
        tags[42113] = (2, str(nodata).encode("ascii") + b"\0")
    tags.update(override or {})
    for t in drop:
        tags.pop(t, None)
    head = 16 if bigtiff else 8
    ent, inline = (20, 8) if bigtiff else (12, 4)
    pos = head + (8 if bigtiff else 2) + ent * len(tags) + (8 if bigtiff else 4)

    def size_of(typ, vals):
        return len(vals) if typ in (2, 7) else _SIZE[typ] * len(vals)
    where = {}
    for t in sorted(tags):
        if size_of(*tags[t]) > inline:
            pos += pos & 1
            where[t] = pos
            pos += size_of(*tags[t])
    offs = []
    for p in packed:
        pos += pos & 1
        offs.append(pos)
        pos += len(p)
    key = 324 if tile is not None else 273
    if key in tags and not (override and key in override):
        tags[key] = (off_t, tuple(offs))
    out = bytearray((b"MM" if big_endian else b"II") + (struct.pack(bo + "HHHQ", 43, 8, 0, head) if bigtiff else struct.pack(bo + "HI", 42, head)))
    out += struct.pack(bo + ("Q" if bigtiff else "H"), len(tags))
    blobs = []
    for t in sorted(tags):
        typ, vals = tags[t]
        data = bytes(vals) if typ in (2, 7) else struct.pack(bo + _FMT[typ] * len(vals), *vals)
        count = len(vals)
        out += struct.pack(bo + "HH" + ("Q" if bigtiff else "I"), t, typ, count)
        if t in where:
            out += struct.pack(bo + ("Q" if bigtiff else "I"), where[t])
            blobs.append((where[t], data))
        else:
            out += data.ljust(inline, b"\0")
    out += struct.pack(bo + ("Q" if bigtiff else "I"), 0)
    for off, data in blobs + list(zip(offs, packed)):
        out += b"\0" * (off - len(out)) + data
    with open(path, "wb") as fh:
        fh.write(out)
    return path


# ---- rasters -------------------------------------------------------------------------------------------------------------------------------
FLOAT_SPECIALS = np.array([0x7FC00001, 0xFFC12345, 0x7F800000, 0xFF800000, 0x80000000, 0x00000001, 0x807FFFFF, 0x7F7FFFFF, 0x7FA00000], np.uint32)


def sample(shape, dtype, seed):
    """A raster [H, W, C] of the dtype: full-range random integers; floats of every magnitude with NaNs (two payloads, one of them
    signalling), +-inf, -0.0 and denormals sprinkled in, so a decoder that goes through float arithmetic shows."""
    rng = np.random.default_rng(seed)
    H, W, C = shape
    dt = np.dtype(dtype)
    if dt.kind == "u":
        return rng.integers(0, 2 ** (8 * dt.itemsize), size=shape, dtype=np.uint64).astype(dt)
    bits = rng.integers(0, 2 ** 32, size=shape, dtype=np.uint64).astype(np.uint32)
    bits[(bits & 0x7F800000) == 0x7F800000] &= 0xBFFFFFFF        # no accidental NaN / inf: the special values are placed on purpose
    flat = bits.reshape(-1)
    idx = rng.permutation(flat.size)[:min(flat.size, 4 * len(FLOAT_SPECIALS))]
    flat[idx] = np.resize(FLOAT_SPECIALS, idx.size)
    return bits.view(np.float32)


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    return np.array_equal(a.view(np.uint32), b.view(np.uint32)) if a.dtype == np.float32 else np.array_equal(a, b)


# ---- the stand-in --------------------------------------------------------------------------------------------------------------------------
class TiffAssembleMixin:
    """tiff_assemble of the model's scene interface on the CPU: the numpy restatement of the device step (geotiff.assemble_ref), logged."""

    def tiff_assemble(self, scene, flat, table, table_dev=None):
        from sam_road_amd.geotiff import assemble_ref
        assert flat.dtype == torch.uint8 and flat.dim() == 1 and (table_dev is None or np.array_equal(table_dev.numpy(), table))
        self.calls.append(("tiff_assemble", tuple(scene.shape), str(scene.dtype), int(table.shape[0])))
        return torch.from_numpy(assemble_ref(scene, flat.numpy(), table))


def tiff_calls(net):
    return [c for c in net.calls if c[0] == "tiff_assemble"]
