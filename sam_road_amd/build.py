"""Build libsamroad_hip.so for gfx950 in-tree with hipcc (no torch extension machinery: the
library is a plain C-ABI shared object, see include/samroad_hip.h)."""
import hashlib
import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
LIB = os.path.join(HERE, "libsamroad_hip.so")
SOURCES = ["api_ctx.hip", "api_weights.hip", "api_model.hip", "api_scene.hip", "api_ops.hip", "gemm.hip", "gemm_z192.hip", "norm.hip", "patch.hip", "attention.hip", "attention_hdx.hip", "decoder.hip", "scene_valid.hip", "scene_window.hip", "scene_tta.hip", "scene_pad.hip", "scene_group.hip", "scene_bands.hip", "scene_scale.hip", "mask_clean.hip", "scene_nodata.hip", "scene_aoi.hip", "scene_float.hip", "graph_raster.hip", "edge_support.hip", "road_width.hip", "graph_clean.hip", "scene_tiff.hip", "sam_decoder.hip", "topo.hip", "topo_fused.hip", "host_geom.hip"]
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Wall", "-Wno-unused-function", "-Wno-unused-value", "-Wno-unused-result"]

# The softmax row maxima are taken over MFMA results; without this flag every fmaxf operand gets a v_max x, x to quiet a
# possible signalling NaN first (16 extra VALU instructions per 64 keys in a VALU-bound loop).  No NaN arises in these kernels
# (-inf - finite and exp2(-inf) are fine); infinities ARE used, so no -ffinite-math-only.
# PRECONDITION this puts on the callers: q / k / v must be finite.  A NaN already in qkv16 (an fp16 overflow upstream) would no longer
# propagate deterministically through fmaxf / the online softmax; every whole-model test asserts finite outputs (tests/test_gpu_*.py:
# torch.isfinite on embeddings and masks, incl. the heavy-tailed-weights cases that push fp16 hardest), which is where such an input would show.
FILE_FLAGS = {"attention.hip": ["-fno-honor-nans"], "attention_hdx.hip": ["-fno-honor-nans"]}


def _hipcc():
    for cand in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", "hipcc"):
        if cand and (os.path.isabs(cand) and os.path.exists(cand) or not os.path.isabs(cand)):
            return cand
    return "hipcc"


_MARK = b"SRH_BUILD_ID="


def source_id():
    """sha256 over every file the library is built from (csrc/*, the public header, the flags), 16 hex digits.  It is compiled
    into the library (srh_build_id()), so "is this .so the build of THESE sources" is a content check, not an mtime guess."""
    h = hashlib.sha256()
    files = sorted(os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith((".hip", ".hpp", ".h", ".inc")))
    files.append(os.path.join(HERE, "..", "include", "samroad_hip.h"))
    for f in files:
        h.update(os.path.basename(f).encode() + b"\0")
        with open(f, "rb") as fh:
            h.update(fh.read())
        h.update(b"\0")
    h.update(" ".join(FLAGS + SOURCES + [f"{k}:{' '.join(v)}" for k, v in sorted(FILE_FLAGS.items())]).encode())
    return h.hexdigest()[:16]


def library_id(path=LIB):
    """The build id embedded in a built library (read from the file: no dlopen, so a stale library is never mapped)."""
    try:
        with open(path, "rb") as fh:
            data = fh.read()
    except OSError:
        return None
    i = data.find(_MARK)
    return data[i + len(_MARK): i + len(_MARK) + 16].decode("ascii", "replace") if i >= 0 else None


def needs_build():
    return library_id() != source_id()


def build(force=False, verbose=True):
    if not force and not needs_build():
        return LIB
    sid = source_id()
    objdir = os.path.join(HERE, "build")
    os.makedirs(objdir, exist_ok=True)
    hipcc = _hipcc()

    def compile_one(src):
        obj = os.path.join(objdir, src.replace(".hip", ".o"))
        cmd = [hipcc] + FLAGS + FILE_FLAGS.get(src, []) + [f'-DSRH_BUILD_ID_HEX="{sid}"', "-c", os.path.join(CSRC, src), "-o", obj]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError(f"hipcc failed for {src}:\n{r.stderr}")
        if verbose and r.stderr.strip():
            print(r.stderr, file=sys.stderr)
        return obj

    with ThreadPoolExecutor(max_workers=8) as ex:
        objs = list(ex.map(compile_one, SOURCES))
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", LIB] + objs,
                       capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError(f"link failed:\n{r.stderr}")
    if library_id() != sid:
        raise RuntimeError(f"built library carries build id {library_id()}, expected {sid}")
    return LIB


if __name__ == "__main__":
    print(build(force="--force" in sys.argv))
