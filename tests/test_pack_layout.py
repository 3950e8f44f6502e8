"""The packed weight layout on the CPU: tests/pack_layout_check.cpp packs a small model with the host-only packer
(sam_road_amd/csrc/pack_host.hpp) and compares the arena image with the layouts' definitions.  Needs a host compiler with _Float16:
the ROCm clang++."""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "sam_road_amd", "csrc")


def _clangxx():
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    for cand in (os.path.join(rocm, "llvm", "bin", "clang++"), os.path.join(rocm, "lib", "llvm", "bin", "clang++")):
        if os.path.exists(cand):
            return cand
    return None


def test_pack_layout(tmp_path):
    cxx = _clangxx()
    if cxx is None:
        pytest.skip("no ROCm clang++ (the host-only packer needs _Float16)")
    exe = str(tmp_path / "pack_layout_check")
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-I", CSRC, os.path.join(HERE, "pack_layout_check.cpp"), "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "pack layout OK" in r.stdout
