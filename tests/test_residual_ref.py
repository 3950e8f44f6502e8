"""CPU checks of tests/residual_ref.py, the references tests/test_gpu_residual.py compares the residual-stream kernels with: the float64
LayerNorm is pinned to F.layer_norm, the seeded inputs are shown to tell a fold in the wrong order from the right one (with the
reference alone: a wrong reference or inputs that cannot discriminate fail here, on any host), and the C ABI has the test-only entries."""
import ctypes as C
import os
import re

import pytest
import torch
import torch.nn.functional as F

import residual_ref as R
from sam_road_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MIN_DIFFERENT = 0.01         # fraction of the elements on which two orders of the same sum must differ in bits


def _different(a, b):
    assert a.dtype == b.dtype == torch.float32 and a.shape == b.shape
    return (a.view(torch.int32) != b.view(torch.int32)).float().mean().item()


@pytest.mark.parametrize("D,gelu", [(128, True), (256, False), (768, False), (1280, True)])
def test_layernorm64_is_layer_norm(D, gelu):
    t = R.make_inputs(517, D, seed=D)
    x = R.fold_branches(t["x"], t["d1"], t["d2"])
    want = F.layer_norm(x.double(), (D,), t["gamma"].double(), t["beta"].double(), 1e-6)
    if gelu:
        want = F.gelu(want)
    got = R.layernorm64(x, t["gamma"], t["beta"], 1e-6, gelu)
    assert got.dtype == torch.float64
    assert (got - want).abs().max().item() < 1e-12
    # and float32 F.layer_norm, what the op tests compared with so far, is this to float32 rounding
    want32 = F.layer_norm(x, (D,), t["gamma"], t["beta"], 1e-6)
    assert (got - (F.gelu(want32) if gelu else want32).double()).abs().max().item() < 2e-5


def test_fold_is_one_float32_add_per_step():
    """The fold against float64 sums rounded once per step: binary32 + binary32 is exact in float64, so rounding that sum to float32 is
    the IEEE float32 add; an fp16 value converts exactly."""
    t = R.make_inputs(517, 256, seed=1, nslices=3)
    step1 = (t["x"].double() + t["d1"].double()).float()
    assert R.same_bits(R.fold_branches(t["x"], t["d1"]), step1)
    assert R.same_bits(R.fold_branches(t["x"], t["d1"], t["d2"]), (step1.double() + t["d2"].double()).float())
    s = t["slices"]
    a = (s[0].double() + s[1].double()).float()
    a = (a.double() + s[2].double()).float()
    a = (a.double() + t["bias"].double()).float()
    assert R.same_bits(R.fold_slices(t["x"], s, t["bias"]), (a.double() + t["x"].double()).float())
    # one slice: (s0 + bias) + x
    assert R.same_bits(R.fold_slices(t["x"], s[:1], t["bias"]), ((s[0] + t["bias"]) + t["x"]))


def test_fold_reads_x_through_the_period():
    M, D, period = 3 * 64 + 5, 128, 64
    t = R.make_inputs(M, D, seed=2, period=period)
    assert t["x"].shape == (period, D)
    got = R.fold_branches(t["x"], t["d1"], period=period)
    for m in (0, 63, 64, 65, 191, 192, M - 1):
        assert R.same_bits(got[m], t["x"][m % period] + t["d1"][m].float())
    off_by_one = t["x"][torch.arange(M) % (period - 1)] + t["d1"].float()
    assert _different(got, off_by_one) > 0.5


@pytest.mark.parametrize("D", [128, 256, 768, 1024, 1280])
def test_inputs_tell_the_branch_orders_apart(D):
    t = R.make_inputs(517, D, seed=D)
    right = R.fold_branches(t["x"], t["d1"], t["d2"])
    swapped = R.fold_branches(t["x"], t["d2"], t["d1"])
    frac = _different(right, swapped)
    print(f"(x + d1) + d2 vs (x + d2) + d1 at D = {D}: {frac:.3f} of the elements differ in bits")
    assert frac >= MIN_DIFFERENT
    # ... although they are the same sum to about one ulp: a tolerance would not see the swap
    assert ((right - swapped).abs() / right.abs().clamp(min=1.0)).max().item() < 4 * 2.0 ** -23
    # dropping a branch, or a branch with permuted rows / columns, is another x' altogether
    assert _different(right, R.fold_branches(t["x"], t["d1"])) > 0.9
    assert _different(right, R.fold_branches(t["x"], t["d1"].roll(1, 0), t["d2"])) > 0.9
    assert _different(right, R.fold_branches(t["x"], t["d1"], t["d2"].roll(1, 1))) > 0.9


@pytest.mark.parametrize("D", [1024, 1280])
@pytest.mark.parametrize("nslices", [2, 3, 4])
def test_inputs_tell_the_slice_orders_apart(D, nslices):
    t = R.make_inputs(517, D, seed=D + nslices, nslices=nslices)
    x, s, b = t["x"], t["slices"], t["bias"]
    right = R.fold_slices(x, s, b)
    a = s[0] + b                                   # the bias before slice 1: ((s0 + b) + s1 + ...) + x
    for z in range(1, nslices):
        a = a + s[z]
    frac = _different(right, a + x)
    print(f"bias after the slices vs before slice 1 at D = {D}, {nslices} slices: {frac:.3f} differ")
    assert frac >= MIN_DIFFERENT
    if nslices >= 3:                               # right-associated slices: s0 + (s1 + (s2 + ...))
        a = s[nslices - 1]
        for z in range(nslices - 2, -1, -1):
            a = s[z] + a
        frac = _different(right, (a + b) + x)
        print(f"ascending slices vs s0 + (s1 + ...) at D = {D}, {nslices} slices: {frac:.3f} differ")
        assert frac >= MIN_DIFFERENT
    # x before the bias: ((s0 + s1 + ...) + x) + b
    a = s[0]
    for z in range(1, nslices):
        a = a + s[z]
    assert _different(right, (a + x) + b) >= MIN_DIFFERENT
    # a slice left out, or two slices swapped where the order matters (three or more)
    assert _different(right, R.fold_slices(x, s[:-1], b)) > 0.9
    if nslices >= 3:
        assert _different(right, R.fold_slices(x, s[[0, 2, 1] + list(range(3, nslices))], b)) >= MIN_DIFFERENT


def test_same_bits_is_strict():
    z = torch.zeros(4)
    assert R.same_bits(z, z.clone()) and not R.same_bits(z, -z)
    n = torch.full((4,), float("nan"))
    assert R.same_bits(n, n.clone()) and not torch.equal(n, n.clone())
    assert not R.same_bits(z, z.half())


def test_abi_has_the_residual_entries_and_stays_11():
    header = open(os.path.join(ROOT, "include", "samroad_hip.h")).read()
    lib = _lib.load()
    assert lib.srh_abi_version() == _lib.ABI_VERSION == int(re.search(r"#define SRH_ABI_VERSION (\d+)", header).group(1)) == 11
    for name, n_args in (("srh_op_layernorm_ex", 3), ("srh_op_gemm_partials", 10), ("srh_op_gemm_pos", 11)):
        assert hasattr(lib, name) and len(_lib.SYMBOLS[name][1]) == n_args
        decl = re.search(r"\bint %s\(([^;]*)\);" % name, header).group(1)
        assert len(decl.split(",")) == n_args
    # the argument struct: the header's members in the header's order, and the layout a C compiler gives them
    body = re.search(r"typedef struct \{([^}]*)\} srh_op_norm_args;", header).group(1)
    members = [m for decl in body.split(";") for m in re.findall(r"(\w+)\s*(?:,|$)", decl.strip())]
    assert members == [f[0] for f in _lib.OpNormArgs._fields_], members
    assert C.sizeof(_lib.OpNormArgs) == 128 and _lib.OpNormArgs.slice_stride.offset == 88 and _lib.OpNormArgs.out_f16.offset == 120
