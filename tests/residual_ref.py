"""CPU references of the residual-stream passes, for the op-level tests (tests/test_gpu_residual.py).

The encoder keeps the residual stream x in f32 and folds a block's residual adds (the SAM fork's Block.forward: x = shortcut + attn(..),
x = x + mlp(norm2(x)); ImageEncoderViT.forward: x = patch_embed(x) + pos_embed — reference model.py:245-258 builds it) into the
LayerNorm pass that reads x next (norm.hip layernorm_kernel, NormParams).  Two halves:

  - the FOLD, x -> x', in plain torch float32 on the CPU, written in the order the kernel's comments promise.  Every step is ONE IEEE
    binary32 add of two binary32 values (an fp16 value converts exactly), so torch's result is the exact expectation, bit for bit, not
    an approximation: ``fold_branches`` ((x + delta16) + delta16b, x read through ``row % period``) and ``fold_slices``
    (((s0 + s1 + ...) + bias) + x, splitk_reduce_kernel's order);
  - the LayerNorm of x' in float64 (biased variance, eps inside the root, optional exact-erf GELU): ``layernorm64``.

``make_inputs`` draws the seeded inputs of both test files.  tests/test_residual_ref.py pins layernorm64 to F.layer_norm and proves,
on these inputs and with the reference alone, that a fold in another order differs in bits on more than 1 % of the elements — a kernel
that adds in the wrong order cannot pass the equalities by luck.
"""
import math

import torch

SLICE_SCALES = (1.0, 0.37, 2.3, 0.11)      # split-K partials of one product differ in size: a different scale per slice


def make_inputs(M, D, seed, period=0, nslices=0):
    """x f32 [M, D] ([period, D] when period > 0) ~ 3 N(0,1) + 1.5, gamma / beta ~ N(0,1) (tests/test_gpu_ops.py test_layernorm's
    distributions); d1 / d2 fp16 [M, D] ~ N(0,1) plus a pattern that depends on row and on column (a row or column permutation of a
    branch cannot pass); slices f32 [nslices, M, D] ~ SLICE_SCALES[z] N(0,1) and their bias ~ N(0,1)."""
    g = torch.Generator().manual_seed(seed)
    out = {"x": torch.randn(period or M, D, generator=g) * 3 + 1.5,
           "gamma": torch.randn(D, generator=g), "beta": torch.randn(D, generator=g)}
    row = torch.arange(M, dtype=torch.float32).view(M, 1)
    col = torch.arange(D, dtype=torch.float32).view(1, D)
    out["d1"] = (torch.randn(M, D, generator=g) + (row % 7) * 0.125 - (col % 5) * 0.25).half()
    out["d2"] = (torch.randn(M, D, generator=g) - (row % 5) * 0.25 + (col % 3) * 0.125).half()
    if nslices:
        out["slices"] = torch.stack([torch.randn(M, D, generator=g) * SLICE_SCALES[z] + ((row + z) % 3) * 0.0625 for z in range(nslices)])
        out["bias"] = torch.randn(D, generator=g)
    return out


def fold_branches(x, d1, d2=None, period=0):
    """x' = (x[row % period] + d1) + d2 in float32, one add per step (d2 optional; period 0: x[row])."""
    assert x.dtype == torch.float32 and d1.dtype == torch.float16
    M = d1.shape[0]
    v = x[torch.arange(M) % period] if period else x
    v = v + d1.float()
    if d2 is not None:
        assert d2.dtype == torch.float16
        v = v + d2.float()
    return v


def fold_slices(x, slices, bias):
    """x' = ((s0 + s1 + ...) + bias) + x in float32, the slices in ascending order (splitk_reduce_kernel's order)."""
    assert x.dtype == slices.dtype == bias.dtype == torch.float32
    a = slices[0].clone()
    for z in range(1, slices.shape[0]):
        a = a + slices[z]
    a = a + bias
    return a + x


def layernorm64(x, gamma, beta, eps=1e-6, gelu=False):
    """Row LayerNorm from its definition in float64: (x - mean) / sqrt(biased variance + eps) * gamma + beta, then exact-erf GELU."""
    x = x.double()
    u = x.mean(1, keepdim=True)
    v = (x - u).pow(2).mean(1, keepdim=True)
    y = (x - u) / torch.sqrt(v + eps) * gamma.double() + beta.double()
    if gelu:
        y = 0.5 * y * (1.0 + torch.special.erf(y / math.sqrt(2.0)))
    return y


def same_bits(a, b):
    """Bit-for-bit equality of two float tensors (-0.0 != 0.0, equal NaN payloads are equal)."""
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    as_int = {torch.float32: torch.int32, torch.float16: torch.int16, torch.float64: torch.int64}[a.dtype]
    return torch.equal(a.contiguous().view(as_int), b.contiguous().view(as_int))
