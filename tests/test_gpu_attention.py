"""Op-level tests of the encoder's attention kernels (through the C ABI's srh_op_attention / srh_op_attention_hd, which drive
launch_attention exactly as the model does): attn_window_kernel, attn_global_kernel fixed and runtime-S, attention_hdx windowed and
16 x 16 global, attn_generic_kernel<10> — at the smallest shapes that reach each of their routes (tests/attention_ref.py GEOMETRIES).

Against tests/attention_ref.py: inputs with an EXACT answer under a derived bound (uniform: the mean of all win^2 V rows of the window,
pads included, to one fp16 ulp; selector: the target's V row; padsink: b_v), and random / ramp_up / ramp_down / big inputs against the
float64 reference, the kernel's error held to tolerances.ATTN_OP_VS_APRIORI times the a-priori error of the same case (the design's two
fp16 roundings simulated in float64).  tests/test_attention_ref.py proves on the CPU that these cases meet the conditions their answers
rest on and that a list of single mistakes each break a bound by a factor of four or more.  Every output is pre-filled with NaN and
followed by a guard band of NaN rows.  Run on an MI355X: pytest -m gpu."""
import ctypes as C

import pytest
import torch

import attention_ref as A
import tolerances as T

pytestmark = pytest.mark.gpu

GUARD = 8                    # NaN rows after the output
CASES = [(geo, fam) for geo in A.ALL_GEOMETRIES for fam in A.families_of(*geo)]


@pytest.fixture(scope="module")
def ctx():
    from sam_road_amd import _lib
    assert torch.cuda.is_available(), "gpu-marked test needs a GPU"
    return _lib.Context.get(0)


def _p(t):
    return C.c_void_p(t.data_ptr())


def _run(ctx, case):
    """The op on a case's inputs: the output [B S S, D] on the host (float64); NaN pre-fill, finiteness and the guard band asserted."""
    B, S, heads, win, hd = (case[k] for k in ("B", "S", "heads", "win", "hd"))
    rows, D = B * S * S, heads * hd
    out = torch.full((rows + GUARD, D), float("nan"), device="cuda", dtype=torch.half)
    dq, dh, dw, db = case["qkv"].cuda(), case["rel_h"].cuda(), case["rel_w"].cuda(), case["bias"].cuda()
    if hd == 64:
        ctx.check(ctx.lib.srh_op_attention(ctx.handle, _p(dq), _p(dh), _p(dw), _p(db), B, S, heads, win, _p(out), None), "srh_op_attention")
    else:
        ctx.check(ctx.lib.srh_op_attention_hd(ctx.handle, _p(dq), _p(dh), _p(dw), _p(db), B, S, heads, hd, win, _p(out), None),
                  "srh_op_attention_hd")
    torch.cuda.synchronize()
    host = out.cpu()
    assert torch.isfinite(host[:rows].float()).all(), "unwritten or non-finite outputs"
    assert torch.isnan(host[rows:]).all(), "the kernel wrote past its last token"
    return host[:rows].double()


@pytest.mark.parametrize("geo,family", CASES, ids=["%s-S%d-win%d-hd%d" % ((f,) + g) for g, f in CASES])
def test_attention(ctx, geo, family):
    S, win, hd = geo
    case = A.gpu_case(family, S, win, hd)
    got = _run(ctx, case)
    tag = "op_attention64[%s,%s,S=%d,win=%d,hd=%d]" % (A.KERNEL_OF[geo], family, S, win, hd)
    if case["answer"] is not None:
        rows = case["answer_rows"]
        err = (got - case["answer"]).abs()[rows]
        print(f"{tag}: max-abs error against the exact answer {err.max().item():.3e} over {int(rows.sum())} tokens")
        T.check(tag + " error / derived bound", A.answer_excess(case, got), 1.0)
    else:
        exact, rounded = A.attention64_both(*A.case_args(case))
        err, ap = (got - exact).abs(), (rounded - exact).abs()
        print(f"{tag}: max-abs {err.max().item():.3e} (a priori {ap.max().item():.3e}), mean-abs {err.mean().item():.3e} "
              f"(a priori {ap.mean().item():.3e})")
        r_max, r_mean = A.apriori_ratios(got, exact, rounded)
        T.check(tag + " max-abs / a priori", r_max, T.ATTN_OP_VS_APRIORI)
        T.check(tag + " mean-abs / a priori", r_mean, T.ATTN_OP_VS_APRIORI)
