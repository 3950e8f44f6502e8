"""Op-level tests of the residual-stream passes (through the C ABI's test-only exports srh_op_layernorm_ex, srh_op_gemm_partials and
srh_op_gemm_pos): every fused mode of layernorm_kernel that encode_batch (api_model.hip) chooses among — x + delta16, (x + delta16) +
delta16b, pos_embed[row % period] + delta16, the split-K fold, the cast-only fold, the non-finite sentinel — and the two GEMM modes
that feed them (deferred split-K partials, the f32 + pos epilogue).

The fold is compared BIT FOR BIT with tests/residual_ref.py's float32 fold (one IEEE add per step: the exact expectation), the
normalised outputs bit for bit with the plain pass on the folded x' where the template instantiation is the same, and with the
float64 LayerNorm under tests/tolerances.py's bounds.  tests/test_residual_ref.py shows that these inputs tell the add orders apart.
Every output is pre-filled with NaN and followed by a guard band of NaN rows.  Run on an MI355X: pytest -m gpu."""
import ctypes as C

import pytest
import torch

import residual_ref as R
import tolerances as T

pytestmark = pytest.mark.gpu

SRH_ERR_BAD_ARG, SRH_ERR_UNSUPPORTED, SRH_ERR_NONFINITE = -1, -2, -6     # include/samroad_hip.h
GUARD = 8                    # NaN rows after every output (and after a periodic x table)
WIDTHS = (128, 256, 768, 1024, 1280)


def _rows_per_wave(D):
    return 4 if D <= 256 else 1              # norm.hip launch_layernorm: R = 4 at D = 128 / 256


def _second_iteration_rows(D):
    """The launcher caps the grid at 2048 workgroups of 4 waves: 8192 R rows per grid-stride iteration.  8192 R + 517 rows reach the
    second iteration and end in a tail (517 = 4 * 129 + 1)."""
    return 8192 * _rows_per_wave(D) + 517


@pytest.fixture(scope="module")
def ctx():
    from sam_road_amd import _lib
    assert torch.cuda.is_available(), "gpu-marked test needs a GPU"
    return _lib.Context.get(0)


def _p(t):
    return t.data_ptr() if t is not None else None


def _nan(rows, D, dtype=torch.float32):
    return torch.full((rows + GUARD, D), float("nan"), device="cuda", dtype=dtype)


def _guarded(t):
    """A device copy of t [rows, D] followed by GUARD rows of NaN (the same allocation)."""
    buf = _nan(t.shape[0], t.shape[1], t.dtype)
    buf[:t.shape[0]] = t.cuda()
    return buf


def _guard_intact(buf, rows):
    return bool(torch.isnan(buf[rows:]).all())


def _all_nan(*bufs):
    return all(bool(torch.isnan(b).all()) for b in bufs)


def _ln_ex(ctx, x, M, D, gamma=None, beta=None, gelu=0, x_period=0, delta16=None, delta16b=None, x_out=None, slices=None, nslices=0,
           slice_stride=0, slice_bias=None, nf_tag=-1, out_f32=None, out_f16=None, eps=1e-6):
    """srh_op_layernorm_ex on device tensors (or a raw device address for `slices`); returns the status."""
    from sam_road_amd import _lib
    a = _lib.OpNormArgs()
    a.x, a.M, a.D, a.x_period = _p(x), M, D, x_period
    a.gamma, a.beta, a.eps, a.gelu = _p(gamma), _p(beta), eps, gelu
    a.delta16, a.delta16b, a.x_out = _p(delta16), _p(delta16b), _p(x_out)
    a.slices = slices if isinstance(slices, (int, type(None))) else _p(slices)
    a.nslices, a.slice_stride, a.slice_bias = nslices, slice_stride, _p(slice_bias)
    a.nf_tag, a.out_f32, a.out_f16 = nf_tag, _p(out_f32), _p(out_f16)
    return ctx.lib.srh_op_layernorm_ex(ctx.handle, C.byref(a), None)


def _ln_plain(ctx, x, M, D, gamma, beta, gelu):
    """The plain pass (srh_op_layernorm) on a device x: (out_f32, out_f16) with guard bands."""
    o32, o16 = _nan(M, D), _nan(M, D, torch.half)
    ctx.check(ctx.lib.srh_op_layernorm(ctx.handle, _p(x), _p(gamma), _p(beta), 1e-6, M, D, gelu, _p(o32), _p(o16), None), "srh_op_layernorm")
    torch.cuda.synchronize()
    return o32, o16


def _check_against_float64(name, o32, o16, xf, gamma, beta, gelu):
    """out_f32 / out_f16 [M, D] (host) against the float64 LayerNorm of the folded x' (host float32)."""
    ref = R.layernorm64(xf, gamma, beta, 1e-6, bool(gelu))
    T.check(f"op_residual_{name}_f32", (o32.double() - ref).abs().max().item(), T.RESID_LN_F32)
    # fp16: the bound as it stands where |y| < 16, in units of the fp16 spacing beyond (tolerances.RESID_LN_F16: about one output in 10^7
    # of the large shapes lies in [16, 32), where half an fp16 ulp alone is 7.8e-3)
    spacing = torch.exp2(torch.floor(torch.log2(ref.abs().clamp(min=1.0))) - 3).clamp(min=1.0)
    T.check(f"op_residual_{name}_f16", ((o16.double() - ref).abs() / spacing).max().item(), T.RESID_LN_F16)


# ---- fold arithmetic, exact: x + delta16 and (x + delta16) + delta16b ---------------------------------------------------------------
@pytest.mark.parametrize("two", [False, True], ids=["delta", "delta+deltab"])
@pytest.mark.parametrize("big", [False, True], ids=["517", "2nd-iteration"])
@pytest.mark.parametrize("D", WIDTHS)
def test_fold_branches_exact(ctx, D, big, two):
    M = _second_iteration_rows(D) if big else 517
    gelu = int(D == 128)
    t = R.make_inputs(M, D, seed=7 * D + big)
    xf = R.fold_branches(t["x"], t["d1"], t["d2"] if two else None)          # the exact x'
    dx, dg, db = _guarded(t["x"]), t["gamma"].cuda(), t["beta"].cuda()
    d1, d2 = t["d1"].cuda(), (t["d2"].cuda() if two else None)
    # out of place
    xo, o32, o16 = _nan(M, D), _nan(M, D), _nan(M, D, torch.half)
    ctx.check(_ln_ex(ctx, dx, M, D, dg, db, gelu, delta16=d1, delta16b=d2, x_out=xo, out_f32=o32, out_f16=o16), "srh_op_layernorm_ex")
    torch.cuda.synchronize()
    assert R.same_bits(dx[:M].cpu(), t["x"]) and _guard_intact(dx, M), "x changed in an out-of-place pass"
    assert R.same_bits(xo[:M].cpu(), xf), "x_out is not the float32 fold, bit for bit"
    assert _guard_intact(xo, M) and _guard_intact(o32, M) and _guard_intact(o16, M)
    # the normalised outputs: the plain pass over the uploaded x' is the same template instantiation, so the same bits
    p32, p16 = _ln_plain(ctx, xf.cuda(), M, D, dg, db, gelu)
    assert R.same_bits(o32, p32) and R.same_bits(o16, p16), "fused and plain pass differ on the same x'"
    _check_against_float64(f"branches[D={D},M={M},{'two' if two else 'one'}]", o32[:M].cpu(), o16[:M].cpu(), xf, t["gamma"], t["beta"], gelu)
    # in place (x_out == x), as the model runs it
    i32, i16 = _nan(M, D), _nan(M, D, torch.half)
    ctx.check(_ln_ex(ctx, dx, M, D, dg, db, gelu, delta16=d1, delta16b=d2, x_out=dx, out_f32=i32, out_f16=i16), "srh_op_layernorm_ex")
    torch.cuda.synchronize()
    assert R.same_bits(dx, xo), "in place and out of place differ (or the guard band after x was written)"
    assert R.same_bits(i32, o32) and R.same_bits(i16, o16)
    # without x_out the same x' is normalised and nothing else is written
    dx2 = _guarded(t["x"])
    n16 = _nan(M, D, torch.half)
    ctx.check(_ln_ex(ctx, dx2, M, D, dg, db, gelu, delta16=d1, delta16b=d2, out_f16=n16), "srh_op_layernorm_ex")
    torch.cuda.synchronize()
    assert R.same_bits(n16, o16) and R.same_bits(dx2[:M].cpu(), t["x"])


# ---- x_period: pos_embed[row % (S S)] + the patch embedding, block 0's first pass ------------------------------------------------------
# period 400 (S = 20) and 64 with M = 3 period + 5 (a multiple neither of R nor of the period); period 1024 (S = 32) with M = 8709
# puts the modulo into the grid-stride second iteration at the ViT-B width, where the model runs it
@pytest.mark.parametrize("D,period,M", [(D, p, 3 * p + 5) for D in WIDTHS for p in (400, 64)] + [(768, 1024, 8709)])
def test_fold_x_period_exact(ctx, D, period, M):
    gelu = int(D == 128)
    t = R.make_inputs(M, D, seed=11 * D + period, period=period)
    xf = R.fold_branches(t["x"], t["d1"], period=period)
    dx, dg, db, d1 = _guarded(t["x"]), t["gamma"].cuda(), t["beta"].cuda(), t["d1"].cuda()      # a read past the table's last row meets NaN
    xo, o32, o16 = _nan(M, D), _nan(M, D), _nan(M, D, torch.half)
    ctx.check(_ln_ex(ctx, dx, M, D, dg, db, gelu, x_period=period, delta16=d1, x_out=xo, out_f32=o32, out_f16=o16), "srh_op_layernorm_ex")
    torch.cuda.synchronize()
    assert R.same_bits(xo[:M].cpu(), xf), "x_out is not pos[row % period] + delta16, bit for bit"
    assert R.same_bits(dx[:period].cpu(), t["x"]) and _guard_intact(dx, period), "the table was written"
    assert _guard_intact(xo, M) and _guard_intact(o32, M) and _guard_intact(o16, M)
    p32, p16 = _ln_plain(ctx, xf.cuda(), M, D, dg, db, gelu)
    assert R.same_bits(o32, p32) and R.same_bits(o16, p16), "fused and plain pass differ on the same x'"
    _check_against_float64(f"period[D={D},M={M},period={period}]", o32[:M].cpu(), o16[:M].cpu(), xf, t["gamma"], t["beta"], gelu)


# ---- cast-only fold: the neck's first pass over the last block's output ----------------------------------------------------------------
@pytest.mark.parametrize("D,M,mode", [(768, 517, "delta"), (768, 8709, "delta+deltab"), (256, 33285, "delta"), (128, 517, "delta+deltab"),
                                      (1024, 8709, "slices"), (1280, 2048, "slices")])
def test_cast_only_fold(ctx, D, M, mode):
    n = 3 if mode == "slices" else 0
    t = R.make_inputs(M, D, seed=13 * D + M, nslices=n)
    dx = _guarded(t["x"])
    o16 = _nan(M, D, torch.half)
    if mode == "slices":
        xf = R.fold_slices(t["x"], t["slices"], t["bias"])
        ds, dbias = t["slices"].cuda(), t["bias"].cuda()
        ctx.check(_ln_ex(ctx, dx, M, D, slices=ds, nslices=n, slice_stride=M * D, slice_bias=dbias, out_f16=o16), "srh_op_layernorm_ex")
    else:
        two = mode == "delta+deltab"
        xf = R.fold_branches(t["x"], t["d1"], t["d2"] if two else None)
        d1, d2 = t["d1"].cuda(), (t["d2"].cuda() if two else None)
        ctx.check(_ln_ex(ctx, dx, M, D, delta16=d1, delta16b=d2, out_f16=o16), "srh_op_layernorm_ex")
    torch.cuda.synchronize()
    assert R.same_bits(o16[:M].cpu(), xf.half()), "out_f16 is not fp16(x'), bit for bit"
    assert _guard_intact(o16, M)
    assert R.same_bits(dx[:M].cpu(), t["x"]) and _guard_intact(dx, M), "x changed"


# ---- split-K fold: ((s0 + s1 + ...) + bias) + x on synthetic slices ---------------------------------------------------------------------
@pytest.mark.parametrize("nslices", [1, 2, 3, 4])
@pytest.mark.parametrize("M", [2048, 8709])
@pytest.mark.parametrize("D", [1024, 1280])
def test_fold_slices_exact(ctx, D, M, nslices):
    t = R.make_inputs(M, D, seed=17 * D + M + nslices, nslices=nslices)
    xf = R.fold_slices(t["x"], t["slices"], t["bias"])
    dx, dg, db = _guarded(t["x"]), t["gamma"].cuda(), t["beta"].cuda()
    ds, dbias = t["slices"].cuda(), t["bias"].cuda()
    kw = dict(slices=ds, nslices=nslices, slice_stride=M * D, slice_bias=dbias)
    xo, o32, o16 = _nan(M, D), _nan(M, D), _nan(M, D, torch.half)
    ctx.check(_ln_ex(ctx, dx, M, D, dg, db, x_out=xo, out_f32=o32, out_f16=o16, **kw), "srh_op_layernorm_ex")
    torch.cuda.synchronize()
    assert R.same_bits(dx[:M].cpu(), t["x"]) and R.same_bits(ds.cpu(), t["slices"]), "an input changed in an out-of-place pass"
    assert R.same_bits(xo[:M].cpu(), xf), "x_out is not ((s0 + s1 + ...) + bias) + x in float32, bit for bit"
    assert _guard_intact(xo, M) and _guard_intact(o32, M) and _guard_intact(o16, M)
    # this pass is its own template instantiation: float64 is the assertion, equality with the plain pass is reported
    _check_against_float64(f"slices[D={D},M={M},n={nslices}]", o32[:M].cpu(), o16[:M].cpu(), xf, t["gamma"], t["beta"], 0)
    p32, p16 = _ln_plain(ctx, xf.cuda(), M, D, dg, db, 0)
    print(f"split-K fold D={D} M={M} slices={nslices}: same bits as the plain pass on x': f32 {R.same_bits(o32, p32)}, f16 {R.same_bits(o16, p16)}")
    # in place, as the model runs it
    i32, i16 = _nan(M, D), _nan(M, D, torch.half)
    ctx.check(_ln_ex(ctx, dx, M, D, dg, db, x_out=dx, out_f32=i32, out_f16=i16, **kw), "srh_op_layernorm_ex")
    torch.cuda.synchronize()
    assert R.same_bits(dx, xo) and R.same_bits(i32, o32) and R.same_bits(i16, o16), "in place and out of place differ"


# ---- the model's chain on real partials: deferred split-K fc2 -> the next LayerNorm pass ----------------------------------------------------
def _gemm_operands(M, N, K, seed):
    """tests/test_gpu_ops.py test_gemm's operands: A ~ 0.5 N(0,1) with a row ramp in column 0, W ~ 0.05 N(0,1), bias ~ N(0,1)."""
    g = torch.Generator().manual_seed(seed)
    A = (torch.randn(M, K, generator=g) * 0.5).half()
    W = (torch.randn(N, K, generator=g) * 0.05).half()
    A[:, 0] += torch.arange(M).half() * 0.01
    return A, W, torch.randn(N, generator=g), g


def _gemm_bound(scale, K):
    return max(scale, 1.0) * (K / 64) ** 0.5       # times tolerances.RESID_GEMM_F32: test_gemm's bound


# (M, N, K)            kernel (from gemm.hip's dispatch)              slices
# (2048, 1280, 5120)   ping-pong kernel, 128 x 256 tiles (ViT-H fc2)  3
# (3072, 1024, 4096)   ping-pong kernel                               2
# (1024, 1024, 4096)   128 x 128 kernel                               4
# (256, 1280, 5120)    128 x 128 kernel                               4
@pytest.mark.parametrize("M,N,K,slices_expected,with_float64", [(2048, 1280, 5120, 3, False), (3072, 1024, 4096, 2, False),
                                                                (1024, 1024, 4096, 4, True), (256, 1280, 5120, 4, True)])
def test_deferred_splitk_chain(ctx, M, N, K, slices_expected, with_float64):
    A, W, bias, g = _gemm_operands(M, N, K, seed=M + N + K)
    x = torch.randn(M, N, generator=g) * 3 + 1.5
    gamma, beta = torch.randn(N, generator=g), torch.randn(N, generator=g)
    dA, dW, dbias, dg, db = A.cuda(), W.cuda(), bias.cuda(), gamma.cuda(), beta.cuda()
    dx = _guarded(x)
    # fc2 with the reduce deferred, then the pass that folds its partials into x (in place) and normalises
    ws, n = C.c_void_p(), C.c_int(0)
    ctx.check(ctx.lib.srh_op_gemm_partials(ctx.handle, _p(dA), _p(dW), _p(dbias), M, N, K, C.byref(ws), C.byref(n), None), "srh_op_gemm_partials")
    print(f"srh_op_gemm_partials ({M}, {N}, {K}): {n.value} slices")
    assert n.value > 1 and ws.value
    o32, o16 = _nan(M, N), _nan(M, N, torch.half)
    ctx.check(_ln_ex(ctx, dx, M, N, dg, db, x_out=dx, slices=ws.value, nslices=n.value, slice_stride=M * N, slice_bias=dbias,
                     out_f32=o32, out_f16=o16), "srh_op_layernorm_ex")
    torch.cuda.synchronize()
    assert n.value == slices_expected
    # the same layer with the reduce pass and its residual epilogue, then the plain LayerNorm pass
    dx2 = _guarded(x)
    ctx.check(ctx.lib.srh_op_gemm(ctx.handle, _p(dA), _p(dW), _p(dbias), _p(dx2), M, N, K, 0, _p(dx2), None, None), "srh_op_gemm")
    p32, p16 = _ln_plain(ctx, dx2, M, N, dg, db, 0)
    assert _guard_intact(dx, M) and _guard_intact(dx2, M) and _guard_intact(o32, M) and _guard_intact(o16, M)
    assert not torch.isnan(dx[:M]).any()
    assert R.same_bits(dx, dx2), "x' of the deferred fold and of the reduce pass differ"
    assert R.same_bits(o32, p32) and R.same_bits(o16, p16), "the LayerNorm outputs of the two chains differ"
    if with_float64:
        ref = x.double() + A.double() @ W.double().t() + bias.double()
        err = (dx[:M].cpu().double() - ref).abs().max().item()
        T.check(f"op_residual_chain[{M},{N},{K}] max-abs / (scale sqrt(K/64))", err / _gemm_bound(ref.abs().max().item(), K), T.RESID_GEMM_F32)


def test_gemm_partials_refuses_a_shape_without_splitk(ctx):
    M, N, K = 4096, 1024, 1024                     # M >= 4096: gemm_splitk_factor is 1
    A, W, bias, _ = _gemm_operands(M, N, K, seed=3)
    dA, dW, dbias = A.cuda(), W.cuda(), bias.cuda()
    ws, n = C.c_void_p(1), C.c_int(7)
    rc = ctx.lib.srh_op_gemm_partials(ctx.handle, _p(dA), _p(dW), _p(dbias), M, N, K, C.byref(ws), C.byref(n), None)
    assert rc == SRH_ERR_UNSUPPORTED and not ws.value and n.value == 0
    assert b"without split-K" in ctx.lib.srh_last_error(ctx.handle)


# ---- the GEMM's f32 + pos epilogue: the patch embedding where the 256 x 192 kernel is not preferred -----------------------------------
@pytest.mark.parametrize("M,N,K,pos_rows", [(1205, 768, 768, 400), (517, 1280, 768, 64)])
def test_gemm_pos_epilogue(ctx, M, N, K, pos_rows):
    A, W, bias, g = _gemm_operands(M, N, K, seed=M + N + pos_rows)
    pos = torch.randn(pos_rows, N, generator=g) * 3 + 1.5
    dA, dW, dbias, dpos = A.cuda(), W.cuda(), bias.cuda(), _guarded(pos)
    out = _nan(M, N)
    ctx.check(ctx.lib.srh_op_gemm_pos(ctx.handle, _p(dA), _p(dW), _p(dbias), _p(dpos), pos_rows, M, N, K, _p(out), None), "srh_op_gemm_pos")
    torch.cuda.synchronize()
    assert _guard_intact(out, M) and _guard_intact(dpos, pos_rows) and R.same_bits(dpos[:pos_rows].cpu(), pos)
    pos_of_row = pos[torch.arange(M) % pos_rows]
    ref = A.double() @ W.double().t() + bias.double() + pos_of_row.double()
    unit = _gemm_bound(ref.abs().max().item(), K)
    got = out[:M].cpu()
    T.check(f"op_residual_gemm_pos[{M},{N},{K},{pos_rows}] max-abs / (scale sqrt(K/64))", (got.double() - ref).abs().max().item() / unit, T.RESID_GEMM_F32)
    # the same product without pos, the table added on the host
    plain = _nan(M, N)
    ctx.check(ctx.lib.srh_op_gemm(ctx.handle, _p(dA), _p(dW), _p(dbias), None, M, N, K, 0, _p(plain), None, None), "srh_op_gemm")
    torch.cuda.synchronize()
    assert _guard_intact(plain, M)
    T.check(f"op_residual_gemm_pos_vs_host_add[{M},{N},{K},{pos_rows}] max-abs / (scale sqrt(K/64))",
            (got.double() - (plain[:M].cpu().double() + pos_of_row.double())).abs().max().item() / unit, T.RESID_GEMM_F32)


# ---- the non-finite sentinel -----------------------------------------------------------------------------------------------------------
def _check(ctx):
    """srh_ctx_check with synchronisation: (status, message)."""
    rc = ctx.lib.srh_ctx_check(ctx.handle, None, 1)
    return rc, (ctx.lib.srh_last_error(ctx.handle) or b"").decode()


# D = 256: four rows per wave, the last row of M = 33285 is a tail row; D = 768: one row per wave (the ViT-B block passes)
@pytest.mark.parametrize("D", [256, 768])
def test_sentinel_sees_a_non_finite_branch_or_x(ctx, D):
    M = _second_iteration_rows(D)
    t = R.make_inputs(M, D, seed=19 * D)
    dx, dg, db, d1, d2 = _guarded(t["x"]), t["gamma"].cuda(), t["beta"].cuda(), t["d1"].cuda(), t["d2"].cuda()
    o16 = _nan(M, D, torch.half)
    _check(ctx)                                     # whatever an earlier test left is reported there, not here
    tag = 2 * 5 + 1                                 # block 5, norm2

    def run(nf_tag=tag, gamma=dg, beta=db):
        ctx.check(_ln_ex(ctx, dx, M, D, gamma, beta, delta16=d1, delta16b=d2, nf_tag=nf_tag, out_f16=o16), "srh_op_layernorm_ex")

    run()
    assert _check(ctx)[0] == 0, "a clean fused pass was flagged"
    inf, nan = float("inf"), float("nan")
    second = 8192 * _rows_per_wave(D) + 300         # a row of the grid-stride second iteration
    for buf, value, what in ((dx, inf, "+Inf in x"), (dx, nan, "NaN in x"), (d1, inf, "fp16 Inf in delta16"), (d2, inf, "fp16 Inf in delta16b")):
        for row in (0, M - 1, second):
            col = (37 * row + 5) % D
            keep = buf[row, col].clone()
            buf[row, col] = value
            run()
            rc, msg = _check(ctx)
            assert rc == SRH_ERR_NONFINITE, f"{what}, row {row}: not reported (status {rc})"
            assert "encoder block 5, norm2" in msg, msg
            assert _check(ctx)[0] == 0, "the flag was not cleared by its report"      # a non-finite INPUT is data, not a GPU fault
            buf[row, col] = keep
    run()
    assert _check(ctx)[0] == 0, "the restored inputs are still flagged"
    # the tag names the block: an even tag is norm1
    dx[M - 1, 3] = inf
    run(nf_tag=14)
    rc, msg = _check(ctx)
    assert rc == SRH_ERR_NONFINITE and "encoder block 7, norm1" in msg, (rc, msg)
    # no sentinel asked for (nf_tag -1), and the cast-only pass (documented: the sentinel needs gamma): not flagged
    run(nf_tag=-1)
    run(nf_tag=tag, gamma=None, beta=None)
    assert _check(ctx)[0] == 0
    assert torch.isinf(o16[M - 1, 3]), "the cast-only pass should hand the Inf on"


def test_sentinel_sees_a_non_finite_slice(ctx):
    M, D, n = 8709, 1024, 3
    t = R.make_inputs(M, D, seed=23, nslices=n)
    dx, dg, db, ds, dbias = _guarded(t["x"]), t["gamma"].cuda(), t["beta"].cuda(), t["slices"].cuda(), t["bias"].cuda()
    o16 = _nan(M, D, torch.half)
    _check(ctx)
    tag = 2 * 9                                     # block 9, norm1: the pass after a deferred fc2

    def run(gamma=dg, beta=db):
        ctx.check(_ln_ex(ctx, dx, M, D, gamma, beta, slices=ds, nslices=n, slice_stride=M * D, slice_bias=dbias, nf_tag=tag, out_f16=o16),
                  "srh_op_layernorm_ex")

    run()
    assert _check(ctx)[0] == 0, "a clean split-K fold was flagged"
    for z, row in ((0, 0), (2, M - 1), (1, 8192 + 300)):
        keep = ds[z, row, 11].clone()
        ds[z, row, 11] = float("inf")
        run()
        rc, msg = _check(ctx)
        assert rc == SRH_ERR_NONFINITE and "encoder block 9, norm1" in msg, (z, row, rc, msg)
        assert _check(ctx)[0] == 0
        run(None, None)                             # cast-only: not flagged
        assert _check(ctx)[0] == 0
        ds[z, row, 11] = keep
    run()
    assert _check(ctx)[0] == 0


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------
def test_refusals_launch_nothing(ctx):
    M = 517
    bufs = {}

    def call(D, expect, **kw):
        if D not in bufs:
            t = R.make_inputs(M, D, seed=29 + D, nslices=2)
            bufs[D] = {k: v.cuda() for k, v in t.items()}
        b = bufs[D]
        named = {k: (b[v] if isinstance(v, str) else v) for k, v in kw.items()}
        xo, o32, o16 = _nan(M, D), _nan(M, D), _nan(M, D, torch.half)
        rc = _ln_ex(ctx, b["x"], M, D, b["gamma"], b["beta"], x_out=xo, out_f32=o32, out_f16=o16, **named)
        torch.cuda.synchronize()
        assert rc == expect, (D, kw, rc)
        assert _all_nan(xo, o32, o16), f"a refused call wrote an output: D = {D}, {kw}"
        assert ctx.lib.srh_last_error(ctx.handle)

    sl = dict(slices="slices", nslices=2, slice_stride=M * 1024, slice_bias="bias")
    call(1024, SRH_ERR_BAD_ARG, delta16b="d2")                                   # delta16b without delta16
    call(1024, SRH_ERR_BAD_ARG, delta16="d1", nf_tag=64)                         # tags 64 .. are the neck's and the decoder's
    call(1024, SRH_ERR_BAD_ARG, delta16="d1", nf_tag=-2)
    call(1024, SRH_ERR_UNSUPPORTED, delta16="d1", **sl)                          # slices together with a branch
    call(1024, SRH_ERR_UNSUPPORTED, **dict(sl, slice_bias=None))                 # no bias to add after the slices
    call(768, SRH_ERR_UNSUPPORTED, **dict(sl, slice_stride=M * 768))             # slices at a width without the instantiation
    call(512, SRH_ERR_UNSUPPORTED)                                               # no kernel for this width at all
    call(512, SRH_ERR_UNSUPPORTED, delta16="d1")
    assert ctx.lib.srh_op_layernorm_ex(ctx.handle, None, None) == SRH_ERR_BAD_ARG
    assert _check(ctx)[0] == 0


def test_everything_optional_left_out_is_the_plain_pass(ctx):
    M, D = 517, 768
    t = R.make_inputs(M, D, seed=31)
    dx, dg, db = _guarded(t["x"]), t["gamma"].cuda(), t["beta"].cuda()
    o32, o16 = _nan(M, D), _nan(M, D, torch.half)
    ctx.check(_ln_ex(ctx, dx, M, D, dg, db, out_f32=o32, out_f16=o16), "srh_op_layernorm_ex")
    torch.cuda.synchronize()
    p32, p16 = _ln_plain(ctx, dx, M, D, dg, db, 0)
    assert R.same_bits(o32, p32) and R.same_bits(o16, p16)
    assert R.same_bits(dx[:M].cpu(), t["x"])
