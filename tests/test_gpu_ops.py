"""Op-level parity of the HIP kernels (through the C ABI) against plain PyTorch fp32 on the same
fp16-representable inputs.  Run on an MI355X: pytest -m gpu."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import tolerances

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from sam_road_amd import _lib
    assert torch.cuda.is_available(), "gpu-marked test needs a GPU"
    return _lib.Context.get(0)


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _sync():
    torch.cuda.synchronize()


@pytest.mark.parametrize("M,N,K,act,resid", [(256, 128, 64, 0, False), (300, 256, 192, 1, False),
                                              (1000, 768, 768, 0, True), (128, 384, 3072, 2, False),
                                              # small-M layers of ViT-H at 256 px: the deterministic split-K paths — 3 slices of 128 x 256
                                              # tiles on the ping-pong kernel (fc2), the ring kernel without split (proj), 4 slices of 128 x 128
                                              (2048, 1280, 5120, 0, True), (2048, 1280, 1280, 1, False), (256, 768, 3072, 0, True),
                                              # one round of 128 x 256 tiles on the ping-pong kernel: ragged M, the shortest k-loops (6 / 7 k-tiles)
                                              (2000, 3840, 384, 1, False), (2048, 3840, 448, 0, True), (1536, 4096, 1024, 2, True),
                                              # ViT-H fc1 at M = 2048: 640 tiles of 128x128 -> the 128x160 kernel (512 tiles, one round);
                                              # with a ragged M (1990 rows: the last tile row is partly empty) and with a residual
                                              (2048, 5120, 320, 1, False), (1990, 5120, 192, 0, True)])
def test_gemm(ctx, M, N, K, act, resid):
    g = torch.Generator().manual_seed(M + N + K)
    A = (torch.randn(M, K, generator=g) * 0.5).half()
    W = (torch.randn(N, K, generator=g) * 0.05).half()
    # asymmetric structure so a transposed C-write cannot pass
    A[:, 0] += torch.arange(M).half() * 0.01
    bias = torch.randn(N, generator=g)
    R = torch.randn(M, N, generator=g) if resid else None
    ref = A.float() @ W.float().t() + bias
    if act == 1:
        ref = F.gelu(ref)
    elif act == 2:
        ref = F.relu(ref)
    if resid:
        ref = ref + R
    dA, dW, db = A.cuda(), W.cuda(), bias.cuda()
    dR = R.cuda() if resid else None
    o32 = torch.full((M, N), float("nan"), device="cuda")
    o16 = torch.zeros((M, N), device="cuda", dtype=torch.half)
    ctx.check(ctx.lib.srh_op_gemm(ctx.handle, _p(dA), _p(dW), _p(db), _p(dR), M, N, K, act, _p(o32), _p(o16), None),
              "srh_op_gemm")
    _sync()
    err = (o32.cpu() - ref).abs().max().item()
    scale = ref.abs().max().item()
    assert err <= 2e-4 * max(scale, 1.0) * (K / 64) ** 0.5, (err, scale)
    assert (o16.cpu().float() - ref).abs().max().item() <= 2e-3 * max(scale, 1.0)
    # the same call again gives the same bits (split-K partial sums are added in a fixed order)
    o32b = torch.full((M, N), float("nan"), device="cuda")
    ctx.check(ctx.lib.srh_op_gemm(ctx.handle, _p(dA), _p(dW), _p(db), _p(dR), M, N, K, act, _p(o32b), None, None), "srh_op_gemm")
    _sync()
    assert torch.equal(o32, o32b)


@pytest.mark.parametrize("M,N,K,act,use_bias", [
    (8192, 768, 768, 0, True),        # z192: 128 tiles, one per workgroup: only the exposed (LDS-staged) epilogue
    (16384, 2304, 768, 1, True),      # z192: 768 tiles = 3 per workgroup: deferred epilogue with GELU riding the next tile
    (16384, 768, 3072, 0, True),      # z192: 48 k-tiles per tile (four 12-k-tile bodies), one tile per workgroup
    (12288, 1536, 768, 0, True),      # z192: 384 tiles on 256 workgroups: some walk two tiles, some one
    (16384, 768, 3072, 2, False),     # ReLU, no bias: no generated body -> the 256 x 256 LDS-DMA kernel (gemm_glds256_kernel)
    (8192, 1536, 768, 0, False),      # no bias -> the 256 x 256 kernel
    (2048, 3840, 1280, 0, True),      # ViT-H qkv at 256 px: 240 tiles of 128 x 256, one round of the ping-pong kernel (gemm_pp_kernel)
])
def test_gemm_big_fp16_layers(ctx, M, N, K, act, use_bias):
    """fp16-output layers: the persistent 256 x 192 kernel (csrc/gemm_z192.hip, generated body) where it applies — bias, act none /
    GELU, N % 192 == 0, K % 768 == 0, >= 128 tiles — and the kernels the dispatch (csrc/gemm.hip launch_gemm) falls back to where it
    does not; compare with a plain fp32 torch matmul of the same fp16 operands.  Tolerance: one fp16 rounding of the result."""
    g = torch.Generator().manual_seed(M + N + K + act)
    A = (torch.randn(M, K, generator=g) * 0.5).half().cuda()
    W = (torch.randn(N, K, generator=g) * 0.05).half().cuda()
    A[:, 0] += (torch.arange(M, device="cuda") % 64).half() * 0.01   # row-dependent structure: catches transposed / permuted writes
    W[:, 1] += (torch.arange(N, device="cuda") % 48).half() * 0.01
    bias = torch.randn(N, generator=g).cuda() if use_bias else None
    ref = A.float() @ W.float().t()
    if use_bias:
        ref = ref + bias
    if act == 1:
        ref = F.gelu(ref)
    elif act == 2:
        ref = F.relu(ref)
    o16 = torch.full((M, N), float("nan"), device="cuda", dtype=torch.half)
    ctx.check(ctx.lib.srh_op_gemm(ctx.handle, _p(A), _p(W), _p(bias), None, M, N, K, act, None, _p(o16), None), "srh_op_gemm")
    _sync()
    assert torch.isfinite(o16).all()
    err = (o16.float() - ref).abs().max().item()
    scale = ref.abs().max().item()
    tolerances.check("op_gemm_f16out[%d,%d,%d,act%d,bias%d] max-abs / scale" % (M, N, K, act, use_bias), err / max(scale, 1.0), tolerances.GEMM_F16_OUT)


def to_blocked16(a):
    """Row-major [M, N] -> the blocked-16 layout of include/samroad_hip.h (srh_op_gemm_ex), flat."""
    M, N = a.shape
    return a.reshape(M // 32, 32, N // 16, 2, 8).permute(0, 2, 3, 1, 4).contiguous().reshape(-1)


def from_blocked16(flat, M, N):
    return flat.reshape(M // 32, N // 16, 2, 32, 8).permute(0, 3, 1, 2, 4).contiguous().reshape(M, N)


def _mlp_operands(M, D, H, seed):
    g = torch.Generator().manual_seed(seed)
    A = (torch.randn(M, D, generator=g) * 0.5).half().cuda()
    W1 = (torch.randn(H, D, generator=g) * 0.05).half().cuda()
    W2 = (torch.randn(D, H, generator=g) * 0.05).half().cuda()
    A[:, 0] += (torch.arange(M, device="cuda") % 64).half() * 0.01      # row- / column-dependent structure: a permutation confined to
    W1[:, 1] += (torch.arange(H, device="cuda") % 48).half() * 0.01     # an M tail or to odd tile rows cannot pass
    W2[:, 2] += (torch.arange(D, device="cuda") % 40).half() * 0.01
    return A, W1, W2, torch.randn(H, generator=g).cuda(), torch.randn(D, generator=g).cuda()


# (M, D, H): fc1 = [M, D] x [H, D]^T, fc2 = [M, H] x [D, H]^T.  Tile counts (256 x 192 tiles on 256 workgroups):
#   (8192, 768, 3072)   fc1 512 = 2 per workgroup            fc2 128 = half the workgroups, one each
#   (12288, 768, 3072)  fc1 768 = 3 per workgroup            fc2 192
#   (16384, 768, 3072)  fc1 1024 = 4 (the model at B = 16)   fc2 256 = one each
#   (65536, 768, 3072)  fc1 4096 = 16 (INFER_BATCH_SIZE 64)  fc2 1024 = 4 per workgroup, A operand 400 MB
#   (12288, 768, 1536)  fc1 384: some walk two tiles, some one; fc2 K = 1536 = two 12-k-tile bodies
#   (24576, 1536, 3072) fc1 K = 1536; fc2 768 tiles = 3 per workgroup with the blocked A operand
_MLP_SHAPES = [(8192, 768, 3072), (12288, 768, 3072), (16384, 768, 3072), (65536, 768, 3072), (12288, 768, 1536), (24576, 1536, 3072)]


@pytest.mark.parametrize("M,D,H", _MLP_SHAPES)
def test_gemm_z192_blocked_fc1_body(ctx, M, D, H):
    """gemm_z192_kernel<3> — what the model's fc1 runs (csrc/api_model.hip: GELU, hidden activation WRITTEN in the blocked-16 layout) — alone,
    against fp32 torch; and bit-identical to the row-major GELU body (kernel<1>) on the same operands."""
    from sam_road_amd._lib import SRH_GEMM_OUT_BLOCKED16
    A, W1, _, b1, _ = _mlp_operands(M, D, H, M + H)
    ref = F.gelu(A.float() @ W1.float().t() + b1)
    blk = torch.full((M * H,), float("nan"), device="cuda", dtype=torch.half)
    ctx.check(ctx.lib.srh_op_gemm_ex(ctx.handle, _p(A), _p(W1), _p(b1), None, M, H, D, 1, None, _p(blk), SRH_GEMM_OUT_BLOCKED16, None), "srh_op_gemm_ex")
    rm = torch.full((M, H), float("nan"), device="cuda", dtype=torch.half)
    ctx.check(ctx.lib.srh_op_gemm(ctx.handle, _p(A), _p(W1), _p(b1), None, M, H, D, 1, None, _p(rm), None), "srh_op_gemm")
    _sync()
    got = from_blocked16(blk, M, H)
    assert torch.isfinite(got).all()
    tolerances.check("op_gemm_z192_body3[%d,%d,%d] max-abs / scale" % (M, H, D), (got.float() - ref).abs().max().item() / max(ref.abs().max().item(), 1.0),
                     tolerances.GEMM_F16_OUT)
    assert torch.equal(got, rm), "blocked-16 and row-major GELU bodies differ"


@pytest.mark.parametrize("M,D,H", _MLP_SHAPES)
def test_gemm_z192_blocked_fc2_body(ctx, M, D, H):
    """gemm_z192_kernel<2> — the model's fc2 (A operand READ in the blocked-16 layout) — alone, against fp32 torch; and bit-identical to
    the row-major body (kernel<0>) on the same operand."""
    from sam_road_amd._lib import SRH_GEMM_A_BLOCKED16
    _, _, W2, _, b2 = _mlp_operands(M, D, H, M + D)
    g = torch.Generator().manual_seed(M + 7)
    Hid = (torch.randn(M, H, generator=g) * 0.5).half().cuda()
    Hid[:, 0] += (torch.arange(M, device="cuda") % 64).half() * 0.01
    Hid[:, 5] += (torch.arange(M, device="cuda") // 32 % 16).half() * 0.02            # differs between 32-row blocks
    ref = Hid.float() @ W2.float().t() + b2
    hb = to_blocked16(Hid)
    o_b = torch.full((M, D), float("nan"), device="cuda", dtype=torch.half)
    ctx.check(ctx.lib.srh_op_gemm_ex(ctx.handle, _p(hb), _p(W2), _p(b2), None, M, D, H, 0, None, _p(o_b), SRH_GEMM_A_BLOCKED16, None), "srh_op_gemm_ex")
    o_r = torch.full((M, D), float("nan"), device="cuda", dtype=torch.half)
    ctx.check(ctx.lib.srh_op_gemm(ctx.handle, _p(Hid), _p(W2), _p(b2), None, M, D, H, 0, None, _p(o_r), None), "srh_op_gemm")
    _sync()
    assert torch.isfinite(o_b).all()
    tolerances.check("op_gemm_z192_body2[%d,%d,%d] max-abs / scale" % (M, D, H), (o_b.float() - ref).abs().max().item() / max(ref.abs().max().item(), 1.0),
                     tolerances.GEMM_F16_OUT)
    assert torch.equal(o_b, o_r), "blocked-16-A and row-major bodies differ"


@pytest.mark.parametrize("M,D,H", _MLP_SHAPES)
def test_gemm_z192_mlp_pair_blocked_hidden(ctx, M, D, H):
    """fc1 (body 3) -> fc2 (body 2) with the hidden activation handed over in the blocked-16 layout, exactly as srh_encode_decode
    chains them (csrc/api_model.hip; reference: the SAM fork's MLPBlock via model.py:245-258), against fp32 torch on the fp16-rounded hidden
    activation — and against the row-major pair bit for bit."""
    from sam_road_amd._lib import SRH_GEMM_A_BLOCKED16, SRH_GEMM_OUT_BLOCKED16
    A, W1, W2, b1, b2 = _mlp_operands(M, D, H, M + D + H)
    hid_ref = F.gelu(A.float() @ W1.float().t() + b1).half()
    ref = hid_ref.float() @ W2.float().t() + b2
    hid = torch.full((M * H,), float("nan"), device="cuda", dtype=torch.half)
    out = torch.full((M, D), float("nan"), device="cuda", dtype=torch.half)
    ctx.check(ctx.lib.srh_op_gemm_ex(ctx.handle, _p(A), _p(W1), _p(b1), None, M, H, D, 1, None, _p(hid), SRH_GEMM_OUT_BLOCKED16, None), "srh_op_gemm_ex")
    ctx.check(ctx.lib.srh_op_gemm_ex(ctx.handle, _p(hid), _p(W2), _p(b2), None, M, D, H, 0, None, _p(out), SRH_GEMM_A_BLOCKED16, None), "srh_op_gemm_ex")
    hid_r = torch.full((M, H), float("nan"), device="cuda", dtype=torch.half)
    out_r = torch.full((M, D), float("nan"), device="cuda", dtype=torch.half)
    ctx.check(ctx.lib.srh_op_gemm(ctx.handle, _p(A), _p(W1), _p(b1), None, M, H, D, 1, None, _p(hid_r), None), "srh_op_gemm")
    ctx.check(ctx.lib.srh_op_gemm(ctx.handle, _p(hid_r), _p(W2), _p(b2), None, M, D, H, 0, None, _p(out_r), None), "srh_op_gemm")
    _sync()
    assert torch.isfinite(out).all()
    # the hidden activation the kernel produced can differ from torch's by one fp16 ulp on a few elements (the GELU fit, 1.6e-6): the
    # pair's bound is the single-GEMM bound plus that
    tolerances.check("op_gemm_z192_mlp_pair[%d,%d,%d] max-abs / scale" % (M, D, H), (out.float() - ref).abs().max().item() / max(ref.abs().max().item(), 1.0),
                     tolerances.GEMM_MLP_PAIR)
    assert torch.equal(out, out_r), "blocked-16 and row-major MLP pairs differ"


def test_gemm_ex_refuses_what_no_body_covers(ctx):
    """The blocked-16 flags exist only for the generated bodies: other combinations return SRH_ERR_UNSUPPORTED instead of running a
    kernel that would misread the layout."""
    from sam_road_amd._lib import SRH_GEMM_A_BLOCKED16, SRH_GEMM_OUT_BLOCKED16, SrhError
    A, W1, W2, b1, b2 = _mlp_operands(8192, 768, 3072, 1)
    out = torch.zeros((8192 * 3072,), device="cuda", dtype=torch.half)
    for args in ((A, W1, b1, 8192, 3072, 768, 0, SRH_GEMM_OUT_BLOCKED16),                          # blocked output without GELU
                 (A, W1, b1, 8192, 3072, 768, 1, SRH_GEMM_OUT_BLOCKED16 | SRH_GEMM_A_BLOCKED16),   # both
                 (A, W1, None, 8192, 3072, 768, 1, SRH_GEMM_OUT_BLOCKED16),                        # no bias
                 (A[:1024], W1, b1, 1024, 3072, 768, 1, SRH_GEMM_OUT_BLOCKED16)):                  # 64 tiles: not the persistent kernel's range
        a, w, b, M, N, K, act, flags = args
        with pytest.raises(SrhError):
            ctx.check(ctx.lib.srh_op_gemm_ex(ctx.handle, _p(a), _p(w), _p(b), None, M, N, K, act, None, _p(out), flags, None), "srh_op_gemm_ex")
    _sync()


def test_ctx_memory_is_flat_over_batch_sizes(ctx):
    """gemm_z192 keeps one tile-order table per (shape, pitch) on the device.  They live in ONE bounded slab the context owns
    (ZTileTables, csrc/gemm_z192.hip): cycling through more distinct row counts than the slab has slots (32) neither grows the context
    nor the device's used memory, and a shape that was evicted still computes the same bits when it comes back."""
    D, N = 768, 1536
    g = torch.Generator().manual_seed(11)
    Mmax = 8192 + 256 * 47
    A = (torch.randn(Mmax, D, generator=g) * 0.5).half().cuda()
    W = (torch.randn(N, D, generator=g) * 0.05).half().cuda()
    b = torch.randn(N, generator=g).cuda()
    out = torch.zeros((Mmax, N), device="cuda", dtype=torch.half)

    def run(M):
        ctx.check(ctx.lib.srh_op_gemm(ctx.handle, _p(A), _p(W), _p(b), None, M, N, D, 0, None, _p(out), None), "srh_op_gemm")
    run(8192)
    _sync()
    first = out[:8192].clone()
    ctx_bytes = ctx.lib.srh_ctx_device_bytes(ctx.handle)
    free0 = torch.cuda.mem_get_info()[0]
    assert ctx_bytes > 0
    for k in range(48):                                   # 48 distinct shapes through a 32-slot slab
        run(8192 + 256 * k)
    run(8192)                                             # evicted meanwhile: rebuilt
    _sync()
    assert torch.equal(out[:8192], first)
    assert ctx.lib.srh_ctx_device_bytes(ctx.handle) == ctx_bytes
    assert abs(torch.cuda.mem_get_info()[0] - free0) <= (8 << 20), "device memory moved while cycling GEMM shapes"


def test_gemm_inplace_residual(ctx):
    M, N, K = 384, 256, 128
    g = torch.Generator().manual_seed(5)
    A = torch.randn(M, K, generator=g).half()
    W = (torch.randn(N, K, generator=g) * 0.1).half()
    X = torch.randn(M, N, generator=g)
    ref = X + A.float() @ W.float().t()
    dX, dA, dW = X.cuda(), A.cuda(), W.cuda()   # keep the device tensors alive across the async call
    ctx.check(ctx.lib.srh_op_gemm(ctx.handle, _p(dA), _p(dW), None, _p(dX), M, N, K, 0, _p(dX), None, None),
              "srh_op_gemm")
    _sync()
    assert (dX.cpu() - ref).abs().max().item() < 1e-3


# (3, 32, 256, 256): the neck's shape (ViT-B tiles) with three images — taps must not cross from one image into the next;
# (1, 64, 64, 128): one k-tile per tap, a 1024-px tile's grid
@pytest.mark.parametrize("B,S,Cc,N", [(2, 16, 128, 128), (3, 32, 256, 256), (1, 64, 64, 128)])
def test_conv3x3(ctx, B, S, Cc, N):
    g = torch.Generator().manual_seed(9 + B + S)
    x = torch.randn(B, Cc, S, S, generator=g).half()
    w = (torch.randn(N, Cc, 3, 3, generator=g) * 0.05).half()
    ref = F.conv2d(x.float(), w.float(), padding=1).permute(0, 2, 3, 1)          # [B,S,S,N]
    a = x.permute(0, 2, 3, 1).contiguous().cuda()                                  # channels-last
    wg = w.permute(0, 2, 3, 1).reshape(N, 9 * Cc).contiguous().cuda()              # k = tap*C + c
    out = torch.zeros((B, S, S, N), device="cuda")
    ctx.check(ctx.lib.srh_op_conv3x3(ctx.handle, _p(a), _p(wg), B, S, Cc, N, _p(out), None), "srh_op_conv3x3")
    _sync()
    assert (out.cpu() - ref).abs().max().item() < 2e-3


@pytest.mark.parametrize("D,gelu", [(768, 0), (256, 0), (128, 1), (1024, 0), (1280, 0)])
def test_layernorm(ctx, D, gelu):
    M = 517
    g = torch.Generator().manual_seed(D)
    x = torch.randn(M, D, generator=g) * 3 + 1.5
    gm, bt = torch.randn(D, generator=g), torch.randn(D, generator=g)
    ref = F.layer_norm(x, (D,), gm, bt, 1e-6)
    if gelu:
        ref = F.gelu(ref)
    o32 = torch.zeros((M, D), device="cuda")
    o16 = torch.zeros((M, D), device="cuda", dtype=torch.half)
    dx, dg, db = x.cuda(), gm.cuda(), bt.cuda()
    ctx.check(ctx.lib.srh_op_layernorm(ctx.handle, _p(dx), _p(dg), _p(db), 1e-6, M, D, gelu,
                                       _p(o32), _p(o16), None), "srh_op_layernorm")
    _sync()
    assert (o32.cpu() - ref).abs().max().item() < 2e-5
    assert (o16.cpu().float() - ref).abs().max().item() < 5e-3
    # cast-only mode
    ctx.check(ctx.lib.srh_op_layernorm(ctx.handle, _p(dx), None, None, 0.0, M, D, 0, None, _p(o16), None),
              "srh_op_layernorm(cast)")
    _sync()
    assert torch.equal(o16.cpu(), x.half())


def ref_sam_attention(qkv, rel_h, rel_w, bias, B, S, heads, win, hd=64):
    """SURVEY App. B.2-B.4 on a fused qkv tensor [B,S,S,3D] (fp32 math): window partition with pad
    tokens = qkv bias, decomposed rel-pos from the unscaled q, softmax, un-partition + crop."""
    D = heads * hd
    x = qkv.float().view(B, S, S, 3 * D)
    if win < S:
        pad = (win - S % win) % win
        Sp = S + pad
        full = bias.float().view(1, 1, 1, 3 * D).expand(B, Sp, Sp, 3 * D).clone()
        full[:, :S, :S] = x
        nw = Sp // win
        xw = full.view(B, nw, win, nw, win, 3 * D).permute(0, 1, 3, 2, 4, 5).reshape(-1, win, win, 3 * D)
    else:
        xw, Sp, nw = x, S, 1
    Bp = xw.shape[0]
    q, k, v = xw.reshape(Bp, win * win, 3, heads, hd).permute(2, 0, 3, 1, 4).reshape(3, Bp * heads, win * win, hd).unbind(0)
    attn = (q * hd ** -0.5) @ k.transpose(-2, -1)
    idx = torch.arange(win)[:, None] - torch.arange(win)[None, :] + (win - 1)
    Rh, Rw = rel_h.float()[idx], rel_w.float()[idx]
    rq = q.reshape(-1, win, win, hd)
    attn = (attn.view(-1, win, win, win, win) + torch.einsum("bhwc,hkc->bhwk", rq, Rh)[:, :, :, :, None]
            + torch.einsum("bhwc,wkc->bhwk", rq, Rw)[:, :, :, None, :]).view(-1, win * win, win * win)
    out = (attn.softmax(-1) @ v).view(Bp, heads, win, win, hd).permute(0, 2, 3, 1, 4).reshape(Bp, win, win, D)
    if win < S:
        out = out.view(B, nw, nw, win, win, D).permute(0, 1, 3, 2, 4, 5).reshape(B, Sp, Sp, D)[:, :S, :S]
    return out.reshape(B * S * S, D)


# hd = 80 is ViT-H (toponet_vith_256.yaml, BASELINE configs[4]): windows of 14 and the 16x16 global window run
# attention_hdx.hip, the 32x32 global window of a 512-pixel ViT-H tile the generic kernel.  Same peaked-softmax
# inputs as hd = 64 (q, k ~ N(0, 1.5), rel-pos tables 0.3): logits reach tens, which whole-model tests with
# 0.02-std weights never produce.
# (64, 64, 64): the global window of 1024-px tiles (toponet_vitb_1024.yaml) — attn_global_kernel<64>: a key tile is half a window row,
# the two rel-pos tables (127 rows) fill both ring stages; heads = 4 there so that B * heads = 8 takes the XCD-aware workgroup order.
# (48, 14) and (64, 14): window geometries the 512-px path never produces — 3 query tiles (a wave without work), 4 (one each), 2 of
# 64 and 36 queries (key split) — for the windowed kernel's work split.
@pytest.mark.parametrize("S,win,hd", [(32, 14, 64), (32, 32, 64), (16, 14, 64), (16, 16, 64), (48, 14, 64), (64, 14, 64), (64, 64, 64),
                                      (16, 14, 80), (16, 16, 80), (32, 14, 80), (32, 32, 80),
                                      # attention_hdx's workgroup slots (window, part of four query tiles): 25 slots with 3- and 2-tile edge
                                      # windows at S = 48, 41 slots at S = 64 (1024-px ViT-H tiles)
                                      (48, 14, 80), (64, 14, 80)])
def test_sam_attention(ctx, S, win, hd):
    B, heads = 2, (4 if (S, win) == (64, 64) else 3)
    D = heads * hd
    g = torch.Generator().manual_seed(S * 100 + win + hd)
    qkv = (torch.randn(B * S * S, 3 * D, generator=g) * 1.5).half()
    bias = (torch.randn(3 * D, generator=g) * 0.5).half()
    rel_h = (torch.randn(2 * win - 1, hd, generator=g) * 0.3).half()
    rel_w = (torch.randn(2 * win - 1, hd, generator=g) * 0.3).half()
    ref = ref_sam_attention(qkv, rel_h, rel_w, bias, B, S, heads, win, hd)
    out = torch.zeros((B * S * S, D), device="cuda", dtype=torch.half)
    dq, dh, dw, db = qkv.cuda(), rel_h.cuda(), rel_w.cuda(), bias.cuda()
    if hd == 64:        # the original export stays covered
        ctx.check(ctx.lib.srh_op_attention(ctx.handle, _p(dq), _p(dh), _p(dw), _p(db),
                                           B, S, heads, win, _p(out), None), "srh_op_attention")
    else:
        ctx.check(ctx.lib.srh_op_attention_hd(ctx.handle, _p(dq), _p(dh), _p(dw), _p(db),
                                              B, S, heads, hd, win, _p(out), None), "srh_op_attention_hd")
    _sync()
    err = (out.cpu().float() - ref).abs()
    assert torch.isfinite(out.cpu().float()).all()
    tag = "op_attention[S=%d,win=%d,hd=%d]" % (S, win, hd)
    tolerances.check(tag + " max-abs", err.max().item(), tolerances.ATTN_OP_MAX)
    tolerances.check(tag + " mean-abs", err.mean().item(), tolerances.ATTN_OP_MEAN)
