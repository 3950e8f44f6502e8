"""Plain float64 CPU references of the heads after the encoder, for the op-level tests (tests/test_gpu_heads.py).

Each restates one reference operation directly from its definition, independent of the HIP kernels' layouts:
  - ``map_decoder_ref``: the naive map_decoder (reference model.py:286-295: ConvTranspose2d k2 s2 x4, LayerNorm2d, exact-erf GELU)
    + sigmoid + NCHW -> NHWC (model.py:445-446);
  - ``sample_ref``: BilinearSampler (model.py:34-58: F.grid_sample, bilinear, align_corners=False, zero padding) over
    channels-last embeddings;
  - ``pair_gather_ref``: the pair rows TopoNet feeds pair_proj (model.py:104-116: src | tgt features | tgt - src offset),
    laid out as the library's pair buffer (zero padding up to the row stride).
tests/test_heads_ref.py pins each of them to oracle/samroad.py's fp32 modules, so a wrong reference fails on any host.
"""
import math

import torch

_MD_LAYERS = ((0, 256, 128), (3, 128, 64), (5, 64, 32), (7, 32, 2))     # (Sequential index, Cin, Cout) of the four ConvT layers
# ConvT weight scales of the decoder tests: with LayerNorm2d gamma in +-[1, 2] and beta in [-1.5, 1.5] and N(0, 1) inputs and biases the
# pre-activations of every GELU reach about +-8 and the logits about +-15
DECODER_STDS = (0.1, 0.085, 0.16, 0.45)


def _convt2x2(x, w, b):
    """ConvTranspose2d(kernel 2, stride 2) from its definition: out[n, co, 2y + ky, 2x + kx] = b[co] + sum_ci x[n, ci, y, x] w[ci, co, ky, kx]."""
    n, _, h, wd = x.shape
    co = w.shape[1]
    y = torch.einsum("ncyx,cokl->noykxl", x, w)
    return y.reshape(n, co, 2 * h, 2 * wd) + b.view(1, co, 1, 1)


def _gelu(x):
    return 0.5 * x * (1.0 + torch.special.erf(x / math.sqrt(2.0)))


def map_decoder_ref(emb_tokens, sd, tiles_per_step=2):
    """emb_tokens [B, S, S, 256] (channels-last neck output), sd = the map_decoder.* entries of a state dict
    -> (logits, scores) float64 [B, 16 S, 16 S, 2] (NHWC).  Computed a few tiles at a time (a 512-px tile's layer-5 activation is 16 MB)."""
    p = {k: v.detach().cpu().to(torch.float64) for k, v in sd.items() if k.startswith("map_decoder.")}
    B, S = emb_tokens.shape[0], emb_tokens.shape[1]
    P = 16 * S
    logits = torch.empty(B, P, P, 2, dtype=torch.float64)
    for b0 in range(0, B, tiles_per_step):
        x = emb_tokens[b0:b0 + tiles_per_step].to(torch.float64).permute(0, 3, 1, 2)
        for i, (idx, _, _) in enumerate(_MD_LAYERS):
            x = _convt2x2(x, p[f"map_decoder.{idx}.weight"], p[f"map_decoder.{idx}.bias"])
            if idx == 0:        # LayerNorm2d(128), eps 1e-6, biased variance
                u = x.mean(1, keepdim=True)
                v = (x - u).pow(2).mean(1, keepdim=True)
                x = (x - u) / torch.sqrt(v + 1e-6)
                x = p["map_decoder.1.weight"].view(1, -1, 1, 1) * x + p["map_decoder.1.bias"].view(1, -1, 1, 1)
            if i < 3:
                x = _gelu(x)
        logits[b0:b0 + tiles_per_step] = x.permute(0, 2, 3, 1)
    return logits, 1.0 / (1.0 + torch.exp(-logits))


def sample_ref(emb, points, patch, point_tile=None):
    """emb [n_tiles, h, w, C] channels-last, points [B, N, 2] (x, y) pixels of a ``patch``-px tile, point_tile [B*N] (optional: tile
    of every point, clamped into [0, n_tiles); default tile b for batch b) -> float64 [B*N, C].  grid = p / patch * 2 - 1
    (model.py:47), then ATen's unnormalisation with align_corners=False: i = ((g + 1) * size - 1) / 2; four taps, a tap outside
    the map contributes zero."""
    e = emb.to(torch.float64)
    n_tiles, h, w, C = e.shape
    B, N = points.shape[0], points.shape[1]
    pts = points.reshape(B * N, 2).to(torch.float64)
    if point_tile is None:
        tile = torch.arange(B).repeat_interleave(N)
    else:
        tile = point_tile.reshape(-1).long().clamp(0, n_tiles - 1)
    g = pts / patch * 2.0 - 1.0
    ix = ((g[:, 0] + 1.0) * w - 1.0) / 2.0
    iy = ((g[:, 1] + 1.0) * h - 1.0) / 2.0
    x0, y0 = torch.floor(ix), torch.floor(iy)
    out = torch.zeros(B * N, C, dtype=torch.float64)
    for dy in (0, 1):
        for dx in (0, 1):
            xx, yy = x0 + dx, y0 + dy
            wgt = (1.0 - (ix - xx).abs()) * (1.0 - (iy - yy).abs())
            inside = (xx >= 0) & (xx < w) & (yy >= 0) & (yy < h)
            xi, yi = xx.clamp(0, w - 1).long(), yy.clamp(0, h - 1).long()
            v = e[tile, yi, xi]
            out += torch.where(inside[:, None], v * wgt[:, None], torch.zeros((), dtype=torch.float64))
    return out


def pair_gather_ref(pf, points, pairs, ld, zero_offset=False, index_base=0):
    """pf [B, N, 128] point features (relu(feature_proj)), points [B, N, 2], pairs [B, Ns, K, 2] (source, target) -> float64
    [B*Ns*K, ld] = src features | tgt features | tgt - src (zeros with TOPONET_VERSION no_offset) | zeros.  Indices are
    ``pairs - index_base``; with index_base 0 a negative one wraps as Python's does (model.py:104-108 indexes with the pairs as
    given), with a non-zero base (a chunk of a longer row list) it must lie in [0, N)."""
    B, N = pf.shape[0], pf.shape[1]
    idx = pairs.reshape(B, -1, 2).long() - index_base
    lo = -N if index_base == 0 else 0
    assert bool(((idx >= lo) & (idx < N)).all()), "out-of-range pair index (an IndexError in the reference)"
    idx = torch.where(idx < 0, idx + N, idx)
    bidx = torch.arange(B).view(-1, 1).expand(-1, idx.shape[1])
    f = pf.to(torch.float64)
    p = points.to(torch.float64)
    src, tgt = idx[..., 0], idx[..., 1]
    off = p[bidx, tgt] - p[bidx, src]
    if zero_offset:
        off = torch.zeros_like(off)
    rows = torch.cat([f[bidx, src], f[bidx, tgt], off], dim=2).reshape(-1, 258)
    out = torch.zeros(rows.shape[0], ld, dtype=torch.float64)
    out[:, :258] = rows
    return out
