"""Plain float64 CPU references of the heads after the encoder, for the op-level tests (tests/test_gpu_heads.py).

Each restates one reference operation directly from its definition, independent of the HIP kernels' layouts:
  - ``map_decoder_ref``: the naive map_decoder (reference model.py:286-295: ConvTranspose2d k2 s2 x4, LayerNorm2d, exact-erf GELU)
    + sigmoid + NCHW -> NHWC (model.py:445-446);
  - ``sample_ref``: BilinearSampler (model.py:34-58: F.grid_sample, bilinear, align_corners=False, zero padding) over
    channels-last embeddings;
  - ``pair_gather_ref``: the pair rows TopoNet feeds pair_proj (model.py:104-116: src | tgt features | tgt - src offset),
    laid out as the library's pair buffer (zero padding up to the row stride);
  - ``topo_trunk_ref``: TopoNet after the gather (model.py:118-148: pair_proj, the three post-LN encoder layers, output_proj, sigmoid)
    as explicit math, and ``toponet_ref``, the chain of the four (tests/test_gpu_topo_trunk.py), with ``topo_fill`` /
    ``topo_trunk_inputs``, the O(1)-parameter model and the inputs those tests and their CPU pins share.
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


# ---- the TopoNet trunk (model.py:118-148): pair_proj, three post-LN encoder layers, output_proj, sigmoid ---------------------------------
_TL = "topo_net.transformer_encoder.layers."
TOPO_HEADS, TOPO_HD, TOPO_D = 4, 32, 128


def _r16(x):
    return x.to(torch.float16).to(torch.float64)


def _layernorm(y, gamma, beta):
    u = y.mean(-1, keepdim=True)
    v = (y - u).pow(2).mean(-1, keepdim=True)                  # biased variance
    return (y - u) / torch.sqrt(v + 1e-5) * gamma + beta


def topo_key_mask(valid, K, no_flip=False):
    """valid [nseq, K] (any non-zero byte counts) -> bool [nseq, K]: the keys a sequence attends to; one without any valid slot attends
    to all of them (model.py:129-130)."""
    m = valid.reshape(-1, K) != 0
    if not no_flip:
        m = m | ~m.any(-1, keepdim=True)
    return m


def topo_trunk_ref(rows, valid, sd, K, round_points=False, mutate=None, probe=None):
    """rows [nseq*K, >= 258] pair rows (src | tgt features | dx dy | anything), valid [nseq, K], sd = the topo_net.* entries of a state
    dict (without encoder layers: TOPONET_VERSION no_transformer) -> (logits, scores) float64 [nseq*K].

    Explicit math, no nn.TransformerEncoder (whose fast path rewrites masked slots): x = relu(pair_proj(row)); per layer
    q, k, v = in_proj(x) in 4 heads of 32, S = q k^T / sqrt(32), masked keys -> -inf, P = softmax(S), x = LN1(x + out_proj(P v)),
    x = LN2(x + linear2(relu(linear1(x)))) with eps 1e-5 and the biased variance; logit = output_proj(x).

    round_points: round to fp16 wherever csrc/topo_fused.hip does — every MFMA operand made from the residual stream (the pair_proj
    output and each LayerNorm output; the stream itself stays unrounded), q, k, v, the unnormalised P = exp(S - max) (its sum is
    taken before the rounding), O, and the FFN's hidden activation.  The a-priori error estimate of tests/tolerances.py.

    mutate (tests/test_heads_ref.py, the mistakes a fused kernel could make; parameter mix-ups are made in `sd` instead):
      scale: the softmax scale; ignore_mask; mask_shift: roll the key mask by that many keys; no_flip: an all-invalid sequence
      attends to nothing (P = 0); swap_v_heads (a, b); leak: sequence i also attends to the keys of sequence i ^ 1, its tile mate
      where the kernel packs two or more sequences into one tile (K <= 8).
    probe: a dict that receives layer 0's raw logits ``s`` [nseq, 4, K, K] (query, key), ``p`` and the key mask ``mask``."""
    mu = dict(mutate or {})
    r = _r16 if round_points else (lambda t: t)
    p = {k: v.detach().cpu().to(torch.float64) for k, v in sd.items() if k.startswith("topo_net.")}
    n_layers = len({k[len(_TL):].split(".")[0] for k in p if k.startswith(_TL)})
    x = rows[:, :258].to(torch.float64)
    nseq = x.shape[0] // K
    assert x.shape[0] == nseq * K and tuple(valid.shape) == (nseq, K)
    x = torch.relu(x @ p["topo_net.pair_proj.weight"].T + p["topo_net.pair_proj.bias"])
    mask = topo_key_mask(valid, K, no_flip=bool(mu.get("no_flip")))
    if mu.get("ignore_mask"):
        mask = torch.ones_like(mask)
    if mu.get("mask_shift"):
        mask = torch.roll(mask, int(mu["mask_shift"]), dims=1)
    mate = None
    if mu.get("leak"):
        mate = torch.arange(nseq) ^ 1
        mate_ok = mate < nseq
        mate = mate.clamp(max=nseq - 1)
        mask = torch.cat([mask, mask[mate] & mate_ok[:, None]], 1)
    scale = float(mu.get("scale", TOPO_HD ** -0.5))
    for L in range(n_layers):
        pre = f"{_TL}{L}."
        xo = r(x)
        qkv = r(xo @ p[pre + "self_attn.in_proj_weight"].T + p[pre + "self_attn.in_proj_bias"])
        q, k, v = (t.reshape(nseq, K, TOPO_HEADS, TOPO_HD).permute(0, 2, 1, 3) for t in qkv.split(TOPO_D, dim=1))
        if mu.get("swap_v_heads"):
            a, b = mu["swap_v_heads"]
            v = v.clone()
            v[:, [a, b]] = v[:, [b, a]]
        if mate is not None:
            k, v = torch.cat([k, k[mate]], 2), torch.cat([v, v[mate]], 2)
        s = q @ k.transpose(2, 3)                              # [nseq, head, query, key], unscaled
        sm = s.masked_fill(~mask[:, None, None, :], float("-inf"))
        top = sm.amax(-1, keepdim=True)
        e = torch.exp((sm - torch.where(torch.isfinite(top), top, torch.zeros_like(top))) * scale)
        den = e.sum(-1, keepdim=True)
        o = r((r(e) @ v) / torch.where(den > 0, den, torch.ones_like(den)))
        if probe is not None and L == 0:
            probe.update(s=s * scale, p=e / den, mask=mask)
        o = o.permute(0, 2, 1, 3).reshape(nseq * K, TOPO_D)
        y = x + o @ p[pre + "self_attn.out_proj.weight"].T + p[pre + "self_attn.out_proj.bias"]
        x = _layernorm(y, p[pre + "norm1.weight"], p[pre + "norm1.bias"])
        h = r(torch.relu(r(x) @ p[pre + "linear1.weight"].T + p[pre + "linear1.bias"]))
        y = x + h @ p[pre + "linear2.weight"].T + p[pre + "linear2.bias"]
        x = _layernorm(y, p[pre + "norm2.weight"], p[pre + "norm2.bias"])
    logits = x @ p["topo_net.output_proj.weight"][0] + p["topo_net.output_proj.bias"][0]
    return logits, 1.0 / (1.0 + torch.exp(-logits))


def toponet_ref(emb, points, pairs, valid, sd, patch, zero_offset=False, round_points=False):
    """The whole TopoNet head as srh_toponet chains it: emb [B, h, w, 256] channels-last, points [B, N, 2], pairs [B, Ns, K, 2], valid
    [B, Ns, K] -> (logits, scores) float64 [B*Ns*K].  sample_ref, feature_proj + ReLU, pair_gather_ref, topo_trunk_ref, with the fp16
    roundings of the product path between the launches (the sampled features, the projected point features and the pair rows are
    fp16 buffers there), which are part of the operation and not of round_points."""
    K = pairs.shape[2]
    B, N = points.shape[0], points.shape[1]
    feats = _r16(sample_ref(emb, points, patch))
    w, b = (sd["topo_net.feature_proj." + n].detach().cpu().to(torch.float64) for n in ("weight", "bias"))
    pf = _r16(torch.relu(feats @ w.T + b)).reshape(B, N, TOPO_D)
    rows = _r16(pair_gather_ref(pf, points, pairs, 320, zero_offset=zero_offset))
    return topo_trunk_ref(rows, valid.reshape(-1, K), sd, K, round_points=round_points)


# Weight scales of the trunk tests (topo_fill), chosen on the CPU so that tests/test_heads_ref.py's assertions hold: the shares of
# peaked and flat layer-0 softmax rows, and every mutation's margin.  Matrices are N(0, 1 / fan_in) on inputs of O(1), except:
#   - the q rows are small: q = Wq x + bq is half bias, so a misplaced q bias changes the attention;
#   - the k rows grow head by head, from flat (head 3: the logits of a row differ by well under 1) to peaked (head 0) softmax rows, and
#     layer by layer, since the LayerNorm outputs that layers 1 and 2 read differ less from token to token than layer 0's input does
#     (every LayerNorm adds the same beta ~ N(0, 1) to all tokens);
#   - pair_proj's dx, dy columns are scaled down: the offsets reach +-528 against features of O(1).
TOPO_Q_STD = 0.05
TOPO_K_HEAD_STD = (0.6, 0.3, 0.1, 0.03)
TOPO_K_LAYER_GAIN = (2.0, 2.0, 3.0)
TOPO_OFFSET_COL_SCALE = 1.0 / 64


def _f16(t):
    return t.to(torch.float16).to(torch.float32)


def _signed_1_2(n, g):
    return (1.0 + torch.rand(n, generator=g)) * torch.sign(torch.randn(n, generator=g))


def topo_fill(sd, seed):
    """The topo_net.* entries of the trunk tests' model, replacing those of ``sd`` (which decides whether there are encoder layers):
    every matrix fp16-representable (the kernel's fp16 copies are exact), every bias, every LayerNorm beta and output_proj's bias
    ~ N(0, 1), every gamma in +-[1, 2], so that a misplaced additive parameter moves the output by O(1) and not by 0.02."""
    g = torch.Generator().manual_seed(seed)
    out = {}

    def mat(rows, cols, std=None):
        return _f16(torch.randn(rows, cols, generator=g) * (std if std is not None else cols ** -0.5))

    out["topo_net.output_proj.weight"] = mat(1, TOPO_D)
    out["topo_net.output_proj.bias"] = torch.randn(1, generator=g)
    for name in ("feature_proj", "pair_proj"):
        cols = sd[f"topo_net.{name}.weight"].shape[1]
        w = mat(TOPO_D, cols)
        if name == "pair_proj":
            w[:, 256:] = _f16(w[:, 256:] * TOPO_OFFSET_COL_SCALE)
        out[f"topo_net.{name}.weight"] = w
        out[f"topo_net.{name}.bias"] = torch.randn(TOPO_D, generator=g)
    L = 0
    while f"{_TL}{L}.norm1.weight" in sd:
        pre = f"{_TL}{L}."
        w = mat(3 * TOPO_D, TOPO_D)
        for h, std in enumerate(TOPO_K_HEAD_STD):
            w[h * TOPO_HD:(h + 1) * TOPO_HD] = mat(TOPO_HD, TOPO_D, TOPO_Q_STD)
            w[TOPO_D + h * TOPO_HD:TOPO_D + (h + 1) * TOPO_HD] = mat(TOPO_HD, TOPO_D, std * TOPO_K_LAYER_GAIN[L])
        out[pre + "self_attn.in_proj_weight"] = w
        out[pre + "self_attn.in_proj_bias"] = torch.randn(3 * TOPO_D, generator=g)
        for name in ("self_attn.out_proj", "linear1", "linear2"):
            out[pre + name + ".weight"] = mat(TOPO_D, TOPO_D)
            out[pre + name + ".bias"] = torch.randn(TOPO_D, generator=g)
        for name in ("norm1", "norm2"):
            out[pre + name + ".weight"] = _signed_1_2(TOPO_D, g)
            out[pre + name + ".bias"] = torch.randn(TOPO_D, generator=g)
        L += 1
    assert set(out) == {k for k in sd if k.startswith("topo_net.")}, "topo_fill must set every TopoNet parameter"
    return out


TOPO_VALID_KINDS = ("all", "none", "first", "last", "middle", "alternating", "random")


def topo_trunk_inputs(nseq, K, seed, ld=320):
    """Pair rows fp16 [nseq*K, ld] as the pair gather writes them (features >= 0 as ReLU outputs are, integer dx, dy up to +-528,
    zeros from column 258) and valid u8 [nseq, K]: per sequence, cycling through TOPO_VALID_KINDS; valid bytes are 1 or 255."""
    g = torch.Generator().manual_seed(seed)
    rows = torch.zeros(nseq * K, ld, dtype=torch.float16)
    # sparse features (two thirds are zero), the source half shared by the K rows of a sequence as the gather shares it, and a per-row
    # magnitude between 0.5 and 2: some rows' features (and so their attention logits) are small, others large
    def feats(n):
        return torch.relu(torch.randn(n, 128, generator=g) - 0.4) * 2.5
    mag = 0.5 + 1.5 * torch.rand(nseq * K, 1, generator=g)
    rows[:, :128] = feats(nseq).repeat_interleave(K, 0).to(torch.float16)
    rows[:, 128:256] = (feats(nseq * K) * mag).to(torch.float16)
    rows[:, 256:258] = torch.randint(-528, 529, (nseq * K, 2), generator=g).to(torch.float16)
    valid = torch.zeros(nseq, K, dtype=torch.bool)
    kind = torch.arange(nseq) % len(TOPO_VALID_KINDS)
    valid[kind == 0] = True
    valid[kind == 2, 0] = True
    valid[kind == 3, K - 1] = True
    valid[kind == 4, K // 2] = True
    valid[kind == 5, ::2] = True
    rnd = torch.rand(nseq, K, generator=g) < 0.5
    valid[kind == 6] = rnd[kind == 6]
    byte = torch.where(torch.rand(nseq, K, generator=g) < 0.5, 1, 255).to(torch.uint8)
    return rows, torch.where(valid, byte, torch.zeros_like(byte))


def toponet_chain_inputs(K, i64, patch=256, B=2, N=40, Ns=12):
    """A small srh_toponet problem: embeddings [B, patch / 16, patch / 16, 256] channels-last of O(3), N points per tile up to 24 px outside
    it (i64 or fractional f32), random pairs [B, Ns, K, 2], valid at 0.6 with one all-invalid and one all-valid sequence."""
    g = torch.Generator().manual_seed(10 * K + int(i64))
    emb = torch.randn(B, patch // 16, patch // 16, 256, generator=g) * 3.0
    if i64:
        points = torch.randint(-24, patch + 24, (B, N, 2), generator=g)
    else:
        points = torch.rand(B, N, 2, generator=g) * (patch + 48) - 24
    pairs = torch.randint(0, N, (B, Ns, K, 2), generator=g)
    valid = torch.rand(B, Ns, K, generator=g) < 0.6
    valid[0, 0] = False                                        # the flip
    valid[0, 1] = True
    return emb, points, pairs, valid


def topo_op_bounds(tolerances, version):
    """(logit, score) bounds of the op-level trunk tests: without encoder layers nothing is rounded to fp16 and the bounds are f32's."""
    if version == "no_transformer":
        return tolerances.TOPO_OP_NOATT_LOGIT, tolerances.TOPO_OP_NOATT_SCORE
    return tolerances.TOPO_OP_LOGIT, tolerances.TOPO_OP_SCORE


def topo_defined(valid):
    """Slots whose output is part of the contract: the valid ones, and every slot of a sequence without any (model.py:129-130)."""
    v = valid != 0
    return v | ~v.any(-1, keepdim=True)
