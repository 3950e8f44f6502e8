"""Plain float64 CPU reference of the SAM MaskDecoder branch (USE_SAM_DECODER), for the op-level tests (tests/test_gpu_samdec.py).

Written from oracle/sam_decoder.py as explicit math, independent of the HIP kernels' layouts (csrc/sam_decoder.hip, sam_decode() in
csrc/api_model.hip): PromptEncoder's no-prompt path (no_mask_embed, the random-Fourier encoding of the S x S grid), the
TwoWayTransformer over the 4 output tokens and the S*S image tokens, the two ConvTranspose upscalings, the hyper-network dot products,
masks 1 and 2 of the 3, bilinear x4 (align_corners=False), sigmoid.  With it: ``samdec_fill``, the O(1)-parameter model the op tests
run, and ``samdec_inputs``, their embeddings.  tests/test_samdec_ref.py pins ``samdec_ref`` to the oracle's modules in float64 and
shows that the model and the inputs tell a subtly wrong kernel from a right one, on any host.
"""
import math

import torch

HEADS = 8
_PE, _MD, _TR = "prompt_encoder.", "mask_decoder.", "mask_decoder.transformer."
T2I_NAMES = ("layers.0.cross_attn_token_to_image", "layers.1.cross_attn_token_to_image", "final_attn_token_to_image")
I2T_NAMES = ("layers.0.cross_attn_image_to_token", "layers.1.cross_attn_image_to_token")


def _r16(x):
    return x.to(torch.float16).to(torch.float64)


def _gelu(x):
    return 0.5 * x * (1.0 + torch.special.erf(x / math.sqrt(2.0)))


def _layernorm(y, gamma, beta, eps, dim=-1):
    u = y.mean(dim, keepdim=True)
    v = (y - u).pow(2).mean(dim, keepdim=True)                 # biased variance
    shape = [1] * y.dim()
    shape[dim] = -1
    return (y - u) / torch.sqrt(v + eps) * gamma.reshape(shape) + beta.reshape(shape)


def _convt2x2(x, w, b):
    """ConvTranspose2d(kernel 2, stride 2): out[n, co, 2y + ky, 2x + kx] = b[co] + sum_ci x[n, ci, y, x] w[ci, co, ky, kx]."""
    n, _, h, wd = x.shape
    co = w.shape[1]
    y = torch.einsum("ncyx,cokl->noykxl", x, w)
    return y.reshape(n, co, 2 * h, 2 * wd) + b.view(1, co, 1, 1)


def dense_pe(gauss, S):
    """PositionEmbeddingRandom of the S x S grid -> float64 [S*S, 256], row y*S + x: coordinates ((x + .5) / S, (y + .5) / S) mapped to
    [-1, 1], times the [2, 128] gaussian matrix, times 2 pi, sin | cos."""
    c = 2.0 * ((torch.arange(S, dtype=torch.float64) + 0.5) / S) - 1.0
    g = gauss.to(torch.float64)
    a = 2.0 * math.pi * (c.view(1, S, 1) * g[0].view(1, 1, -1) + c.view(S, 1, 1) * g[1].view(1, 1, -1))   # [y, x, 128]
    return torch.cat([torch.sin(a), torch.cos(a)], dim=-1).reshape(S * S, 256)


def upsample4_ref(low, align_corners=False, clamp_low=True):
    """F.interpolate(low [..., L, L], scale 4, mode="bilinear") from its definition, in the dtype of ``low``.  clamp_low=False leaves the
    source coordinate of the first two output rows / columns negative (-0.375, -0.125): the taps stay 0 and 1 and the weights extrapolate."""
    L = low.shape[-1]
    P = 4 * L
    i = torch.arange(P, dtype=low.dtype)
    if align_corners:
        s = i * (L - 1) / (P - 1)
    else:
        s = (i + 0.5) * 0.25 - 0.5
        if clamp_low:
            s = s.clamp(min=0.0)
    i0 = s.clamp(min=0.0).floor().long().clamp(max=L - 1)
    i1 = (i0 + 1).clamp(max=L - 1)
    w = s - i0.to(low.dtype)
    cols = low[..., i0] * (1.0 - w) + low[..., i1] * w                                   # along x
    return cols[..., i0, :] * (1.0 - w).view(-1, 1) + cols[..., i1, :] * w.view(-1, 1)   # along y


def _attention(q, k, v, scale, extra_den=0.0, swap=None):
    """q [B, Nq, C], k / v [B, Nk, C] in HEADS heads -> (out [B, Nq, C], probabilities [B, HEADS, Nq, Nk])."""
    B, Nq, C = q.shape
    hd = C // HEADS
    qh, kh, vh = (t.reshape(B, t.shape[1], HEADS, hd).transpose(1, 2) for t in (q, k, v))
    s = (qh @ kh.transpose(2, 3)) * scale
    e = torch.exp(s - s.amax(-1, keepdim=True))
    p = e / (e.sum(-1, keepdim=True) + extra_den)
    o = p @ vh
    if swap:
        a, b = swap
        o = o.clone()
        o[:, [a, b]] = o[:, [b, a]]
    return o.transpose(1, 2).reshape(B, Nq, C), p


MUTATIONS = {
    "t2i_scale": dict(t2i_scale=32 ** -0.5),          # token -> image scale 1/sqrt(32) instead of 1/sqrt(16)
    "self_scale": dict(self_scale=0.25),              # self-attention scale 1/4 instead of 1/sqrt(32)
    "swap_t2i_heads": dict(swap_t2i_heads=(0, 7)),    # two heads exchanged in the token -> image output
    "no_key_pe": dict(no_key_pe=True),                # the positional term left off the keys
    "no_imgq_pe": dict(no_imgq_pe=True),              # the positional term left off the image-side queries
    "layer0_adds": dict(layer0_adds=True),            # layer 0 adds the self-attention to the queries instead of replacing them
    "idle_exp0": dict(idle_exp0=192),                 # S = 8: the 192 threads without a key each add exp(0) to the denominator
    "mask_tokens_01": dict(mask_tokens=(0, 1)),       # masks of mask tokens 0, 1 instead of 1, 2
    "swap_kykx_1": dict(swap_kykx=1),                 # the 2 x 2 sub-pixel order of the first / second ConvT with ky and kx exchanged
    "swap_kykx_2": dict(swap_kykx=2),
    "hyper_shift": dict(hyper_shift=True),            # the hyper-network of mask token i applied to mask token i + 1
    "align_corners": dict(align_corners=True),
    "no_low_clamp": dict(no_low_clamp=True),          # the upsample without the clamp at the low border
}


def samdec_ref(emb, sd, S, round_points=False, mutate=None, probe=None):
    """emb [B*S*S, 256] (token-major neck output; any shape that reshapes to [B, S*S, 256]), sd = a state dict with the fork's
    prompt_encoder.* / mask_decoder.* entries -> float64 (logits [B, P, P, 2], scores, tokens_out [B, 4, 256], low_res [B, 2, 4S, 4S]),
    P = 16 S.  tokens_out are the queries after norm_final_attn, low_res the logits of mask tokens 1 and 2 before the upsample.

    round_points: round to fp16 wherever the library does — the fp16 copy of the keys that every image-side GEMM reads (the f32 keys of the
    residual stay unrounded), the projected K and V of the token -> image attentions and Q of the image -> token ones (after the bias and
    the positional addend), the image -> token attention output, the two upscaling activations, and the fp16 weight matrices of the
    image-side GEMMs (the positional addend pe W^T is made from the unrounded W, as at pack time).  The a-priori error of a correct kernel.

    mutate: one deliberate error (MUTATIONS).  probe: a dict that receives ``t2i`` / ``i2t`` / ``self`` (lists of attention probabilities
    [B, 8, query, key] in model order) and ``f16`` (name -> max |value| of every tensor the library stores as fp16)."""
    mu = dict(mutate or {})
    r = _r16 if round_points else (lambda t: t)
    p = {k: v.detach().cpu().to(torch.float64) for k, v in sd.items() if k.startswith(_PE) or k.startswith(_MD)}
    HW = S * S
    emb = emb.detach().cpu().to(torch.float64).reshape(-1, HW, 256)
    B = emb.shape[0]
    seen = {"t2i": [], "i2t": [], "self": [], "f16": {}}

    def f16(name, t):
        t = r(t)
        seen["f16"][name] = max(seen["f16"].get(name, 0.0), t.abs().max().item())
        return t

    def lin(x, base, image_side=False):
        w = p[base + ".weight"]
        return x @ (r(w) if image_side else w).T + p[base + ".bias"]

    def ln(y, base, eps=1e-5):
        return _layernorm(y, p[base + ".weight"], p[base + ".bias"], eps)

    pe = dense_pe(p[_PE + "pe_layer.positional_encoding_gaussian_matrix"], S)
    tok = torch.cat([p[_MD + "iou_token.weight"], p[_MD + "mask_tokens.weight"]], dim=0)          # [4, 256]
    keys = emb + p[_PE + "no_mask_embed.weight"].reshape(1, 1, 256)
    keys16 = f16("keys", keys)
    queries = tok.unsqueeze(0).expand(B, -1, -1)

    def t2i(queries, keys16, base, norm):
        q = lin(queries + tok, base + ".q_proj")
        k = lin(keys16, base + ".k_proj", True)
        if not mu.get("no_key_pe"):
            k = k + pe @ p[base + ".k_proj.weight"].T
        k, v = f16("t2i_k", k), f16("t2i_v", lin(keys16, base + ".v_proj", True))
        o, pr = _attention(q, k, v, float(mu.get("t2i_scale", 0.25)), float(mu.get("idle_exp0", 0.0)), mu.get("swap_t2i_heads"))
        seen["t2i"].append(pr)
        return ln(queries + lin(o, base + ".out_proj"), norm)

    for l in range(2):
        L = f"{_TR}layers.{l}."
        qa = queries if l == 0 else queries + tok                                                   # skip_first_layer_pe
        a, pr = _attention(lin(qa, L + "self_attn.q_proj"), lin(qa, L + "self_attn.k_proj"), lin(queries, L + "self_attn.v_proj"),
                           float(mu.get("self_scale", 32 ** -0.5)))
        seen["self"].append(pr)
        a = lin(a, L + "self_attn.out_proj")
        queries = ln(a if l == 0 and not mu.get("layer0_adds") else queries + a, L + "norm1")
        queries = t2i(queries, keys16, L + "cross_attn_token_to_image", L + "norm2")
        queries = ln(queries + lin(torch.relu(lin(queries, L + "mlp.lin1")), L + "mlp.lin2"), L + "norm3")
        base = L + "cross_attn_image_to_token"
        qi = lin(keys16, base + ".q_proj", True)
        if not mu.get("no_imgq_pe"):
            qi = qi + pe @ p[base + ".q_proj.weight"].T
        o, pr = _attention(f16("i2t_q", qi), lin(queries + tok, base + ".k_proj"), lin(queries, base + ".v_proj"), 0.25)
        seen["i2t"].append(pr)
        keys = ln(keys + lin(f16("i2t_out", o), base + ".out_proj", True), L + "norm4")
        keys16 = f16("keys", keys)
    tokens_out = t2i(queries, keys16, _TR + "final_attn_token_to_image", _TR + "norm_final_attn")

    # output_upscaling: ConvT(256 -> 64), LayerNorm2d(64) eps 1e-6, GELU, ConvT(64 -> 32), GELU
    up = _MD + "output_upscaling."
    w0, w1 = r(p[up + "0.weight"]), r(p[up + "3.weight"])
    if mu.get("swap_kykx") == 1:
        w0 = w0.transpose(2, 3)
    if mu.get("swap_kykx") == 2:
        w1 = w1.transpose(2, 3)
    x = _convt2x2(keys16.reshape(B, S, S, 256).permute(0, 3, 1, 2), w0, p[up + "0.bias"])
    x = f16("up0", _gelu(_layernorm(x, p[up + "1.weight"], p[up + "1.bias"], 1e-6, dim=1)))
    x = f16("up1", _gelu(_convt2x2(x, w1, p[up + "3.bias"])))                                     # [B, 32, 4S, 4S]
    hyper = []
    for i in range(3):
        h = tokens_out[:, 1 + ((i + 1) % 3 if mu.get("hyper_shift") else i)]
        for j in range(3):
            h = lin(h, f"{_MD}output_hypernetworks_mlps.{i}.layers.{j}")
            h = torch.relu(h) if j < 2 else h
        hyper.append(h)
    masks = torch.einsum("bic,bcyx->biyx", torch.stack(hyper, dim=1), x)                            # [B, 3, 4S, 4S]
    low_res = masks[:, list(mu.get("mask_tokens", (1, 2)))].contiguous()                            # multimask_output
    logits = upsample4_ref(low_res, align_corners=bool(mu.get("align_corners")), clamp_low=not mu.get("no_low_clamp"))
    logits = logits.permute(0, 2, 3, 1).contiguous()
    if probe is not None:
        probe.update(seen)
    return logits, 1.0 / (1.0 + torch.exp(-logits)), tokens_out, low_res


# ---- the model of the op tests -----------------------------------------------------------------------------------------------------------
# Chosen on the CPU so that the assertions of tests/test_samdec_ref.py hold: the conditions on every (S, B) of SHAPES, and every
# mutation's margin.  Matrices are N(0, 1 / fan_in) on inputs of O(1); biases, betas, no_mask_embed and the gaussian matrix N(0, 1);
# gammas in +-[1, 2]; except:
#   - the k projections are scaled head by head.  Token -> image: heads 0, 2, 4 peaked on 64 .. 4096 keys, heads 1, 6 flat, heads 3, 5, 7
#     in between (where a wrong scale changes the weights most), and more from attention to attention, since the keys differ less from
#     image token to image token after every norm4 (whose beta they all share).  Image -> token: peaked to flat.  Self-attention among
#     the 4 tokens: all but one head in between;
#   - the v rows of the in-between token -> image heads are larger, so that those heads carry weight in the token stream;
#   - the output tokens are N(0, 3): they are all that tells the 4 queries apart;
#   - the hyper-networks read their token with a gain (the mask tokens differ by ~ 10 % after norm_final_attn) and their last layer is
#     scaled so that the mask logits reach +-20 with a quarter of the scores undecided.
K_HEAD_GAIN = (3.0, 0.02, 1.5, 0.1, 2.0, 0.4, 0.05, 2.5)                     # image -> token
T2I_K_HEAD_GAIN = (5.0, 0.02, 2.5, 0.1, 4.0, 0.5, 0.05, 0.7)
T2I_K_ATTN_GAIN = {"layers.0.": 1.0, "layers.1.": 2.0, "final_attn": 4.0}
T2I_V_HEAD_GAIN = (1.0, 1.0, 1.0, 4.0, 1.0, 4.0, 1.0, 4.0)
SELF_K_HEAD_GAIN = (0.15, 0.02, 0.1, 0.12, 0.1, 0.2, 0.05, 0.12)
SELF_OUT_GAIN = 3.0
TOKEN_STD = 3.0
HYPER_IN_GAIN = 3.0
HYPER_OUT_GAIN = 0.075
SHAPES = ((8, 3), (9, 2), (16, 2), (16, 5), (25, 1), (32, 1), (64, 1))       # (S, B) of the GPU tests

_IMAGE_SIDE = ("cross_attn_token_to_image.k_proj.weight", "cross_attn_token_to_image.v_proj.weight",
               "final_attn_token_to_image.k_proj.weight", "final_attn_token_to_image.v_proj.weight",
               "cross_attn_image_to_token.q_proj.weight", "cross_attn_image_to_token.out_proj.weight",
               "output_upscaling.0.weight", "output_upscaling.3.weight")


def _f16(t):
    return t.to(torch.float16).to(torch.float32)


def _signed_1_2(shape, g):
    return (1.0 + torch.rand(shape, generator=g)) * torch.sign(torch.randn(shape, generator=g))


def samdec_fill(sd, seed):
    """The prompt_encoder.* / mask_decoder.* entries of the op tests' model, replacing those of ``sd`` (which supplies names and shapes):
    image-side matrices fp16-representable (the library's fp16 copies are exact), every bias and beta ~ N(0, 1), every gamma in +-[1, 2],
    so that a misplaced additive parameter moves the output by O(1) and not by 0.02."""
    g = torch.Generator().manual_seed(seed)
    out = {}
    for k, v in sd.items():
        if not (k.startswith(_PE) or k.startswith(_MD)):
            continue
        shape = tuple(v.shape)
        if k.endswith("_token.weight") or k.endswith("_tokens.weight"):
            t = torch.randn(shape, generator=g) * TOKEN_STD
        elif k.endswith("positional_encoding_gaussian_matrix") or "embed" in k:
            t = torch.randn(shape, generator=g)
        elif k.endswith(".bias"):
            t = torch.randn(shape, generator=g)
        elif len(shape) == 1:                                  # LayerNorm / LayerNorm2d gamma
            t = _signed_1_2(shape, g)
        elif len(shape) == 4:                                  # ConvTranspose2d [Cin, Cout, 2, 2] (Conv2d of the unused mask_downscaling alike)
            t = torch.randn(shape, generator=g) * shape[0] ** -0.5
        else:
            t = torch.randn(shape, generator=g) * shape[1] ** -0.5
            if k.endswith("k_proj.weight"):
                gain = torch.tensor(K_HEAD_GAIN)
                if "self_attn" in k:
                    gain = torch.tensor(SELF_K_HEAD_GAIN)
                if "token_to_image" in k:
                    gain = torch.tensor(T2I_K_HEAD_GAIN) * next(v for n, v in T2I_K_ATTN_GAIN.items() if n in k)
                t = t * gain.repeat_interleave(shape[0] // HEADS).view(-1, 1)
            if "self_attn.out_proj" in k:
                t = t * SELF_OUT_GAIN
            if "token_to_image.v_proj" in k:
                t = t * torch.tensor(T2I_V_HEAD_GAIN).repeat_interleave(shape[0] // HEADS).view(-1, 1)
            if "output_hypernetworks_mlps" in k and k.endswith("layers.0.weight"):
                t = t * HYPER_IN_GAIN
            if "output_hypernetworks_mlps" in k and k.endswith("layers.2.weight"):
                t = t * HYPER_OUT_GAIN
        if any(k.endswith(n) for n in _IMAGE_SIDE):
            t = _f16(t)
        out[k] = t.to(v.dtype)
    return out


def case_seed(S, B):
    """The seed of samdec_inputs for a shape of the op tests (the CPU conditions and the GPU tests use the same embeddings)."""
    return 100 * S + B


def samdec_inputs(B, S, seed):
    """Embeddings like the neck's output, f32 [B*S*S, 256] token-major: every row has mean 0 and variance 1 over its channels (the neck
    ends in a LayerNorm2d), and is a mix of noise, a vector of its tile, one of its grid row and one of its grid column, all different,
    so a transposed grid or a tile read from its neighbour gives other masks."""
    g = torch.Generator().manual_seed(seed)
    noise = torch.randn(B, S, S, 256, generator=g)
    tile, row, col = (torch.randn(n, 256, generator=g) for n in (B, S, S))
    x = 0.6 * noise + 0.5 * tile.view(B, 1, 1, 256) + 0.45 * row.view(1, S, 1, 256) + 0.45 * col.view(1, 1, S, 256)
    x = (x - x.mean(-1, keepdim=True)) / x.std(-1, keepdim=True, unbiased=False)
    return x.reshape(B * S * S, 256).contiguous()


def attention_stats(probe):
    """Per attention of a probe: the median over the rows of each head's maximum probability -> dict name -> [8] list."""
    out = {}
    for kind in ("t2i", "i2t", "self"):
        for i, pr in enumerate(probe[kind]):
            top = pr.amax(-1)                                   # [B, 8, rows]
            out[f"{kind}{i}"] = [top[:, h].reshape(-1).median().item() for h in range(HEADS)]
    return out
