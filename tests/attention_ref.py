"""CPU reference of the encoder's attention op and the input families of its op-level tests (tests/test_gpu_attention.py).

``attention64`` is a literal float64 transcription of the semantics in the header of sam_road_amd/csrc/attention.hip: the tile is padded
to whole windows AFTER the qkv projection, so a pad token is a REAL key with k = b_k, v = b_v (it receives softmax mass) while pad
queries are cropped; the decomposed rel-pos bias q . rel_h[qy - ky + win - 1] + q . rel_w[qx - kx + win - 1] comes from the UNSCALED q;
softmax; un-partition and crop.  S < win is one partly padded window.  It works per (image, head) and per block of queries, so the
64 x 64 global window stays within a few hundred MB.

``round_points=True`` is the a-priori error model of the MFMA kernels (the method of tests/samdec_ref.py): the two fp16 roundings of the
design, simulated in float64 — the softmax numerators exp(s - max) are rounded before the P.V product (they are its fp16 MFMA operand;
the row sum is taken from the unrounded f32 values, attention.hip tile_exp) and the output is rounded when it is stored.  Everything
else the kernels do is f32.  attn_generic_kernel keeps P in f32, so only the second rounding is its own.

``MUTATIONS`` are deliberate single mistakes of the reference; tests/test_attention_ref.py shows that each one moves some family by at
least four times the bound that family is held to, so the GPU tests cannot pass a kernel that makes it.

``make_case`` draws the seeded fp16 inputs of one family.  Every tensor depends on the token and on the column, so no permutation of
rows, heads or columns passes.  Families with a known answer return it (``answer``: float64 [B S S, D]; ``answer_rows``: the tokens it
holds for) together with the per-element bound derived below.
"""
import math

import torch

MUTATIONS = ("rel_scaled_q",    # rel-pos from the scaled q
             "rel_sign",        # rel index k - q + win - 1
             "rel_swap",        # rel_h and rel_w swapped
             "pad_zero",        # pad keys with k = v = 0
             "pad_masked",      # pad keys masked out of the softmax
             "drop_last",       # key win^2 - 1 of every window dropped
             "drop_27",         # key 27 of every window dropped
             "no_rescale")      # online softmax over 32-key tiles that never rescales what it has accumulated
PAD_MUTATIONS = ("pad_zero", "pad_masked")
FAMILIES = ("random", "uniform", "selector", "padsink", "ramp_up", "ramp_down", "big")
MASS_CAP = 1e-4                 # selector: softmax mass off the target; padsink: mass on real keys (float64 reference, every query)
_CHUNK = 1 << 22                # logits of one block of queries: at most this many float64 values (32 MB)


# The geometries (S, win, hd) of tests/test_gpu_attention.py, by the kernel that runs them: the smallest shapes that reach each route.
GEOMETRIES = {
    # attn_window_kernel: (14, 14) one window and no pad key; (32, 14) windows of 7, 2 and 1 query tiles (full waves, the 2-way and
    # the 4-way key split); (24, 14) windows of 7, 5 and 4 query tiles
    "window": [(14, 14, 64), (32, 14, 64), (24, 14, 64)],
    "global_fixed": [(16, 16, 64), (32, 32, 64), (64, 64, 64)],
    # the runtime-S form, width classes WP 16 / 32 / 64; 25 x 25 = 625 queries end on a partial query block
    "global_any": [(8, 8, 64), (25, 25, 64), (40, 40, 64)],
    "hdx": [(14, 14, 80), (32, 14, 80), (24, 14, 80), (16, 16, 80)],
    # attn_generic_kernel<10>: nkeys < KC (8), a partial last query block (625 = 2 * 256 + 113), KC = 128 (25, 32) and 64 (40, 64),
    # and at 64 the largest dynamic-LDS request, 161 792 of the 163 840 bytes it opts in to
    "generic": [(8, 8, 80), (25, 25, 80), (32, 32, 80), (40, 40, 80), (64, 64, 80)],
}
KERNEL_OF = {geo: name for name, geos in GEOMETRIES.items() for geo in geos}
ALL_GEOMETRIES = [geo for geos in GEOMETRIES.values() for geo in geos]
# ramp_up, ramp_down and big: one geometry per kernel (two for attention_hdx: windowed and 16 x 16 global)
RAMP_GEOMETRIES = [(32, 14, 64), (32, 32, 64), (25, 25, 64), (32, 14, 80), (16, 16, 80), (25, 25, 80)]


def batch_of(S, win, hd):
    """(B, heads) of a geometry in the GPU tests."""
    return (1, 2) if S == 64 else (2, 3)


def has_pad_keys(S, win):
    return S % win != 0


def families_of(S, win, hd):
    fam = ["random", "uniform", "selector"]
    if has_pad_keys(S, win):
        fam.append("padsink")
    if (S, win, hd) in RAMP_GEOMETRIES:
        fam += ["ramp_up", "ramp_down", "big"]
    return fam


def gpu_case(family, S, win, hd):
    """The case the GPU tests run for (family, geometry): tests/test_attention_ref.py proves its conditions on exactly these inputs."""
    B, heads = batch_of(S, win, hd)
    return make_case(family, B, S, heads, win, hd, seed=10007 * FAMILIES.index(family) + S * 100 + win + hd)


def selector_gain(win):
    """q = gain * code: gain 4 keeps the off-target mass under MASS_CAP up to 32 x 32 keys, 64 x 64 needs 8."""
    return 8.0 if win * win > 1024 else 4.0


def _windows(t, B, nw, win):
    """[B, Sp, Sp, C] -> [B, nw * nw, win * win, C]"""
    C = t.shape[-1]
    return t.view(B, nw, win, nw, win, C).permute(0, 1, 3, 2, 4, 5).reshape(B, nw * nw, win * win, C)


def _partition(qkv, bias, B, S, heads, win, hd):
    """The padded, window-partitioned qkv in float64 [B, nw^2, win^2, 3 D] and the real-token mask [nw^2, win^2]."""
    D = heads * hd
    nw = -(-S // win)
    Sp = nw * win
    full = bias.double().view(1, 1, 1, 3 * D).expand(B, Sp, Sp, 3 * D).clone()
    full[:, :S, :S] = qkv.double().view(B, S, S, 3 * D)
    real = torch.zeros(1, Sp, Sp, 1, dtype=torch.bool)
    real[:, :S, :S] = True
    return _windows(full, B, nw, win), _windows(real, 1, nw, win)[0, :, :, 0], nw, Sp


def _attention64(qkv, rel_h, rel_w, bias, B, S, heads, win, hd, want_exact=True, want_rounded=False, mutate=None, probe=None):
    assert mutate is None or mutate in MUTATIONS, mutate
    assert qkv.shape == (B * S * S, 3 * heads * hd) and rel_h.shape == rel_w.shape == (2 * win - 1, hd) and bias.shape == (3 * heads * hd,)
    D, n = heads * hd, win * win
    scale = hd ** -0.5
    xw, real, nw, Sp = _partition(qkv, bias, B, S, heads, win, hd)
    th, tw = rel_h.double(), rel_w.double()
    if mutate == "rel_swap":
        th, tw = tw, th
    a = torch.arange(win)
    idx = (a[None, :] - a[:, None] if mutate == "rel_sign" else a[:, None] - a[None, :]) + (win - 1)      # [q, k]
    Rh, Rw = th[idx], tw[idx]                                                                               # [win(q), win(k), hd]
    pad = ~real                                                                                             # [nw^2, n]
    outs = [torch.zeros(B, nw * nw, n, D, dtype=torch.float64) if w else None for w in (want_exact, want_rounded)]
    step = max(1, _CHUNK // (nw * nw * n))
    for b in range(B):
        for h in range(heads):
            q = xw[b, :, :, h * hd:(h + 1) * hd]
            k = xw[b, :, :, D + h * hd:D + (h + 1) * hd]
            v = xw[b, :, :, 2 * D + h * hd:2 * D + (h + 1) * hd]
            if mutate == "pad_zero":
                k = k.masked_fill(pad[:, :, None], 0.0)
                v = v.masked_fill(pad[:, :, None], 0.0)
            kt = k.transpose(1, 2).contiguous()
            for q0 in range(0, n, step):
                q1 = min(n, q0 + step)
                qc = q[:, q0:q1]                                                                            # [nw^2, c, hd]
                s = (qc * scale) @ kt                                                                       # [nw^2, c, n]
                qr = qc * scale if mutate == "rel_scaled_q" else qc
                qi = torch.arange(q0, q1)
                bh = torch.einsum("wqc,qkc->wqk", qr, Rh[qi // win])                                        # [nw^2, c, win(ky)]
                bw = torch.einsum("wqc,qkc->wqk", qr, Rw[qi % win])                                         # [nw^2, c, win(kx)]
                s = (s.view(nw * nw, q1 - q0, win, win) + bh[:, :, :, None] + bw[:, :, None, :]).view(nw * nw, q1 - q0, n)
                if mutate == "pad_masked":
                    s = s.masked_fill(pad[:, None, :], -math.inf)
                elif mutate == "drop_last":
                    s[:, :, n - 1] = -math.inf
                elif mutate == "drop_27":
                    s[:, :, 27] = -math.inf
                if mutate == "no_rescale":
                    nt = -(-n // 32)
                    st = torch.full((nw * nw, q1 - q0, nt * 32), -math.inf, dtype=torch.float64)
                    st[:, :, :n] = s
                    run = st.view(nw * nw, q1 - q0, nt, 32).amax(-1).cummax(-1).values                      # the running max after each tile
                    e = torch.exp(s - run.repeat_interleave(32, -1)[:, :, :n])
                else:
                    e = torch.exp(s - s.amax(-1, keepdim=True))
                den = e.sum(-1, keepdim=True)
                if probe is not None:
                    probe(b, h, q0, q1, e / den, real)
                if want_exact:
                    outs[0][b, :, q0:q1, h * hd:(h + 1) * hd] = (e @ v) / den
                if want_rounded:
                    outs[1][b, :, q0:q1, h * hd:(h + 1) * hd] = ((e.half().double() @ v) / den).half().double()

    def crop(o):
        o = o.view(B, nw, nw, win, win, D).permute(0, 1, 3, 2, 4, 5).reshape(B, Sp, Sp, D)
        return o[:, :S, :S].reshape(B * S * S, D)

    return [crop(o) if o is not None else None for o in outs]


def attention64(qkv, rel_h, rel_w, bias, B, S, heads, win, hd, round_points=False, mutate=None, probe=None):
    """The attention op in float64: qkv fp16 [B S S, 3 D] (q | k | v, heads in the columns), rel_h / rel_w [2 win - 1, hd], bias [3 D]
    -> float64 [B S S, D].  round_points: the a-priori error model (module docstring).  mutate: one of MUTATIONS.  probe: called as
    probe(image, head, q0, q1, p, real) with the probabilities p [windows, q1 - q0, win^2] of the window-local queries q0 .. q1 - 1
    and the mask real [windows, win^2] of the keys that are tokens of the tile."""
    return _attention64(qkv, rel_h, rel_w, bias, B, S, heads, win, hd, not round_points, round_points, mutate, probe)[int(round_points)]


def attention64_both(qkv, rel_h, rel_w, bias, B, S, heads, win, hd):
    """(attention64(), attention64(round_points=True)) from one pass over the logits."""
    return tuple(_attention64(qkv, rel_h, rel_w, bias, B, S, heads, win, hd, True, True))


# ---- input families -------------------------------------------------------------------------------------------------------------------
def _token_windows(S, win):
    """Per window (in window order): the tokens y * S + x of its real keys in window order, and their window-local key indices."""
    nw = -(-S // win)
    out = []
    for wy in range(nw):
        for wx in range(nw):
            ys = torch.arange(wy * win, min(S, (wy + 1) * win))
            xs = torch.arange(wx * win, min(S, (wx + 1) * win))
            tok = (ys[:, None] * S + xs[None, :]).reshape(-1)
            loc = ((ys[:, None] - wy * win) * win + (xs[None, :] - wx * win)).reshape(-1)
            out.append((tok, loc, len(ys) * len(xs) < win * win))
    return out


def fp16_ulp(x):
    """The spacing of fp16 at |x| (float64 tensor): 2^(floor(log2 |x|) - 10), 2^-24 in the subnormal range."""
    e = torch.floor(torch.log2(x.abs().clamp(min=2.0 ** -14)))
    return torch.exp2(e - 10)


def _codes(shape, g):
    return (torch.randint(0, 2, shape, generator=g) * 2 - 1).float()


def make_case(family, B, S, heads, win, hd, seed):
    """One seeded case: dict(qkv, rel_h, rel_w, bias: fp16; answer, answer_rows, bound: float64 / bool / float64 or None; target: the
    window-local key each query must select [B S S] (selector) or None).  The module docstring and the comments below say what each
    family is for and where its bound comes from."""
    assert family in FAMILIES, family
    D, T, n = heads * hd, S * S, win * win
    g = torch.Generator().manual_seed(seed)
    case = dict(family=family, B=B, S=S, heads=heads, win=win, hd=hd, answer=None, answer_rows=None, bound=None, target=None)

    def tables(std):
        return (torch.randn(2 * win - 1, hd, generator=g) * std).half(), (torch.randn(2 * win - 1, hd, generator=g) * std).half()

    if family == "random":
        # tests/test_gpu_ops.py test_sam_attention's distributions, drawn in its order: a peaked softmax, logits of tens
        qkv = (torch.randn(B * T, 3 * D, generator=g) * 1.5).half()
        bias = (torch.randn(3 * D, generator=g) * 0.5).half()
        rel_h, rel_w = tables(0.3)
    elif family == "uniform":
        # q = 0: every logit is 0 whatever k and the tables hold, P = 1 exactly, and the answer is the mean over ALL win^2 keys of the
        # query's window, pads included.  v and b_v are multiples of 1/16 in [-4, 4]: every partial sum, in any order, is a multiple of
        # 1/16 below 4 win^2 <= 2^14, exact in f32.  What is left: v_rcp_f32 and the product round once each (f32), the store once
        # (fp16): one fp16 ulp of |answer| plus 2^-24.
        qkv = (torch.randn(B * T, 3 * D, generator=g) * 1.5).half()
        bias = (torch.randn(3 * D, generator=g) * 0.5).half()
        qkv[:, :D] = 0
        qkv[:, 2 * D:] = (torch.randint(-64, 65, (B * T, D), generator=g).float() / 16).half()
        bias[2 * D:] = (torch.randint(-64, 65, (D,), generator=g).float() / 16).half()
        rel_h, rel_w = tables(0.3)
        xw, _, nw, Sp = _partition(qkv, bias, B, S, heads, win, hd)
        mean = xw[:, :, :, 2 * D:].mean(2, keepdim=True).expand(B, nw * nw, n, D)
        ans = mean.reshape(B, nw, nw, win, win, D).permute(0, 1, 3, 2, 4, 5).reshape(B, Sp, Sp, D)[:, :S, :S].reshape(B * T, D)
        case.update(answer=ans.contiguous(), answer_rows=torch.ones(B * T, dtype=torch.bool))
        case["bound"] = fp16_ulp(case["answer"]) + 2.0 ** -24
    elif family in ("selector", "padsink"):
        # k rows are +-1 codes (one per token and head), b_k one more code.  selector: q = gain * (the code of a target key, chosen by a
        # fixed permutation of the real keys of the query's own window): logit gain sqrt(hd) = 32 .. 72 on the target, gain N(0, 1) on
        # every other key, so the answer is the target's V row.  padsink: q = gain * b_k for every query: in a window with pad keys the
        # answer is b_v.  Bound per element: the result's fp16 rounding (2^-10 |answer|, one ulp), the mass that lands elsewhere
        # (<= MASS_CAP, asserted on the float64 reference by tests/test_attention_ref.py) times the largest distance between two V
        # values (2 max|v|), and 2^-24.
        gain = selector_gain(win)
        qkv = (torch.randn(B * T, 3 * D, generator=g) * 1.5).half()
        bias = (torch.randn(3 * D, generator=g) * 0.5).half()
        qkv[:, D:2 * D] = _codes((B * T, D), g).half()
        bias[D:2 * D] = _codes((D,), g).half()
        rel_h, rel_w = tables(0.02)
        vmax = max(qkv[:, 2 * D:].abs().max().item(), bias[2 * D:].abs().max().item())
        kq = qkv[:, D:2 * D].view(B, T, D)
        vq = qkv[:, 2 * D:].view(B, T, D)
        if family == "selector":
            q = torch.zeros(B, T, D, dtype=torch.half)
            ans = torch.zeros(B, T, D, dtype=torch.float64)
            target = torch.zeros(T, dtype=torch.long)
            for tok, loc, _ in _token_windows(S, win):
                perm = torch.randperm(len(tok), generator=g)
                q[:, tok] = kq[:, tok[perm]] * gain
                ans[:, tok] = vq[:, tok[perm]].double()
                target[tok] = loc[perm]
            rows = torch.ones(B * T, dtype=torch.bool)
            case["target"] = target.repeat(B)
        else:
            assert has_pad_keys(S, win), "padsink needs pad keys"
            q = (bias[D:2 * D] * gain).view(1, 1, D).expand(B, T, D)
            ans = bias[2 * D:].double().view(1, 1, D).expand(B, T, D)
            rows = torch.zeros(T, dtype=torch.bool)
            for tok, _, padded in _token_windows(S, win):
                rows[tok] = padded
            rows = rows.repeat(B)
        qkv[:, :D] = q.reshape(B * T, D)
        case.update(answer=ans.reshape(B * T, D).contiguous(), answer_rows=rows)
        case["bound"] = 2.0 ** -10 * case["answer"].abs() + 2 * MASS_CAP * vmax + 2.0 ** -24
    elif family in ("ramp_up", "ramp_down"):
        # q = a e, k_j = t_j e with e a +-1 code per head, a in [3/4, 1] per query and t monotone over the window's real keys in window
        # order: logits a t_j sqrt(hd) from 0 to 40 .. 60 nats. ramp_up: the running max of an online softmax moves in EVERY key tile (and most of
        # what was accumulated before is rescaled to nothing); ramp_down: never after the first tile.  Pad keys (b_k = -e / 2) stay
        # below the ramp.  V is random.  No closed form: compared with attention64 under the a-priori rule.
        qkv = (torch.randn(B * T, 3 * D, generator=g) * 1.5).half()
        bias = (torch.randn(3 * D, generator=g) * 0.5).half()
        e = _codes((D,), g)
        a = torch.randint(48, 65, (B, T, heads), generator=g).float() / 64
        top = 60.0 / math.sqrt(hd)
        t = torch.zeros(B, T)
        for tok, loc, _ in _token_windows(S, win):
            r = torch.arange(len(tok)).float() / (len(tok) - 1)           # over the window's real keys, in window order
            for b in range(B):
                t[b, tok] = top * (1 - 0.1 * b) * (r if family == "ramp_up" else 1 - r)
        qkv[:, :D] = (a[:, :, :, None] * e.view(1, 1, heads, hd)).reshape(B * T, D).half()
        qkv[:, D:2 * D] = (t.half().float()[:, :, None] * e.view(1, 1, D)).reshape(B * T, D).half()
        bias[D:2 * D] = (-0.5 * e).half()
        rel_h, rel_w = tables(0.02)
    else:
        # big: |q|, |k| in [4, 8] with random signs: logits of +-37 sigma, a few hundred at the extremes, where float32 logits carry
        # errors of 1e-5 .. 1e-4 and a float32 reference stops being good enough
        qkv = (torch.randn(B * T, 3 * D, generator=g) * 1.5).half()
        bias = (torch.randn(3 * D, generator=g) * 0.5).half()
        qkv[:, :2 * D] = (_codes((B * T, 2 * D), g) * (4 + 4 * torch.rand(B * T, 2 * D, generator=g))).half()
        bias[:2 * D] = (_codes((2 * D,), g) * (4 + 4 * torch.rand(2 * D, generator=g))).half()
        rel_h, rel_w = tables(0.3)
    case.update(qkv=qkv, rel_h=rel_h, rel_w=rel_w, bias=bias)
    return case


def case_args(case):
    """The positional arguments of attention64 for a case."""
    return (case["qkv"], case["rel_h"], case["rel_w"], case["bias"], case["B"], case["S"], case["heads"], case["win"], case["hd"])


def stray_mass(case):
    """selector: the largest softmax mass OFF the target over every query; padsink: the largest mass ON real keys over the queries of the
    windows with pad keys.  From the float64 reference alone."""
    B, S, heads, win = case["B"], case["S"], case["heads"], case["win"]
    n = win * win
    worst = [0.0]
    if case["family"] == "selector":
        # window-local target per (image, window, local query); -1 at pad queries
        tgt = torch.full((B, len(_token_windows(S, win)), n), -1, dtype=torch.long)
        t = case["target"].view(B, S * S)
        for w, (tok, loc, _) in enumerate(_token_windows(S, win)):
            tgt[:, w, loc] = t[:, tok]

        def probe(b, h, q0, q1, p, real):
            tq = tgt[b, :, q0:q1]
            on = p.gather(2, tq.clamp(min=0)[:, :, None])[:, :, 0]
            off = torch.where(tq >= 0, 1.0 - on, torch.zeros_like(on))
            worst[0] = max(worst[0], off.max().item())
    else:
        padded = torch.tensor([w[2] for w in _token_windows(S, win)])

        def probe(b, h, q0, q1, p, real):
            mass = (p * real[:, None, :]).sum(-1)                          # [windows, c]
            mass = mass * (real[:, q0:q1] & padded[:, None])               # real queries of padded windows only
            worst[0] = max(worst[0], mass.max().item())
    attention64(*case_args(case), probe=probe)
    return worst[0]


# ---- how far an output is from what a case allows ------------------------------------------------------------------------------------
def answer_excess(case, out):
    """A family with a known answer: the largest |out - answer| / bound over the rows the answer holds for (< 1 passes)."""
    r = case["answer_rows"]
    return ((out.double() - case["answer"]).abs() / case["bound"])[r].max().item()


def apriori_ratios(out, exact, rounded):
    """A family held to the a-priori rule: (max-abs error of out / max-abs a-priori error, the same for mean-abs); each must stay
    below tolerances.ATTN_OP_VS_APRIORI."""
    err, ap = (out.double() - exact).abs(), (rounded - exact).abs()
    return err.max().item() / ap.max().item(), err.mean().item() / ap.mean().item()
