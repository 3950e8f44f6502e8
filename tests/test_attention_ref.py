"""CPU checks of tests/attention_ref.py, the reference and the input families tests/test_gpu_attention.py compares the attention kernels
with: attention64 is pinned to the float32 reference the op tests used so far and to the oracle's _Attention module run in float64;
the conditions the families' closed-form answers rest on hold for every case the GPU file runs (with the reference alone: inputs that
do not meet them fail here, on any host); every mistake of attention_ref.MUTATIONS moves some family by at least MUTANT_FACTOR times the
bound that family is held to; and tolerances.ATTN_OP_MAX / ATTN_OP_MEAN are twice the a-priori error of the older op tests' cases."""
import functools

import pytest
import torch

import attention_ref as A
import tolerances as T
from oracle.sam_encoder import _Attention
from test_gpu_ops import ref_sam_attention

MUTANT_FACTOR = 4.0
GEO_IDS = ["S%d-win%d-hd%d" % g for g in A.ALL_GEOMETRIES]


@functools.lru_cache(maxsize=None)
def _case(family, geo):
    return A.gpu_case(family, *geo)


@functools.lru_cache(maxsize=None)
def _both(family, geo):
    return A.attention64_both(*A.case_args(_case(family, geo)))


# ---- the reference is the operation ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S,win,hd", [(14, 14, 64), (24, 14, 64), (32, 14, 80), (16, 16, 80), (25, 25, 64), (8, 14, 64), (10, 14, 80)])
def test_attention64_is_the_float32_reference(S, win, hd):
    B, heads = 2, 3
    c = A.make_case("random", B, S, heads, win, hd, seed=S + win + hd)
    got = A.attention64(*A.case_args(c))
    assert got.dtype == torch.float64 and got.shape == (B * S * S, heads * hd)
    if S >= win:
        want = ref_sam_attention(c["qkv"], c["rel_h"], c["rel_w"], c["bias"], B, S, heads, win, hd)
    else:       # one partly padded window: the tile padded with the qkv bias is one S = win window (test_gpu_patch_sizes._ref_attention)
        C3 = 3 * heads * hd
        full = c["bias"].view(1, 1, 1, C3).expand(B, win, win, C3).clone()
        full[:, :S, :S] = c["qkv"].view(B, S, S, C3)
        want = ref_sam_attention(full.reshape(B * win * win, C3), c["rel_h"], c["rel_w"], c["bias"], B, win, heads, win, hd)
        want = want.view(B, win, win, -1)[:, :S, :S].reshape(B * S * S, -1)
    assert (got - want.double()).abs().max().item() < 1e-4


@pytest.mark.parametrize("win,hd", [(14, 64), (16, 80)])
def test_attention64_is_the_oracle_module_in_float64(win, hd):
    """oracle.sam_encoder._Attention on one window in float64, with an identity proj; attention64 gets the module's own qkv = W x + b
    (float64 values: it converts whatever it is given) and rel-pos tables."""
    B, heads = 2, 3
    D = heads * hd
    torch.manual_seed(win + hd)
    m = _Attention(D, heads, win).double()
    x = torch.randn(B, win, win, D, dtype=torch.float64) * 3
    with torch.no_grad():
        m.qkv.bias.normal_()
        m.rel_pos_h.normal_(std=0.3)
        m.rel_pos_w.normal_(std=0.3)
        m.proj.weight.copy_(torch.eye(D, dtype=torch.float64))
        m.proj.bias.zero_()
        want = m(x)
        qkv = m.qkv(x).reshape(B * win * win, 3 * D)
        got = A.attention64(qkv, m.rel_pos_h, m.rel_pos_w, m.qkv.bias, B, win, heads, win, hd)
    assert qkv.abs().max().item() > 3 and want.abs().max().item() > 1
    assert (got - want.reshape(B * win * win, D)).abs().max().item() < 1e-12


def test_round_points_is_the_two_fp16_roundings():
    """round_points on a case small enough to write the two roundings out by hand, from attention64's own probabilities."""
    c = A.make_case("random", 1, 8, 1, 8, 64, seed=3)
    got = A.attention64(*A.case_args(c), round_points=True)
    ps = []
    A.attention64(*A.case_args(c), probe=lambda b, h, q0, q1, p, real: ps.append(p))
    p = ps[0][0]                                                       # [64, 64], rows sum to 1
    v = c["qkv"][:, 128:].double()
    e = p / p.amax(-1, keepdim=True)                                   # exp(s - max)
    want = ((e.half().double() @ v) / e.sum(-1, keepdim=True)).half().double()
    assert torch.equal(got, want)
    exact = A.attention64(*A.case_args(c))
    assert 0 < (got - exact).abs().max().item() < 2.0 ** -9 * 1.01     # |out| < 4: half an fp16 ulp, and a little from P


# ---- the families' conditions, on the GPU file's own cases ---------------------------------------------------------------------------------
@pytest.mark.parametrize("geo", A.ALL_GEOMETRIES, ids=GEO_IDS)
def test_family_conditions(geo):
    S, win, hd = geo
    B, heads = A.batch_of(*geo)
    D = heads * hd
    assert A.KERNEL_OF[geo] in A.GEOMETRIES
    for fam in A.families_of(*geo):
        c = _case(fam, geo)
        for name in ("qkv", "rel_h", "rel_w", "bias"):
            assert c[name].dtype == torch.float16 and torch.isfinite(c[name].float()).all()
        # every tensor depends on the token and on the column: a roll of either changes it
        assert not torch.equal(c["qkv"], c["qkv"].roll(1, 0)) and not torch.equal(c["qkv"], c["qkv"].roll(1, 1))
    # uniform: q = 0; v, b_v multiples of 1/16 in [-4, 4]: the sum of win^2 of them, in any order, is exact in f32
    c = _case("uniform", geo)
    v16 = torch.cat([c["qkv"][:, 2 * D:].reshape(-1), c["bias"][2 * D:]]).double() * 16
    assert (c["qkv"][:, :D] == 0).all() and torch.equal(v16, v16.round()) and v16.abs().max().item() <= 64
    assert 64 * win * win < 2 ** 24
    exact = A.attention64(*A.case_args(c))
    assert (exact - c["answer"]).abs().max().item() < 1e-13, "the closed form is not the float64 reference"
    assert A.answer_excess(c, _both("uniform", geo)[1]) <= 0.5 + 1e-9      # the simulated kernel: half an ulp of the bound's one
    # selector / padsink: the mass that does not land where the answer says, in the float64 reference
    for fam in ("selector", "padsink"):
        if fam == "padsink" and not A.has_pad_keys(S, win):
            continue
        c = _case(fam, geo)
        stray = A.stray_mass(c)
        print(f"{fam} S={S} win={win} hd={hd}: stray mass {stray:.2e}")
        assert stray <= A.MASS_CAP
        assert c["answer_rows"].any() and (fam == "padsink" or c["answer_rows"].all())
        assert A.answer_excess(c, _both(fam, geo)[0]) < 1 and A.answer_excess(c, _both(fam, geo)[1]) < 1
    if A.has_pad_keys(S, win):       # padsink's answer covers exactly the windows with a pad key
        rows = _case("padsink", geo)["answer_rows"].view(B, S, S)
        inner = (S // win) * win
        assert not rows[:, :inner, :inner].any() and rows[:, inner:].all() and rows[:, :, inner:].all()
    # selector targets: a real key of the query's own window, a permutation (every key of a window is selected once)
    c = _case("selector", geo)
    tg = c["target"].view(B, S, S)
    assert torch.equal(tg[0], tg[-1]) and 0 <= tg.min().item() and tg.max().item() < win * win
    assert len(set(tg[0, :min(S, win), :min(S, win)].reshape(-1).tolist())) == min(S, win) ** 2


@pytest.mark.parametrize("geo", A.RAMP_GEOMETRIES, ids=["S%d-win%d-hd%d" % g for g in A.RAMP_GEOMETRIES])
def test_ramp_and_big_reach_what_they_are_for(geo):
    S, win, hd = geo
    n = win * win
    tiles = {}
    for fam in ("ramp_up", "ramp_down", "big"):
        c = _case(fam, geo)
        # logits from the probabilities: log p_max - log p_min over the real keys is the span
        span, moves = [], []

        def probe(b, h, q0, q1, p, real, span=span, moves=moves):
            lp = torch.log(p.clamp(min=1e-300))
            rq = real[:, q0:q1]                                          # real queries
            lo = lp.masked_fill(~real[:, None, :], 0.0).amin(-1)
            span.append((lp.amax(-1) - lo)[rq])
            nt = -(-n // 32)
            t = torch.full(lp.shape[:2] + (nt * 32,), -1e300, dtype=torch.float64)
            t[:, :, :n] = lp.masked_fill(~real[:, None, :], -1e300)
            run = t.view(lp.shape[0], lp.shape[1], nt, 32).amax(-1).cummax(-1).values
            moves.append(((run[:, :, 1:] > run[:, :, :-1]).sum(-1))[rq])
        A.attention64(*A.case_args(c), probe=probe)
        span, moves = torch.cat(span), torch.cat(moves)
        tiles[fam] = moves
        print(f"{fam} S={S} win={win} hd={hd}: logit span {span.min():.1f} .. {span.max():.1f} nats, "
              f"running-max moves per query {moves.min()} .. {moves.max()}")
        if fam == "big":
            assert span.max().item() > 200
        else:
            assert 35 < span.min().item() and span.max().item() < 70       # a in [3/4, 1], 54 .. 60 nats at a = 1
    assert tiles["ramp_down"].max().item() == 0, "ramp_down: the running max must never move after the first key tile"
    # ramp_up: it moves in every later tile that holds a real key (all of them in a window without pad keys)
    last = -(-n // 32) - 1
    assert tiles["ramp_up"].max().item() == last and tiles["ramp_up"].min().item() >= (1 if A.has_pad_keys(S, win) else last)


# ---- the tests are sharp: every mutant is out of bounds somewhere -----------------------------------------------------------------------------
def _excess(fam, geo, out):
    """How many times its bound `out` misses the case by (>= 1 fails the GPU test)."""
    c = _case(fam, geo)
    if c["answer"] is not None:
        return A.answer_excess(c, out)
    exact, rounded = _both(fam, geo)
    return max(A.apriori_ratios(out, exact, rounded)) / T.ATTN_OP_VS_APRIORI


FAMILIES_FOR = {"rel_scaled_q": ("random",), "rel_sign": ("random",), "rel_swap": ("random",), "pad_zero": ("random", "uniform", "padsink"),
                "pad_masked": ("random", "uniform", "padsink"), "drop_last": ("uniform", "random"), "drop_27": ("uniform", "random")}


@pytest.mark.parametrize("geo", A.ALL_GEOMETRIES, ids=GEO_IDS)
def test_mutants_are_out_of_bounds(geo):
    S, win, hd = geo
    for mut, fams in FAMILIES_FOR.items():
        if mut in A.PAD_MUTATIONS and not A.has_pad_keys(S, win):
            continue
        seen = {}
        for fam in fams:
            out = A.attention64(*A.case_args(_case(fam, geo)), mutate=mut)
            seen[fam] = _excess(fam, geo, out)
        print(f"{mut} S={S} win={win} hd={hd}: " + ", ".join(f"{f} {x:.3g} x its bound" for f, x in seen.items()))
        assert max(seen.values()) >= MUTANT_FACTOR, (mut, seen)
        if mut in ("drop_last", "drop_27"):        # per-key accounting is what uniform is for: it alone must see a dropped key
            assert seen["uniform"] >= MUTANT_FACTOR, (mut, seen)
    # the unmutated reference, rounded as the kernels round, is within every bound
    for fam in A.families_of(*geo):
        assert _excess(fam, geo, _both(fam, geo)[1]) <= 0.5 + 1e-9


@pytest.mark.parametrize("geo", A.RAMP_GEOMETRIES, ids=["S%d-win%d-hd%d" % g for g in A.RAMP_GEOMETRIES])
def test_skipped_rescale_is_caught_by_ramp_up_only(geo):
    up = _excess("ramp_up", geo, A.attention64(*A.case_args(_case("ramp_up", geo)), mutate="no_rescale"))
    down_out = A.attention64(*A.case_args(_case("ramp_down", geo)), mutate="no_rescale")
    down = _excess("ramp_down", geo, down_out)
    print(f"no_rescale S={geo[0]} win={geo[1]} hd={geo[2]}: ramp_up {up:.3g} x its bound, ramp_down {down:.3g} x")
    assert up >= MUTANT_FACTOR
    assert down < 1e-6 and torch.allclose(down_out, _both("ramp_down", geo)[0], rtol=0, atol=1e-12)


# ---- the older op tests' bounds ---------------------------------------------------------------------------------------------------------------
# (B, S, heads, win, hd, seed) of tests/test_gpu_ops.py test_sam_attention and tests/test_gpu_patch_sizes.py _attention_case
OLD_CASES = ([(2, S, 4 if (S, win) == (64, 64) else 3, win, hd, S * 100 + win + hd)
              for S, win, hd in [(32, 14, 64), (32, 32, 64), (16, 14, 64), (16, 16, 64), (48, 14, 64), (64, 14, 64), (64, 64, 64), (16, 14, 80),
                                 (16, 16, 80), (32, 14, 80), (32, 32, 80), (48, 14, 80), (64, 14, 80)]]
             + [(2, S, heads, S, 64, 7000 + S) for S, heads in [(8, 3), (12, 4), (20, 3), (24, 4), (25, 3), (40, 4), (48, 3), (63, 3)]]
             + [(2, S, 3, 14, hd, 8000 + S + hd) for hd in (64, 80) for S in (8, 24, 25, 40)])


def test_old_bounds_are_twice_the_a_priori_error():
    """ATTN_OP_MAX / ATTN_OP_MEAN = tolerances.ATTN_OP_VS_APRIORI x the worst a-priori error over the 29 cases that are held to them
    (make_case("random") draws test_sam_attention's inputs in its order, so these are those tests' own inputs)."""
    worst_max = worst_mean = 0.0
    for B, S, heads, win, hd, seed in OLD_CASES:
        c = A.make_case("random", B, S, heads, win, hd, seed)
        exact, rounded = A.attention64_both(*A.case_args(c))
        ap = (rounded - exact).abs()
        worst_max, worst_mean = max(worst_max, ap.max().item()), max(worst_mean, ap.mean().item())
    print(f"a-priori over {len(OLD_CASES)} cases: max-abs {worst_max:.4e}, mean-abs {worst_mean:.4e}")
    assert abs(T.ATTN_OP_MAX / (T.ATTN_OP_VS_APRIORI * worst_max) - 1) < 0.005
    assert abs(T.ATTN_OP_MEAN / (T.ATTN_OP_VS_APRIORI * worst_mean) - 1) < 0.005


def test_old_cases_inputs_are_the_random_family():
    """The generator order of test_sam_attention, written out: qkv, bias, rel_h, rel_w."""
    B, S, heads, win, hd = 2, 16, 3, 14, 80
    g = torch.Generator().manual_seed(S * 100 + win + hd)
    qkv = (torch.randn(B * S * S, 3 * heads * hd, generator=g) * 1.5).half()
    bias = (torch.randn(3 * heads * hd, generator=g) * 0.5).half()
    rel_h = (torch.randn(2 * win - 1, hd, generator=g) * 0.3).half()
    rel_w = (torch.randn(2 * win - 1, hd, generator=g) * 0.3).half()
    c = A.make_case("random", B, S, heads, win, hd, S * 100 + win + hd)
    assert torch.equal(c["qkv"], qkv) and torch.equal(c["bias"], bias) and torch.equal(c["rel_h"], rel_h) and torch.equal(c["rel_w"], rel_w)
