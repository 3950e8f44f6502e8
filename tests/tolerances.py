"""The stated floating-point tolerances of the HIP path against the oracle / the reference-run fixtures, in ONE place.

Every bound is <= 3x the worst value measured on an MI355X for that quantity (profiles/r03_parity_measured.json is the
record these were set from: every ``check`` call writes its measured value there when the suite runs on the GPU box), so a
kernel change that costs a factor ~3 in accuracy fails the suite instead of hiding under a generic 1e-2.  Integer / byte /
index stages are compared bit-exactly in the tests themselves and have no entry here.

Arithmetic of the path: fp16 MFMA operands, fp32 accumulation, fp32 residual stream / LayerNorm / softmax,
fp16 inter-kernel activations — against the reference's eager fp32.
"""
import json
import os

# ---- encoder + map_decoder (post-LayerNorm2d embeddings are O(1); mask scores are sigmoid outputs) -------------------------
EMB_REL_L2 = 3e-3            # measured 7.5e-4 .. 9.6e-4 (12 .. 32 blocks, ViT-B / L / H, heavy-tailed weights)
EMB_MAX_ABS = 1.7e-2         # measured 4.4e-3 .. 5.6e-3
EMB_REL_L2_SHALLOW = 2e-3    # 1-2 block stacks: measured <= 6e-4
MASK_SCORE = 5e-4            # measured 9e-5 .. 1.4e-4 (3.8e-4 worst case of the randomised sweep)
MASK_LOGIT = 7e-3            # logits are O(3..10); measured 2.3e-3
U8_WITHIN1 = 0.999           # fraction of u8 mask pixels within +-1 level (max +-2 asserted separately)
# ---- TopoNet ------------------------------------------------------------------------------------------------------------------
TOPO_SCORE = 3e-3            # measured 5.1e-4 .. 7.6e-4
TOPO_LOGIT = 2e-2            # logits of the pair classifier, O(1..5)
TOPO_DECISIONS = 0.998       # fraction of (score > 0.5) decisions equal; measured 0.9994 .. 0.9995
TOPO_GOLDEN = 1.2e-3         # vs the reference's own TopoNet source (AST fixture); measured 3.7e-4
# ---- SAM MaskDecoder branch (archived USE_SAM_DECODER configs) ------------------------------------------------------------------
SAMDEC_SCORE = 2e-3          # measured 3.7e-4 (reference-run fixture) / 6.2e-4 (oracle, 512^2)
SAMDEC_LOGIT = 2e-2
# ---- batch-composition independence (the same tile in a batch of 16 / 64 vs a batch of 2: different GEMM kernels) ------------------
BATCH_INDEP_EMB_REL = 2e-3
BATCH_INDEP_SCORE = 5e-4

# ---- attention op level (tests/test_gpu_attention.py, against tests/attention_ref.py attention64 in float64; the record of the measured
# values is profiles/parity_measured_op_attention.json) ------------------------------------------------------------------------------------
# A priori: the design has two fp16 roundings, the softmax numerators exp(s - max) as the MFMA operand of P.V (the row sum is taken from
# the unrounded f32 values) and the stored output; both simulated in float64 on the same inputs (attention64 round_points=True).  A case
# that has no closed-form answer (random: q, k ~ 1.5 N(0, 1), rel-pos 0.3, a peaked softmax; ramp_up / ramp_down: logits that rise / fall
# over 40 .. 60 nats along the keys; big: logits of a few hundred) is held, in max-abs and in mean-abs, to this factor times the a-priori
# error of the SAME case, computed in the test.  The factor covers P rounded against a running maximum instead of the final one, the f32
# accumulation order, v_exp_f32 and v_rcp_f32.  A priori over the 36 such cases: max-abs 4.3e-4 .. 2.2e-3 (half an fp16 ulp of the largest
# outputs, 2^-9 in [2, 4)), mean-abs 4.9e-5 .. 1.6e-4.  Measured / a priori, worst per kernel (max-abs, mean-abs): attn_window_kernel
# 1.00, 1.00; attn_global_kernel fixed 1.05, 1.00, runtime-S 1.00, 1.00; attention_hdx windowed 1.01, 1.00, 16 x 16 global 1.02, 1.00;
# attn_generic_kernel<10> 1.00, 0.98 (it keeps P in f32: 0.67 .. 0.98 of the simulated mean).  Over all 36: 0.74 .. 1.05 and 0.67 .. 1.00.
ATTN_OP_VS_APRIORI = 2.0
# The cases with an exact answer are held to bounds derived in tests/attention_ref.py make_case, as error / bound < 1.  Measured: uniform
# (one fp16 ulp + 2^-24) 0 .. 0.50: half an ulp, the store's rounding alone, on all 18 geometries; selector 0 .. 0.08, padsink 0.
# tests/test_gpu_ops.py test_sam_attention and tests/test_gpu_patch_sizes.py _attention_case (random inputs against a float32 reference,
# head dims 64 and 80, windowed / global): ATTN_OP_VS_APRIORI x the worst a-priori error over their 29 cases, max-abs 2.046e-3 and mean-abs
# 1.616e-4 (tests/test_attention_ref.py test_old_bounds_are_twice_the_a_priori_error computes both).  They were 2e-2 and 1.5e-3.
ATTN_OP_MAX = 4.09e-3        # measured 1.74e-3 .. 2.05e-3
ATTN_OP_MEAN = 3.23e-4       # measured 1.04e-4 .. 1.60e-4

# ---- GEMM op level, fp16 output (f32 accumulate, one rounding of the result): max-abs error / max(|ref|, 1) ------------------------------
GEMM_F16_OUT = 1.5e-3        # half an fp16 ulp of the largest magnitude is 4.9e-4 at |ref| in [4, 8); measured <= 5e-4 in round 4's probe
GEMM_MLP_PAIR = 2.5e-3       # fc1 -> fc2 against torch on torch's fp16 hidden activation (a one-ulp difference in a few hidden values)

# ---- heads after the encoder at op level (tests/test_gpu_heads.py, against float64 references) ----------------------------------------
# map_decoder on weights that reach pre-activations of +-8 and logits of +-15 (tests/heads_ref.py DECODER_STDS), fp16 inputs and weights.
# A priori: the kernel rounds the activations to fp16 at three layer boundaries (the MFMA B operands of layers 3, 5 and 7) and uses
# gelu_fast (|error| <= 1.6e-6, negligible); the same three roundings simulated in float64 on 4 tiles of 256 px give logits 6.6e-3
# and scores 1.3e-3 max-abs (the sigmoid's slope is 1/4 where the logits are small).
DEC_OP_LOGIT = 2e-2          # measured 5.2e-3 .. 7.8e-3 (S = 16 .. 64)
DEC_OP_SCORE = 3e-3          # measured 1.01e-3 .. 1.06e-3
# bilinear sampler, f32 in and out, max-abs error / max|emb|.  A priori: f32 rounding only — mostly of the unnormalised coordinate
# ((g + 1) * w rounds at |value| <= 2 w: <= w 2^-23 in each of ix, iy), so at most ~2 w 2^-23 ~ 8e-6 of max|emb| at w = 32; the
# typical rounding is far below that worst case, and integer points are exact up to the taps' products.
SAMPLE_OP_F32 = 2e-6         # measured 2.6e-7 .. 7.1e-7 (f32 points), 5.3e-8 .. 8.8e-8 (i64 points)

# ---- residual-stream passes at op level (tests/test_gpu_residual.py, against float64 references; the folds themselves are exact;
# the record of the measured values is profiles/parity_measured_op_residual.json) ----------
# LayerNorm of the folded x' at tests/test_gpu_ops.py test_layernorm's distributions (x ~ 3 N(0,1) + 1.5, gamma / beta ~ N(0,1)), max-abs.
# A priori: outputs reach |y| ~ 16 on 10^7 elements; f32: a few ulp of that (2e-6 each); f16: half an fp16 ulp of the output, 3.9e-3 at |y| in [8, 16).
RESID_LN_F32 = 6e-6          # measured 8.4e-7 .. 2.3e-6 (47 cases: every width, 197 .. 33285 rows, every fused mode); test_layernorm's bound is 2e-5
# The fp16 bound is absolute for |y| < 16 and counts in units of the fp16 spacing relative to [8, 16) beyond (x 2 in [16, 32)): a handful of
# the 10^7 outputs of the large shapes exceed 16 (seen on the CPU, in the float64 reference alone), where half an ulp is 7.8e-3 by itself.
RESID_LN_F16 = 5e-3          # measured 1.9e-3 .. 3.91e-3 (half an fp16 ulp in [8, 16)); test_layernorm's bound
# GEMM f32 output (the deferred split-K chain's x', the pos epilogue): max-abs error / (max(|ref|, 1) * sqrt(K / 64)), test_gemm's formula
# (its coefficient there is 2e-4, against a float32 product; against float64, with f32 accumulation of K <= 5120 terms of O(0.03):)
RESID_GEMM_F32 = 1e-7        # measured 1.8e-8 .. 2.3e-8 (split-K chain), 2.5e-8 .. 3.7e-8 (pos epilogue), 8.2e-9 .. 8.7e-9 (pos against a host-side add)

# ---- the fused TopoNet trunk at op level (tests/test_gpu_topo_trunk.py, against tests/heads_ref.py topo_trunk_ref / toponet_ref in float64;
# the record of the measured values is profiles/parity_measured_op_topo.json) ---------------------------------------------------------
# heads_ref.topo_fill's model (fp16-representable matrices, biases and betas ~ N(0, 1), gammas in +-[1, 2], peaked and flat softmax rows;
# logits of O(1..5)), max-abs over the defined slots of every sequence count of a case.  A priori: the kernel's fp16 roundings (every
# MFMA operand: the pair_proj and LayerNorm outputs, q, k, v, the unnormalised P, O, the FFN's hidden activation) simulated in float64
# on the same inputs (topo_trunk_ref round_points=True) give logits 1.35e-3 .. 2.07e-3 and scores 2.8e-4 .. 4.4e-4 over the 13 K; the
# kernel lands on them (K = 1: 1.353e-3 simulated and measured), so its f32 arithmetic, exp2 and rsqrt add nothing visible.
TOPO_OP_LOGIT = 4.5e-3       # measured 1.35e-3 .. 2.19e-3 (K = 1 .. 64: packed slots, one wave, wave groups of 2 .. 4)
TOPO_OP_SCORE = 9.5e-4       # measured 2.8e-4 .. 4.6e-4
# TOPONET_VERSION no_transformer: pair_proj, ReLU and output_proj only; the fp16 inputs and weights are exact, the rest is f32.  A priori:
# f32 accumulation of 258 products of O(1) and of 128 of O(1): a few 1e-7 of logits of O(5) (round_points changes nothing here).
TOPO_OP_NOATT_LOGIT = 2.5e-6 # measured 6.8e-7 .. 9.5e-7
TOPO_OP_NOATT_SCORE = 5e-7   # measured 1.3e-7 .. 1.8e-7
# srh_toponet (sampler, feature_proj, pair gather, trunk) on the same model against toponet_ref, which rounds the three fp16 buffers
# between the launches as the library does.  A priori (the trunk's roundings on top): logits 9.2e-4 .. 1.42e-3, scores 2.0e-4 .. 3.1e-4;
# the measured values reach 1.4x that: the library rounds f32 sampler and GEMM results to fp16, the reference float64 ones, and a value
# that falls on the other side of a rounding boundary enters the trunk one fp16 ulp off.
TOPO_CHAIN_LOGIT = 5e-3      # measured 8.7e-4 .. 2.03e-3 (K = 5, 16, 33; f32 and i64 points)
TOPO_CHAIN_SCORE = 1e-3      # measured 1.7e-4 .. 4.3e-4

# ---- the SAM MaskDecoder branch at op level (tests/test_gpu_samdec.py, against tests/samdec_ref.py samdec_ref in float64; the record of
# the measured values is profiles/parity_measured_op_samdec.json) ------------------------------------------------------------------------
# samdec_ref.samdec_fill's model (fp16-representable image-side matrices, biases and betas ~ N(0, 1), gammas in +-[1, 2], peaked, in-between
# and flat heads in every attention; mask logits up to +-20, projected keys up to +-130), max-abs over every element, seven shapes from
# S = 8 to 64.  A priori: the library's fp16 roundings (the fp16 copy of the keys, the projected K / V / Q of the image side, the
# image -> token attention output, the two upscaling activations) simulated in float64 on the same inputs (samdec_ref round_points=True;
# tests/test_samdec_ref.py test_round_points_is_the_a_priori_error) give logits 7.5e-3 .. 9.1e-3, scores 1.7e-3 .. 2.1e-3, tokens_out
# 9.7e-4 .. 2.4e-3 and low_res 9.8e-3 .. 1.12e-2 over the seven shapes.  The kernels land on the logits, scores and low_res (worst over
# worst 1.04 x, 1.12 x, 1.06 x; per shape at most 1.2 x).  tokens_out: worst over worst 1.18 x, but 1.6 x at S = 64 and 1.45 x at S = 32.
# Both figures are the largest of 1 k .. 5 k values and hang on a handful of projected keys of |k| ~ 100 (fp16 spacing 0.0625) in the
# peaked token -> image heads, where the library rounds an f32 GEMM result and the simulation a float64 one: with f32-level noise
# (+-2^-23) put on every value before its simulated fp16 rounding, the simulated tokens_out error itself moves between 0.9 x and 1.7 x
# (1.8e-3 -> 3.0e-3 at S = 16, B = 5) and the logits' by up to 1.15 x.  So the same mechanism as the TopoNet chain's 1.4 x, nothing added
# by the kernels' f32 arithmetic, __expf or gelu_fast.
SAMDEC_OP_LOGIT = 1.4e-2     # measured 7.2e-3 .. 9.4e-3 (S = 8 .. 64)
SAMDEC_OP_SCORE = 3.5e-3     # measured 1.5e-3 .. 2.3e-3
SAMDEC_OP_TOKENS = 4.5e-3    # measured 1.4e-3 .. 2.9e-3 (values of O(3))
SAMDEC_OP_LOWRES = 1.8e-2    # measured 8.8e-3 .. 1.19e-2 (values up to +-24)
# sd_upsample_kernel on the low_res the device returned: f32 arithmetic on given inputs, max-abs error / max|low_res|.  A priori: the
# source coordinates and weights are exact (multiples of 1/8); two lerps = four products and two sums, each rounded once: at most
# 4 x 2^-24 = 2.4e-7 of max|low_res|, the result's own rounding included.
SAMDEC_UPSAMPLE_F32 = 3e-7   # measured 1.08e-7 .. 1.37e-7 (every pixel; 3.9e-8 .. 6.8e-8 on the rows and columns with clamped taps)
# the scores against the float64 sigmoid of the returned logits, max-abs.  A priori: 1 / (1 + __expf(-x)): the exponent's argument and
# exp2 round once each (relative (1 + |x|) 6e-8 on e, times the slope s (1 - s) <= 1/4), 1 + e, the division and the result round once
# each (6e-8, 6e-8 and 3e-8 of s <= 1): about 1.2e-7.
SAMDEC_SIGMOID_F32 = 2.5e-7  # measured 9.0e-8 .. 9.3e-8

_REC = {}


def check(name, value, bound, at_least=False):
    """Assert ``value < bound`` (``value >= bound`` with at_least) and record the measurement."""
    value = float(value)
    _REC[name] = {"measured": value, "bound": float(bound), "kind": "at_least" if at_least else "below"}
    print(f"[parity] {name}: measured {value:.3e}  bound {'>=' if at_least else '<'} {bound:.3e}")
    out = os.path.join(os.environ.get("GRAFT_REPO_ROOT", "."), "gpurun_out")
    if os.path.isdir(out):
        path = os.path.join(out, "parity_measured.json")
        try:
            prev = json.load(open(path))
        except Exception:
            prev = {}
        prev.update(_REC)
        with open(path, "w") as f:
            json.dump(prev, f, indent=1, sort_keys=True)
    if at_least:
        assert value >= bound, (name, value, bound)
    else:
        assert value < bound, (name, value, bound)
