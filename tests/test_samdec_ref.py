"""CPU checks of tests/samdec_ref.py, the float64 reference tests/test_gpu_samdec.py compares the SAM MaskDecoder branch with: samdec_ref is
pinned to oracle/sam_decoder.py's PromptEncoder + MaskDecoder + F.interpolate run in float64 on the same state dict; the test model
(samdec_fill) and inputs (samdec_inputs) meet the conditions under which a wrong kernel shows, for every shape of the GPU tests; each
single mistake of a list moves the reference's outputs by >= 10x the bounds of the GPU tests; and the C ABI has the test-only entry.
A wrong reference, or a model that cannot discriminate, fails here, on any host."""
import os
import re
import warnings

import pytest
import torch
import torch.nn.functional as F

import samdec_ref as R
import tolerances as T
from oracle.sam_decoder import MaskDecoder, PromptEncoder, TwoWayTransformer
from oracle.samroad import AttrDict, SAMRoadOracle
from oracle.synth import synth_state_dict

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 2
EPS = 2.0 ** -52
# float64 against float64: the two differ in the order of their sums only.  Measured here: 4 .. 6 eps max|logit| for S = 8, 9, 16.
PIN_EPS_MULTIPLE = 50

_SD = {}


def _state_dicts():
    """(the op tests' model, the synthetic weights of the whole-model tests) as state dicts of a SAMRoad with USE_SAM_DECODER."""
    if not _SD:
        warnings.simplefilter("ignore")
        cfg = dict(SAM_VERSION="vit_b", PATCH_SIZE=256, TOPONET_VERSION="normal", SAM_CKPT_PATH="", ENCODER_DEPTH=1,
                   ENCODER_GLOBAL_ATTN_INDEXES=[], USE_SAM_DECODER=True)
        torch.manual_seed(0)
        synth = synth_state_dict(SAMRoadOracle(AttrDict(cfg)).eval(), SEED)
        _SD["synth"] = synth
        _SD["fill"] = dict(synth) | R.samdec_fill(synth, SEED)
    return _SD["fill"], _SD["synth"]


_REFS = {}


def _ref(S, B):
    """(emb, outputs, probe) of the unmutated reference on the op tests' model, computed once per shape."""
    if (S, B) not in _REFS:
        emb, probe = R.samdec_inputs(B, S, R.case_seed(S, B)), {}
        _REFS[S, B] = emb, R.samdec_ref(emb, _state_dicts()[0], S, probe=probe), probe
    return _REFS[S, B]


def _oracle_run(emb, sd, S):
    """oracle/sam_decoder.py in float64: PromptEncoder (no-prompt path), MaskDecoder (multimask_output), F.interpolate x4, NHWC."""
    pe = PromptEncoder(embed_dim=256, image_embedding_size=(S, S), input_image_size=(16 * S, 16 * S), mask_in_chans=16)
    dec = MaskDecoder(num_multimask_outputs=2, transformer=TwoWayTransformer(depth=2, embedding_dim=256, mlp_dim=2048, num_heads=8),
                      transformer_dim=256, iou_head_depth=3, iou_head_hidden_dim=256)
    for mod, prefix in ((pe, "prompt_encoder."), (dec, "mask_decoder.")):
        mod.load_state_dict({k[len(prefix):]: v for k, v in sd.items() if k.startswith(prefix)}, strict=True)
        mod.double().eval()
    B = emb.shape[0] // (S * S)
    with torch.no_grad():
        sparse, dense = pe(points=None, boxes=None, masks=None)
        # get_dense_pe builds its grid in float32 whatever the module's dtype: the same three lines on a float64 grid, through the
        # module's own _pe_encoding
        grid = torch.ones((S, S), dtype=torch.float64)
        coords = torch.stack([(grid.cumsum(dim=1) - 0.5) / S, (grid.cumsum(dim=0) - 0.5) / S], dim=-1)
        image_pe = pe.pe_layer._pe_encoding(coords).permute(2, 0, 1).unsqueeze(0)
        low, _ = dec(emb.double().reshape(B, S, S, 256).permute(0, 3, 1, 2), image_pe, sparse.double(), dense, multimask_output=True)
        logits = F.interpolate(low, (16 * S, 16 * S), mode="bilinear", align_corners=False)
    return logits.permute(0, 2, 3, 1), low


@pytest.mark.parametrize("S", [8, 9, 16])
def test_samdec_ref_matches_oracle_in_float64(S):
    sd, _ = _state_dicts()
    emb, (logits, scores, tokens, low), _ = _ref(S, 2)
    want, want_low = _oracle_run(emb, sd, S)
    scale = want.abs().max().item()
    assert scale >= 5
    d, dl = (logits - want).abs().max().item(), (low - want_low).abs().max().item()
    print(f"[samdec pin S={S}] logits {d:.3e} = {d / (EPS * scale):.0f} eps max|logit| ({scale:.1f}), low_res {dl:.3e}")
    assert d < PIN_EPS_MULTIPLE * EPS * scale and dl < PIN_EPS_MULTIPLE * EPS * scale
    assert (scores - torch.sigmoid(want)).abs().max().item() < PIN_EPS_MULTIPLE * EPS
    assert tuple(tokens.shape) == (2, 4, 256) and tuple(low.shape) == (2, 2, 4 * S, 4 * S)


def test_upsample4_ref_matches_interpolate():
    g = torch.Generator().manual_seed(1)
    low = torch.randn(2, 2, 36, 36, generator=g, dtype=torch.float64) * 5
    for ac in (False, True):
        want = F.interpolate(low, (144, 144), mode="bilinear", align_corners=ac)
        # align_corners=True (a mutation only) rounds its source coordinate i (L - 1) / (P - 1) next to whole numbers
        assert (R.upsample4_ref(low, align_corners=ac) - want).abs().max().item() < (1e-12 if ac else 1e-13)
    # without the clamp only the first two rows and columns differ
    d = (R.upsample4_ref(low, clamp_low=False) - R.upsample4_ref(low)).abs()
    assert d[..., 2:, 2:].max().item() == 0 and d[..., :2, :].max().item() > 0.1 and d[..., :, :2].max().item() > 0.1


def _conditions(probe, outputs, HW):
    """The figures the input conditions are about."""
    logits, scores = outputs[0], outputs[1]
    st = R.attention_stats(probe)
    return dict(t2i=[st[f"t2i{i}"] for i in range(3)], i2t=[st[f"i2t{i}"] for i in range(2)],
                undecided=((scores > 0.05) & (scores < 0.95)).double().mean().item(), max_logit=logits.abs().max().item(),
                f16_max=max(probe["f16"].values()))


@pytest.mark.parametrize("S,B", R.SHAPES)
def test_inputs_meet_the_conditions(S, B):
    """Conditions, not measurements: peaked and flat heads in every attention, undecided scores, large logits, fp16 range."""
    HW = S * S
    emb, outputs, probe = _ref(S, B)
    assert all(torch.isfinite(t).all() for t in outputs)
    c = _conditions(probe, outputs, HW)
    print(f"[samdec conditions S={S} B={B}] undecided {c['undecided']:.3f} max|logit| {c['max_logit']:.1f} fp16 max {c['f16_max']:.0f}")
    for i, heads in enumerate(c["t2i"]):
        print(f"    token->image {i}: median row maximum per head " + " ".join(f"{v:.4f}" for v in heads) + f"   (8/HW = {8 / HW:.4f})")
        assert sum(v >= 0.5 for v in heads) >= 2, f"token->image attention {i}: fewer than two peaked heads"
        assert min(heads) <= 8.0 / HW, f"token->image attention {i}: no flat head"
    for i, heads in enumerate(c["i2t"]):
        print(f"    image->token {i}: median row maximum per head " + " ".join(f"{v:.4f}" for v in heads))
        assert max(heads) >= 0.9 and min(heads) <= 0.4, f"image->token attention {i}"
    assert c["undecided"] >= 0.20
    assert c["max_logit"] >= 5
    assert c["f16_max"] < 65504 / 2
    # rows of unit variance; tiles, grid rows and grid columns all differ
    e = emb.reshape(B, S, S, 256).double()
    assert (e.var(-1, unbiased=False) - 1).abs().max().item() < 1e-5 and e.mean(-1).abs().max().item() < 1e-6
    assert (e - e.transpose(1, 2)).abs().mean().item() > 0.5
    if B > 1:
        assert (e[0] - e[1]).abs().mean().item() > 0.5


def test_synthetic_weights_are_never_peaked():
    """The recorded number behind "never peaked": with synth_state_dict weights (those of the three whole-model tests) the most peaked
    head of any token->image attention puts 0.042 on its best key at S = 16 and 0.015 at S = 32 (median over its rows; 11 x and 16 x the
    uniform weight), the most peaked image->token head 0.27 of 1 on its best of 4 keys, and max|logit| is 1.7: every score is undecided."""
    _, synth = _state_dicts()
    for S, B in ((16, 2), (32, 1)):
        emb, probe = R.samdec_inputs(B, S, R.case_seed(S, B)), {}
        c = _conditions(probe, R.samdec_ref(emb, synth, S, probe=probe), S * S)
        t2i, i2t = max(max(h) for h in c["t2i"]), max(max(h) for h in c["i2t"])
        print(f"[samdec synth S={S}] token->image: largest median row maximum {t2i:.4f} ({t2i * S * S:.1f} x uniform); image->token: "
              f"{i2t:.3f} (uniform 0.25); undecided {c['undecided']:.3f}, max|logit| {c['max_logit']:.2f}")
        assert t2i < 0.1 and i2t < 0.4 and c["max_logit"] < 5, "the synthetic weights meet a condition: update this docstring and test_gpu_samdec's"


# which outputs a mutation is judged on, besides the mask logits
_ALSO = {"t2i_scale": ("tokens",), "swap_t2i_heads": ("tokens",), "no_key_pe": ("tokens",), "layer0_adds": ("tokens",), "idle_exp0": ("tokens",),
         "mask_tokens_01": ("low",), "swap_kykx_1": ("low",), "swap_kykx_2": ("low",), "hyper_shift": ("low",)}


@pytest.mark.parametrize("name", list(R.MUTATIONS))
def test_every_mutation_moves_the_outputs(name):
    """Each single mistake moves the mask logits (and tokens_out / low_res where it acts on them) by >= 10x the GPU tests' bound."""
    sd, _ = _state_dicts()
    for S, B in ((8, 3), (9, 2)):
        if name == "idle_exp0" and S != 8:       # only HW < 256 leaves waves of sd_t2i_attn_kernel without a key; at S = 8, 192 threads
            continue
        emb, (logits, scores, tokens, low), _ = _ref(S, B)
        m_logits, _, m_tokens, m_low = R.samdec_ref(emb, sd, S, mutate=R.MUTATIONS[name])
        moved = dict(logits=(m_logits - logits).abs().max().item(), tokens=(m_tokens - tokens).abs().max().item(),
                     low=(m_low - low).abs().max().item())
        bound = dict(logits=T.SAMDEC_OP_LOGIT, tokens=T.SAMDEC_OP_TOKENS, low=T.SAMDEC_OP_LOWRES)
        print(f"[samdec mutation {name} S={S}] " + " ".join(f"{k} {v:.3e} ({v / bound[k]:.0f}x)" for k, v in moved.items()))
        for k in ("logits",) + _ALSO.get(name, ()):
            assert moved[k] >= 10 * bound[k], (name, S, k, moved[k], bound[k])


def test_round_points_is_the_a_priori_error():
    """The a-priori error of a correct kernel (tests/tolerances.py quotes these): the fp16 roundings of the library, simulated in float64,
    stay below the GPU tests' bounds on every shape, so the bounds are not below what a correct kernel needs."""
    sd, _ = _state_dicts()
    worst = dict(logits=0.0, scores=0.0, tokens=0.0, low=0.0)
    for S, B in R.SHAPES:
        emb, ref, _ = _ref(S, B)
        got = R.samdec_ref(emb, sd, S, round_points=True)
        err = {k: (a - b).abs().max().item() for k, a, b in zip(worst, got, ref)}
        print(f"[samdec a priori S={S} B={B}] " + " ".join(f"{k} {v:.3e}" for k, v in err.items()))
        worst = {k: max(worst[k], err[k]) for k in worst}
    print("[samdec a priori worst] " + " ".join(f"{k} {v:.3e}" for k, v in worst.items()))
    assert worst["logits"] <= T.SAMDEC_OP_LOGIT and worst["scores"] <= T.SAMDEC_OP_SCORE
    assert worst["tokens"] <= T.SAMDEC_OP_TOKENS and worst["low"] <= T.SAMDEC_OP_LOWRES


def test_abi_has_the_sam_decoder_entry_and_stays_11():
    from sam_road_amd import _lib
    header = open(os.path.join(ROOT, "include", "samroad_hip.h")).read()
    lib = _lib.load()
    assert lib.srh_abi_version() == _lib.ABI_VERSION == int(re.search(r"#define SRH_ABI_VERSION (\d+)", header).group(1)) == 11
    assert hasattr(lib, "srh_op_sam_decoder") and len(_lib.SYMBOLS["srh_op_sam_decoder"][1]) == 9
    decl = re.search(r"\bint srh_op_sam_decoder\(([^;]*)\);", header).group(1)
    assert len(decl.split(",")) == 9
