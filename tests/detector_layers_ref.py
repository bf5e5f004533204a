"""Fixture, float64 references, yardstick and named mistakes of the detector's encoder triples (fusion, text enhancer,
deformable layer) and decoder layers, shared by tests/test_detector_layers_gpu.py (GDinoEngine._enc_layer / _dec_layer /
decoder against float64) and tests/test_detector_layers_plan_cpu.py (that the fixture is well conditioned and that the
yardstick tells the named mistakes apart, on the CPU).

Everything here is float64 on the CPU and built from oracle/gdino_ref.py's own functions and constants.

The fixture.  Seeded weights (seed 77, 2 encoder + 2 decoder layers, gamma_v / gamma_l as test_gdino_gpu.small_dino) make
the decoder's 900-query self-attention an argmax: score std ~330, median max-probability 1.000, and the float64 layer moves
by up to 2.3 on O(1) outputs when its linear operands are rounded to f16 - a yardstick of "2x the emulated error" accepts
anything there.  So the q and k rows of decoder.layers.*.self_attn.in_proj_{weight,bias} and of ...ca_text.in_proj_* are
scaled by QK_SCALE = 1/16 (scores 256x smaller).  The second layer of decoder.ref_point_head (the consumer of the 4-d
sine embedding) is scaled by RPH_SCALE = 1.5: as seeded, exchanging x / y in that embedding lands 93x outside the bound at
the maximum, with the scale 120x.  Everything else stays as seeded.  tests/test_detector_layers_plan_cpu.py holds these
facts: the fixture's emulated error has max <= 16x its median, the seeded decoder's does not, every named mistake is
>= 100x outside the bound."""
import functools
from types import SimpleNamespace

import numpy as np
import torch

from oracle import gdino_ref as G
from oracle import sam_ref

F32, F64 = torch.float32, torch.float64
SEED = 77
QK_SCALE = 1.0 / 16                       # q / k rows of the decoder's self-attention and text cross-attention
RPH_SCALE = 1.5                           # decoder.ref_point_head.layers.1: the query position embedding's weight
LAYER_ABS = 2.0 ** -12                    # SWIN_BLOCK_ABS / BLOCK_ABS: a quarter of an f16 ulp of the largest update
BOX_ABS = 1e-6                            # test_box_refine's bound
QUANTILES = (0.5, 0.9, 0.99, 0.999, 1.0)
CONDITION_CAP = 16.0                      # max / median of the emulated-f16 error of a layer
DEFAULT_IDS = (101, 4874, 1012, 102)      # [CLS] object . [SEP]: tokens 1-2 form one self-attention block
SHORT_IDS = (101, 4874, 102)              # T = 3: every token attends to itself only
T = "transformer."

ENCODER_MISTAKES = ("no-pos query", "ref x/y exchanged", "text layer without pos_text", "text self-mask ignored")
DECODER_MISTAKES = ("qpos dropped from the text cross-attention query", "x/y exchanged in sine_embed_4d",
                    "inverse_sigmoid left out of the box update", "image 1 reads image 0's text rows")


def config(num_queries=300, dec_layers=2):
    return G.GDinoConfig(enc_layers=2, dec_layers=dec_layers, num_queries=num_queries)


@functools.lru_cache(maxsize=None)
def seeded_sd():
    """The f32 state dict as seeded (the saturated decoder), gamma_v / gamma_l as in small_dino."""
    sd = sam_ref.seeded_state_dict(G.gdino_param_shapes(config()), SEED)
    for k in sd:
        if k.endswith("gamma_v") or k.endswith("gamma_l"):
            sd[k] = 0.3 * torch.ones_like(sd[k]) + 0.05 * sd[k]
    return sd


@functools.lru_cache(maxsize=None)
def fixture_sd():
    """The fixture: seeded_sd() with the q and k rows (the first 512 of in_proj) of the decoder's two attentions x 1/16
    and decoder.ref_point_head.layers.1 x 1.5."""
    sd = dict(seeded_sd())
    for leaf in ("weight", "bias"):
        k = f"{T}decoder.ref_point_head.layers.1.{leaf}"
        sd[k] = sd[k] * RPH_SCALE
    for k in sd:
        if k.startswith(T + "decoder.layers.") and (".self_attn.in_proj_" in k or ".ca_text.in_proj_" in k):
            x = sd[k].clone()
            x[:512] *= QK_SCALE
            sd[k] = x
    return sd


def to64(sd):
    """The transformer's and the box head's parameters in float64 (the Swin backbone and input_proj are not used here)."""
    return {k: v.double() for k, v in sd.items() if k.startswith(T) or k.startswith("bbox_embed.")}


@functools.lru_cache(maxsize=None)
def fixture_sd64(scaled=True):
    return to64(fixture_sd() if scaled else seeded_sd())


def levels(h, w):
    """The four feature levels of an h x w input: Swin stages 1-3 (strides 8, 16, 32, each a ceil-halving) and the
    3x3 / stride 2 / pad 1 extra level.  300 x 412 -> 38x52, 19x26, 10x13, 5x7 (S = 2635 = 20 * 128 + 75)."""
    half = lambda n: (n + 1) // 2
    H, W = half(-(-h // 4)), half(-(-w // 4))
    out = [(H, W)]
    for _ in range(2):
        H, W = half(H), half(W)
        out.append((H, W))
    out.append(((H - 1) // 2 + 1, (W - 1) // 2 + 1))
    return out


@functools.lru_cache(maxsize=None)
def consts(hw, B, ids=DEFAULT_IDS):
    """What detector_forward builds ahead of its encoder loop, from the oracle's own functions: pos [B,S,256] (sine + level
    embedding), the encoder's reference points [B,S,4,2], the text position embedding [B,T,256], the text self-mask."""
    cfg, sd = config(), fixture_sd()
    shapes = levels(*hw)
    pos = torch.cat([G.pos_sine_hw(cfg, B, h, w).flatten(2).transpose(1, 2) + sd[T + "level_embed"][l].view(1, 1, -1)
                     for l, (h, w) in enumerate(shapes)], 1).double()
    ref2 = G.enc_reference_points(shapes)[None, :, None, :].expand(B, -1, cfg.num_feature_levels, -1).double()
    mask, pid = G.text_masks_and_position_ids(list(ids))
    pos_text = G.sine_pos_embed_1d(pid.float())[None].expand(B, -1, -1).double()
    return SimpleNamespace(shapes=shapes, S=sum(a * b for a, b in shapes), pos=pos, ref2=ref2, pos_text=pos_text,
                           mask=mask, ids=tuple(ids))


# ---------------------------------------------------------------------------------------------------------------
# inputs (f32, as the engine receives them)
# ---------------------------------------------------------------------------------------------------------------
def encoder_inputs(hw, B, n_text, seed=0):
    """src [B,S,256] ~ N(0,1), a different draw per image; text [B,T,256] of std 0.5, a different draw per image."""
    S = sum(a * b for a, b in levels(*hw))
    g = torch.Generator().manual_seed(1000 + seed)
    return torch.randn(B, S, 256, generator=g), 0.5 * torch.randn(B, n_text, 256, generator=g)


def edge_boxes(g):
    """Centre 0, centre 1, the whole-image-sized box at centre 1, a 1e-3-sized box."""
    size = lambda: 0.02 + 0.6 * torch.rand(2, generator=g)
    return torch.stack([torch.cat([torch.zeros(2), size()]), torch.cat([torch.ones(2), size()]), torch.ones(4),
                        torch.cat([torch.rand(2, generator=g), torch.full((2,), 1e-3)])])


N_EDGE = 4


def decoder_inputs(hw, B, n_text, nq, seed=0):
    """output [B,nq,256] ~ N(0,1), reference boxes [B,nq,4] (random centres, sizes 0.02 ... 0.62; rows 0-3 of every image
    are edge_boxes), memory [B,S,256] ~ N(0,1), text [B,T,256] of std 0.5; every image has its own draw."""
    S = sum(a * b for a, b in levels(*hw))
    g = torch.Generator().manual_seed(2000 + seed)
    output = torch.randn(B, nq, 256, generator=g)
    ref = torch.cat([torch.rand(B, nq, 2, generator=g), 0.02 + 0.6 * torch.rand(B, nq, 2, generator=g)], -1)
    for b in range(B):
        ref[b, :N_EDGE] = edge_boxes(g)
    memory = torch.randn(B, S, 256, generator=g)
    return output, ref, memory, 0.5 * torch.randn(B, n_text, 256, generator=g)


# ---------------------------------------------------------------------------------------------------------------
# float64 references and their mistaken variants
# ---------------------------------------------------------------------------------------------------------------
def emulated(fn, *a, **kw):
    """fn under gdino_ref.f16_operands(): both operands of every linear rounded to f16 (the yardstick)."""
    with G.f16_operands():
        return fn(*a, **kw)


def encoder_triple(sd, cfg, i, src, text, c, mistake=None, want=("src", "text")):
    """Iteration i of detector_forward's encoder loop on float64 src [B,S,256] / text [B,T,256]; c = consts(...).
    want: the outputs to compute (the text layer feeds only `text`, the deformable layer only `src`); the other is None."""
    assert mistake is None or mistake in ENCODER_MISTAKES
    pos, ref2, pos_text, mask = c.pos, c.ref2, c.pos_text, c.mask
    if mistake == "no-pos query":                       # src instead of src + pos as the deformable attention's query
        pos = torch.zeros_like(pos)
    if mistake == "ref x/y exchanged":
        ref2 = ref2.flip(-1)
    if mistake == "text layer without pos_text":
        pos_text = torch.zeros_like(pos_text)
    if mistake == "text self-mask ignored":
        mask = torch.ones_like(mask)
    src, text = G.fusion_layer(sd, f"{T}encoder.fusion_layers.{i}.", src, text)
    text = G.text_layer(sd, f"{T}encoder.text_layers.{i}.", text, pos_text, mask) if "text" in want else None
    src = G.deform_enc_layer(sd, f"{T}encoder.layers.{i}.", cfg, src, pos, ref2, c.shapes) if "src" in want else None
    return src, text


def decoder_layer(sd, cfg, i, output, ref, text, memory, shapes, mistake=None):
    """gdino_ref.decoder_layer restated from the same gdino_ref functions so that a mistake can be planted inside it
    (the plan test holds the restatement with mistake=None to gdino_ref.decoder_layer, bit for bit)."""
    assert mistake is None or mistake in DECODER_MISTAKES
    p = f"{T}decoder.layers.{i}."
    ref_in = ref[:, :, None, :].expand(-1, -1, cfg.num_feature_levels, -1)
    box = ref_in[:, :, 0, :]
    if mistake == "x/y exchanged in sine_embed_4d":
        box = box[..., [1, 0, 2, 3]]
    qpos = G.mlp(sd, T + "decoder.ref_point_head.", G.sine_embed_4d(box), 2)
    q = output + qpos
    output = G._ln(output + G.mha(sd, p + "self_attn.", q, q, output, cfg.nheads), sd, p + "norm2")
    tq = output if mistake == "qpos dropped from the text cross-attention query" else output + qpos
    tx = text[:1].expand_as(text) if mistake == "image 1 reads image 0's text rows" else text
    output = G._ln(output + G.mha(sd, p + "ca_text.", tq, tx, tx, cfg.nheads), sd, p + "catext_norm")
    output = G._ln(output + G.msda_module(sd, p + "cross_attn.", cfg, output + qpos, ref_in, memory, shapes),
                   sd, p + "norm1")
    f = G.F.linear(G.F.relu(G.F.linear(output, sd[p + "linear1.weight"], sd[p + "linear1.bias"])),
                   sd[p + "linear2.weight"], sd[p + "linear2.bias"])
    output = G._ln(output + f, sd, p + "norm3")
    old = ref if mistake == "inverse_sigmoid left out of the box update" else G.inverse_sigmoid(ref)
    return output, (G.mlp(sd, "bbox_embed.0.", output, 3) + old).sigmoid()


def decode(sd, cfg, memory, text, shapes, force_topk=None):
    """The part of detector_forward after its encoder: selection, cfg.dec_layers decoder layers, heads.  Returns a
    namespace of topk, topk_logits [B,S], ref0, hs (per layer, before decoder.norm), refs, logits, boxes."""
    order, sel_logits, ref_unsig = G.two_stage_selection(sd, cfg, memory, text, shapes, force_topk)
    ref = ref_unsig.sigmoid()
    output = sd[T + "tgt_embed.weight"][None].expand(memory.shape[0], -1, -1)
    hs, refs = [], [ref]
    for i in range(cfg.dec_layers):
        output, ref = G.decoder_layer(sd, cfg, i, output, ref, text, memory, shapes)
        hs.append(output)
        refs.append(ref)
    last = G._ln(hs[-1], sd, T + "decoder.norm")
    boxes = (G.mlp(sd, "bbox_embed.0.", last, 3) + G.inverse_sigmoid(refs[-2])).sigmoid()
    return SimpleNamespace(topk=order, topk_logits=sel_logits, ref0=refs[0], hs=hs, refs=refs,
                           logits=last @ text.transpose(-1, -2), boxes=boxes)


# ---------------------------------------------------------------------------------------------------------------
# the yardstick
# ---------------------------------------------------------------------------------------------------------------
def _q(err):
    return np.quantile(err.reshape(-1).numpy(), QUANTILES)


def bound(ref, emul, update):
    """The project's layer yardstick (test_swin_block_matches_float64, test_vith_block_matches_float64), per quantile
    of QUANTILES: 2x the error of the float64 reference re-run under f16_operands() + LAYER_ABS * max|layer update|, for
    what that emulation does not round.  update None: a box output, + BOX_ABS instead."""
    a = BOX_ABS if update is None else LAYER_ABS * float(update.abs().max())
    return 2 * _q((emul - ref).abs()) + a


def groups(ref, extra=None):
    """The row groups each held to the bound: the whole tensor [B, N, C], each image, and `extra` (name -> rows of
    dim 1).  No element is exempt; a mistake confined to one image or to some rows cannot hide in the quantiles of the rest."""
    g = {"all": (slice(None), slice(None))}
    for b in range(ref.shape[0]):
        g[f"image {b}"] = (slice(b, b + 1), slice(None))
    for name, rows in (extra or {}).items():
        g[name] = (slice(None), rows)
    return g


def ratios(got, ref, emul, update, extra=None):
    """{group: (error quantiles of got, of emul, error / bound)}: bound() of each group's rows, with the update term
    taken over the whole tensor."""
    out = {}
    for name, (bi, ri) in groups(ref, extra).items():
        r, e = ref[bi][:, ri], emul[bi][:, ri]
        gq = _q((got[bi][:, ri] - r).abs().nan_to_num(nan=float("inf")))
        out[name] = (gq, _q((e - r).abs()), gq / bound(r, e, update))
    return out


def assert_within(got, ref, emul, update, what, extra=None):
    """Prints HIP / emulated / ratio per quantile (group "all") and the worst ratio of every group, asserts every
    quantile of every group; returns the worst ratio."""
    res = ratios(got.double().cpu(), ref, emul, update, extra)
    for qt, hq, eq, r in zip(QUANTILES, *res["all"]):
        print(f"{what} q{qt}: HIP {hq:.2e}  emulated-f16 {eq:.2e}  -> {r:.3f}x the bound")
    worst = {name: float(r.max()) for name, (_, _, r) in res.items()}
    print(f"{what}: worst ratio per group " + ", ".join(f"{n} {v:.3f}" for n, v in worst.items()))
    for name, (gq, eq, r) in res.items():
        assert (r <= 1.0).all(), (what, name, dict(zip(QUANTILES, zip(gq.tolist(), eq.tolist(), r.tolist()))))
    return max(worst.values())


def condition(ref, emul):
    """max / median of the emulated-f16 error."""
    e = (emul - ref).abs()
    return float(e.max() / e.median())
