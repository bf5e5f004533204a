"""The fixture of tests/test_detector_layers_gpu.py, checked on the CPU in float64 (tests/detector_layers_ref.py): that it
is well conditioned (the emulated-f16 error of each layer has max <= 16x its median - and that the decoder as seeded,
a saturated 900-query softmax, is NOT), that the yardstick tells every named mistake apart (>= 100x outside the bound at
the maximum, >= 20x at every quantile from the median up), and that the helper's restatements are the oracle's.  No GPU."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import detector_layers_ref as R
from oracle import gdino_ref

HW, B, NQ = (300, 412), 2, 900

# mistake -> (output, row group) in which it has to show.  A mistake confined to some rows is measured in the group of
# the rows it touches; the GPU tests hold every such group to the bound on its own (detector_layers_ref.groups).
ENCODER_SHOWS = {"no-pos query": ("src", "all"), "ref x/y exchanged": ("src", "all"),
                 "text layer without pos_text": ("text", "block tokens"),      # [CLS] / [SEP] attend to themselves only
                 "text self-mask ignored": ("text", "all")}
DECODER_SHOWS = {"qpos dropped from the text cross-attention query": ("output", "all"),
                 "x/y exchanged in sine_embed_4d": ("output", "all"),
                 "inverse_sigmoid left out of the box update": ("boxes", "all"),
                 "image 1 reads image 0's text rows": ("output", "image 1")}
BLOCK_TOKENS = {"block tokens": torch.tensor([1, 2])}


def _assert_discriminates(wrong, ref, emul, update, group, what, extra=None):
    r = R.ratios(wrong, ref, emul, update, extra)[group][2]
    print(f"mistake '{what}' ({group}): " + "  ".join(f"q{q} {v:.0f}x" for q, v in zip(R.QUANTILES, r)))
    assert r[-1] >= 100, f"the bound cannot tell the mistake '{what}' apart at the maximum: {r[-1]:.1f}x"
    assert (r >= 20).all(), f"the bound cannot tell the mistake '{what}' apart at every quantile: {r.tolist()}"


@pytest.mark.parametrize("hw", [(300, 412), (160, 224), (800, 1066)])
def test_levels_and_constants_are_the_plan_s(hw):
    """levels() and consts() (from gdino_ref) against the engine's host-built plan: level shapes, pos, encoder reference
    points, and the two-stage anchors of encoder_proposals."""
    from inklayer_amd import gdino
    lvl = R.fixture_sd()["transformer.level_embed"]
    eng = SimpleNamespace(cfg=gdino.GDinoConfig(), dev=torch.device("cpu"), level_embed_cpu=lvl)
    pl = gdino._Plan(eng, hw[0], hw[1], 1)
    assert [tuple(s) for s in pl.shapes] == R.levels(*hw)
    if hw == (300, 412):
        assert R.levels(*hw) == [(38, 52), (19, 26), (10, 13), (5, 7)] and pl.S == 2635 == 20 * 128 + 75
    if hw == (800, 1066):
        return
    c = R.consts(hw, 1)
    assert (pl.pos.double() - c.pos[0]).abs().max().item() <= 2.0 ** -22       # f32 sum against float64 sum
    assert torch.equal(pl.enc_ref.double(), c.ref2[0, :, 0])
    props, valid = gdino_ref.encoder_proposals(c.shapes)
    assert torch.equal(pl.props_unsig, props) and torch.equal(pl.valid_map >= 0, valid)


@torch.no_grad()
def test_encoder_triple_is_conditioned_and_its_mistakes_show():
    """Layer 0 on the random inputs, layer 1 on layer 0's float64 output (the emulated run on the emulated output), as
    tests/test_detector_layers_gpu.py runs them: both outputs of both layers meet the conditioning cap, and every
    encoder mistake planted in either layer shows in the output it touches."""
    sd, cfg, c = R.fixture_sd64(), R.config(), R.consts(HW, B)
    rs, rt = es, et = tuple(t.double() for t in R.encoder_inputs(HW, B, 4))
    for i in (0, 1):
        src, text = rs, rt
        rs, rt = R.encoder_triple(sd, cfg, i, src, text, c)
        ws_wt = {m: R.encoder_triple(sd, cfg, i, src, text, c, m, want=ENCODER_SHOWS[m][:1]) for m in R.ENCODER_MISTAKES}
        es, et = R.emulated(R.encoder_triple, sd, cfg, i, es, et, c)
        cs, ct = R.condition(rs, es), R.condition(rt, et)
        print(f"encoder triple {i}: emulated-f16 error max / median of src {cs:.1f}, of text {ct:.1f}")
        assert cs <= R.CONDITION_CAP and ct <= R.CONDITION_CAP
        for m, (ws, wt) in ws_wt.items():
            which, group = ENCODER_SHOWS[m]
            if which == "src":
                _assert_discriminates(ws, rs, es, rs - src, group, f"{m}, layer {i}")
            else:
                _assert_discriminates(wt, rt, et, rt - text, group, f"{m}, layer {i}", BLOCK_TOKENS)


@torch.no_grad()
def test_decoder_layer_is_conditioned_and_its_mistakes_show():
    """... and the decoder as seeded (no 1/16 on q / k) is rejected by the same condition."""
    cfg, shapes = R.config(), R.levels(*HW)
    output, ref, memory, text = (t.double() for t in R.decoder_inputs(HW, B, 4, NQ))
    args = (output, ref, text, memory, shapes)
    for i in (0, 1):
        for scaled in (True, False):
            sd = R.fixture_sd64(scaled)
            ro, rr = gdino_ref.decoder_layer(sd, cfg, i, *args)
            eo, er = R.emulated(gdino_ref.decoder_layer, sd, cfg, i, *args)
            cond = R.condition(ro, eo)
            print(f"decoder layer {i}, {'fixture' if scaled else 'as seeded'}: emulated-f16 error max / median {cond:.1f} "
                  f"(boxes {R.condition(rr, er):.1f})")
            assert (cond <= R.CONDITION_CAP) == scaled
            if scaled:
                assert R.condition(rr, er) <= R.CONDITION_CAP
            if not (scaled and i == 0):
                continue
            vo, vr = R.decoder_layer(sd, cfg, i, *args)                       # the restatement is the oracle's
            assert torch.equal(vo, ro) and torch.equal(vr, rr)
            for m in R.DECODER_MISTAKES:
                wo, wr = R.decoder_layer(sd, cfg, i, *args, mistake=m)
                which, group = DECODER_SHOWS[m]
                if which == "output":
                    _assert_discriminates(wo, ro, eo, ro - output, group, m)
                else:
                    _assert_discriminates(wr, rr, er, None, group, m)


@torch.no_grad()
def test_decode_is_the_tail_of_detector_forward():
    """detector_layers_ref.decode restates detector_forward after its encoder: same selection, hs, refs, logits and
    boxes, bit for bit, from detector_forward's own memory / memory_text (f32, 128 x 160 image: S = 426 >= 300 queries)."""
    sd, cfg = R.fixture_sd(), R.config()
    g = torch.Generator().manual_seed(5)
    img = torch.randn(1, 3, 128, 160, generator=g)
    text = 0.5 * torch.randn(4, 256, generator=g)
    mask, pid = gdino_ref.text_masks_and_position_ids(list(R.DEFAULT_IDS))
    st = {}
    logits, boxes = gdino_ref.detector_forward(sd, cfg, img, text, mask, pid, stages=st)
    d = R.decode(sd, cfg, st["memory"], st["memory_text"], R.levels(128, 160))
    assert torch.equal(d.topk, st["topk"]) and torch.equal(d.topk_logits, st["topk_logits"])
    assert torch.equal(d.ref0, st["refs"][0]) and len(d.refs) == len(st["refs"]) == 3
    dec_norm = lambda h: gdino_ref._ln(h, sd, "transformer.decoder.norm")
    assert all(torch.equal(dec_norm(a), b) for a, b in zip(d.hs, st["hs"]))
    assert all(torch.equal(a, b) for a, b in zip(d.refs, st["refs"]))
    assert torch.equal(d.logits, logits) and torch.equal(d.boxes, boxes)
    forced = st["topk"].flip(1)
    d2 = R.decode(sd, cfg, st["memory"], st["memory_text"], R.levels(128, 160), force_topk=forced)
    assert torch.equal(d2.topk, forced) and not torch.equal(d2.boxes, boxes)
