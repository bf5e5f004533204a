"""The detector's encoder triples (fusion, text enhancer, deformable layer) and decoder layers as GDinoEngine composes them
(_enc_layer, _dec_layer, decoder) against float64 built from oracle/gdino_ref.py, on the well-conditioned fixture of
tests/detector_layers_ref.py (tests/test_detector_layers_plan_cpu.py shows on the CPU that its yardstick tells the named
mistakes apart).  Yardstick: at every error quantile, the maximum included, HIP <= 2x the float64 reference re-run with
f16-rounded linear operands + 2^-12 max|layer update| (boxes: + 1e-6), over the whole tensor and over each image on its
own; no query and no element is exempt.  Inputs are 300 x 412 (levels 38x52 ... 5x7, S = 2635 = 20 * 128 + 75: a ragged
last workgroup of ffn256_fused / msda_fused, odd level sizes) and 160 x 224 (S = 747).  GPU box only."""
import functools

import pytest
import torch

import detector_layers_ref as R

pytestmark = pytest.mark.gpu

F16, F32 = torch.float16, torch.float32
NAN = float("nan")
BIG, SMALL = (300, 412), (160, 224)


@pytest.fixture(scope="module")
def engines(dev):
    """(2-encoder / 2-decoder engine, 0-encoder / 1-decoder engine) from the fixture's weights, T = 4."""
    from inklayer_amd import gdino
    text0 = 0.5 * torch.randn(4, 256, generator=torch.Generator().manual_seed(3))
    mk = lambda e, d: gdino.GDinoEngine(R.fixture_sd(), gdino.GDinoConfig(enc_layers=e, dec_layers=d, num_queries=300), dev,
                                        encoded_text=text0, token_ids=R.DEFAULT_IDS)
    return mk(2, 2), mk(0, 1), text0


def _with_ids(eng, text0, ids):
    """The engine's caption set to len(ids) tokens (the text rows themselves are passed to _enc_layer by the test)."""
    eng.set_text(text0[:len(ids)], ids)


# ---------------------------------------------------------------------------------------------------------------
# encoder triple
# ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _encoder_reference(hw, B, ids):
    """Inputs and, per layer (layer 1 on layer 0's output), float64 (src, text), the same under f16_operands (layer 1
    on the emulated layer 0), and the layer's float64 update of each."""
    sd, cfg, c = R.fixture_sd64(), R.config(), R.consts(hw, B, ids)
    src, text = R.encoder_inputs(hw, B, len(ids), seed=len(ids))
    ref, emul, upd = [], [], []
    rs, rt = es, et = src.double(), text.double()
    for i in (0, 1):
        ps, pt = rs, rt
        rs, rt = R.encoder_triple(sd, cfg, i, rs, rt, c)
        es, et = R.emulated(R.encoder_triple, sd, cfg, i, es, et, c)
        ref.append((rs, rt)); emul.append((es, et)); upd.append((rs - ps, rt - pt))
    return src, text, ref, emul, upd


def _run_encoder(eng, dev, hw, B, src, text, n_layers):
    """_enc_layer 0 .. n_layers-1 on one pair of operand buffers (NaN before layer 0 writes them), as encoder() does."""
    pl = eng.plan(hw[0], hw[1], B)
    S, T = pl.S, text.shape[1]
    assert eng.T == T and src.shape[1] == S and [tuple(s) for s in pl.shapes] == R.levels(*hw)
    s, t = src.reshape(B * S, 256).to(dev).contiguous(), text.reshape(B * T, 256).to(dev).contiguous()
    s16 = torch.full((B * S, 256), NAN, device=dev, dtype=F16)
    s16p = torch.full((B * S, 256), NAN, device=dev, dtype=F16)
    outs = []
    for i in range(n_layers):
        s, t = eng._enc_layer(i, s, t, pl, B, s16, s16p)
        outs.append((s.clone().view(B, S, 256), t.clone().view(B, T, 256)))
    return outs


def _hold_encoder(outs, hw, B, ids, what):
    _, _, ref, emul, upd = _encoder_reference(hw, B, ids)
    extra = {"block tokens": torch.tensor([1, 2])} if tuple(ids) == R.DEFAULT_IDS else None
    worst = 0.0
    for i, (s, t) in enumerate(outs):
        worst = max(worst, R.assert_within(s, ref[i][0], emul[i][0], upd[i][0], f"{what} src after layer {i}"),
                    R.assert_within(t, ref[i][1], emul[i][1], upd[i][1], f"{what} text after layer {i}", extra))
    print(f"{what}: worst HIP / bound ratio {worst:.3f}")


@torch.no_grad()
@pytest.mark.parametrize("ids", [R.DEFAULT_IDS, R.SHORT_IDS], ids=["T4", "T3"])
@pytest.mark.parametrize("hw,B", [(BIG, 2), (SMALL, 3)], ids=["300x412-B2", "160x224-B3"])
def test_encoder_triple_matches_float64(dev, engines, hw, B, ids):
    """Product flags: layer 0, then layer 1 on layer 0's output and on the operand buffers layer 0's fold pass wrote; both
    outputs (src, text) held after one layer and after two."""
    eng, _, text0 = engines
    src, text = _encoder_reference(hw, B, ids)[:2]
    assert eng.fold_fusion and eng.fuse_ffn and eng.fuse_ffn_pre
    try:
        _with_ids(eng, text0, ids)
        outs = _run_encoder(eng, dev, hw, B, src, text, 2)
    finally:
        _with_ids(eng, text0, R.DEFAULT_IDS)
    _hold_encoder(outs, hw, B, ids, f"encoder {hw} B={B} T={len(ids)}")


@torch.no_grad()
@pytest.mark.parametrize("flag,hw,B,ids", [("fuse_ffn_pre", BIG, 2, R.DEFAULT_IDS), ("fuse_ffn", BIG, 2, R.DEFAULT_IDS),
                                           ("fold_fusion", BIG, 2, R.DEFAULT_IDS), ("fold_fusion", SMALL, 3, R.SHORT_IDS)],
                         ids=["fuse_ffn_pre", "fuse_ffn", "fold_fusion", "fold_fusion-160x224-B3-T3"])
def test_encoder_triple_other_branches_match_float64(dev, engines, flag, hw, B, ids):
    """The branches of _enc_layer the product flags switch off: out_proj GEMM + norm1 ahead of the fused FFN
    (fuse_ffn_pre = False), the two-GEMM FFN + LayerNorm (fuse_ffn = False), the unfolded fusion layer on the general
    kernel biattn_wide (fold_fusion = False; also at a ragged T = 3, B = 3).  One layer, the same bound."""
    eng, _, text0 = engines
    src, text = _encoder_reference(hw, B, ids)[:2]
    cls = type(eng)
    assert getattr(cls, flag) is True and flag not in vars(eng)
    try:
        setattr(eng, flag, False)
        _with_ids(eng, text0, ids)
        outs = _run_encoder(eng, dev, hw, B, src, text, 1)
    finally:
        delattr(eng, flag)
        _with_ids(eng, text0, R.DEFAULT_IDS)
    assert getattr(eng, flag) is True
    _hold_encoder(outs, hw, B, ids, f"encoder {flag}=False {hw} B={B} T={len(ids)}")


@torch.no_grad()
def test_encoder_triple_images_are_independent(dev, engines):
    """Image 0's src replaced: image 1's rows of both outputs, after two layers, are bit-equal."""
    eng, _, _ = engines
    src, text = _encoder_reference(BIG, 2, R.DEFAULT_IDS)[:2]
    a = _run_encoder(eng, dev, BIG, 2, src, text, 2)[-1]
    other = src.clone()
    other[0] = 3 * torch.randn(src.shape[1:], generator=torch.Generator().manual_seed(11)) + 1
    b = _run_encoder(eng, dev, BIG, 2, other, text, 2)[-1]
    assert torch.equal(a[0][1], b[0][1]) and torch.equal(a[1][1], b[1][1])
    assert not torch.equal(a[0][0], b[0][0]) and not torch.equal(a[1][0], b[1][0])


# ---------------------------------------------------------------------------------------------------------------
# decoder layer
# ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _decoder_reference(hw, B, nq, i):
    sd, cfg, shapes = R.fixture_sd64(), R.config(), R.levels(*hw)
    inp = R.decoder_inputs(hw, B, 4, nq, seed=nq)
    output, ref, memory, text = (t.double() for t in inp)
    r = R.G.decoder_layer(sd, cfg, i, output, ref, text, memory, shapes)
    e = R.emulated(R.G.decoder_layer, sd, cfg, i, output, ref, text, memory, shapes)
    return inp, r, e, r[0] - output


def _run_decoder_layer(eng, dev, hw, B, i, output, ref, memory, text):
    """_dec_layer and the box refinement that follows it in decoder(): (output [B,nq,256], boxes [B,nq,4])."""
    from inklayer_amd import ops
    pl = eng.plan(hw[0], hw[1], B)
    nq = output.shape[1]
    flat = lambda t: t.reshape(-1, t.shape[-1]).to(dev).contiguous()
    assert memory.shape[1] == pl.S
    ref_d = flat(ref)
    out = eng._dec_layer(i, flat(output), ref_d, ops.add_cvt_f16(flat(memory)), ops.add_cvt_f16(flat(text)), pl, B)
    boxes = ops.box_refine(eng._mlp3("box", ops.add_cvt_f16(out)), ref_d)
    return out.view(B, nq, 256), boxes.view(B, nq, 4)


@torch.no_grad()
@pytest.mark.parametrize("i", [0, 1])
@pytest.mark.parametrize("hw,B,nq", [(BIG, 2, 900), (SMALL, 3, 300)], ids=["300x412-B2-nq900", "160x224-B3-nq300"])
def test_decoder_layer_matches_float64(dev, engines, hw, B, nq, i):
    """_dec_layer on random queries, boxes (with the edge boxes: centre 0, centre 1, w = h = 1 at centre 1, 1e-3-sized),
    memory and per-image text; the output and the refined boxes box_refine(_mlp3("box", .), ref) are held."""
    eng, _, _ = engines
    (output, ref, memory, text), (ro, rb), (eo, eb), upd = _decoder_reference(hw, B, nq, i)
    out, boxes = _run_decoder_layer(eng, dev, hw, B, i, output, ref, memory, text)
    what = f"decoder layer {i} {hw} B={B} nq={nq}"
    worst = max(R.assert_within(out, ro, eo, upd, what + " output"), R.assert_within(boxes, rb, eb, None, what + " boxes"))
    print(f"{what}: worst HIP / bound ratio {worst:.3f}")


@torch.no_grad()
def test_decoder_layer_images_are_independent(dev, engines):
    """Image 0's output / ref / memory replaced: image 1's rows of the output and of the refined boxes are bit-equal."""
    eng, _, _ = engines
    output, ref, memory, text = _decoder_reference(BIG, 2, 900, 0)[0]
    a = _run_decoder_layer(eng, dev, BIG, 2, 0, output, ref, memory, text)
    o2, r2, m2, _ = R.decoder_inputs(BIG, 2, 4, 900, seed=12345)
    o2[1], r2[1], m2[1] = output[1], ref[1], memory[1]
    b = _run_decoder_layer(eng, dev, BIG, 2, 0, o2, r2, m2, text)
    assert torch.equal(a[0][1], b[0][1]) and torch.equal(a[1][1], b[1][1])
    assert not torch.equal(a[0][0], b[0][0])


# ---------------------------------------------------------------------------------------------------------------
# selection, heads, whole decoder
# ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _decode_reference(dec_layers):
    """Random memory [2,S,256] / text [2,4,256] and decode() in float64, then under f16_operands with the float64
    selection pinned."""
    sd, cfg, shapes = R.fixture_sd64(), R.config(dec_layers=dec_layers), R.levels(*BIG)
    _, _, memory, text = R.decoder_inputs(BIG, 2, 4, 300, seed=7)
    m64, t64 = memory.double(), text.double()
    r = R.decode(sd, cfg, m64, t64, shapes)
    e = R.emulated(R.decode, sd, cfg, m64, t64, shapes, force_topk=r.topk)
    assert torch.equal(e.topk, r.topk)
    return memory, text, r, e


def _run_decode(eng, dev, memory, text, topk):
    B, S = memory.shape[:2]
    pl = eng.plan(BIG[0], BIG[1], B)
    assert pl.S == S
    st = {"force_topk": topk}
    logits, boxes = eng.decoder(memory.reshape(B * S, 256).to(dev).contiguous(), text.reshape(-1, 256).to(dev).contiguous(),
                                pl, B, st)
    assert torch.equal(st["topk"].cpu().long(), topk)
    return logits, boxes, st


@torch.no_grad()
def test_selection_and_heads_match_float64(dev, engines):
    """decoder() of a 1-layer engine (its only layer is the last: decoder.norm, the box head on the selection's boxes, the
    per-image contrastive logits) with the float64 selection pinned.  Held: the selection logits (max over the text tokens
    of every encoder token), ref0, hs[0], the final logits and boxes.  The two logit outputs are no residual update:
    their absolute term is 2^-12 of their own largest magnitude.  f16_operands() rounds the operands of linear / conv2d
    only, not of the plain `@` of the contrastive head, whose operands the HIP path does round to f16; so for the logits
    the emulated error is what the rounding upstream (enc_output, the decoder layer) leaves in the head's operands, and
    the head's own rounding has to fit in the factor 2 and the absolute term."""
    _, eng1, _ = engines
    memory, text, r, e = _decode_reference(1)
    B, nq = 2, 300
    logits, boxes, st = _run_decode(eng1, dev, memory, text, r.topk)
    tgt = R.fixture_sd64()["transformer.tgt_embed.weight"]
    checks = [
        ("selection logits", st["topk_logits"].max(-1)[0][..., None], r.topk_logits[..., None], e.topk_logits[..., None],
         r.topk_logits),
        ("ref0", st["ref0"].view(B, nq, 4), r.ref0, e.ref0, None),
        ("hs[0]", st["hs"][0].view(B, nq, 256), r.hs[0], e.hs[0], r.hs[0] - tgt),
        ("logits", logits, r.logits, e.logits, r.logits),
        ("boxes", boxes, r.boxes, e.boxes, None)]
    assert len(st["hs"]) == 1 and len(st["refs"]) == 2 and torch.equal(st["refs"][0], st["ref0"])
    worst = max(R.assert_within(got, ref, emul, upd, "1-layer decoder() " + name) for name, got, ref, emul, upd in checks)
    print(f"1-layer decoder(): worst HIP / bound ratio {worst:.3f}")


@torch.no_grad()
def test_two_layer_decoder_matches_float64(dev, engines):
    """decoder() of the 2-layer engine on the same memory / text, the float64 selection pinned: the boxes and logits are
    held at every quantile, the maximum included, with no exempt share; so are the recorded hs and refs of both layers."""
    eng, _, _ = engines
    memory, text, r, e = _decode_reference(2)
    B, nq = 2, 300
    logits, boxes, st = _run_decode(eng, dev, memory, text, r.topk)
    tgt = R.fixture_sd64()["transformer.tgt_embed.weight"]
    assert len(st["hs"]) == 2 and len(st["refs"]) == 3
    checks = [("hs[0]", st["hs"][0].view(B, nq, 256), r.hs[0], e.hs[0], r.hs[0] - tgt),
              ("hs[1]", st["hs"][1].view(B, nq, 256), r.hs[1], e.hs[1], r.hs[1] - r.hs[0]),
              ("refs[1]", st["refs"][1].view(B, nq, 4), r.refs[1], e.refs[1], None),
              ("refs[2]", st["refs"][2].view(B, nq, 4), r.refs[2], e.refs[2], None),
              ("logits", logits, r.logits, e.logits, r.logits),
              ("boxes", boxes, r.boxes, e.boxes, None)]
    worst = max(R.assert_within(got, ref, emul, upd, "2-layer decoder() " + name) for name, got, ref, emul, upd in checks)
    print(f"2-layer decoder(): worst HIP / bound ratio {worst:.3f}")
