"""The detector with a multi-phrase caption of 23 tokens: the T > 4 path of GDinoEngine (unfolded fusion layer on
ops.biattn_wide, text attentions on ops.attn_midkeys) stage by stage against oracle/gdino_ref.py, predict() against a
numpy restatement of the reference's, and a switch back to a 4-token caption.  GPU box only.

Fixture: test_gdino_gpu.small_dino's recipe (seeded weights 77, 2 + 2 layers, 300 queries, gamma_v / gamma_l around
0.3), a 224 x 288 image, 23 token ids with three sub-sentences - the special ids 101 / 1012 / 102 in place, the others
arbitrary - and random [23, 256] text features."""
import bisect
import contextlib

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

#        [CLS] ----- 6 words ----- .    ------- 8 words -------------------- .    ---- 4 words ---- .   [SEP]
IDS23 = (101, 2001, 2002, 2003, 2004, 2005, 2006, 1012, 3001, 3002, 3003, 3004, 3005, 3006, 3007, 3008, 1012,
         4001, 4002, 4003, 4004, 1012, 102)
IDS4 = (101, 4874, 1012, 102)


def _rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).abs().max() / b.abs().max().clamp(min=1e-30)).item(), ((a - b).norm() / b.norm()).item()


@pytest.fixture(scope="module")
def caption_dino(dev):
    from oracle import gdino_ref, sam_ref
    from inklayer_amd import gdino
    assert len(IDS23) == 23
    oc = gdino_ref.GDinoConfig(enc_layers=2, dec_layers=2, num_queries=300)
    ec = gdino.GDinoConfig(enc_layers=2, dec_layers=2, num_queries=300)
    sd = sam_ref.seeded_state_dict(gdino_ref.gdino_param_shapes(oc), 77)
    for k in sd:
        if k.endswith("gamma_v") or k.endswith("gamma_l"):
            sd[k] = 0.3 * torch.ones_like(sd[k]) + 0.05 * sd[k]
    rs = np.random.RandomState(3)
    text4 = torch.from_numpy((0.5 * rs.standard_normal((4, 256))).astype(np.float32))
    text23 = torch.from_numpy((0.5 * rs.standard_normal((23, 256))).astype(np.float32))
    img = np.random.RandomState(12).randint(0, 256, size=(224, 288, 3)).astype(np.uint8)
    eng = gdino.GDinoEngine(sd, ec, dev, encoded_text=text23, token_ids=IDS23)
    return dict(sd=sd, oc=oc, ec=ec, eng=eng, text4=text4, text23=text23, img=img)


@torch.no_grad()
def test_caption_stages_match_oracle(dev, caption_dino):
    """memory, memory_text and topk_logits within test_detector_stages_match_oracle's relative bounds; boxes and logits
    with the selection pinned (force_topk): every quantile of the HIP error, the maximum included, at most 2x the
    fp32 oracle's own movement when its operands are rounded to f16 (gdino_ref.f16_operands), plus 1e-3 - that test's
    yardstick, measured in the run and not fixed."""
    from oracle import gdino_ref
    c = caption_dino
    sd, oc, eng, text, img = c["sd"], c["oc"], c["eng"], c["text23"], c["img"]
    assert eng.T == 23 and eng._text_attn.__name__ == "attn_midkeys"
    mean, std = torch.tensor([0.485, 0.456, 0.406]), torch.tensor([0.229, 0.224, 0.225])
    x = ((torch.from_numpy(img).permute(2, 0, 1).float() / 255.0) - mean.view(3, 1, 1)) / std.view(3, 1, 1)
    sm, pid = gdino_ref.text_masks_and_position_ids(list(IDS23))
    st = {}
    ref_logits, ref_boxes = gdino_ref.detector_forward(sd, oc, x[None], text, sm, pid, stages=st)
    est = {"force_topk": st["topk"]}
    logits, boxes = eng.forward([torch.from_numpy(img).to(dev)], stages=est)
    assert tuple(logits.shape) == (1, 300, 23) and tuple(boxes.shape) == (1, 300, 4)
    mx, l2 = _rel(est["memory"], st["memory"][0])
    print(f"encoder memory: max-rel {mx:.2e} l2-rel {l2:.2e}")
    assert mx < 3e-2 and l2 < 5e-3
    mx, l2 = _rel(est["memory_text"], st["memory_text"][0])
    print(f"memory_text: max-rel {mx:.2e} l2-rel {l2:.2e}")
    assert mx < 2e-2 and l2 < 5e-3
    assert tuple(est["topk_logits"].shape) == (1, eng.plan(224, 288, 1).S, 23)
    mine = est["topk_logits"].max(-1)[0][0].cpu()
    mx, _ = _rel(mine, st["topk_logits"][0])
    print(f"topk logits max-rel {mx:.2e}")
    got = set(torch.sort(mine, descending=True, stable=True)[1][:300].tolist())
    overlap = len(got & set(st["topk"][0].tolist())) / 300
    print("topk set overlap", overlap)
    assert overlap >= 0.97
    d = (boxes[0].cpu() - ref_boxes[0]).abs().max(-1)[0]
    dl = (logits[0].cpu() - ref_logits[0]).abs().max(-1)[0] / ref_logits.abs().max()
    pst = {"force_topk": st["topk"]}
    with gdino_ref.f16_operands():
        pl, pb = gdino_ref.detector_forward(sd, oc, x[None], text, sm, pid, stages=pst)
    eb = (pb[0] - ref_boxes[0]).abs().max(-1)[0]
    el = (pl[0] - ref_logits[0]).abs().max(-1)[0] / ref_logits.abs().max()
    fails = []
    for name, hip, emul in (("box", d, eb), ("logit", dl, el)):
        for qt in (0.5, 0.75, 0.9, 0.99, 1.0):
            hq, eq = hip.quantile(qt).item(), emul.quantile(qt).item()
            print(f"{name} err q{qt}: HIP {hq:.2e}  emulated-f16 oracle {eq:.2e}")
            if not hq <= 2.0 * eq + 1e-3:
                fails.append((name, qt, hq, eq))
    assert not fails, fails


def _predict_ref(logits, boxes, ids, box_threshold, text_threshold, remove_combined):
    """GD/util/inference.py:70-97 and get_phrases_from_posmap (GD/util/utils.py:599-610) in numpy on raw logits [nq, T]
    and boxes [nq, 4]; phrases as tuples of ids without "." (1012), the tokenizer-free form of decode().replace(".", "")."""
    prob = torch.from_numpy(logits).sigmoid().numpy()          # float32 sigmoid, as `.cpu().sigmoid()` of the reference
    keep = prob.max(1) > box_threshold
    sep_idx = [i for i, t in enumerate(ids) if t in (101, 102, 1012)]
    phrases = []
    for row in prob[keep]:
        posmap = row > text_threshold
        left, right = 0, 255
        if remove_combined:
            at = bisect.bisect_left(sep_idx, int(row.argmax()))
            right, left = sep_idx[at], sep_idx[at - 1]
        posmap[:left + 1] = False
        posmap[right:] = False
        phrases.append(tuple(ids[i] for i in np.nonzero(posmap)[0] if ids[i] != 1012))
    return np.nonzero(keep)[0], boxes[keep], prob[keep].max(1), phrases


@torch.no_grad()
@pytest.mark.parametrize("remove_combined", [False, True])
def test_predict_matches_reference_postprocess(dev, caption_dino, remove_combined):
    """With random weights every score saturates, so (as test_detect_threshold_path_matches_oracle_postprocess) the
    decoder's final LayerNorm is scaled by 0.05 and the box threshold is the median score; the text threshold is the
    median probability, so that phrases are proper subsets.  Same kept set, boxes, scores and phrase ids as the numpy
    restatement applied to the engine's own logits."""
    from inklayer_amd import gdino
    c = caption_dino
    sd = dict(c["sd"])
    for leaf in ("weight", "bias"):
        sd[f"transformer.decoder.norm.{leaf}"] = sd[f"transformer.decoder.norm.{leaf}"] * 0.05
    eng = gdino.GDinoEngine(sd, c["ec"], dev, encoded_text=c["text4"], token_ids=IDS4)
    eng.set_caption(IDS23, encoded_text=c["text23"])
    assert eng.T == 23 and eng.token_ids == IDS23
    dimg = torch.from_numpy(c["img"]).to(dev)
    logits, boxes = eng.forward([dimg], allow_graph=False)
    logits, boxes = logits[0].cpu().numpy(), boxes[0].cpu().numpy()
    prob = torch.from_numpy(logits).sigmoid()
    bt, tt = prob.max(1)[0].median().item(), prob.median().item()
    want_idx, want_boxes, want_scores, want_phrases = _predict_ref(logits, boxes, IDS23, bt, tt, remove_combined)
    (got_boxes, got_scores, got_phrases), = eng.predict([dimg], bt, tt, remove_combined=remove_combined)
    assert 100 <= len(want_idx) <= 200
    assert np.array_equal(got_boxes.numpy(), want_boxes) and np.array_equal(got_scores.numpy(), want_scores)
    assert got_phrases == want_phrases
    assert len(set(got_phrases)) > 1 and any(0 < len(p) < 18 for p in got_phrases)
    if remove_combined:      # a phrase never crosses a separator
        groups = [set(IDS23[1:7]), set(IDS23[8:16]), set(IDS23[17:21])]
        assert all(any(set(p) <= g for g in groups) for p in got_phrases)


@torch.no_grad()
def test_caption_switch_back_to_four_tokens_is_bitwise(dev, caption_dino):
    """After a 23-token caption, set_caption with 4 tokens gives the logits and boxes of a fresh 4-token engine bit for
    bit, eager and through the graph path: the caches are cleared and the T <= 4 path is untouched."""
    from inklayer_amd import gdino
    c = caption_dino
    dimg = torch.from_numpy(c["img"]).to(dev)
    fresh = gdino.GDinoEngine(c["sd"], c["ec"], dev, encoded_text=c["text4"], token_ids=IDS4)
    want = fresh.forward([dimg], allow_graph=False)
    eng = gdino.GDinoEngine(c["sd"], c["ec"], dev, encoded_text=c["text4"], token_ids=IDS4)
    for _ in range(3):                                   # the third call replays a captured graph of the 4-token caption
        eng.forward([dimg])
    eng.set_caption(IDS23, encoded_text=c["text23"])
    wide = eng.forward([dimg])
    assert tuple(wide[0].shape) == (1, 300, 23)
    eng.set_caption(IDS4, encoded_text=c["text4"])
    assert eng.T == 4 and eng.fold_fusion and eng._text_attn.__name__ == "attn_fewkeys"
    for _ in range(3):
        got = eng.forward([dimg])
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    eng.set_caption(IDS4)                                # served from the caption cache: no features, no checkpoint
    got = eng.forward([dimg], allow_graph=False)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])


@torch.no_grad()
def test_caption_graph_replay_and_batch2(dev, caption_dino):
    """The 23-token path (T % 4 != 0: ContrastiveEmbed's padded text rows, the -inf bias, the [:, :, :T] views) through a
    captured graph - first sight eager, second captures, third replays, new pixels in the static buffer - bit for bit
    the eager forward; and B = 2 against two B = 1 forwards within test_detector_batch2_and_detect_api's bounds."""
    eng = caption_dino["eng"]
    assert eng.T == 23 and eng.Tc == 24 and eng.logit_bias is not None
    rs = np.random.RandomState(21)
    imgs = [torch.from_numpy(rs.randint(0, 256, size=(224, 256, 3)).astype(np.uint8)).to(dev) for _ in range(3)]
    eager = [tuple(t.clone() for t in eng._forward_eager([im])) for im in imgs]
    eng._graphs.clear()
    eng._seen.clear()
    for im, (el, eb) in zip(imgs + imgs, eager + eager):
        gl, gb = eng.forward([im])
        assert tuple(gl.shape) == (1, 300, 23) and torch.equal(gl, el) and torch.equal(gb, eb)
    assert len(eng._graphs) == 1
    l2_, b2_ = eng.forward([imgs[0], imgs[1]])
    assert tuple(l2_.shape) == (2, 300, 23) and torch.isfinite(l2_).all()
    for i in range(2):
        assert (b2_[i] - eager[i][1][0]).abs().max().item() < 1e-5
        assert (l2_[i] - eager[i][0][0]).abs().max().item() < 1e-4
    (boxes, scores, phrases), (_, _, _) = eng.predict([imgs[0], imgs[1]], 0.5, 0.5)
    assert boxes.shape[1] == 4 and len(scores) == len(boxes) == len(phrases)


@torch.no_grad()
def test_plugin_predict_leaves_the_default_caption(dev, tmp_path, monkeypatch):
    """The shim's predict / run_gdino_on_sketch on the module's singleton (INKLAYER_RANDOM_WEIGHTS=1, Swin-T, the
    decoder's final LayerNorm scaled by 0.05 as test_plugin_runs_swin_b does): a caption of 9 token ids gives a label
    per box, and run_ft_dino_on_sketch returns the same dict before and after it - the engine is back on "object" with its
    4-token kernels.  An engine held on another caption gets that one back."""
    from PIL import Image
    import InkLayer.detector.gdino as DET
    from inklayer_amd import gdino, synthetic
    png = tmp_path / "sketch.png"
    Image.fromarray(synthetic.synthetic_sketch(3, 240, 320)).save(png)
    monkeypatch.setenv("INKLAYER_RANDOM_WEIGHTS", "1")
    monkeypatch.delenv("INKLAYER_GDINO_MODEL", raising=False)
    monkeypatch.delenv("INKLAYER_BERT_VOCAB", raising=False)
    monkeypatch.setattr(DET, "model", None)
    monkeypatch.setattr(DET, "_tokenizer", None)
    ids = (101, 2001, 2002, 1012, 3001, 1012, 4001, 1012, 102)
    try:
        eng = DET.get_model()
        eng.w["dec.norm.w"].mul_(0.05)
        eng.w["dec.norm.b"].mul_(0.05)
        before = DET.run_ft_dino_on_sketch(str(png))
        out = DET.run_gdino_on_sketch(str(png), ids, box_threshold=0.5, text_threshold=0.5)
        assert tuple(eng.token_ids) == tuple(gdino.DEFAULT_TOKEN_IDS) and eng.T == 4 and eng.fold_fusion
        after = DET.run_ft_dino_on_sketch(str(png))
        again = DET.run_gdino_on_sketch(str(png), ids, box_threshold=0.5, text_threshold=0.5)
        after2 = DET.run_ft_dino_on_sketch(str(png))
        boxes, scores, phrases = DET.predict(eng, np.asarray(Image.open(png).convert("RGB")), ids, 0.5, 0.5,
                                             remove_combined=True)
        eng.set_caption(ids)                              # a caller's own caption survives a predict with another one
        DET.predict(eng, str(png), gdino.DEFAULT_TOKEN_IDS, 0.5, 0.5)
        assert tuple(eng.token_ids) == ids
    finally:
        DET.model = None
        DET._tokenizer = None
        torch.cuda.empty_cache()
    assert before == after == after2 and len(before["bboxes"]) > 0 and before["labels"] == ["object"] * len(before["bboxes"])
    n = len(out["bboxes"])
    assert n > 0 and out == again and len(out["scores"]) == n and len(out["labels"]) == n
    vocab = wordpiece_available()
    if not vocab:                                         # without a vocabulary the labels are id tuples of the caption's words
        words = set(ids) - {101, 102, 1012}
        assert all(isinstance(p, tuple) and set(p) <= words | {102} for p in out["labels"])
        assert len(boxes) == len(scores) == len(phrases) and all(len(p) <= 2 for p in phrases)
    bx = np.asarray(out["bboxes"])
    assert bx.shape == (n, 4) and np.isfinite(bx).all() and (bx[:, 2] >= bx[:, 0]).all()


def wordpiece_available():
    from inklayer_amd import wordpiece
    return wordpiece.default_vocab_path() is not None
