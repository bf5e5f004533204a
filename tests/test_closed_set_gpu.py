"""Closed-set detection at the engine and plugin level: GDinoEngine.predict_classes (shared caption, eager and graph
replay; one class list per image) and predict_spans against tests/closed_set_ref.py applied to the engine's OWN forward
logits and boxes, then the plugin functions and the runner's `classes` on random weights.  GPU box only.

Fixture: test_gdino_caption_gpu.caption_dino (seeded weights 77, 2 + 2 layers, 300 queries, a 224 x 288 image, the 23
token ids IDS23), with the decoder's final LayerNorm scaled by 0.05 so that the scores spread out instead of saturating
(tests/test_runner_gpu.py does the same); this module's instance of the fixture is its own.

Comparing a float32 selection with a float64 one: the k-th best score of one is within the scores' bound of the k-th
best of the other whatever the order of near-ties, so SCORES are compared position by position; labels and boxes are
compared at the positions whose float64 score is further than twice the bound from both neighbours ("isolated": there
the order cannot differ), and most positions must be isolated.  The bound is the one of tests/test_closed_set_ops_gpu.py
(four times the error of the reference's own float32 arithmetic on the same logits, at least 2^-22)."""
import json

import numpy as np
import pytest
import torch

import closed_set_ref as ref
from test_caption_cpu import TOY
from test_gdino_caption_gpu import IDS4, IDS23, caption_dino  # noqa: F401

pytestmark = pytest.mark.gpu
FLOOR = 2.0 ** -22
IDS9 = (101, 2001, 2002, 1012, 3001, 1012, 4001, 1012, 102)


def rows_map(rows, width=256):
    """A normalised positive map [len(rows), width] from lists of token positions."""
    pm = torch.zeros(len(rows), width)
    for c, cols in enumerate(rows):
        pm[c, cols] = 1.0
    return pm / (pm.sum(-1)[:, None] + 1e-6)


#  IDS23: [CLS] 1-6 . 8-15 . 17-20 . [SEP]
MAP23 = rows_map([[1, 2], [3, 4, 5, 6], [8, 9, 10, 11, 12, 13, 14, 15], [17], [18, 19, 20]])
MAP9 = rows_map([[1, 2], [4]])                   # IDS9: [CLS] 1 2 . 4 . 6 . [SEP]
MAP4 = rows_map([[1]])                           # IDS4: [CLS] 1 . [SEP]


def bound(logits, pm):
    f64 = ref.class_scores_f64(logits, pm)
    own = (ref.class_scores_f32(logits, pm).double() - f64).abs().max().item()
    return max(4.0 * own, FLOOR)


def check_against_post_process(got, logits_b, boxes_b, pm, size, num_select, what):
    """One image's (boxes, scores, labels) of predict_classes against PostProcessCocoGrounding on logits_b [nq, T] and
    boxes_b [nq, 4] (CPU), see the module docstring."""
    boxes, scores, labels = got
    h, w = size
    want = ref.post_process(logits_b[None], boxes_b[None], pm, torch.tensor([[float(h), float(w)]]), num_select)[0]
    k = min(num_select, logits_b.shape[0] * pm.shape[0])
    assert tuple(boxes.shape) == (k, 4) and tuple(scores.shape) == (k,) and tuple(labels.shape) == (k,)
    assert boxes.dtype == torch.float32 and scores.dtype == torch.float32 and labels.dtype == torch.int64
    tol = bound(logits_b, pm)
    assert (scores[:-1] >= scores[1:]).all()
    err = (scores.double() - want["scores"]).abs().max().item()
    ws = want["scores"]
    gap = torch.full((k,), float("inf"), dtype=torch.float64)
    gap[1:] = torch.minimum(gap[1:], ws[:-1] - ws[1:])
    gap[:-1] = torch.minimum(gap[:-1], ws[:-1] - ws[1:])
    iso = gap > 2 * tol
    if k == num_select:                               # the next pair outside the selection is a neighbour too
        allp = ref.class_scores_f64(logits_b, pm).flatten().sort(descending=True)[0]
        iso[-1] &= bool(allp[k - 1] - allp[k] > 2 * tol)
    print(f"{what}: scores within {err:.3e} (bound {tol:.3e}), {int(iso.sum())} of {k} positions isolated")
    assert err <= tol and iso.sum().item() >= 0.9 * k
    assert torch.equal(labels[iso], want["labels"][iso])
    assert (boxes[iso].double() - want["boxes"][iso]).abs().max().item() <= max(h, w, 1) * 2.0 ** -22


@pytest.fixture(scope="module")
def eng(caption_dino):
    e = caption_dino["eng"]
    e.w["dec.norm.w"].mul_(0.05)
    e.w["dec.norm.b"].mul_(0.05)
    e._graphs.clear()
    return e


@torch.no_grad()
def test_predict_classes_shared_form_eager_and_graph(dev, caption_dino, eng):
    img = torch.from_numpy(caption_dino["img"]).to(dev)
    eng.set_caption(IDS23, encoded_text=caption_dino["text23"])
    logits, boxes = eng.forward([img], allow_graph=False)
    assert tuple(logits.shape) == (1, 300, 23) and logits.stride(1) == 24        # rows of the 24-column GEMM output
    lg, bx = logits[0].cpu().contiguous(), boxes[0].cpu()
    graphs = []
    for call in range(3):                             # eager, capture, replay (GDinoEngine._forward_graphed)
        got = eng.predict_classes([img], MAP23, num_select=300, sizes=[(224, 288)])[0]
        graphs.append(len(eng._graphs))
        check_against_post_process(got, lg, bx, MAP23[:, :23], (224, 288), 300, f"call {call}")
    assert graphs == [0, 1, 1]
    # normalised boxes without sizes; fewer pairs than num_select; a map cut to the caption's width
    got = eng.predict_classes([img], MAP23[:, :23].contiguous(), num_select=2000)[0]
    check_against_post_process(got, lg, bx, MAP23[:, :23], (1, 1), 2000, "normalised, all 1500 pairs")
    assert got[0].shape[0] == 1500
    got = eng.predict_classes([img], MAP23[:1], num_select=7)[0]
    check_against_post_process(got, lg, bx, MAP23[:1, :23], (1, 1), 7, "one class, 7 pairs")
    with pytest.raises(ValueError):
        eng.predict_classes([img], rows_map([[1], [23]]))            # token 23 is not in this caption
    with pytest.raises(ValueError):
        eng.predict_classes([img], MAP23, sizes=[(1, 1), (2, 2)])


@torch.no_grad()
def test_predict_classes_per_image_form(dev, caption_dino, eng):
    """Three images, three captions, three class lists: every image's result is PostProcessCocoGrounding on its own
    columns of the batch's logits, and bit for bit what the scoring tail gives for that image alone."""
    from inklayer_amd import ops
    rs = np.random.RandomState(41)
    imgs = [torch.from_numpy(caption_dino["img"]).to(dev)] + \
           [torch.from_numpy(rs.randint(0, 256, size=(224, 288, 3)).astype(np.uint8)).to(dev) for _ in range(2)]
    texts = [caption_dino["text23"], torch.from_numpy((0.5 * rs.standard_normal((9, 256))).astype(np.float32)),
             caption_dino["text4"]]
    caps, maps, sizes = (IDS23, IDS9, IDS4), [MAP23, MAP9, MAP4], [(224, 288), (448, 576), (100, 50)]
    eng.set_captions(caps, encoded_texts=texts)
    try:
        assert eng.captions is not None and eng.Tmax == 23
        logits, boxes = eng.forward(imgs)
        res = eng.predict_classes(imgs, maps, num_select=120, sizes=sizes)
        with pytest.raises(ValueError):
            eng.predict_classes(imgs, MAP23)                            # one map for three captions
        with pytest.raises(ValueError):
            eng.predict_classes(imgs, [MAP23, MAP23, MAP4])             # image 1's caption has 9 tokens
        assert len(res) == 3
        for b, (ids, pm, size) in enumerate(zip(caps, maps, sizes)):
            T = len(ids)
            assert torch.isinf(logits[b, :, T:]).all() and torch.isfinite(logits[b, :, :T]).all()
            lg, bx = logits[b, :, :T].cpu().contiguous(), boxes[b].cpu()
            check_against_post_process(res[b], lg, bx, pm[:, :T], size, 120, f"image {b}")
            # the tail on this image alone, in the shared form
            C = pm.shape[0]
            k = min(120, 300 * C)
            prob = ops.class_scores(logits[b:b + 1, :, :T].contiguous(), pm[:, :T].contiguous().to(dev))
            idx, val = ops.topk_rowmax(prob.view(1, 300 * C, 1), k, want_values=True)
            scale = torch.tensor([[float(size[1]), float(size[0])]], device=dev)
            xyxy, labels, _ = ops.select_boxes(idx, boxes[b:b + 1].contiguous(), scale, C)
            assert torch.equal(res[b][1], val[0].cpu()) and torch.equal(res[b][2], labels[0].cpu().long())
            assert torch.equal(res[b][0], xyxy[0].cpu())
    finally:
        eng.set_caption(IDS23, encoded_text=caption_dino["text23"])


@torch.no_grad()
def test_predict_spans_matches_the_given_phrase_mode(dev, caption_dino, eng):
    img = torch.from_numpy(caption_dino["img"]).to(dev)
    eng.set_caption(IDS23, encoded_text=caption_dino["text23"])
    logits, boxes = eng.forward([img], allow_graph=False)
    lg, bx = logits[0].cpu().contiguous(), boxes[0].cpu()
    pm = MAP23[:, :23]
    tol = bound(lg, pm)
    f64 = ref.class_scores_f64(lg, pm)                                   # [nq, P]
    thr = float(f64.flatten().median())
    got_boxes, got_scores, got_phrase = eng.predict_spans([img], MAP23, thr)[0]
    want_boxes, want_scores, want_phrase = ref.phrase_filter(lg, bx, pm, thr)
    assert got_phrase.dtype == torch.int64 and (got_phrase[:-1] <= got_phrase[1:]).all()     # phrase order
    n_sure = 0
    for p in range(pm.shape[0]):
        sure_in = torch.nonzero(f64[:, p] > thr + tol).flatten().tolist()
        sure_out = set(torch.nonzero(f64[:, p] < thr - tol).flatten().tolist())
        mine = got_phrase == p
        # the queries of this phrase, identified by their box (copied unchanged from the forward): in query order
        q = [int(torch.nonzero((bx == b_).all(-1))[0]) for b_ in got_boxes[mine]]
        assert q == sorted(q) and set(sure_in) <= set(q) and not (set(q) & sure_out), p
        assert (got_scores[mine].double() - f64[q, p]).abs().max().item() <= tol
        n_sure += len(sure_in)
    assert 0.3 * f64.numel() < n_sure <= len(got_boxes) and abs(len(got_boxes) - len(want_boxes)) <= 0.01 * f64.numel()
    print(f"predict_spans: {len(got_boxes)} (phrase, query) pairs above {thr:.4f}, the restatement keeps {len(want_boxes)}")
    none = eng.predict_spans([img], MAP23, 2.0)[0]
    assert tuple(none[0].shape) == (0, 4) and none[1].numel() == 0 and none[2].numel() == 0


@torch.no_grad()
def test_plugin_functions_and_runner_classes(dev, tmp_path, monkeypatch):
    """The four plugin functions on the module's singleton (INKLAYER_RANDOM_WEIGHTS=1, toy vocabulary), each leaving
    the engine on the caption it came with - run_ft_dino_on_sketch answers as before -, and
    run_inklayer_pipeline(..., classes=[...]) writing class names into bboxes.json."""
    from PIL import Image
    import InkLayer.detector.gdino as DET
    import InkLayer.refinement.depth_sort as DS
    import InkLayer.runner as R
    import InkLayer.segmentor.sam as SEG
    from inklayer_amd import closed_set, gdino, synthetic
    pngs = []
    for i in range(2):
        pngs.append(tmp_path / f"sketch{i}.png")
        Image.fromarray(synthetic.synthetic_sketch(3 + i, 240, 320)).save(pngs[-1])
    vocab = tmp_path / "vocab.txt"
    vocab.write_text("\n".join(TOY) + "\n", encoding="utf-8")
    monkeypatch.setenv("INKLAYER_RANDOM_WEIGHTS", "1")
    monkeypatch.setenv("INKLAYER_SAM_MODEL", "vit_b")                  # the smallest models: the runner's wiring is the subject
    monkeypatch.delenv("INKLAYER_GDINO_MODEL", raising=False)
    monkeypatch.setattr(DS, "encoder", "vits")
    monkeypatch.setattr(DET, "model", None)
    from inklayer_amd.wordpiece import WordPiece
    monkeypatch.setattr(DET, "_tokenizer", WordPiece(str(vocab)))      # the toy vocabulary, whatever models/ holds
    monkeypatch.setattr(SEG, "_engine", None)
    monkeypatch.setattr(DS, "_engine", None)
    nouns = ["cat", "tea pots", "Dog"]

    def on_default():
        return tuple(eng.token_ids) == tuple(gdino.DEFAULT_TOKEN_IDS) and eng.T == 4 and eng.captions is None

    try:
        eng = DET.get_model()
        eng.w["dec.norm.w"].mul_(0.05)
        eng.w["dec.norm.b"].mul_(0.05)
        before = DET.run_ft_dino_on_sketch(str(pngs[0]))
        # run_gdino_on_sketch_classes: the dict of gdino_mmdetection.py:83-98
        out = DET.run_gdino_on_sketch_classes(str(pngs[0]), nouns, score_threshold=0.0)
        assert on_default() and sorted(out) == ["bboxes", "labels", "scores"]
        assert len(out["bboxes"]) == len(out["labels"]) == len(out["scores"]) == 300
        assert set(out["labels"]) <= set(nouns) and all(len(b) == 4 for b in out["bboxes"])
        assert all(a >= b for a, b in zip(out["scores"], out["scores"][1:]))
        assert all(b[0] <= b[2] and b[1] <= b[3] and -0.5 < b[0] and b[3] < 1.5 for b in out["bboxes"])     # normalised xyxy
        thr = out["scores"][150]
        cut = DET.run_gdino_on_sketch_classes(str(pngs[0]), nouns, score_threshold=thr)
        n = sum(s >= thr for s in out["scores"])
        assert 150 < n < 300 or out["scores"][-1] >= thr
        assert cut == {k: v[:n] for k, v in out.items()} and min(cut["scores"]) >= thr and on_default()
        after = DET.run_ft_dino_on_sketch(str(pngs[0]))
        # predict_classes: pixel boxes of the original image, labels index the class list
        boxes, scores, labels = DET.predict_classes(eng, str(pngs[0]), nouns, num_select=40)
        assert on_default() and tuple(boxes.shape) == (40, 4) and labels.dtype == torch.int64 and int(labels.max()) < 3
        assert torch.equal(scores, torch.tensor(out["scores"][:40]))
        assert [nouns[i] for i in labels.tolist()] == out["labels"][:40]
        want_px = torch.tensor(out["bboxes"][:40], dtype=torch.float64) * torch.tensor([320.0, 240.0, 320.0, 240.0], dtype=torch.float64)
        assert (boxes.double() - want_px).abs().max().item() <= 320 * 2.0 ** -22
        # a ready ClassPrompt needs no vocabulary and gives the same answer
        prompt = closed_set.class_prompt(DET.get_tokenizer(), nouns)
        again = DET.predict_classes(eng, np.asarray(Image.open(pngs[0]).convert("RGB")), prompt, num_select=40)
        assert all(torch.equal(a, b) for a, b in zip(again, (boxes, scores, labels)))
        # predict_classes_batch: one class list per image, in the per-image form, stateless
        res = DET.predict_classes_batch(eng, [str(p) for p in pngs], [nouns, ["a", "sitting cat"]], num_select=40)
        assert on_default() and len(res) == 2
        for (b_, s_, l_), n_cls in zip(res, (3, 2)):
            assert tuple(b_.shape) == (40, 4) and (s_[:-1] >= s_[1:]).all() and 0 <= int(l_.min()) and int(l_.max()) < n_cls
            assert float(s_.min()) >= 0.0                                # no pair of a class the image does not have
        with pytest.raises(ValueError):
            DET.predict_classes_batch(eng, [str(pngs[0])], [nouns, nouns])
        with pytest.raises(ValueError, match="classes fit"):
            DET.predict_classes(eng, str(pngs[0]), ["teapots"] * 80)
        assert on_default()
        # predict_spans: the given-phrase mode; spans are positions in the preprocessed caption "cat . tea pots . dog."
        sb, ss, sp = DET.predict_spans(eng, str(pngs[0]), "Cat . tea pots . Dog", [[(0, 3)], [(6, 9), (10, 14)], [(17, 20)]], 0.0)
        nq = eng.cfg.num_queries
        assert on_default() and tuple(sb.shape) == (3 * nq, 4) and tuple(ss.shape) == (3 * nq,)
        assert sp == ["cat"] * nq + ["tea pots"] * nq + ["dog"] * nq
        after2 = DET.run_ft_dino_on_sketch(str(pngs[0]))
        # the runner with classes: the detector leg is run_gdino_on_sketch_classes (here cut to its 3 best boxes, to keep
        # the segmentor's share of this test small), and bboxes.json carries the class names
        real = DET.run_gdino_on_sketch_classes
        seen = {}

        def best3(sketch_path, nouns_, *a, **k):
            full = real(sketch_path, nouns_, *a, **k)
            seen["nouns"], seen["out"] = list(nouns_), {key: v[:3] for key, v in full.items()}
            return seen["out"]

        monkeypatch.setattr(DET, "run_gdino_on_sketch_classes", best3)
        out_dir = R.run_inklayer_pipeline(str(pngs[1]), str(tmp_path / "out"), classes=nouns)
        saved = json.loads((tmp_path / "out" / "sketch1" / "bboxes.json").read_text())
        assert out_dir == str(tmp_path / "out" / "sketch1") and seen["nouns"] == nouns
        assert saved["labels"] == seen["out"]["labels"] and len(saved["labels"]) == 3 and set(saved["labels"]) <= set(nouns)
        assert saved["scores"] == seen["out"]["scores"] and len(saved["bboxes"]) == 3
        assert (tmp_path / "out" / "sketch1" / "bboxes.png").exists() and on_default()
    finally:
        DET.model = None
        SEG._engine = None
        DS._engine = None
        torch.cuda.empty_cache()
    assert before == after == after2 and len(before["bboxes"]) > 0
