"""Host side of closed-set detection, no GPU: character offsets of the WordPiece tokenizer on the toy vocabulary of
tests/test_caption_cpu.py (hand-worked), class lists -> caption and spans (against tests/closed_set_ref.py), positive maps
(hand-worked properties, the restatement, and tests/golden/gdino_classes_small.npz - the reference's own vl_utils
functions over HuggingFace's BertTokenizerFast on the same vocabulary, see make_gdino_classes_golden.py), the refusal of
a class list that does not fit, and the argument contracts of ink_class_scores / ink_select_boxes with fake pointers."""
import json
from pathlib import Path

import numpy as np
import pytest
import torch

import closed_set_ref as ref
from test_caption_cpu import TOY, _ids

GOLDEN = Path(__file__).resolve().parent / "golden" / "gdino_classes_small.npz"


@pytest.fixture(scope="module")
def tok(tmp_path_factory):
    from inklayer_amd.wordpiece import WordPiece
    p = tmp_path_factory.mktemp("vocab") / "vocab.txt"
    p.write_text("\n".join(TOY) + "\n", encoding="utf-8")
    return WordPiece(str(p))


# --------------------------------------------------------------------------------------------------------------- offsets
def test_offsets_multi_piece_word_and_punctuation(tok):
    #       0123456789012
    ids, off = tok.encode_with_offsets("teapots, cat.", preprocess=False)
    assert ids == _ids("[CLS]", "tea", "##pot", "##s", ",", "cat", ".", "[SEP]")
    assert off == [(0, 0), (0, 3), (3, 6), (6, 7), (7, 8), (9, 12), (12, 13), (0, 0)]


def test_offsets_accent_case_and_double_spaces(tok):
    #                       01234567890123
    ids, off = tok.encode_with_offsets("Café  DOG  cat", preprocess=False)       # "é" is one character: stripped to "e"
    assert ids == _ids("[CLS]", "cafe", "dog", "cat", "[SEP]")
    assert off == [(0, 0), (0, 4), (6, 9), (11, 14), (0, 0)]
    # the same word with a COMBINING accent (two characters for "é"): the span still covers the original characters
    ids, off = tok.encode_with_offsets("cafe\u0301 cat", preprocess=False)
    assert ids == _ids("[CLS]", "cafe", "cat", "[SEP]") and off == [(0, 0), (0, 4), (6, 9), (0, 0)]


def test_offsets_follow_preprocess_caption_and_unknown_words(tok):
    # preprocess_caption: lower, strip, a trailing "." - the offsets are positions in THAT string
    ids, off = tok.encode_with_offsets("  Zebra sitting ")
    assert ids == _ids("[CLS]", "[UNK]", "sit", "##ting", ".", "[SEP]")
    assert off == [(0, 0), (0, 5), (6, 9), (9, 13), (13, 14), (0, 0)]               # "zebra sitting."
    ids, off = tok.encode_with_offsets("猫cat don't", preprocess=False)
    assert ids == _ids("[CLS]", "猫", "cat", "don", "'", "t", "[SEP]")
    assert off == [(0, 0), (0, 1), (1, 4), (5, 8), (8, 9), (9, 10), (0, 0)]


@pytest.mark.parametrize("caption", ["Cat . Dog", "Teapots, Café", "don't  sit\tdown.", "a\x00b\u200dc 猫cat", "   ", "",
                                     "ΣΑΣ teapotx " + "a" * 101, "it's a dog!", "İs it"])
def test_encode_with_offsets_returns_encodes_ids(tok, caption):
    from inklayer_amd.wordpiece import basic_tokenize, basic_tokenize_with_offsets, preprocess_caption
    for pre in (True, False):
        ids, off = tok.encode_with_offsets(caption, preprocess=pre)
        assert ids == tok.encode(caption, preprocess=pre) and len(off) == len(ids)
        text = preprocess_caption(caption) if pre else caption
        assert [w for w, _ in basic_tokenize_with_offsets(text)] == basic_tokenize(text)
        assert off[0] == (0, 0) and off[-1] == (0, 0)
        inner = off[1:-1]
        assert all(0 <= s < e <= len(text) for s, e in inner)
        assert all(a[1] <= b[0] for a, b in zip(inner, inner[1:]))                  # in order, never overlapping


def test_char_to_token(tok):
    from inklayer_amd.wordpiece import char_to_token
    #                                   0123456789
    _, off = tok.encode_with_offsets("cat  dog.", preprocess=False)
    assert [char_to_token(off, i) for i in range(-1, 11)] == [None, 1, 1, 1, None, None, 2, 2, 2, 3, None, None]


# --------------------------------------------------------------------------------------------------- caption and spans
CLASS_LISTS = [["cat", "hot dog", "a"], ["Tea Pots", " dog ", "s"], ["cat", "", "  ", "dog"], ["cat/dog", "a"],
               ["dog", "dog"]]


@pytest.mark.parametrize("classes", CLASS_LISTS)
@pytest.mark.parametrize("lower", [True, False])
def test_caption_and_spans_match_the_restatement(classes, lower):
    from inklayer_amd.closed_set import build_captions_and_token_span
    cap, spans = build_captions_and_token_span(classes, lower)
    rcap, rspans = ref.build_captions_and_token_span(classes, lower)
    assert cap == rcap and [[list(s) for s in sp] for sp in spans] == rspans


def test_caption_and_spans_by_hand():
    from inklayer_amd.closed_set import build_captions_and_token_span
    #                                                       0123456789012345
    cap, spans = build_captions_and_token_span(["Cat", "hot dog", "a"])
    assert cap == "cat . hot dog . a ." and spans == [[(0, 3)], [(6, 9), (10, 13)], [(16, 17)]]
    assert [cap[s:e] for sp in spans for s, e in sp] == ["cat", "hot", "dog", "a"]
    assert build_captions_and_token_span(["Cat"], force_lowercase=False)[0] == "Cat ."
    # a name with "/" is taken as written (the reference draws a random alternative): the same caption every time
    assert {build_captions_and_token_span(["cat/dog"])[0] for _ in range(8)} == {"cat/dog ."}
    assert build_captions_and_token_span(["", "cat"]) == ("cat .", [[], [(0, 3)]])


# ------------------------------------------------------------------------------------------------------- positive maps
def test_positive_map_rows(tok):
    from inklayer_amd.closed_set import build_captions_and_token_span, positive_map_from_spans
    from inklayer_amd.wordpiece import char_to_token
    classes = ["teapots", "sitting cat", "a", "", "dog"]
    cap, spans = build_captions_and_token_span(classes)
    ids, off = tok.encode_with_offsets(cap, preprocess=False)
    assert ids == _ids("[CLS]", "tea", "##pot", "##s", ".", "sit", "##ting", "cat", ".", "a", ".", "dog", ".", "[SEP]")
    pm = positive_map_from_spans(off, spans)
    assert pm.dtype == torch.float32 and tuple(pm.shape) == (5, 256)
    want = [[1, 2, 3], [5, 6, 7], [9], [], [11]]
    for row, cols in zip(pm, want):
        assert torch.nonzero(row).flatten().tolist() == cols                        # exactly its words' tokens
        n = len(cols)
        assert row.sum().item() == pytest.approx(n / (n + 1e-6), abs=1e-6)
        if n:
            assert torch.equal(row[cols], torch.full((n,), 1.0) / (torch.tensor(float(n)) + 1e-6))
    assert torch.equal(pm, ref.create_positive_map_from_span(lambda i: char_to_token(off, i), spans))
    assert tuple(positive_map_from_spans(off, spans, max_text_len=32).shape) == (5, 32)


def test_positive_map_retries_and_whitespace(tok):
    from inklayer_amd.closed_set import positive_map_from_spans
    #                                   012345678901234567
    _, off = tok.encode_with_offsets("cat      dog . a", preprocess=False)          # cat 0-3, dog 9-12, "." 13, a 15
    pm = positive_map_from_spans(off, [[(0, 4)], [(8, 12)], [(7, 12)], [(4, 7)], [(0, 5)], [(0, 6)], [(6, 12)], [(0, 3), (15, 16)]])
    got = [torch.nonzero(r).flatten().tolist() for r in pm]
    assert got[0] == [1]            # ends on a blank: the character before it (end - 2)
    assert got[1] == [2]            # begins on a blank: beg + 1
    assert got[2] == [2]            # ... two blanks: beg + 2
    assert got[3] == [] and pm[3].sum().item() == 0.0           # blanks only: skipped, a zero row
    assert got[4] == [1]            # two blanks at the end: end - 3
    assert got[5] == []             # three: out of retries, skipped
    assert got[6] == []             # three blanks at the start: skipped
    assert got[7] == [1, 4]         # two spans, one row: [CLS] cat dog . a [SEP]
    assert pm[7, 1].item() == pytest.approx(0.5, abs=1e-6)


@pytest.mark.skipif(not GOLDEN.exists(), reason="golden file missing")
def test_maps_match_the_references_own_functions(tmp_path):
    """tests/golden/gdino_classes_small.npz: vl_utils.build_captions_and_token_span + create_positive_map_from_span over
    HuggingFace's BertTokenizerFast.  Caption, spans, ids, offsets and maps, exactly."""
    from inklayer_amd.closed_set import build_captions_and_token_span, class_prompt, positive_map_from_spans, span_prompt
    from inklayer_amd.wordpiece import WordPiece
    g = np.load(GOLDEN)
    vocab = tmp_path / "vocab.txt"
    vocab.write_text("\n".join(json.loads(str(g["vocab"]))) + "\n", encoding="utf-8")
    tok = WordPiece(str(vocab))
    seen = 0
    for name in g.files:
        if not name.startswith("classes_") or name.endswith("_map"):
            continue
        case = json.loads(str(g[name]))
        cap, spans = build_captions_and_token_span(case["classes"])
        assert cap == case["caption"] and [[list(s) for s in sp] for sp in spans] == case["spans"]
        ids, off = tok.encode_with_offsets(cap, preprocess=False)
        assert ids == case["ids"] and [list(o) for o in off] == case["offsets"]
        want = torch.from_numpy(g[name + "_map"])
        assert torch.equal(positive_map_from_spans(off, spans), want)
        prompt = class_prompt(tok, case["classes"])
        assert list(prompt.token_ids) == case["ids"] and torch.equal(prompt.positive_map, want)
        assert prompt.caption == cap and list(prompt.names) == case["classes"]
        seen += 1
    assert seen == 3
    case = json.loads(str(g["spans"]))
    ids, off = tok.encode_with_offsets(case["caption_in"])
    assert ids == case["ids"] and [list(o) for o in off] == case["offsets"]
    want = torch.from_numpy(g["spans_map"])
    assert torch.equal(positive_map_from_spans(off, case["spans"]), want)
    assert [torch.nonzero(r).flatten().tolist() for r in want] == [[1], [2, 3, 4], [], [2, 3, 4], [6, 9], [7, 8], [3]]
    prompt = span_prompt(tok, case["caption_in"], case["spans"])
    assert torch.equal(prompt.positive_map, want) and prompt.caption == case["caption"]
    assert prompt.names[4] == "café dog" and prompt.names[5] == "sitting"


# ----------------------------------------------------------------------------------------------------- too many classes
def test_class_list_longer_than_the_caption_limit(tok):
    from inklayer_amd.closed_set import class_prompt
    classes = ["cat", "teapots", "dog"] * 40          # 2 + 40 * (2 + 4 + 2) = 322 tokens
    with pytest.raises(ValueError, match=r"only the first 95 classes fit"):        # 2 + 31 * 8 + 2 + 4 = 256
        class_prompt(tok, classes)
    fits = class_prompt(tok, classes[:95])
    assert len(fits.token_ids) == 256 and tuple(fits.positive_map.shape) == (95, 256)
    assert torch.nonzero(fits.positive_map[94]).flatten().tolist() == [251, 252, 253]
    with pytest.raises(ValueError, match=r"only the first 3 classes fit"):
        class_prompt(tok, ["cat", "dog", "a", "teapots"], max_text_len=8)           # 2 + 2 + 2 + 2 = 8, then + 4
    with pytest.raises(ValueError):
        class_prompt(tok, [])


# -------------------------------------------------------------------------------------------------- argument contracts
def test_abi_version_is_unchanged():
    from inklayer_amd import _lib
    assert _lib.lib().ink_abi_version() == 10


def test_class_scores_argument_contract():
    """ink_class_scores returns 1 before any launch.  Fake non-null pointers: none of these calls may be accepted."""
    from inklayer_amd import _lib
    fn = _lib.lib().ink_class_scores
    p = 4096
    ok = dict(logits=p, ld=24, pm=p, pm_stride=0, n_cls=None, B=2, nq=9, T=23, C=5, out=p)

    def call(**kw):
        return fn(*{**ok, **kw}.values(), None)

    for ptr in ("logits", "pm", "out"):
        assert call(**{ptr: None}) == 1                  # null pointers
        assert call(**{ptr: p + 2}) == 1                 # 4-byte loads and stores
    assert call(n_cls=p + 2) == 1
    assert call(T=0) == 1 and call(T=257, ld=260) == 1 and call(C=0) == 1 and call(nq=0) == 1 and call(B=0) == 1
    assert call(ld=22) == 1                              # a row stride below T
    assert call(pm_stride=5 * 23 - 1) == 1               # per-image maps that overlap
    assert call(pm_stride=-1) == 1
    assert call(nq=1 << 20, C=1 << 12) == 1              # a (query, class) index past int32
    assert call(B=65536) == 1


def test_select_boxes_argument_contract():
    from inklayer_amd import _lib
    fn = _lib.lib().ink_select_boxes
    p = 4096
    ok = dict(idx=p, boxes=p, scale=p, B=2, K=30, nq=9, Cmax=5, out=p, labels=p, query=p)

    def call(**kw):
        return fn(*{**ok, **kw}.values(), None)

    for ptr in ("idx", "boxes", "scale", "out", "labels", "query"):
        assert call(**{ptr: None}) == 1
    assert call(boxes=p + 8) == 1 and call(out=p + 8) == 1          # 16-byte box loads and stores
    assert call(idx=p + 2) == 1 and call(labels=p + 2) == 1 and call(query=p + 2) == 1 and call(scale=p + 2) == 1
    assert call(B=0) == 1 and call(K=0) == 1 and call(nq=0) == 1 and call(Cmax=0) == 1
    assert call(nq=1 << 20, Cmax=1 << 12) == 1
    assert call(B=1 << 16, K=1 << 15) == 1


def test_engine_refuses_maps_of_another_caption():
    """GDinoEngine._positive_maps on a weightless engine: one map needs the shared form, a list one map per image, and a
    map that marks tokens beyond the caption is refused."""
    from inklayer_amd import gdino
    eng = gdino.GDinoEngine.text_state_only()
    eng.set_text(torch.zeros(6, 256), (101, 7, 1012, 8, 1012, 102))
    pm = torch.zeros(2, 256)
    pm[0, 1] = pm[1, 3] = 1.0
    m, n_cls, counts = eng._positive_maps(pm, 3)
    assert tuple(m.shape) == (2, 6) and n_cls is None and counts == [2, 2, 2]
    m, n_cls, counts = eng._positive_maps([pm, pm[:1], pm], 3)
    assert tuple(m.shape) == (3, 2, 6) and n_cls.tolist() == [2, 1, 2] and counts == [2, 1, 2]
    assert torch.equal(m[1, 1], torch.zeros(6)) and torch.equal(m[1, 0], pm[0, :6])
    bad = pm.clone()
    bad[1, 6] = 1.0
    with pytest.raises(ValueError, match="another caption"):
        eng._positive_maps(bad, 1)
    with pytest.raises(ValueError):
        eng._positive_maps([pm, pm], 3)
    with pytest.raises(ValueError):
        eng._positive_maps(pm[:, :4], 1)
    eng.set_captions([(101, 7, 1012, 102), (101, 7, 1012, 8, 1012, 102)], encoded_texts=[torch.zeros(4, 256), torch.zeros(6, 256)])
    with pytest.raises(ValueError, match="one map per image"):
        eng._positive_maps(pm, 2)
    m, n_cls, _ = eng._positive_maps([pm[:1], pm], 2)
    assert tuple(m.shape) == (2, 2, 6) and n_cls.tolist() == [1, 2]
    with pytest.raises(ValueError, match="another caption"):
        eng._positive_maps([pm[:1], bad], 2)            # image 1's caption has 6 tokens, the map marks token 6
