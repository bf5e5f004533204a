"""Host side of free-text captions, no GPU: the WordPiece tokenizer on a toy vocabulary (hand-worked expectations -
parity with HuggingFace is unpinned offline, see inklayer_amd/wordpiece.py), the caption's masks and position ids
against the oracle, phrase extraction at the separator boundaries, truncation at 256 tokens, and the argument refusals
of the two new C entry points."""
import ctypes

import pytest
import torch

TOY = ["[PAD]", "[UNK]", "[CLS]", "[SEP]", ".", ",", "'", "?", "!", "cat", "dog", "tea", "##pot", "##s", "cafe", "a",
       "s", "don", "t", "n't", "is", "it", "'s", "sit", "##ting", "猫"]


@pytest.fixture(scope="module")
def tok(tmp_path_factory):
    from inklayer_amd.wordpiece import WordPiece
    p = tmp_path_factory.mktemp("vocab") / "vocab.txt"
    p.write_text("\n".join(TOY) + "\n", encoding="utf-8")
    return WordPiece(str(p))


def _ids(*tokens):
    return [TOY.index(t) for t in tokens]


def test_preprocess_caption():
    from inklayer_amd.wordpiece import preprocess_caption
    assert preprocess_caption("  Cat . Dog ") == "cat . dog."
    assert preprocess_caption("cat.") == "cat."


def test_basic_tokenize():
    from inklayer_amd.wordpiece import basic_tokenize
    assert basic_tokenize("Café, TEApots!") == ["cafe", ",", "teapots", "!"]           # lower, NFD accent strip, punctuation
    assert basic_tokenize("don't  sit\tdown.") == ["don", "'", "t", "sit", "down", "."]
    assert basic_tokenize("a\x00b\u200dc 猫cat") == ["abc", "猫", "cat"]                 # control chars go, CJK stands alone
    assert basic_tokenize("   ") == []


def test_encode_pieces_unknowns_and_trailing_dot(tok):
    assert tok.encode("Cat . Dog") == _ids("[CLS]", "cat", ".", "dog", ".", "[SEP]")   # the trailing "." is added
    assert tok.encode("cat . dog .") == _ids("[CLS]", "cat", ".", "dog", ".", "[SEP]")  # ... once
    assert tok.encode("Teapots, Café") == _ids("[CLS]", "tea", "##pot", "##s", ",", "cafe", ".", "[SEP]")
    assert tok.tokenize("teapotx") == ["[UNK]"]              # a piece without a match makes the WORD unknown
    assert tok.tokenize("zebra cat") == ["[UNK]", "cat"]
    assert tok.tokenize("a" * 101) == ["[UNK]"] and tok.tokenize("sitting") == ["sit", "##ting"]
    assert tok.encode("猫cat", preprocess=False) == _ids("[CLS]", "猫", "cat", "[SEP]")
    assert tok("dog") == tok.encode("dog")


def test_decode_cleanup(tok):
    assert tok.decode(_ids("tea", "##pot", "##s", ",", "cat", ".")) == "teapots, cat."
    assert tok.decode(_ids("it", "'s", "a", "dog", "!")) == "it's a dog!"
    assert tok.decode(_ids("don", "'", "t", "sit", "?")) == "don't sit?"
    assert tok.decode(_ids("is", "n't", "it")) == "isn't it"
    assert tok.decode([]) == ""


def test_missing_vocabulary_is_an_error(tmp_path, monkeypatch):
    from inklayer_amd import wordpiece
    monkeypatch.delenv("INKLAYER_BERT_VOCAB", raising=False)
    if wordpiece.default_vocab_path() is None:
        with pytest.raises(FileNotFoundError):
            wordpiece.WordPiece()
    bad = tmp_path / "v.txt"
    bad.write_text("cat\ndog\n")
    with pytest.raises(ValueError):
        wordpiece.WordPiece(str(bad))
    good = tmp_path / "vocab.txt"
    good.write_text("\n".join(TOY) + "\n", encoding="utf-8")
    monkeypatch.setenv("INKLAYER_BERT_VOCAB", str(good))
    assert wordpiece.default_vocab_path() is not None


# ---------------------------------------------------------------------------------------------------------------
IDS = (101, 2001, 2002, 1012, 3001, 1012, 4001, 4002, 4003, 1012, 102)
#       0     1     2     3     4     5     6     7     8     9    10


def test_masks_and_position_ids_match_oracle():
    from oracle import gdino_ref
    from inklayer_amd import gdino
    for ids in (IDS, gdino.DEFAULT_TOKEN_IDS, IDS[:-1], (101, 7, 1029, 8, 9, 1012, 102)):
        m, p = gdino.text_masks_and_position_ids(list(ids))
        rm, rp = gdino_ref.text_masks_and_position_ids(list(ids))
        assert torch.equal(m, rm.bool().reshape(m.shape)) and torch.equal(p, rp.long().reshape(p.shape)), ids
    m, p = gdino.text_masks_and_position_ids(list(IDS))
    assert m[1, 3] and m[3, 1] and not m[1, 4] and not m[0, 1] and m[6:10, 6:10].all() and not m[9, 10]
    assert p.tolist() == [0, 0, 1, 2, 0, 1, 0, 1, 2, 3, 0]


def test_phrases_at_the_separator_boundaries():
    from inklayer_amd import gdino
    T = len(IDS)
    probs = torch.zeros(6, T)
    probs[0, [1, 2, 4]] = torch.tensor([0.9, 0.5, 0.3])        # strongest token in phrase 1, phrase 2 above the threshold
    probs[1, [4, 1]] = torch.tensor([0.8, 0.4])                # strongest token is phrase 2's only word
    probs[2, [3, 2, 6]] = torch.tensor([0.9, 0.5, 0.4])        # strongest token IS a separator: the phrase before it
    probs[3, [0, 7]] = torch.tensor([0.9, 0.5])                # strongest token is [CLS]: right = 0, left wraps to [SEP]
    probs[4, [10, 8]] = torch.tensor([0.9, 0.5])               # strongest token is [SEP]: nothing lies between the last "." and it
    probs[5, [9, 6, 8, 1]] = torch.tensor([0.9, 0.2, 0.6, 0.6])
    plain = gdino.phrases_from_probs(probs, IDS, 0.25)
    # position 0 is always cut; a [SEP] above the threshold stays, as in the reference (right_idx = 255)
    assert plain == [(2001, 2002, 3001), (2001, 3001), (2002, 4001), (4002,), (4003, 102), (2001, 4003)]
    comb = gdino.phrases_from_probs(probs, IDS, 0.25, remove_combined=True)
    assert comb == [(2001, 2002), (3001,), (2002,), (), (), (4003,)]
    assert gdino.phrases_from_probs(probs[:0], IDS, 0.25) == []
    # a caption cut before its [SEP]: the strongest token lies past the last separator
    cut = IDS[:9]
    pc = torch.zeros(1, 9)
    pc[0, [7, 6, 1]] = torch.tensor([0.9, 0.5, 0.5])
    assert gdino.phrases_from_probs(pc, cut, 0.25, remove_combined=True) == [(4001, 4002)]
    # posmap indices, as get_phrases_from_posmap's left_idx / right_idx
    assert gdino.phrase_token_ids([True] * T, IDS) == list(IDS[1:])
    assert gdino.phrase_token_ids([True] * T, IDS, 3, 5) == [3001]

    class Decoder:
        def decode(self, ids):
            return " ".join(str(i) for i in ids) + " ."

    assert gdino.phrases_from_probs(probs[:1], IDS, 0.25, tokenizer=Decoder()) == ["2001 2002 3001 "]


def test_set_text_truncates_at_256_tokens():
    from inklayer_amd import gdino
    eng = gdino.GDinoEngine.text_state_only()
    ids = [101] + [2000 + i if i % 7 else 1012 for i in range(1, 299)] + [102]
    assert len(ids) == 300
    eng._graphs.put("stale", object())
    eng.set_caption(ids, encoded_text=torch.randn(300, 256))
    assert eng.T == 256 and eng.token_ids == tuple(ids[:256]) and len(eng._graphs) == 0
    assert tuple(eng.text0.shape) == (256, 256) and tuple(eng.text_blocked.shape) == (256, 256)
    assert tuple(eng.pos_text.shape) == (256, 256)
    assert eng._text_attn.__name__ == "attn_midkeys"
    m, _ = gdino.text_masks_and_position_ids(ids[:256])
    assert torch.equal(eng.text_blocked.bool(), ~m)
    eng.set_caption(ids[:17], encoded_text=torch.randn(17, 256))
    assert eng.T == 17 and eng._text_attn.__name__ == "attn_midkeys"
    eng.set_caption(ids[:16], encoded_text=torch.randn(16, 256))
    assert eng.T == 16 and eng._text_attn.__name__ == "attn_fewkeys"
    eng.set_caption(ids[:5], encoded_text=torch.randn(5, 256))
    assert eng.T == 5 and eng._text_attn.__name__ == "attn_fewkeys"
    eng.set_caption(gdino.DEFAULT_TOKEN_IDS, encoded_text=torch.randn(4, 256))
    assert eng.T == 4 and eng.fold_fusion and eng._text_attn.__name__ == "attn_fewkeys"
    eng.set_caption(ids)                                       # the cache serves the truncated caption
    assert eng.T == 256
    with pytest.raises(ValueError):
        eng.set_caption([101, 5, 102])                         # neither features nor a checkpoint
    with pytest.raises(ValueError):
        eng.set_text(None, [101, 102])


# ---------------------------------------------------------------------------------------------------------------
def test_biattn_wide_argument_contract():
    """ink_biattn_wide / ink_biattn_wide_workspace return 1 before any launch.  Fake non-null pointers: none of these
    calls may be accepted."""
    from inklayer_amd import _lib
    l = _lib.lib()
    p = 4096
    args = dict(QV=p, KL=p, B=1, S=100, T=5, E=1024, scale=0.0625, ws=p, ov=p, ol=p)
    call = lambda **kw: l.ink_biattn_wide(*{**args, **kw}.values(), None)
    assert call(T=0) == 1 and call(T=257) == 1 and call(T=-1) == 1
    assert call(E=512) == 1 and call(E=2048) == 1
    assert call(S=0) == 1 and call(S=-5) == 1 and call(S=32769) == 1 and call(B=0) == 1
    for name in ("QV", "KL", "ws", "ov", "ol"):
        assert call(**{name: None}) == 1, name
        assert call(**{name: p + 8}) == 1, name                # 16-byte fragment loads and stores
    need = ctypes.c_int64(-1)
    assert l.ink_biattn_wide_workspace(1, 100, 0, ctypes.byref(need)) == 1
    assert l.ink_biattn_wide_workspace(1, 100, 257, ctypes.byref(need)) == 1
    assert l.ink_biattn_wide_workspace(1, 0, 5, ctypes.byref(need)) == 1
    assert l.ink_biattn_wide_workspace(65536, 100, 5, ctypes.byref(need)) == 1 and call(B=65536) == 1
    assert l.ink_biattn_wide_workspace(0, 100, 5, ctypes.byref(need)) == 1
    assert l.ink_biattn_wide_workspace(1, 100, 5, None) == 1 and need.value == -1
    # the header's formula: B * 4 * (128 Tp + ceil(S / 128) Tp + 258 ceil(S / 1024) Tp) floats, Tp = 32 ceil(T / 32)
    for B, S, T in ((1, 100, 5), (2, 13294, 256), (3, 1025, 33)):
        assert l.ink_biattn_wide_workspace(B, S, T, ctypes.byref(need)) == 0
        Tp = -(-T // 32) * 32
        assert need.value == B * 4 * Tp * (128 + -(-S // 128) + 258 * -(-S // 1024)), (B, S, T)


def test_attn_midkeys_argument_contract():
    from inklayer_amd import _lib
    l = _lib.lib()
    p = 4096
    args = dict(Q=p, ldq=256, K=p, ldk=256, V=p, ldv=256, B=1, nq=7, nk=40, nh=8, hd=32, scale=0.25, blocked=None, O=p,
                ldo=256)
    call = lambda **kw: l.ink_attn_midkeys(*{**args, **kw}.values(), None)
    assert call(nk=257) == 1 and call(nk=0) == 1 and call(nq=0) == 1 and call(B=0) == 1 and call(nh=0) == 1
    assert call(hd=16) == 1 and call(hd=48) == 1 and call(hd=128) == 1
    assert call(ldq=12) == 1 and call(ldk=260) == 1 and call(ldv=4) == 1 and call(ldo=257) == 1
    for name in ("Q", "K", "V", "O"):
        assert call(**{name: None}) == 1, name
        assert call(**{name: p + 8}) == 1, name


def test_caption_cache_belongs_to_one_checkpoint(monkeypatch):
    """Cached features are served per token ids; a new state dict drops them, so that no caption keeps the features
    another checkpoint's BERT gave it.  encode_caption_from_checkpoint is replaced by a stand-in that marks its source."""
    from inklayer_amd import gdino, text_branch
    calls = []

    def fake(sd, ids):
        calls.append(tuple(ids))
        return torch.full((len(ids), 256), float(sd["feat_map.bias"][0]))

    monkeypatch.setattr(text_branch, "encode_caption_from_checkpoint", fake)
    eng = gdino.GDinoEngine.text_state_only()
    a, b = {"feat_map.bias": torch.tensor([1.0]), "other": torch.zeros(1)}, {"module.feat_map.bias": torch.tensor([2.0])}
    eng.set_caption(IDS, sd=a)
    assert eng.text0[0, 0] == 1.0 and set(eng.text_weights) == {"feat_map.bias"}
    eng.set_caption(gdino.DEFAULT_TOKEN_IDS)
    eng.set_caption(IDS)                                       # cached: BERT is not folded again
    assert calls == [IDS, gdino.DEFAULT_TOKEN_IDS] and eng.text0[0, 0] == 1.0
    eng.set_caption(IDS, sd=b)
    assert eng.text0[0, 0] == 2.0 and calls[-1] == IDS and len(calls) == 3
    eng.set_text(torch.zeros(4, 256), gdino.DEFAULT_TOKEN_IDS)  # set_text leaves its caption in the cache too
    eng.set_caption(IDS)
    eng.set_caption(gdino.DEFAULT_TOKEN_IDS)
    assert eng.text0.abs().max() == 0 and len(calls) == 3
