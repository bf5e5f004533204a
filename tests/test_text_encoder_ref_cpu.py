"""Host side of the GPU text encoder (inklayer_amd/text_encoder.py, csrc/text_bert.hip): the float64 reference of its
GPU tests against the f32 statement that tests/test_text_branch_cpu.py pins to HuggingFace, the argument contracts of the
two new entry points, and the engine's choice between the GPU encoder and the host fold.  No GPU."""
import pytest
import torch

import text_encoder_ref as R


def test_float64_reference_matches_bert_encode():
    """The two captions of tests/test_text_branch_cpu.py on a 2-layer model, within that test's 5e-6.  Their ids reach
    4937, so this one model has a vocabulary of 5120 rows; every other random BERT of these tests has 2048."""
    from inklayer_amd import text_branch, weights_init
    sd = weights_init.random_bert_state_dict(n_layers=2, vocab_size=5120, seed=0)
    assert R.n_layers(sd) == 2
    for ids in R.BRANCH_CAPTIONS:
        ref = R.hidden64(sd, ids)
        got = text_branch.bert_encode(sd, ids)
        err = (got.double() - ref).abs().max().item()
        print(f"T={len(ids)}: bert_encode (f32) vs float64 max abs diff {err:.3g}")
        assert got.shape == ref.shape == (len(ids), 768) and err < 5e-6
        feat = text_branch.encode_caption_from_checkpoint(sd, ids)
        assert (feat.double() - R.encode64(sd, ids)).abs().max().item() < 5e-6
        # the block mask matters to the reference too
        if len(ids) > 4:
            plain = R.embed64(sd, ids)
            for i in range(2):
                plain = R.layer64(sd, i, plain, torch.ones(len(ids), len(ids), dtype=torch.bool))
            assert (plain - ref).abs().max().item() > 1e-3


def test_random_bert_state_dict_is_seeded_and_shaped():
    from inklayer_amd import weights_init
    a = weights_init.random_bert_state_dict(n_layers=1, vocab_size=2048, seed=3)
    b = weights_init.random_bert_state_dict(n_layers=1, vocab_size=2048, seed=3)
    assert a.keys() == b.keys() and all(torch.equal(a[k], b[k]) for k in a)
    assert a["bert.embeddings.word_embeddings.weight"].shape == (2048, 768)
    assert a["bert.encoder.layer.0.intermediate.dense.weight"].shape == (3072, 768) and a["feat_map.weight"].shape == (256, 768)
    assert (a["bert.encoder.layer.0.output.LayerNorm.weight"] - 1).abs().max() > 0.1          # perturbed, as _hf does
    assert a["bert.encoder.layer.0.output.LayerNorm.bias"].abs().max() > 0.05


def test_reference_captions_are_what_they_claim():
    for ids in (R.IDS4, R.IDS9, R.IDS23, R.IDS256, R.IDS1):
        assert max(ids) < 2048 and ids[0] == 101
    assert (len(R.IDS23), len(R.IDS256)) == (23, 256) and R.IDS256[-1] == 102
    allowed, pos = R.masks_and_pos(R.IDS256)
    assert allowed.diagonal().all() and not allowed[:64, 192:].any() and int(pos.max()) < 8    # block-diagonal: tiles to skip


def test_abi_version_and_symbols():
    from inklayer_amd import _lib
    l = _lib.lib()
    assert l.ink_abi_version() == 10
    assert "ink_text_embed_ln" in _lib.SIGNATURES and "ink_attn_text_f32" in _lib.SIGNATURES
    assert l.ink_text_embed_ln and l.ink_attn_text_f32


def test_text_embed_ln_argument_contract():
    from inklayer_amd import _lib
    l = _lib.lib()
    p = 4096
    args = dict(ids=p, pos_ids=p, R=5, word=p, V=64, pos=p, P=16, type_row=p, gamma=p, beta=p, eps=1e-12, C=768, out=p,
                split=p)
    call = lambda **kw: l.ink_text_embed_ln(*{**args, **kw}.values(), None)
    assert call(R=0) == 1 and call(V=0) == 1 and call(P=0) == 1
    assert call(C=0) == 1 and call(C=770) == 1 and call(C=2052) == 1
    for name in ("ids", "pos_ids", "word", "pos", "type_row", "gamma", "beta", "out", "split"):
        assert call(**{name: None}) == 1, name
        assert call(**{name: p + 2}) == 1, name
    for name in ("word", "pos", "type_row", "gamma", "beta", "out", "split"):
        assert call(**{name: p + 8}) == 1, name


def test_attn_text_f32_argument_contract():
    from inklayer_amd import _lib
    l = _lib.lib()
    p = 4096
    args = dict(Q=p, ldq=2304, K=p, ldk=2304, V=p, ldv=2304, row_start=p, B=2, R=30, Tmax=23, nh=12, hd=64, scale=0.125,
                blocked=p, bstride=23 * 23, out=p, ldo=2304, out32=None, ldf=0)
    call = lambda **kw: l.ink_attn_text_f32(*{**args, **kw}.values(), None)
    assert call(Tmax=257) == 1 and call(Tmax=0) == 1 and call(B=0) == 1 and call(B=65536) == 1 and call(R=0) == 1
    assert call(nh=0) == 1 and call(hd=32) == 1 and call(hd=16) == 1 and call(hd=128) == 1
    assert call(ldq=2306) == 1 and call(ldk=2305) == 1 and call(ldv=766) == 1 and call(ldq=764) == 1
    assert call(ldo=2308) == 1 and call(ldo=2296) == 1                 # f16 rows: multiples of 8, and three segments fit
    assert call(out32=p, ldf=770) == 1 and call(out32=p, ldf=764) == 1
    assert call(bstride=-1) == 1 and call(blocked=None, bstride=529) == 1
    for name in ("Q", "K", "V", "row_start", "out"):
        assert call(**{name: None}) == 1, name
        assert call(**{name: p + 2}) == 1, name
    for name in ("Q", "K", "V", "out"):
        assert call(**{name: p + 8}) == 1, name
    assert call(out32=p + 8, ldf=768) == 1


def test_auto_on_a_cpu_engine_is_the_host_fold(monkeypatch):
    """A text_state_only engine under "auto" - the engine of every CPU test of caption handling - folds on the host,
    even with a 768-wide BERT in text_weights; "host" does the same; the missing captions of a batch are folded once
    each."""
    from inklayer_amd import gdino, text_branch, text_encoder
    calls = []

    def fake(sd, ids):
        calls.append(tuple(ids))
        return torch.full((len(ids), 256), float(len(ids)))

    monkeypatch.setattr(text_branch, "encode_caption_from_checkpoint", fake)
    monkeypatch.setattr(text_encoder.BertTextEncoder, "__init__", lambda *a, **k: pytest.fail("GPU encoder built"))
    sd = {"bert.embeddings.word_embeddings.weight": torch.zeros(8, 768), "feat_map.bias": torch.zeros(256)}
    for mode in ("auto", "host"):
        calls.clear()
        eng = gdino.GDinoEngine.text_state_only()
        assert gdino.GDinoEngine.text_encoder == "auto"
        eng.text_encoder = mode
        eng.set_captions([R.IDS9, R.IDS4, R.IDS9], sd=sd)
        assert calls == [R.IDS9, R.IDS4]
        assert eng.text0.shape == (27, 256) and eng.text0[0, 0] == 9 and eng.text0[9, 0] == 4 and eng.text0[13:18].abs().max() == 0
        eng.set_caption(R.IDS4)
        assert len(calls) == 2 and eng._text_enc is None
        eng.release_text_encoder()


def test_gpu_on_a_cpu_engine_is_an_error(monkeypatch):
    from inklayer_amd import gdino, text_branch
    monkeypatch.setattr(text_branch, "encode_caption_from_checkpoint", lambda sd, ids: torch.zeros(len(ids), 256))
    eng = gdino.GDinoEngine.text_state_only()
    eng.text_encoder = "gpu"
    with pytest.raises(ValueError, match="GPU"):
        eng.set_caption(R.IDS4, sd={"feat_map.bias": torch.zeros(256)})
    with pytest.raises(ValueError, match="GPU"):
        eng.set_captions([R.IDS4, R.IDS9])
    eng.text_encoder = "cpu"
    with pytest.raises(ValueError, match="text_encoder"):
        eng.set_caption(R.IDS4)
    with pytest.raises(ValueError):
        from inklayer_amd.text_encoder import BertTextEncoder
        BertTextEncoder({}, "cpu")
