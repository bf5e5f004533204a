"""The detector engine on the GPU text encoder (GDinoEngine.text_encoder, inklayer_amd/text_encoder.py): a batch of
fresh captions is encoded in one pass without the host fold, deduplicated and cached as before; "host" stays the
earlier path bit for bit.  GPU box only.

Setup: the small detector of the neighbouring tests (2 + 2 layers, 300 queries, seeded random weights), a 2-layer random
BERT with a random feat_map as the checkpoint's text tensors.  The features of every caption are folded on the host
FIRST (text_branch.encode_caption_from_checkpoint, with the float64 result next to them); then that function is
replaced by one that raises, so anything below that passes did not go through it."""
import numpy as np
import pytest
import torch

import text_encoder_ref as R

pytestmark = pytest.mark.gpu

CAPS = (R.IDS9, R.IDS23, R.IDS4)
FRESH = R.caption_ids(12, first=700)


@pytest.fixture(scope="module")
def setup(dev):
    from inklayer_amd import gdino, text_branch, weights_init
    cfg = gdino.GDinoConfig(enc_layers=2, dec_layers=2, num_queries=300)
    sd = weights_init.random_gdino_state_dict(cfg, dev, seed=5)
    sd.update(weights_init.random_bert_state_dict(n_layers=2, vocab_size=2048, seed=4))
    host, f64 = {}, {}
    for ids in CAPS + (FRESH,):
        host[ids] = text_branch.encode_caption_from_checkpoint(sd, ids)
        f64[ids] = R.encode64(sd, ids)
    return dict(cfg=cfg, sd=sd, host=host, f64=f64)


def _engine(setup, dev):
    from inklayer_amd import gdino
    return gdino.GDinoEngine(setup["sd"], setup["cfg"], dev, encoded_text=setup["host"][R.IDS4], token_ids=R.IDS4)


def _count_encodes(monkeypatch):
    from inklayer_amd.text_encoder import BertTextEncoder
    calls, real = [], BertTextEncoder.encode

    def counting(self, id_lists):
        calls.append([tuple(i) for i in id_lists])
        return real(self, id_lists)

    monkeypatch.setattr(BertTextEncoder, "encode", counting)
    return calls


def _no_host_fold(monkeypatch):
    from inklayer_amd import text_branch

    def refuse(sd, ids):
        raise AssertionError("the host fold was called")

    monkeypatch.setattr(text_branch, "encode_caption_from_checkpoint", refuse)


def _padded(feats, caps):
    Tmax = max(len(c) for c in caps)
    out = torch.zeros(len(caps), Tmax, 256, dtype=feats[caps[0]].dtype)
    for b, c in enumerate(caps):
        out[b, :len(c)] = feats[c]
    return out


@torch.no_grad()
def test_batch_of_fresh_captions_on_the_gpu_encoder(dev, setup, monkeypatch):
    eng = _engine(setup, dev)
    assert eng.text_encoder == "auto" and eng._text_enc is None
    calls = _count_encodes(monkeypatch)
    _no_host_fold(monkeypatch)
    eng.set_captions(CAPS, sd=setup["sd"])
    assert calls == [list(CAPS)] and eng._text_enc is not None            # one pass (the new sd emptied the cache)
    assert set(eng.text_weights) == {k for k in setup["sd"] if k.startswith(("bert.", "feat_map."))}
    # text0 against the host-folded padded features, by the encoder tests' yardstick (8 x the host's own error against
    # float64, floor 8 x 2^-24 |ref|max); the pad rows exactly zero
    got = eng.text0.cpu().view(3, 23, 256)
    ref64, host = _padded(setup["f64"], CAPS), _padded(setup["host"], CAPS)
    e_host = (host.double() - ref64).abs().max().item()
    e_gpu = (got.double() - ref64).abs().max().item()
    bound = max(8 * e_host, 8 * 2.0 ** -24 * ref64.abs().max().item())
    print(f"text0: host f32 {e_host:.3g}, gpu {e_gpu:.3g} against float64 (bound {bound:.3g}); "
          f"gpu - host {(got - host).abs().max().item():.3g}")
    assert e_gpu <= bound and (got - host).abs().max().item() <= bound + e_host
    for b, c in enumerate(CAPS):
        assert (got[b, len(c):] == 0).all()
    # a forward on two images
    eng.set_captions([R.IDS9, R.IDS23])
    assert len(calls) == 1                                             # both cached now: nothing encoded
    rs = np.random.RandomState(7)
    imgs = [torch.from_numpy(rs.randint(0, 256, size=(256, 320, 3)).astype(np.uint8)).to(dev) for _ in range(2)]
    logits, boxes = eng.forward(imgs)
    assert logits.shape[:2] == (2, 300) and boxes.shape == (2, 300, 4) and torch.isfinite(boxes).all()
    for b, T in enumerate((9, 23)):
        assert torch.isfinite(logits[b, :, :T]).all()
    # repeating the first call encodes nothing
    eng.set_captions(CAPS)
    assert len(calls) == 1
    # two equal captions in a batch of fresh ones: each distinct caption once
    a, b2 = R.caption_ids(7, first=900), R.caption_ids(15, first=1000)
    eng.set_captions([a, b2, a, R.IDS4])
    assert calls[1:] == [[a, b2]]
    assert torch.equal(eng.text0.view(4, 15, 256)[0], eng.text0.view(4, 15, 256)[2])
    # set_caption with a fresh caption encodes exactly that one
    eng.set_caption(FRESH)
    assert calls[2:] == [[FRESH]] and eng.T == 12
    assert (eng.text0.cpu().double() - setup["f64"][FRESH]).abs().max().item() <= bound


@torch.no_grad()
def test_host_mode_is_the_host_fold_bit_for_bit(dev, setup, monkeypatch):
    eng = _engine(setup, dev)
    eng.text_encoder = "host"
    calls = _count_encodes(monkeypatch)
    eng.set_captions(CAPS, sd=setup["sd"])
    assert not calls and eng._text_enc is None
    assert torch.equal(eng.text0.cpu().view(3, 23, 256), _padded(setup["host"], CAPS))
    eng.set_caption(FRESH)
    assert torch.equal(eng.text0.cpu(), setup["host"][FRESH]) and not calls


@torch.no_grad()
def test_new_state_dict_drops_cache_and_encoder(dev, setup, monkeypatch):
    from inklayer_amd import weights_init
    eng = _engine(setup, dev)
    calls = _count_encodes(monkeypatch)
    _no_host_fold(monkeypatch)
    eng.set_caption(R.IDS9, sd=setup["sd"])
    first, enc = eng.text0.clone(), eng._text_enc
    assert calls == [[R.IDS9]] and enc is not None
    eng.release_text_encoder()
    assert eng._text_enc is None
    eng.set_caption(R.IDS9)                                            # cached: no encoder is built for it
    assert len(calls) == 1 and eng._text_enc is None
    other = weights_init.random_bert_state_dict(n_layers=2, vocab_size=2048, seed=9)
    eng.set_caption(R.IDS23)
    assert len(calls) == 2 and eng._text_enc is not None
    built = eng._text_enc
    eng.set_caption(R.IDS9, sd=other)                                  # a new checkpoint: cache and encoder go
    assert calls[2:] == [[R.IDS9]] and eng._text_enc is not None and eng._text_enc is not built
    assert not torch.equal(eng.text0, first)
    eng.set_caption(R.IDS23)
    assert calls[3:] == [[R.IDS23]]                                    # the other checkpoint's features were dropped
