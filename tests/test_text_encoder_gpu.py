"""inklayer_amd.text_encoder.BertTextEncoder (BERT + feat_map for a batch of captions on the library's kernels) against
the float64 statement of tests/text_encoder_ref.py.  GPU box only.

Yardstick, computed in each test: e_host, the largest error of the host f32 path (text_branch.bert_encode /
encode_caption_from_checkpoint, the path the encoder replaces) against the same float64 result.  The encoder runs every
product on split-f16 operands, whose documented grade is 2^-21 relative against f32's 2^-24, so it
must stay within 8 e_host, with a floor of 8 x 2^-24 |ref|max for the batches where the host happens to land closer
than its own rounding unit allows to rely on.  Both errors are printed."""
import pytest
import torch

import text_encoder_ref as R

pytestmark = pytest.mark.gpu

BATCHES = {"one4": [R.IDS4], "mixed": [R.IDS9, R.IDS23, R.IDS4], "long256": [R.IDS256], "one_token": [R.IDS1]}
_HOST = {}


@pytest.fixture(scope="module")
def sd2():
    from inklayer_amd import weights_init
    return weights_init.random_bert_state_dict(n_layers=2, vocab_size=2048, seed=1)


@pytest.fixture(scope="module")
def enc2(dev, sd2):
    from inklayer_amd.text_encoder import BertTextEncoder
    enc = BertTextEncoder(sd2, dev)
    assert (enc.n_layers, enc.vocab_size, enc.max_positions, enc.intermediate_size) == (2, 2048, 512, 3072)
    assert enc.launches_per_pass == 18
    return enc


def _yardsticks(sd, ids, tag):
    """float64 hidden / features of one caption and the host f32 path's errors against them, once per caption."""
    key = (tag, tuple(ids))
    if key not in _HOST:
        from inklayer_amd import text_branch
        h64 = R.hidden64(sd, ids)
        f64 = R.encode64(sd, ids, h64)
        eh = (text_branch.bert_encode(sd, ids).double() - h64).abs().max().item()
        ef = (text_branch.encode_caption_from_checkpoint(sd, ids).double() - f64).abs().max().item()
        _HOST[key] = (h64, f64, eh, ef)
    return _HOST[key]


def _bound(e_host, ref):
    return max(8.0 * e_host, 8.0 * 2.0 ** -24 * ref.abs().max().item())


def _check(enc, sd, batch, tag):
    ys = [_yardsticks(sd, ids, tag) for ids in batch]
    lens = [len(i) for i in batch]
    hid = enc.hidden(batch)
    feats = enc.encode(batch)
    assert hid.shape == (sum(lens), 768) and hid.dtype == torch.float32 and hid.is_cuda
    assert [tuple(f.shape) for f in feats] == [(n, 256) for n in lens]
    h64, f64 = torch.cat([y[0] for y in ys]), torch.cat([y[1] for y in ys])
    e_host_h, e_host_f = max(y[2] for y in ys), max(y[3] for y in ys)
    e_h = (hid.cpu().double() - h64).abs().max().item()
    e_f = (torch.cat(feats).cpu().double() - f64).abs().max().item()
    print(f"{tag} T={lens}: hidden |ref|max {h64.abs().max().item():.3g} host f32 {e_host_h:.3g} gpu {e_h:.3g} "
          f"(bound {_bound(e_host_h, h64):.3g}); features |ref|max {f64.abs().max().item():.3g} host f32 {e_host_f:.3g} "
          f"gpu {e_f:.3g} (bound {_bound(e_host_f, f64):.3g})")
    assert e_h <= _bound(e_host_h, h64) and e_f <= _bound(e_host_f, f64)
    return feats


@torch.no_grad()
@pytest.mark.parametrize("name", list(BATCHES))
def test_encoder_matches_float64(enc2, sd2, name):
    _check(enc2, sd2, BATCHES[name], "2-layer " + name)


@torch.no_grad()
def test_caption_in_a_batch_is_bitwise_the_caption_alone(enc2):
    a, b, c = R.IDS9, R.IDS23, R.IDS4
    batch, alone = enc2.encode([a, b, c]), enc2.encode([b])
    assert torch.equal(batch[1], alone[0])
    assert torch.equal(enc2.encode([c, b])[1], alone[0])
    hb, ha = enc2.hidden([a, b, c]), enc2.hidden([b])
    assert torch.equal(hb[len(a):len(a) + len(b)], ha)


@torch.no_grad()
def test_encode_into_fills_the_padded_rows(enc2, dev):
    batch = [R.IDS9, R.IDS23, R.IDS4]
    Tmax = 24                                              # one row more than the longest caption: all three are padded
    feats = enc2.encode(batch)
    out = torch.zeros(len(batch) * Tmax, 256, device=dev)
    assert enc2.encode_into(batch, out, Tmax) is out
    out = out.view(len(batch), Tmax, 256)
    for b, ids in enumerate(batch):
        assert torch.equal(out[b, :len(ids)], feats[b])
        assert (out[b, len(ids):] == 0).all()


def test_encoder_refuses_what_it_cannot_serve(enc2, sd2, dev):
    from inklayer_amd.text_encoder import BertTextEncoder
    with pytest.raises(ValueError):
        enc2.encode([[101, 2048, 102]])                    # id past the vocabulary
    with pytest.raises(ValueError):
        enc2.encode([])
    with pytest.raises(ValueError):
        enc2.encode([list(R.IDS256) + [102]])              # 257 tokens
    narrow = {k: (v[:, :512] if k == "bert.embeddings.word_embeddings.weight" else v) for k, v in sd2.items()}
    with pytest.raises(ValueError):
        BertTextEncoder(narrow, dev)
    assert 2 * 7.0e6 * 6 < enc2.nbytes < 2 * 9.0e6 * 6 + 3.0e7       # two layers of 7.1 M weights at three f16 each, + tables


@torch.no_grad()
def test_twelve_layers_compound_within_the_bound(dev):
    """BERT-base's depth on one T = 23 caption: the same bound holds through 12 layers."""
    from inklayer_amd import weights_init
    from inklayer_amd.text_encoder import BertTextEncoder
    sd = weights_init.random_bert_state_dict(n_layers=12, vocab_size=2048, seed=2)
    enc = BertTextEncoder(sd, dev)
    assert enc.n_layers == 12 and enc.launches_per_pass == 98
    print(f"12-layer encoder, vocabulary 2048: {enc.nbytes / 2 ** 20:.0f} MiB on the device")
    _check(enc, sd, [R.IDS23], "12-layer")
