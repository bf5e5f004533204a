"""One caption per image in a batch, host side (no GPU): the oracle run alone with each caption against the REFERENCE's
padded batch (tests/golden/gdino_captions_small.npz, made by tests/golden/make_gdino_captions_golden.py from the
reference's own modules), GDinoEngine.set_captions' host state against the reference's masks, the dispatch between the
shared and the per-image form, and the argument refusals of the two new C entry points."""
import ctypes
from pathlib import Path

import numpy as np
import pytest
import torch

from test_oracle_gdino import SMALL, _close, _close_rows, _weights

GOLD = Path(__file__).parent / "golden" / "gdino_captions_small.npz"
IDS23 = (101, 2001, 2002, 2003, 2004, 2005, 2006, 1012, 3001, 3002, 3003, 3004, 3005, 3006, 3007, 3008, 1012,
         4001, 4002, 4003, 4004, 1012, 102)
IDS9 = (101, 2001, 2002, 1012, 3001, 1012, 4001, 1012, 102)
IDS4 = (101, 4874, 1012, 102)


def _golden_captions(g):
    return [tuple(int(t) for t in g["token_ids"][b][:g["t_len"][b]]) for b in range(2)]


def test_golden_is_the_padded_batch_of_the_issue():
    g = np.load(GOLD)
    assert _golden_captions(g) == [IDS23, IDS9] and (g["token_ids"][1][9:] == 0).all()
    assert np.array_equal(g["text_token_mask"], g["token_ids"] != 0)
    assert GOLD.stat().st_size < (Path(__file__).parent / "golden" / "gdino_small.npz").stat().st_size // 4


@torch.no_grad()
def test_masked_batch_is_each_image_alone():
    """The reference's padded batch of two captions gives, for each image, what the oracle gives for that image ALONE
    with its own unpadded caption: logits [:, :T_b], boxes and memory_text[:T_b], within test_oracle_gdino's tolerances
    for the same quantities; the reference's logits at t >= T_b are -inf.

    Both sides are float64 (the float32 weights, image and features widened; the golden stores float32 roundings of
    float64 results).  In float32 the comparison has a floor above the bound that has nothing to do with masks: the
    oracle itself moves by 1.5e-4 of the logits' range (90th percentile; 9e-3 at the worst row) between B = 1 and B = 2
    of the SAME caption, because torch's CPU kernels sum in another order and a few queries of these random weights are
    ill-conditioned (see _close_rows).  In float64 that movement is 1e-9, so the tolerances below hold the masked
    batch's arithmetic and nothing else."""
    from oracle import gdino_ref
    g = np.load(GOLD)
    small = np.load(Path(__file__).parent / "golden" / "gdino_small.npz")
    sd = {k: v.double() for k, v in _weights(int(g["seed"])).items()}
    img0 = torch.from_numpy(small["image"]).double()
    images = [img0, img0.flip(-1).contiguous()]
    assert bool(g["logits_past_longest_is_neginf"])
    for b, ids in enumerate(_golden_captions(g)):
        T = len(ids)
        sm, pid = gdino_ref.text_masks_and_position_ids(list(ids))
        st = {}
        text = torch.from_numpy(g["encoded_text"][b, :T]).double()
        logits, boxes = gdino_ref.detector_forward(sd, SMALL, images[b], text, sm, pid, stages=st)
        assert logits.dtype == torch.float64
        _close(st["memory_text"][0], g["memory_text"][b, :T], 5e-5)
        _close_rows(boxes[0], g["pred_boxes"][b], 5e-5, 2e-3)
        _close_rows(logits[0], g["pred_logits"][b, :, :T], 5e-5, 2e-3)
        assert np.isneginf(g["pred_logits"][b, :, T:]).all() and np.isfinite(g["pred_logits"][b, :, :T]).all()


def test_set_captions_host_state_matches_reference_masks():
    from inklayer_amd import gdino
    g = np.load(GOLD)
    caps = _golden_captions(g)
    eng = gdino.GDinoEngine.text_state_only()
    feats = [torch.from_numpy(g["encoded_text"][b, :len(c)]) for b, c in enumerate(caps)]
    eng.set_captions(caps, encoded_texts=feats)
    assert eng.captions == tuple(caps) and eng.T is None and eng.Tmax == 23 and eng.Tc == 24
    assert eng.t_len.dtype == torch.int32 and eng.t_len.tolist() == [23, 9] and eng.t_lens == (23, 9)
    assert eng.text_blocked.dtype == torch.uint8 and tuple(eng.text_blocked.shape) == (2, 23, 23)
    assert np.array_equal(~eng.text_blocked.bool().numpy(), g["self_mask"])
    assert np.array_equal(eng.text_position_ids.numpy(), g["position_ids"])
    dim_t = 10000.0 ** (2 * torch.div(torch.arange(256, dtype=torch.float32), 2, rounding_mode="floor") / 256)
    want_pos = gdino._interleaved_sincos(torch.from_numpy(g["position_ids"]).reshape(-1).float()[:, None]
                                         * (2 * np.pi) / dim_t)
    assert tuple(eng.pos_text.shape) == (46, 256) and torch.equal(eng.pos_text, want_pos)
    assert tuple(eng.logit_bias.shape) == (2, 24)
    want_bias = np.zeros((2, 24), np.float32)
    want_bias[0, 23:], want_bias[1, 9:] = -np.inf, -np.inf
    assert np.array_equal(eng.logit_bias.numpy(), want_bias)
    text0 = eng.text0.view(2, 23, 256)
    assert torch.equal(text0[0], feats[0]) and torch.equal(text0[1, :9], feats[1]) and (text0[1, 9:] == 0).all()


def test_dispatch_between_the_shared_and_the_per_image_form():
    from inklayer_amd import gdino
    eng = gdino.GDinoEngine.text_state_only()
    f4, f9, f23 = torch.randn(4, 256), torch.randn(9, 256), torch.randn(23, 256)
    eng.set_captions([IDS4, list(IDS4)], encoded_texts=[f4, None])          # equal captions: the shared form
    assert eng.T == 4 and eng.token_ids == IDS4 and eng.captions is None and eng.t_len is None and eng.Tmax is None
    assert eng.fold_fusion and eng._text_attn.__name__ == "attn_fewkeys" and tuple(eng.text_blocked.shape) == (4, 4)
    assert torch.equal(eng.text0, f4)
    eng._graphs.put("stale", object())
    eng.set_captions([IDS23, IDS9, IDS4], encoded_texts=[f23, f9, None])    # IDS4 from the caption cache
    assert eng.captions == (IDS23, IDS9, IDS4) and eng.T is None and eng.token_ids is None and len(eng._graphs) == 0
    assert eng.t_lens == (23, 9, 4) and torch.equal(eng.text0.view(3, 23, 256)[2, :4], f4)
    with pytest.raises(ValueError):
        eng.forward([torch.zeros(8, 8, 3, dtype=torch.uint8)] * 2)          # three captions, two images
    with pytest.raises(ValueError):
        eng.forward([])
    eng.set_caption(IDS9)                                                   # back to the shared form, from the cache
    assert eng.T == 9 and eng.captions is None and eng.t_len is None and eng.t_lens is None and eng.Tmax is None
    assert eng.text_position_ids is None and tuple(eng.text_blocked.shape) == (9, 9) and eng.logit_bias.shape == (12,)
    eng.set_captions([IDS23, IDS9])
    eng.set_text(f4, IDS4)
    assert eng.T == 4 and eng.captions is None
    # a caption over 256 ids is truncated, as set_text does
    long_ids = [101] + [2000 + i if i % 7 else 1012 for i in range(1, 299)] + [102]
    eng.set_captions([long_ids, IDS9], encoded_texts=[torch.randn(300, 256), None])
    assert eng.Tmax == 256 and eng.Tc == 256 and eng.t_lens == (256, 9) and eng.captions[0] == tuple(long_ids[:256])
    assert tuple(eng.text0.shape) == (512, 256) and tuple(eng.text_blocked.shape) == (2, 256, 256)
    m, _ = gdino.text_masks_and_position_ids(long_ids[:256])
    assert torch.equal(eng.text_blocked[0].bool(), ~m)
    with pytest.raises(ValueError):
        eng.set_captions([])
    with pytest.raises(ValueError):
        eng.set_captions([IDS9, (101, 5, 102)])                             # neither features nor a checkpoint


def test_biattn_wide_varlen_argument_contract():
    """ink_biattn_wide_varlen returns 1 before any launch.  Fake non-null pointers: none of these calls may be accepted."""
    from inklayer_amd import _lib
    l = _lib.lib()
    p = 4096
    args = dict(QV=p, KL=p, B=2, S=100, Tmax=23, t_len=p, E=1024, scale=0.0625, ws=p, ov=p, ol=p)
    call = lambda **kw: l.ink_biattn_wide_varlen(*{**args, **kw}.values(), None)
    assert call(Tmax=0) == 1 and call(Tmax=257) == 1 and call(Tmax=-1) == 1
    assert call(E=512) == 1 and call(S=0) == 1 and call(S=32769) == 1 and call(B=0) == 1 and call(B=65536) == 1
    assert call(t_len=None) == 1 and call(t_len=p + 2) == 1
    for name in ("QV", "KL", "ws", "ov", "ol"):
        assert call(**{name: None}) == 1, name
        assert call(**{name: p + 8}) == 1, name                # 16-byte fragment loads and stores


def test_attn_midkeys_varlen_argument_contract():
    from inklayer_amd import _lib
    l = _lib.lib()
    p = 4096
    args = dict(Q=p, ldq=256, K=p, ldk=256, V=p, ldv=256, B=2, nq=7, nk=40, nh=8, hd=32, scale=0.25, blocked=p,
                bstride=280, k_len=p, O=p, ldo=256)
    call = lambda **kw: l.ink_attn_midkeys_varlen(*{**args, **kw}.values(), None)
    assert call(nk=257) == 1 and call(nk=0) == 1 and call(nq=0) == 1 and call(B=0) == 1 and call(nh=0) == 1
    assert call(hd=16) == 1 and call(hd=48) == 1 and call(hd=128) == 1
    assert call(ldq=12) == 1 and call(ldk=260) == 1 and call(ldv=4) == 1 and call(ldo=257) == 1
    assert call(bstride=-1) == 1 and call(blocked=None) == 1   # a stride without a matrix
    assert call(k_len=p + 2) == 1
    for name in ("Q", "K", "V", "O"):
        assert call(**{name: None}) == 1, name
        assert call(**{name: p + 8}) == 1, name


def test_abi_stays_10_and_exports_both_symbols():
    from inklayer_amd import _lib
    l = _lib.lib()
    assert l.ink_abi_version() == 10
    raw = ctypes.CDLL(l._name)
    assert hasattr(raw, "ink_biattn_wide_varlen") and hasattr(raw, "ink_attn_midkeys_varlen")
    header = (Path(__file__).parents[1] / "include" / "inklayer_hip.h").read_text()
    assert "int ink_biattn_wide_varlen(" in header and "int ink_attn_midkeys_varlen(" in header
