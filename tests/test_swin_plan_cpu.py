"""The host-built tables of the Swin-T window attention, checked on the CPU: the plan's window maps (pad, cyclic shift,
window partition) and SW-MSA masks against gdino_ref's construction and an independent statement of the mask, the
dense relative-position bias against gdino_ref.swin_rel_index, and ink_flash_attn's bias_mode 3 argument checks.
No GPU."""
import ctypes
import functools
from types import SimpleNamespace

import pytest
import torch
import torch.nn.functional as Fn

WS, SHIFT = 7, 3
SCALE = 32 ** -0.5
SIZES = [(800, 800), (800, 1066), (800, 1333), (300, 412), (100, 412)]


@functools.lru_cache(maxsize=None)
def _plan(h, w, B):
    """GDinoEngine.plan(h, w, B) built on the CPU (as in test_detector_ops_gpu._plan)."""
    from inklayer_amd import gdino
    eng = SimpleNamespace(cfg=gdino.GDinoConfig(), dev=torch.device("cpu"), level_embed_cpu=torch.zeros(4, 256))
    return gdino._Plan(eng, h, w, B)


def _padded(H, W):
    return -(-H // WS) * WS, -(-W // WS) * WS


@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("hw", SIZES)
def test_win_map_is_pad_roll_partition_of_the_token_index(hw, B):
    """win_map[i][shifted] equals gdino_ref.swin_block's pad / roll(-3, -3) / window partition applied to the token
    index image b*H*W + y*W + x (-1 in the padding), exactly."""
    pl = _plan(*hw, B)
    for i, (H, W) in enumerate(pl.stage_hw):
        Hp, Wp = _padded(H, W)
        idx = torch.arange(B * H * W, dtype=torch.float64).view(B, H, W, 1)
        idx = Fn.pad(idx, (0, 0, 0, Wp - W, 0, Hp - H), value=-1)
        for shifted in (0, 1):
            y = torch.roll(idx, shifts=(-SHIFT, -SHIFT), dims=(1, 2)) if shifted else idx
            win = y.view(B, Hp // WS, WS, Wp // WS, WS, 1).permute(0, 1, 3, 2, 4, 5).reshape(-1)
            got = pl.win_map[i][shifted]
            assert got.dtype == torch.int32 and got.numel() == B * pl.nW[i] * WS * WS
            assert torch.equal(got, win.to(torch.int32)), (hw, B, i, shifted)
        # every token appears exactly once per map; the padding is -1
        for m in pl.win_map[i]:
            live = m[m >= 0].long()
            assert torch.equal(live.sort()[0], torch.arange(B * H * W))
            assert int((m < 0).sum()) == B * (Hp * Wp - H * W)


def _independent_mask(Hp, Wp):
    """Tokens i, j of a shifted window are masked exactly when they disagree on wrapping in y or in x; a token wraps in y
    when its padded y before the roll, (wy*7 + iy + 3) % Hp, is < 3 (and likewise in x)."""
    wy, wx, iy, ix = torch.meshgrid(torch.arange(Hp // WS), torch.arange(Wp // WS), torch.arange(WS), torch.arange(WS),
                                    indexing="ij")
    ry = ((wy * WS + iy + SHIFT) % Hp < SHIFT).reshape(-1, WS * WS)
    rx = ((wx * WS + ix + SHIFT) % Wp < SHIFT).reshape(-1, WS * WS)
    return (ry[:, :, None] != ry[:, None, :]) | (rx[:, :, None] != rx[:, None, :])


@pytest.mark.parametrize("hw", SIZES)
def test_shift_mask(hw):
    """shift_mask[i] [nW, 49, 64] is gdino_ref.swin_shift_mask / scale (f32, bit for bit) in columns 0-48, zero in 49-63,
    and -100 / scale exactly where the wrap rule says so.  800x1066 has non-square window grids (29x39 at stage 0),
    100x412 a single window row at stage 3 (4x13 tokens, Hp = 7)."""
    from oracle import gdino_ref
    pl = _plan(*hw, 1)
    grids = []
    for i, (H, W) in enumerate(pl.stage_hw):
        Hp, Wp = _padded(H, W)
        grids.append((Hp // WS, Wp // WS))
        m = pl.shift_mask[i]
        assert m.dtype == torch.float32 and tuple(m.shape) == (pl.nW[i], WS * WS, 64)
        want = gdino_ref.swin_shift_mask(Hp, Wp, WS) / SCALE
        assert torch.equal(m[:, :, :WS * WS].view(torch.int32), want.view(torch.int32)), (hw, i)
        assert torch.equal(m[:, :, WS * WS:], torch.zeros(pl.nW[i], WS * WS, 64 - WS * WS))
        ind = _independent_mask(Hp, Wp)
        assert torch.equal(m[:, :, :WS * WS] != 0, ind), (hw, i)
        assert (m[:, :, :WS * WS][ind] == torch.tensor(-100.0) / SCALE).all()
        assert ind.any() and not ind.all()
    if hw == (800, 1066):
        assert grids[0] == (29, 39)
    if hw == (100, 412):
        assert grids[3] == (1, 2) and pl.stage_hw[3] == (4, 13)


@pytest.mark.parametrize("nh", [3, 6, 12, 24])
def test_swin_dense_bias(nh):
    """gdino.swin_dense_bias == table[swin_rel_index(7)] as [nh, q, k], divided by the scale in f32, bit for bit; keys
    49-63 zero; entry (h, q, k) is table[rel(q, k), h] (not the transposed pair, not another head)."""
    from inklayer_amd import gdino
    from oracle import gdino_ref
    g = torch.Generator().manual_seed(nh)
    table = torch.randn((2 * WS - 1) ** 2, nh, generator=g)
    got = gdino.swin_dense_bias(table, WS, nh, SCALE)
    assert got.dtype == torch.float32 and tuple(got.shape) == (nh, WS * WS, 64)
    rel = gdino_ref.swin_rel_index(WS)
    want = table[rel.view(-1)].view(WS * WS, WS * WS, nh).permute(2, 0, 1) / SCALE
    assert torch.equal(got[:, :, :WS * WS].view(torch.int32), want.contiguous().view(torch.int32))
    assert torch.equal(got[:, :, WS * WS:], torch.zeros(nh, WS * WS, 64 - WS * WS))
    q, k, h = 3, 40, nh - 1                         # (0, 3) vs (5, 5): dy = -5, dx = -2
    assert got[h, q, k] == table[(0 - 5 + 6) * 13 + (3 - 5 + 6), h] / SCALE
    assert got[h, k, q] == table[(5 - 0 + 6) * 13 + (5 - 3 + 6), h] / SCALE


def _attn(**kw):
    from inklayer_amd._lib import InkAttn
    p = InkAttn()
    p.Q = p.K = p.V = p.O = 4096
    p.ldq = p.ldk = p.ldv = 3 * 96 + 8
    p.ldo = 96
    p.n_batch, p.n_heads, p.n_q, p.n_k, p.head_dim = 2, 3, 49, 49, 32
    p.scale = SCALE
    p.bias_mode = 3
    p.dense_bias = 8192
    for k, v in kw.items():
        setattr(p, k, v)
    return p


@pytest.mark.parametrize("bad", [dict(n_q=65), dict(n_k=65), dict(dense_bias=None), dict(dense_mask=8192, n_mask=0),
                                 dict(dense_mask=8192, n_mask=-1)],
                         ids=["n_q>64", "n_k>64", "no_bias", "mask_n0", "mask_nneg"])
def test_flash_attn_bias_mode3_rejects_bad_arguments_without_launch(bad):
    """Each case returns INK_ERR_ARG (1) before any launch (the pointers are never dereferenced on the host)."""
    from inklayer_amd import _lib
    l = _lib.lib()
    assert l.ink_flash_attn(ctypes.byref(_attn(**bad)), None) == 1
