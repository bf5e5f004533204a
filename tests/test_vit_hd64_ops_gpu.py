"""float64 parity of the head_dim-64 attention path of SAM ViT-B / ViT-L: relpos_bias in its two forms, the window
form (14 x 14 windows, all keys resident, persistent walk) and the global form (f32 rel tables, streamed K/V) of the
templated flash_attn_kernel.  Mirrors tests/test_vith_ops_gpu.py at 3 heads (D = 192: an odd head count, so a slip in
the head index shows) and at ViT-B's 12 heads (D = 768).  References are in tests/vit_hd64_ref.py, the per-element bounds
are vith_ref's.  Outputs are NaN-prefilled with 64 guard rows (and 64 guard columns where the output has a row
stride).  GPU box only."""
import pytest
import torch

import vit_hd64_ref as W

pytestmark = pytest.mark.gpu

NAN = float("nan")


def _gen(dev, seed):
    return torch.Generator(device=dev).manual_seed(seed)


def _report(what, worst):
    print(f"  {what}: worst error {worst:.3f}x the bound")


# ---------------------------------------------------------------------------------------------------------------
# relpos_bias
# ---------------------------------------------------------------------------------------------------------------
def _relpos_wrongs(q, Rh, Rw, S, qrows, heads, ref, tol, valid=None):
    for what, kw in (("rel_h / rel_w swapped", dict(swap=True)), ("k - q indexing", dict(flip=True)),
                     ("q of head h + 1", dict(head_shift=1)), ("scale multiplied", dict(scale_mode="mul")),
                     ("scale omitted", dict(scale_mode="none"))):
        wr = W.relpos_ref(q, Rh, Rw, S, qrows, heads, **kw)
        wrong = torch.cat([wr[0], wr[1]], -1)
        if valid is not None:
            wrong = torch.where(valid, wrong, ref)
        W.assert_discriminates(wrong, ref, tol, what)


@torch.no_grad()
@pytest.mark.parametrize("heads,B", [(3, 1), (12, 2)])
def test_relpos_bias_windows_hd64(dev, heads, B):
    """S = 14 rel_aug rows through sam.window_rows(B, 64, 14) (tok_rows), q a column view of a packed [B*4096, 3 D]
    qkv: per (window, head, query) 32 f16 = rel_h[0..13] | rel_w[0..13] | 4 zeros.  Only real query rows carry a
    requirement (padding rows are left untouched).  Bound: vith_ref.relpos_tol (f16 table in LDS, f16 out)."""
    from inklayer_amd import ops, sam
    D = heads * W.HD
    g = _gen(dev, 120 + heads + B)
    qkv = W.qkv_data(B, heads, g, dev)
    q = qkv[:, :D]
    Rh, Rw = W.rel_tables(14, g, dev, std=0.3)
    wm = sam.window_rows(B, 64, 14).to(dev)
    nb = 25 * B
    n = nb * heads * 196
    buf = torch.full((n + 64, 32), NAN, dtype=W.F16, device=dev)
    ops.relpos_bias(q, Rh, Rw, S=14, n_batch=nb, n_heads=heads, head_dim=W.HD, scale=W.SCALE, out=buf[:n], tok_rows=wm)
    assert buf[n:].isnan().all()
    got = buf[:n].double().view(nb, heads, 196, 32)
    qrows = wm.view(nb, 196)
    rh, rw, mh, mw, qa = W.relpos_ref(q, Rh, Rw, 14, qrows, heads)
    valid = (qrows >= 0)[:, None, :, None]
    ref = torch.cat([rh, rw], -1)
    tol = torch.cat([W.relpos_tol(rh, mh, qa, True), W.relpos_tol(rw, mw, qa, True)], -1)
    gv = torch.where(valid, got[..., :28], ref)
    worst = W.assert_within(gv, ref, tol, f"relpos_bias hd64 S=14 heads={heads} B={B}")
    assert (got[..., 28:][valid.expand(-1, heads, -1, 4)] == 0).all()
    assert got[..., :28][(~valid).expand(-1, heads, -1, 28)].isnan().all()          # padding rows: untouched
    _report(f"relpos_bias hd64 S=14 heads={heads} B={B}", worst)
    _relpos_wrongs(q, Rh, Rw, 14, qrows, heads, ref, tol, valid)


@torch.no_grad()
def test_relpos_bias_global_hd64(dev):
    """S = 64 f32 tables [B*3*4096, 64] at 3 heads, B = 2, NaN guard rows.  Bound: vith_ref.relpos_tol."""
    from inklayer_amd import ops
    heads, B = 3, 2
    D = heads * W.HD
    g = _gen(dev, 130)
    qkv = W.qkv_data(B, heads, g, dev)
    q = qkv[:, :D]
    Rh, Rw = W.rel_tables(64, g, dev, std=0.3)
    n = B * heads * 4096
    bh, bw = (torch.full((n + 64, 64), NAN, dtype=W.F32, device=dev) for _ in range(2))
    oh, ow = ops.relpos_bias(q, Rh, Rw, S=64, n_batch=B, n_heads=heads, head_dim=W.HD, scale=W.SCALE, out=(bh[:n], bw[:n]))
    assert oh.dtype == W.F32 and bh[n:].isnan().all() and bw[n:].isnan().all()
    qrows = torch.arange(B * 4096, device=dev).view(B, 4096)
    rh, rw, mh, mw, qa = W.relpos_ref(q, Rh, Rw, 64, qrows, heads)
    ref = torch.cat([rh, rw], -1)
    tol = torch.cat([W.relpos_tol(rh, mh, qa, False), W.relpos_tol(rw, mw, qa, False)], -1)
    got = torch.cat([bh[:n].double().view(B, heads, 4096, 64), bw[:n].double().view(B, heads, 4096, 64)], -1)
    worst = W.assert_within(got, ref, tol, "relpos_bias hd64 S=64")
    _report("relpos_bias hd64 S=64 f32 tables", worst)
    _relpos_wrongs(q, Rh, Rw, 64, qrows, heads, ref, tol)


# ---------------------------------------------------------------------------------------------------------------
# window attention: flash_attn_kernel<64, 2, 7, ALLKV>, the persistent walk over (window, head) items
# ---------------------------------------------------------------------------------------------------------------
def _win_run(dev, qkv, Rh, Rw, pad_k, pad_v, B, heads):
    """relpos_bias + flash_attn exactly as SamEngine._blocks runs a window block; out is a NaN-filled [B*4096, D] view of
    a [B*4096 + 64, D + 64] buffer.  Returns (buffer, rel_aug)."""
    from inklayer_amd import ops, sam
    D = heads * W.HD
    nb = 25 * B
    wm = sam.window_rows(B, 64, 14).to(dev)
    q, k, v = qkv[:, :D], qkv[:, D:2 * D], qkv[:, 2 * D:]
    aug = torch.full((nb * heads * 196, 32), NAN, dtype=W.F16, device=dev)
    ops.relpos_bias(q, Rh, Rw, S=14, n_batch=nb, n_heads=heads, head_dim=W.HD, scale=W.SCALE, out=aug, tok_rows=wm)
    buf = torch.full((B * 4096 + 64, D + 64), NAN, dtype=W.F16, device=dev)
    ops.flash_attn(q, k, v, n_batch=nb, n_heads=heads, head_dim=W.HD, scale=W.SCALE, n_q=196, n_k=196, rel_aug=aug,
                   grid_w=14, tok_rows=wm, pad_k=pad_k, pad_v=pad_v, out=buf[:B * 4096, :D])
    return buf, aug


@torch.no_grad()
@pytest.mark.parametrize("heads,B", [(3, 1), (12, 2)])
def test_window_attention_hd64(dev, heads, B):
    """3 heads at B = 1: 75 (window, head) items, fewer than the CUs (one item per workgroup).  12 heads at B = 2: 600
    items, several per workgroup (the persistent walk with its register prefetch of the next item).  q / k / v column
    views of the packed qkv, the real win_map, random pad_k / pad_v.  The reference takes the kernel's f16 rel_aug as
    input (relpos_bias has its own test).  Every token row is written and holds its own query's value; the 64 guard rows
    and 64 guard columns stay NaN.  Bound: vith_ref.attn_tol per window.  At B = 2 each image must equal, bit for bit, a
    B = 1 run on that image alone: items are independent, so state carried from one item to the next would show."""
    from inklayer_amd import sam
    D = heads * W.HD
    g = _gen(dev, 140 + heads + B)
    qkv = W.qkv_data(B, heads, g, dev)
    Rh, Rw = W.rel_tables(14, g, dev)
    pad_k, pad_v = torch.randn(D, generator=g, device=dev).half(), torch.randn(D, generator=g, device=dev).half()
    buf, aug = _win_run(dev, qkv, Rh, Rw, pad_k, pad_v, B, heads)
    M = B * 4096
    assert buf[M:].isnan().all() and buf[:, D:].isnan().all()
    out = buf[:M, :D]
    assert not out.isnan().any()
    wm = sam.window_rows(B, 64, 14).to(dev).view(25 * B, 196)
    worst = 0.0
    for i in range(B):
        win = torch.arange(25 * i, 25 * i + 25, device=dev)
        q, k, v, bmag, P, s, o, valid = W.win_item_ref(qkv, aug, wm, pad_k, pad_v, win, heads)
        tol = W.attn_tol(q, k, v, bmag, P, s, o)
        rows = wm[win].long()
        got = out[rows.clamp(min=0)].double().view(25, 196, heads, W.HD).permute(0, 2, 1, 3)
        m = valid[:, None, :, None]
        worst = max(worst, W.assert_within(torch.where(m, got, o), o, tol, f"window hd64 heads={heads} B={B} image {i}"))
        if i == 0:
            for what, kw in (("key 0 of the neighbouring window", dict(neighbour_key=True)),
                             ("zero instead of pad_k", dict(zero_pad_k=True)),
                             ("K / V of the previous item", dict(stale_kv=True)), ("key 195 dropped", dict(drop_key=True))):
                wrong = W.win_item_ref(qkv, aug, wm, pad_k, pad_v, win, heads, **kw)[6]
                W.assert_discriminates(torch.where(m, wrong, o), o, tol, what)
        del q, k, v, bmag, P, s, o, tol
    _report(f"window hd64 heads={heads} B={B}", worst)
    if B > 1:
        for i in range(B):
            one = qkv[i * 4096:(i + 1) * 4096].clone()
            b1, aug1 = _win_run(dev, one, Rh, Rw, pad_k, pad_v, 1, heads)
            n1 = 25 * heads * 196
            assert torch.equal(aug1.view(torch.int16), aug[i * n1:(i + 1) * n1].view(torch.int16))   # bits (NaN rows too)
            assert torch.equal(b1[:4096, :D], out[i * 4096:(i + 1) * 4096]), f"image {i}: B = {B} != B = 1"


# ---------------------------------------------------------------------------------------------------------------
# global attention: flash_attn_kernel<64, 1, 8>, f32 rel tables
# ---------------------------------------------------------------------------------------------------------------
def _glob_run(dev, qkv, Rh, Rw, B, heads):
    from inklayer_amd import ops
    D = heads * W.HD
    q, k, v = qkv[:, :D], qkv[:, D:2 * D], qkv[:, 2 * D:]
    rh, rw = ops.relpos_bias(q, Rh, Rw, S=64, n_batch=B, n_heads=heads, head_dim=W.HD, scale=W.SCALE)
    buf = torch.full((B * 4096 + 64, D + 64), NAN, dtype=W.F16, device=dev)
    ops.flash_attn(q, k, v, n_batch=B, n_heads=heads, head_dim=W.HD, scale=W.SCALE, rel_h=rh, rel_w=rw, grid_w=64,
                   out=buf[:B * 4096, :D])
    return buf, rh, rw


@torch.no_grad()
def test_global_attention_hd64(dev):
    """3 heads at B = 2 with f32 rel tables from relpos_bias; logit std ~2 (peaked softmax) with every 16th query near
    uniform; NaN guard rows / columns.  Reference per (image, head) in float64 on the kernel's own rel tables.  Bound:
    vith_ref.attn_tol; a dropped key tile, the rel rows of the previous query tile and rel_h / rel_w exchanged must land
    >= 100x outside it.  Image 1 must equal, bit for bit, a B = 1 run on image 1 alone (its rel tables too)."""
    heads, B = 3, 2
    D = heads * W.HD
    g = _gen(dev, 150)
    qkv = W.qkv_data(B, heads, g, dev)
    Rh, Rw = W.rel_tables(64, g, dev)
    buf, rh, rw = _glob_run(dev, qkv, Rh, Rw, B, heads)
    M = B * 4096
    assert rh.dtype == W.F32 and buf[M:].isnan().all() and buf[:, D:].isnan().all()
    out = buf[:M, :D]
    worst = 0.0
    for b in range(B):
        for h in range(heads):
            q, k, v = (qkv[b * 4096:(b + 1) * 4096, j * D + h * W.HD:j * D + (h + 1) * W.HD].double() for j in range(3))
            bh = b * heads + h
            th, tw = rh.view(-1, 4096, 64)[bh].double(), rw.view(-1, 4096, 64)[bh].double()
            qs, o, P, s, bmag = W.glob_item_ref(q, k, v, th, tw)
            tol = W.attn_tol(qs, k, v, bmag, P, s, o)
            got = out[b * 4096:(b + 1) * 4096, h * W.HD:(h + 1) * W.HD].double()
            worst = max(worst, W.assert_within(got, o, tol, f"global hd64 image {b} head {h}"))
            if h < 2:
                for wname, kw in (("key tile 37 dropped", dict(drop_tile=37)),
                                  ("last query tile: rel rows of the tile before", dict(last_tile_rows=True)),
                                  ("rel_h / rel_w swapped", dict(swap=True))):
                    W.assert_discriminates(W.glob_item_ref(q, k, v, th, tw, **kw)[1], o, tol, wname)
            del P, s, bmag, tol
    _report("global hd64 B=2, 3 heads, f32 tables", worst)
    i = 1
    b1, rh1, rw1 = _glob_run(dev, qkv[i * 4096:(i + 1) * 4096].clone(), Rh, Rw, 1, heads)
    n1 = heads * 4096
    assert torch.equal(rh1, rh[i * n1:(i + 1) * n1]) and torch.equal(rw1, rw[i * n1:(i + 1) * n1])
    assert torch.equal(b1[:4096, :D], out[i * 4096:(i + 1) * 4096])
