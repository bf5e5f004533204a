"""float64 references of the SAM ViT-B / ViT-L encoder attention (head_dim 64: relpos_bias, the window and the global
form of the templated flash_attn_kernel), parameterised on the head count (D = heads * 64), next to tests/vith_ref.py,
which holds the same for ViT-H.  The parts of vith_ref that do not depend on the width are imported, not restated:
assert_within, assert_discriminates, relpos_tol, attn_tol, attn_ref, glob_ref.  attn_ref, attn_tol and glob_ref
multiply q.k and the rel terms by ViT-H's scale 80^-1/2; the float64 q and rel tables are therefore handed to them
pre-multiplied by R = (64^-1/2) / (80^-1/2), which makes them compute - exactly, up to float64 rounding - the scale
64^-1/2 the kernels run with.  The bounds hold unchanged: head_dim 64 has fewer MFMA steps per score (4 + 2 instead of
5 + 2) than they allow for, and the row sum, which these instances accumulate on the VALU from the unrounded p instead
of through a ones-column from the f16 p, leaves o off by sum_k P_k e_k v_k with |e_k| <= 2^-11: inside attn_tol's
2^-11 sum_k P_k (|v_k| + |o|).  Every function runs on whatever device its inputs live on."""
import math

import torch

import vith_ref as V
from vith_ref import (F16, F32, F64, assert_discriminates, assert_within, attn_ref, attn_tol, glob_ref,  # noqa: F401
                      relpos_tol)

HD, T, G, WS = 64, 4096, 64, 14
SCALE = HD ** -0.5
R = SCALE / V.SCALE      # see the module docstring


def qkv_data(B, heads, gen, dev, sigma=1.4):
    """Packed f16 qkv [B*4096, 3 * heads * 64] as the qkv GEMM writes it: q, k ~ N(0, sigma^2) (logit std sigma^2 ~ 2:
    peaked softmax), v ~ N(0, 1); every 16th token's q scaled by 1/40 (near-uniform rows)."""
    D = heads * HD
    qkv = torch.randn(B * T, 3 * D, generator=gen, device=dev)
    qkv[:, :2 * D] *= sigma
    qkv[::16, :D] /= 40
    return qkv.half()


def rel_tables(S, gen, dev, std=0.1):
    return (std * torch.randn(2 * S - 1, HD, generator=gen, device=dev),
            std * torch.randn(2 * S - 1, HD, generator=gen, device=dev))


def relpos_ref(q, Rh, Rw, S, qrows, heads, *, swap=False, flip=False, head_shift=0, scale_mode="div"):
    """vith_ref.relpos_ref at `heads` heads of 64: float64 (rel_h, rel_w, mag_h, mag_w) [n, H, S*S, S] and qabs
    [n, H, S*S, 1] for the f16 query rows q[qrows] ([n, S*S] row indices, -1 = padding: zero query); rel = (q . R_x[q_x -
    j + S - 1]) / scale, mag = sum_d |q_d R_d| / scale, qabs = sum_d |q_d| / scale.  Mistakes: swap (rel_h / rel_w tables
    exchanged), flip (k - q instead of q - k), head_shift (the q of head h + shift), scale_mode 'mul' / 'none'."""
    n = qrows.shape[0]
    qq = torch.where((qrows >= 0)[..., None], q[qrows.clamp(min=0).long()].double(), torch.zeros((), dtype=F64, device=q.device))
    qq = qq.view(n, S * S, heads, HD).permute(0, 2, 1, 3)
    if head_shift:
        qq = qq.roll(-head_shift, 1)
    if swap:
        Rh, Rw = Rw, Rh
    pos = torch.arange(S * S, device=q.device)
    j = torch.arange(S, device=q.device)
    f = {"div": 1 / SCALE, "mul": SCALE, "none": 1.0}[scale_mode]
    outs = []
    for Rt, coord in ((Rh, pos // S), (Rw, pos % S)):
        R64 = Rt.double()
        idx = (j[None, :] - coord[:, None] + S - 1) if flip else (coord[:, None] - j[None, :] + S - 1)
        full = qq @ R64.t()
        absf = qq.abs() @ R64.abs().t()
        gi = idx[None, None].expand(n, heads, S * S, S)
        outs.append((f * full.gather(-1, gi), absf.gather(-1, gi) / SCALE))
    qabs = qq.abs().sum(-1, keepdim=True) / SCALE
    return outs[0][0], outs[1][0], outs[0][1], outs[1][1], qabs


def win_item_ref(qkv, rel_aug, win_rows, pad_k, pad_v, windows, heads, *, neighbour_key=False, zero_pad_k=False,
                 stale_kv=False, drop_key=False):
    """float64 window attention of `windows` (indices into win_rows [nw, 196]) for all heads, with rel_aug f16
    [nw * heads, 196, 32] as the kernel reads it.  Returns (q R, k, v, bias magnitude, P, s, o) as [n, H, 196, ..]
    tensors - the arguments of attn_tol - plus the query-row mask [n, 196].  Mistakes: neighbour_key (key 0 of window w
    taken from window w + 1), zero_pad_k (padded keys get k = 0 instead of pad_k), stale_kv (K / V of the previous
    (window, head) item), drop_key (key 195 left out)."""
    D = heads * HD
    rows = win_rows[windows].long()
    n = rows.shape[0]
    valid = rows >= 0
    kv_rows = win_rows[(windows + 1) % win_rows.shape[0]].long() if neighbour_key else None

    def gather(col0, pad, zero_pad=False, rr=rows):
        t = qkv[rr.clamp(min=0), col0:col0 + D].double()
        fill = torch.zeros(D, dtype=F64, device=qkv.device) if zero_pad else pad.double()
        t = torch.where((rr >= 0)[..., None], t, fill)
        return t.view(n, 196, heads, HD).permute(0, 2, 1, 3)

    q = gather(0, torch.zeros(D, device=qkv.device)) * R
    k = gather(D, pad_k, zero_pad_k)
    v = gather(2 * D, pad_v)
    if neighbour_key:
        k2, v2 = gather(D, pad_k, rr=kv_rows), gather(2 * D, pad_v, rr=kv_rows)
        k[:, :, 0], v[:, :, 0] = k2[:, :, 0], v2[:, :, 0]
    if stale_kv:
        k = k.reshape(n * heads, 196, HD).roll(1, 0).view(n, heads, 196, HD)
        v = v.reshape(n * heads, 196, HD).roll(1, 0).view(n, heads, 196, HD)
    ra = rel_aug.view(-1, heads, 196, 32)[windows].double()
    ra = torch.where(valid[:, None, :, None], ra, torch.zeros((), dtype=F64, device=ra.device))   # padding queries: unwritten
    pos = torch.arange(196, device=qkv.device)
    rh = ra[..., :14][..., pos // 14]
    rw = ra[..., 14:28][..., pos % 14]
    bias = SCALE * (rh + rw)
    bmag = SCALE * (rh.abs() + rw.abs())
    if drop_key:
        bias[..., 195] = -math.inf
    o, P, s = attn_ref(q, k, v, bias)
    return q, k, v, bmag, P, s, o, valid


def glob_item_ref(q, k, v, rh, rw, **mistake):
    """vith_ref.glob_ref at scale 64^-1/2 for one (image, head): q, k, v [4096, 64] f64, rh, rw [4096, 64] the kernel's
    rel tables.  Returns (q R, o, P, s, bias magnitude); mistakes as glob_ref's (drop_tile, last_tile_rows, swap)."""
    o, P, s, bmag = glob_ref(q * R, k, v, rh * R, rw * R, **mistake)
    return q * R, o, P, s, bmag
