"""ops.attn_midkeys (inklayer_amd/csrc/attn_few.hip, attn_midkeys_kernel<32> / <64>: attn_fewkeys' contract for up to
256 keys, f16 rows, f32 math, online softmax over blocks of 8 keys) against float64.  GPU box only.

Bound, per output element, u = 2^-24, from the kernel's arithmetic:
  scores   an fma chain over head_dim exact f16 x f16 products and one multiply by the scale:
           ds <= (head_dim + 1) u scale |q|.|k|;
  weights  exp(s - m): relative ds + u |s - max| + 4 u, and one rescale by exp(m_old - m_new) (3 u) per block of 8
           keys that follows: eps = ds + u |s - max| + (4 + 3 nblk) u;
  sums     the value sum and the normaliser are sequential over the keys (n_k u each, of sum p |v| and of 1), then one
           division, one multiply and the f16 store (2^-11 relative, 2^-25 absolute below the normal range).
A weight error eps_t moves the output by at most sum p_t eps_t |v_t| + (sum p_t eps_t) |out|."""
import pytest
import torch

from attn_few_ref import attn_ref, rows2d, scores64, strided

pytestmark = pytest.mark.gpu

F16 = torch.float16
U = 2.0 ** -24
FORMS = ((32, 8), (64, 4))                    # (head_dim, n_heads): decoder text cross-attention, text self-attention
NKS = (17, 31, 32, 33, 64, 255, 256)          # one key past fewkeys' limit; around a 32-key edge; the 256-key limit
B = 2


def _caption_ids(n):
    """[CLS] w w . w . w w w . ... [SEP]: n token ids with phrases of growing length, as a multi-phrase caption has."""
    ids, size = [101], 2
    while len(ids) < n - 1:
        ids += [2000 + len(ids) + i for i in range(min(size, n - 2 - len(ids)))]
        if len(ids) < n - 1:
            ids.append(1012)
        size = size % 5 + 1
    return (ids + [102])[:n - 1] + [102]


def _blocked(n_q, n_k):
    """The text self-attention's block-diagonal mask of an n_k-token caption; query q takes the row of token q % n_k."""
    from inklayer_amd.gdino import text_masks_and_position_ids
    ids = _caption_ids(n_k)
    assert len(ids) == n_k
    allowed, _ = text_masks_and_position_ids(ids)
    assert allowed.diagonal().all() and not allowed.all()
    return (~allowed[torch.arange(n_q) % n_k]).to(torch.uint8).contiguous()


def _tol(q, k, v, scale, blocked, ref):
    n_k, hd = k.shape[1], k.shape[3]
    nblk = -(-n_k // 8)
    s = scores64(q, k, scale)                                                        # [n, H, n_q, n_k]
    ds = (hd + 1) * U * scale * torch.einsum("bqhd,bkhd->bhqk", q.double().abs(), k.double().abs())
    if blocked is not None:
        s = s.masked_fill(blocked.bool()[None, None], float("-inf"))
    p = s.softmax(-1)
    gap = (s - s.amax(-1, keepdim=True)).abs().masked_fill(p == 0, 0.0)
    pe = p * (ds + U * gap + (4 + 3 * nblk) * U)
    av = v.double().abs()
    return (torch.einsum("bhqk,bkhd->bqhd", pe, av) + pe.sum(-1).transpose(1, 2)[..., None] * ref.abs()
            + (n_k + 2) * U * torch.einsum("bhqk,bkhd->bqhd", p, av)
            + ((n_k + 3) * U + 2.0 ** -11) * ref.abs() + 2.0 ** -25)


def _inputs(hd, H, n_q, n_k):
    g = torch.Generator().manual_seed(1000 * hd + 7 * n_q + n_k)
    return (torch.randn(B, n_q, H, hd, generator=g).half(), (2.0 * torch.randn(B, n_k, H, hd, generator=g)).half(),
            torch.randn(B, n_k, H, hd, generator=g).half())


def _run(dev, q, k, v, scale, blocked, detector_layout):
    from inklayer_amd import ops
    H, hd = q.shape[2], q.shape[3]
    q2, k2, v2 = (rows2d(t).to(dev) for t in (q, k, v))
    if detector_layout:          # k | v as the two halves of one projection output, q the second half of another
        Ew = H * hd
        k2 = strided(k2, 2 * Ew, 0)
        q2, v2 = strided(q2, 2 * Ew, Ew), strided(v2, 2 * Ew, Ew, base=k2._base)
    out = ops.attn_midkeys(q2, k2, v2, B=B, n_heads=H, head_dim=hd, scale=scale,
                           blocked=None if blocked is None else blocked.to(dev))
    return out.cpu().double().view(B, q.shape[1], H, hd)


@torch.no_grad()
@pytest.mark.parametrize("n_q", [37, 900])
@pytest.mark.parametrize("n_k", NKS)
@pytest.mark.parametrize("hd,H", FORMS)
def test_attn_midkeys(dev, hd, H, n_k, n_q):
    """B = 2 (the batch offset is live), dense rows and the detector's sliced projections, with and without the caption's
    block-diagonal mask; 37 * 2 * H threads leave the last workgroup partial, 900 queries are several workgroups."""
    q, k, v = _inputs(hd, H, n_q, n_k)
    scale = hd ** -0.5
    for blocked in (None, _blocked(n_q, n_k)):
        ref = attn_ref(q, k, v, scale, blocked=blocked)
        tol = _tol(q, k, v, scale, blocked, ref)
        for lay in (False, True):
            out = _run(dev, q, k, v, scale, blocked, lay)
            worst = ((out - ref).abs() / tol).max().item()
            print(f"hd={hd} n_k={n_k} n_q={n_q} blocked={blocked is not None} sliced={lay}: worst / bound = {worst:.3f}")
            assert ((out - ref).abs() <= tol).all(), (hd, n_k, n_q, blocked is not None, lay, worst)


@torch.no_grad()
@pytest.mark.parametrize("hd,H", FORMS)
def test_attn_midkeys_agrees_with_fewkeys_at_16(dev, hd, H):
    """At 16 keys both kernels serve the call: they agree within the sum of their bounds (the same arithmetic, fewkeys
    without the rescales)."""
    from inklayer_amd import ops
    n_q, n_k, scale = 37, 16, hd ** -0.5
    q, k, v = _inputs(hd, H, n_q, n_k)
    for blocked in (None, _blocked(n_q, n_k)):
        ref = attn_ref(q, k, v, scale, blocked=blocked)
        tol = _tol(q, k, v, scale, blocked, ref)
        mid = _run(dev, q, k, v, scale, blocked, False)
        few = ops.attn_fewkeys(*(rows2d(t).to(dev) for t in (q, k, v)), B=B, n_heads=H, head_dim=hd, scale=scale,
                               blocked=None if blocked is None else blocked.to(dev))
        few = few.cpu().double().view(B, n_q, H, hd)
        worst = ((mid - few).abs() / (2 * tol)).max().item()
        print(f"hd={hd} blocked={blocked is not None}: midkeys - fewkeys worst / (2 bounds) = {worst:.3f}")
        assert ((mid - few).abs() <= 2 * tol).all()


@torch.no_grad()
def test_attn_midkeys_fully_blocked_row_is_zero(dev):
    """It cannot occur in the detector (a token sees itself); the result is defined as zeros, not NaN."""
    hd, H, n_q, n_k = 32, 8, 37, 40
    q, k, v = _inputs(hd, H, n_q, n_k)
    blocked = _blocked(n_q, n_k)
    blocked[5] = 1
    out = _run(dev, q, k, v, hd ** -0.5, blocked, False)
    assert (out[:, 5] == 0).all() and torch.isfinite(out).all()
    keep = [i for i in range(n_q) if i != 5]
    ref = attn_ref(q[:, keep], k, v, hd ** -0.5, blocked=blocked[keep])
    assert ((out[:, keep] - ref).abs() <= _tol(q[:, keep], k, v, hd ** -0.5, blocked[keep], ref)).all()
