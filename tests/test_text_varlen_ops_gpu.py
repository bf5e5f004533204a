"""ops.biattn_wide_varlen and ops.attn_midkeys_varlen: the two kernels behind a batch with one caption per image
(inklayer_amd/csrc/biattn_wide.hip with a token count per image, attn_midkeys_kernel with a mask and a key count per
batch entry).  GPU box only.

What is held: an entry of a mixed batch gets, BIT FOR BIT, what the uniform sibling gives for that entry alone at its
own length (so the float64 bounds of tests/test_biattn_wide_gpu.py and tests/test_attn_midkeys_gpu.py carry over, and
are applied here too); rows behind an entry's length are filled with NaN and must reach nothing; pad outputs are zeros.
Shapes: S = 300 is a ragged third image-side workgroup, S = 1100 a ragged second text-side chunk; token counts sit at
1, just below, at and just above the 32-column tile edge and at the 256 limit."""
import pytest
import torch

from attn_few_ref import attn_ref, rows2d
from test_attn_midkeys_gpu import _caption_ids, _tol
from test_biattn_wide_gpu import E, H, HD, SCALE, _assert_within, _data, _reference

pytestmark = pytest.mark.gpu

F16 = torch.float16
NAN = float("nan")


def _i32(dev, vals):
    return torch.tensor(vals, dtype=torch.int32, device=dev)


def _wide_padded(B, S, Tmax, t_len, seed):
    """qv, kl [B*Tmax, 2E] with NaN in every pad row of kl."""
    qv, kl = _data(B, S, Tmax, seed)
    for b, n in enumerate(t_len):
        kl[b * Tmax + n:(b + 1) * Tmax] = NAN
    return qv, kl


# ------------------------------------------------------------------------------------------------ biattn_wide_varlen
@torch.no_grad()
@pytest.mark.parametrize("S,T", [(300, 33), (1100, 5)])
def test_biattn_wide_varlen_uniform_lengths_equal_the_uniform_kernel(dev, S, T):
    from inklayer_amd import ops
    qv, kl = _data(2, S, T, 31 * S + T)
    qv, kl = qv.to(dev), kl.to(dev)
    ov, ol = ops.biattn_wide(qv, kl, 2, S, T, SCALE)
    gv, gl = ops.biattn_wide_varlen(qv, kl, 2, S, T, _i32(dev, [T, T]), SCALE)
    assert torch.equal(gv, ov) and torch.equal(gl, ol)


@torch.no_grad()
@pytest.mark.parametrize("S,t_len", [(300, (33, 1, 32)), (1100, (256, 5, 31))])
def test_biattn_wide_varlen_mixed_lengths(dev, S, t_len):
    """Image b of the mixed batch = ops.biattn_wide(B=1, T=t_len[b]) on its rows, bit for bit, and within the float64
    bound of test_biattn_wide_gpu; out_l pad rows are zeros; the NaN pad rows of KL reach nothing."""
    from inklayer_amd import ops
    B, Tmax = len(t_len), max(t_len)
    qv, kl = _wide_padded(B, S, Tmax, t_len, 17 * S + Tmax)
    gv, gl = ops.biattn_wide_varlen(qv.to(dev), kl.to(dev), B, S, Tmax, _i32(dev, t_len), SCALE)
    gv, gl = gv.cpu(), gl.cpu()
    assert not torch.isnan(gv.float()).any() and not torch.isnan(gl.float()).any()
    for b, T in enumerate(t_len):
        qv1, kl1 = qv[b * S:(b + 1) * S].clone(), kl[b * Tmax:b * Tmax + T].clone()
        ov, ol = ops.biattn_wide(qv1.to(dev), kl1.to(dev), 1, S, T, SCALE)
        mv, ml = gv[b * S:(b + 1) * S], gl[b * Tmax:(b + 1) * Tmax]
        assert torch.equal(mv, ov.cpu()), f"out_v of image {b} (T = {T}) differs from its B = 1 run"
        assert torch.equal(ml[:T], ol.cpu()), f"out_l of image {b} (T = {T}) differs from its B = 1 run"
        assert (ml[T:] == 0).all(), f"out_l pad rows of image {b}"
        r = _reference(qv1, kl1, S, T)
        _assert_within(mv.double().view(S, H, HD).transpose(0, 1), r["rv"], r["tv"], f"S={S} out_v image {b} T={T}")
        _assert_within(ml[:T].double().view(T, H, HD).transpose(0, 1), r["rl"], r["tl"], f"S={S} out_l image {b} T={T}")


@torch.no_grad()
def test_biattn_wide_varlen_repeats_and_clamps(dev):
    """A repeated call is bitwise equal; device counts outside 1..Tmax behave as 1 and Tmax (a bounds contract, checked
    on results: every KL row is finite here, so that the clamped launch may read them)."""
    from inklayer_amd import ops
    S, Tmax, t_len = 300, 40, (40, 7, 33)
    qv, kl = _wide_padded(3, S, Tmax, t_len, 5)
    qv, kl, tl = qv.to(dev), kl.to(dev), _i32(dev, t_len)
    a = ops.biattn_wide_varlen(qv, kl, 3, S, Tmax, tl, SCALE)
    b = ops.biattn_wide_varlen(qv, kl, 3, S, Tmax, tl, SCALE)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    qv, kl = (t.to(dev) for t in _data(3, S, Tmax, 6))
    want = ops.biattn_wide_varlen(qv, kl, 3, S, Tmax, _i32(dev, (1, Tmax, 1)), SCALE)
    got = ops.biattn_wide_varlen(qv, kl, 3, S, Tmax, _i32(dev, (0, 999, -7)), SCALE)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])


# ------------------------------------------------------------------------------------------------ attn_midkeys_varlen
def _mid_inputs(hd, Hn, B, n_q, n_k, k_len, seed):
    """q [B, n_q, H, hd], k / v [B, n_k, H, hd] f16, NaN in the key / value rows t >= k_len[b]."""
    g = torch.Generator().manual_seed(seed)
    q = torch.randn(B, n_q, Hn, hd, generator=g).half()
    k = (2.0 * torch.randn(B, n_k, Hn, hd, generator=g)).half()
    v = torch.randn(B, n_k, Hn, hd, generator=g).half()
    for b, n in enumerate(k_len):
        k[b, n:] = NAN
        v[b, n:] = NAN
    return q, k, v


def _caption_blocked(n, Tmax):
    """u8 [Tmax, Tmax]: the block-diagonal mask of an n-token caption in the corner, pads blocked except the diagonal."""
    from inklayer_amd.gdino import text_masks_and_position_ids
    allowed = torch.eye(Tmax, dtype=torch.bool)
    allowed[:n, :n] = text_masks_and_position_ids(_caption_ids(n))[0]
    return (~allowed).to(torch.uint8)


def _check_entry(dev, got_b, q_b, k_b, v_b, n, scale, blocked_b, what):
    """got_b [n_q', H, hd] (f16, CPU) against ops.attn_midkeys(B=1, n_k=n) bit for bit and against float64."""
    from inklayer_amd import ops
    Hn, hd = q_b.shape[1], q_b.shape[2]
    q1, k1, v1 = q_b[None], k_b[None, :n], v_b[None, :n]
    one = ops.attn_midkeys(*(rows2d(t).to(dev) for t in (q1, k1, v1)), B=1, n_heads=Hn, head_dim=hd, scale=scale,
                           blocked=None if blocked_b is None else blocked_b.to(dev))
    assert torch.equal(got_b.reshape(-1, Hn * hd), one.cpu()), f"{what}: differs from its B = 1 run at n_k = {n}"
    ref = attn_ref(q1, k1, v1, scale, blocked=blocked_b)
    tol = _tol(q1, k1, v1, scale, blocked_b, ref)
    _assert_within(got_b.double()[None], ref, tol, what)


@torch.no_grad()
def test_attn_midkeys_varlen_plain_call_equals_attn_midkeys(dev):
    from inklayer_amd import ops
    hd, Hn, B, n = 64, 4, 2, 23
    q, k, v = _mid_inputs(hd, Hn, B, n, n, (n, n), 1)
    blocked = _caption_blocked(n, n).to(dev)
    args = [rows2d(t).to(dev) for t in (q, k, v)]
    kw = dict(B=B, n_heads=Hn, head_dim=hd, scale=hd ** -0.5)
    for bl in (blocked, None):
        assert torch.equal(ops.attn_midkeys_varlen(*args, blocked=bl, **kw), ops.attn_midkeys(*args, blocked=bl, **kw))
    both = blocked[None].repeat(B, 1, 1).contiguous()
    assert torch.equal(ops.attn_midkeys_varlen(*args, blocked=both, k_len=_i32(dev, (n, n)), **kw),
                       ops.attn_midkeys(*args, blocked=blocked, **kw))


@torch.no_grad()
def test_attn_midkeys_varlen_text_enhancer_form(dev):
    """B = 3, 23 x 23, 4 heads x 64, key counts (23, 9, 1), each entry's own block-diagonal mask."""
    from inklayer_amd import ops
    hd, Hn, B, n, k_len = 64, 4, 3, 23, (23, 9, 1)
    q, k, v = _mid_inputs(hd, Hn, B, n, n, k_len, 2)
    blocked = torch.stack([_caption_blocked(c, n) for c in k_len]).contiguous()
    out = ops.attn_midkeys_varlen(*(rows2d(t).to(dev) for t in (q, k, v)), B=B, n_heads=Hn, head_dim=hd,
                                  scale=hd ** -0.5, blocked=blocked.to(dev), k_len=_i32(dev, k_len))
    out = out.cpu().view(B, n, Hn, hd)
    assert not torch.isnan(out.float()).any()
    for b, c in enumerate(k_len):
        _check_entry(dev, out[b, :c], q[b, :c], k[b], v[b], c, hd ** -0.5, blocked[b, :c, :c].contiguous(),
                     f"text form entry {b}")
        assert (out[b, c:] == 0).all(), f"pad query rows of entry {b}"


@torch.no_grad()
def test_attn_midkeys_varlen_decoder_form(dev):
    """B = 3, 37 queries x 256 keys, 8 heads x 32, no mask, key counts (17, 256, 8)."""
    from inklayer_amd import ops
    hd, Hn, B, n_q, n_k, k_len = 32, 8, 3, 37, 256, (17, 256, 8)
    q, k, v = _mid_inputs(hd, Hn, B, n_q, n_k, k_len, 3)
    out = ops.attn_midkeys_varlen(*(rows2d(t).to(dev) for t in (q, k, v)), B=B, n_heads=Hn, head_dim=hd,
                                  scale=hd ** -0.5, k_len=_i32(dev, k_len))
    out = out.cpu().view(B, n_q, Hn, hd)
    assert not torch.isnan(out.float()).any()
    for b, c in enumerate(k_len):
        _check_entry(dev, out[b], q[b], k[b], v[b], c, hd ** -0.5, None, f"decoder form entry {b}")


@torch.no_grad()
def test_attn_midkeys_varlen_zero_keys_and_clamped_counts(dev):
    """k_len[b] = 0 gives zeros for that entry; the device values 300 and -2 behave as 256 and 0 (every row finite)."""
    from inklayer_amd import ops
    hd, Hn, B, n_q, n_k = 32, 8, 4, 37, 256
    q, k, v = _mid_inputs(hd, Hn, B, n_q, n_k, (n_k,) * B, 4)
    args = [rows2d(t).to(dev) for t in (q, k, v)]
    kw = dict(B=B, n_heads=Hn, head_dim=hd, scale=hd ** -0.5)
    got = ops.attn_midkeys_varlen(*args, k_len=_i32(dev, (0, 300, -2, 40)), **kw).view(B, n_q, -1)
    want = ops.attn_midkeys_varlen(*args, k_len=_i32(dev, (0, 256, 0, 40)), **kw).view(B, n_q, -1)
    full = ops.attn_midkeys(*args, **kw).view(B, n_q, -1)
    assert torch.equal(got, want) and (got[0] == 0).all() and (got[2] == 0).all()
    assert torch.equal(got[1], full[1]) and not torch.equal(got[3], full[3])
