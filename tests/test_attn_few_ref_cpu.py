"""tests/attn_few_ref.py on the CPU: the reference equals PyTorch's own attention in float64, and the generated inputs
of tests/test_attn_few_gpu.py do what they claim (a planted key dominates by >= 20 natural-log units, equal plants tie
bit for bit, no block mask empties a row, strided views are aligned slices of a poisoned buffer)."""
import math

import pytest
import torch
import torch.nn.functional as F

import attn_few_ref as R


def _sdpa64(q, k, v, scale, blocked=None):
    qh, kh, vh = (t.double().transpose(1, 2) for t in (q, k, v))                 # [n, H, rows, hd]
    mask = None if blocked is None else ~blocked.bool()
    return F.scaled_dot_product_attention(qh, kh, vh, attn_mask=mask, scale=scale).transpose(1, 2)


@pytest.mark.parametrize("hd,n_q,n_k", [(16, 7, 300), (32, 9, 9), (64, 4, 4)])
def test_reference_matches_sdpa(hd, n_q, n_k):
    q, k, v = R.randn_inputs(hd, n_q, n_k, seed=hd + n_k)
    scale = hd ** -0.5
    assert (R.attn_ref(q, k, v, scale) - _sdpa64(q, k, v, scale)).abs().max().item() < 1e-12
    # the position constants are plain adds in front of the same function
    g = torch.Generator().manual_seed(1)
    qa, ka = torch.randn(n_q, 8 * hd, generator=g), torch.randn(n_k, 8 * hd, generator=g)
    want = _sdpa64(q.double() + qa.double().view(1, n_q, 8, hd), k.double() + ka.double().view(1, n_k, 8, hd), v, scale)
    assert (R.attn_ref(q, k, v, scale, q_add=qa, k_add=ka) - want).abs().max().item() < 1e-12


def test_reference_matches_sdpa_with_block_mask():
    q, k, v = R.randn_inputs(64, 4, 4, seed=5, H=4)
    for blocked in (R.block_diagonal(4), R.random_blocked(4, 4, 3)):
        assert int((blocked == 0).sum(1).min()) >= 1
        got = R.attn_ref(q, k, v, 0.125, blocked=blocked)
        assert (got - _sdpa64(q, k, v, 0.125, blocked)).abs().max().item() < 1e-12
    assert R.block_diagonal(4).tolist() == [[0, 1, 1, 1], [1, 0, 0, 1], [1, 0, 0, 1], [1, 1, 1, 0]]   # the caption's mask


def test_reference_in_float32_is_float32():
    q, k, v = R.randn_inputs(16, 7, 300, seed=2)
    r32 = R.attn_ref(q, k, v, 0.25, dtype=torch.float32)
    assert r32.dtype == torch.float32
    assert 0 < (r32.double() - R.attn_ref(q, k, v, 0.25)).abs().max().item() < 1e-6


def _check_plant(q, k, scale, plant, blocked=None):
    s = R.scores64(q, k, scale)
    gap = R.top_gap(s, plant, blocked)
    assert gap >= 20.0, gap
    by_mult = {}
    for key, mult in plant:
        by_mult.setdefault(mult, []).append(key)
    for keys in by_mult.values():                       # equal mult: bit-identical key rows, so bit-identical scores
        for key in keys[1:]:
            assert torch.equal(k[:, key], k[:, keys[0]]) and torch.equal(s[..., key], s[..., keys[0]])
    return gap, s.abs().max().item()


@pytest.mark.parametrize("n_q", R.FEWQ_NQ)
@pytest.mark.parametrize("n_k,plant", R.FEWQ_PLANTS)
def test_fewq_plants_dominate(n_k, plant, n_q):
    q, k, v, scale = R.planted_inputs(16, n_k, plant, R.plant_seed(n_k, plant), n_q=n_q)
    assert scale == 0.25 and all(float(k[0, key, 0, 0]) == mult * 7.5 for key, mult in plant)
    gap, smax = _check_plant(q, k, scale, plant)
    print(f"n_k={n_k} plant={plant} n_q={n_q}: gap {gap:.1f}  |score|max {smax:.1f}")
    assert smax < 200                                   # 1.4427 x that stays far inside f32's exponent range
    # the float32 evaluation of the reference is itself f32-grade here: the bounds of the GPU tests leave the kernel room
    e32 = (R.attn_ref(q, k, v, scale, dtype=torch.float32).double() - R.attn_ref(q, k, v, scale)).abs().max().item()
    assert e32 < 5e-7, e32


@pytest.mark.parametrize("hd,H,dtype,n_k,plant,blocked_key", R.FEWKEYS_PLANTS)
def test_fewkeys_plants_dominate(hd, H, dtype, n_k, plant, blocked_key):
    q, k, v, scale = R.planted_inputs(hd, n_k, plant, R.plant_seed(n_k, plant), H=H, n_q=R.FEWKEYS_NQ, dtype=dtype)
    blocked = None if blocked_key is None else R.block_key_for_odd_queries(R.FEWKEYS_NQ, n_k, blocked_key)
    gap, smax = _check_plant(q, k, scale, plant, blocked)
    print(f"hd={hd} {dtype} n_k={n_k} plant={plant}: gap {gap:.1f}  |score|max {smax:.1f}")
    if blocked is not None:
        assert int((blocked == 0).sum(1).min()) >= 1 and int(blocked[:, blocked_key].sum()) == R.FEWKEYS_NQ // 2
    if dtype == torch.float16:
        assert R.attn_ref(q, k, v, scale, blocked=blocked).abs().max().item() < 4.0      # TOL_F16's premise


@pytest.mark.parametrize("n_q", R.FEWQ_NQ)
def test_competing_keys_are_one_unit_apart(n_q):
    q, k, v, scale = R.competing_inputs(7, n_q)
    assert not torch.equal(k[:, 5], k[:, 299])
    s = R.scores64(q, k, scale)
    d = s[..., 299] - s[..., 5]
    assert 0.7 < d.min().item() and d.max().item() < 1.3           # (G + 1) / G of a score of 30 (1 +- 0.2)
    rest = s.clone()
    rest[..., [5, 299]] = float("-inf")
    assert (s[..., 5] - rest.max(-1).values).min().item() >= 20.0


def test_block_masks_keep_a_key_per_row():
    for name, n_q, n_k, m in R.blocked_cases():
        assert m.dtype == torch.uint8 and tuple(m.shape) == (n_q, n_k), name
        assert int((m == 0).sum(1).min()) >= 1 and int(m.sum()) > 0, name
        if name.startswith("diag"):
            assert torch.equal(m, m.t()) and int(m.diagonal().sum()) == 0


def test_f16_cases_stay_below_four():
    """TOL_F16 is half an f16 ulp below 4 (9.8e-4) plus the f32 math: every f16 case keeps |ref| < 4."""
    for hd, H in R.F16_FORMS:
        for n_k in R.F16_NK:
            for n_q in (R.FEWKEYS_NQ, n_k):
                q, k, v = R.f16_inputs(hd, H, n_q, n_k)
                assert q.dtype == torch.float16 and R.attn_ref(q, k, v, hd ** -0.5).abs().max().item() <= R.F16_CLAMP
        for _, n_q, n_k, m in R.blocked_cases():
            q, k, v = R.f16_inputs(hd, H, n_q, n_k)
            assert R.attn_ref(q, k, v, hd ** -0.5, blocked=m).abs().max().item() <= R.F16_CLAMP


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
def test_strided_views(dtype):
    t = torch.randn(11, 128).to(dtype)
    for ld, col0 in ((384, 0), (384, 128), (384, 256), (768, 256), (512, 8), (136, 8)):
        view = R.strided(t, ld, col0)
        assert view.stride(1) == 1 and view.stride(0) == ld and view.data_ptr() % 16 == 0
        assert all((view.data_ptr() + r * ld * view.element_size()) % 16 == 0 for r in range(11))
        assert torch.equal(view.contiguous(), t)
        base = view._base
        outside = torch.cat([base[:, :col0], base[:, col0 + 128:]], 1)
        assert outside.numel() == 11 * (ld - 128)
        assert bool(torch.isnan(outside).all()) if dtype == torch.float32 else bool((outside == 65504).all())
    pair = R.strided(t, 256, 0)
    second = R.strided(t + 1, 256, 128, base=pair._base)                # k and v packed in one buffer
    assert second._base is pair._base and torch.equal(pair, t) and torch.equal(second, t + 1)
    with pytest.raises(AssertionError):
        R.strided(t, 380, 0)
    with pytest.raises(AssertionError):
        R.strided(t, 384, 4)


def test_share_rows_table():
    rows = R.share_rows(37)
    assert rows.dtype == torch.int32 and rows.tolist() == [37, 0, 37] and math.prod(rows.shape) == 3
