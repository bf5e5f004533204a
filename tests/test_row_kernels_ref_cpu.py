"""tests/row_kernels_ref.py held to account without a GPU: its LayerNorm is torch's in float64, a float32 host mimic of
layernorm_rows_kernel's own order of operations stays within HALF of the derived bound on every case the GPU tests run
(and on the grid of widths and magnitudes the bound was first checked on), six wrong kernels each land outside the
bound on a committed case, and the exact references of the addition kernels are what their names say."""
import math

import pytest
import torch

import row_kernels_ref as K

F64 = torch.float64


def _all_cases():
    return list(K.CASES) + list(K.headroom_grid())


def test_case_table_covers_every_dispatch_case():
    """NV = ceil(C / 4 / 64) takes every value 1..8 over the widths; the widths straddle each boundary by one vector."""
    nv = sorted({-(-(C // 4) // 64) for C in K.WIDTHS})
    assert nv == [1, 2, 3, 4, 5, 6, 7, 8], nv
    assert len({c.name for c in K.CASES}) == len(K.CASES)
    for C in (256, 512, 1024, 1280):
        assert C in K.WIDTHS and C + 4 in K.WIDTHS


def test_layernorm_ref_is_torch_layer_norm():
    worst = 0.0
    for c in _all_cases():
        x, add, _, dead = c.inputs()
        ref, tol = c.reference()
        z = x.double() if add is None else x.double() + add.double()
        want = torch.nn.functional.layer_norm(z, (c.C,), None if c.gamma is None else c.gamma.double(),
                                              None if c.beta is None else c.beta.double(), c.eps)
        if c.act == "gelu":
            want = torch.nn.functional.gelu(want)
        want[dead] = 0.0
        assert ref.shape == (c.rows, c.C) and tol.shape == ref.shape and (tol[~dead] > 0).all(), c.name
        # two float64 evaluations agree to a few float64 ulps times the row's condition number |z| / sigma (2e4 at
        # offset 1000, spread 0.05): nine orders of magnitude below the f32 bound under test
        cond = max(1.0, (z.abs().amax(-1) / torch.sqrt(z.var(-1, unbiased=False) + c.eps)).max().item())
        err = ((ref - want).abs() / (1.0 + want.abs())).max().item()
        worst = max(worst, err)
        assert err < 64 * 2.0 ** -53 * cond, (c.name, err, cond)
    print(f"layernorm_ref vs torch.nn.functional.layer_norm in float64: worst relative difference {worst:.2g}")


def test_bound_is_an_f32_grade_one():
    """On ordinary rows (offset 0.5, spread 3) the bound is a few f32 ulps of the output, not a loose figure."""
    for C in K.WIDTHS:
        ref, tol = K.CASE[f"width-{C}"].reference()
        assert tol.max().item() < 2e-5 * max(1.0, ref.abs().max().item()), (C, tol.max().item())
        assert (tol / (ref.abs() + 1.0)).max().item() < 64 * K.U * 4, C


def test_f32_mimic_keeps_half_of_the_bound():
    """The kernel's own order of operations in float32 on the host: worst error / bound <= 0.5 on every case, so the
    bound holds with margin before anything runs on a GPU (GELU cases: the LayerNorm part, then torch's float64 GELU of
    the mimic's rows, since the host has no v_rcp / v_exp)."""
    worst = {}
    for c in _all_cases():
        x, add, _, dead = c.inputs()
        got = K.layernorm_mimic(x, c.gamma, c.beta, c.eps, add=add).double()
        if c.act == "gelu":
            got = K.gelu_ref(got)
        got[dead] = 0.0
        ref, tol = c.reference()
        ratio = ((got - ref).abs() / tol.clamp(min=1e-300))[~dead].max().item()
        worst[c.name] = ratio
        assert ratio <= 0.5, (c.name, ratio)
    top = sorted(worst.items(), key=lambda kv: -kv[1])[:5]
    print("f32 mimic worst error / bound, five largest: " + ", ".join(f"{n} {r:.3f}" for n, r in top))


def test_constant_row_is_beta_exactly():
    """C = 256: one vector per lane, (c + c) + (c + c) and the butterfly only double, the division by 256 is exact."""
    for eps in K.EPS_LIST:
        c = K.CASE[f"numerics-eps{eps:g}"]
        got = K.layernorm_mimic(c.x, c.gamma, c.beta, c.eps)
        assert torch.equal(got[K.CONSTANT_ROW], c.beta)
        assert torch.equal(c.reference()[0][K.CONSTANT_ROW], c.beta.double())


# mistake -> the committed cases on which it must show
_SHOWS_ON = {
    "one_pass_variance": ["numerics-eps1e-06", "numerics-eps1e-12"],
    "last_group_dropped": ["width-260", "rows-1", "add-260"],
    "padded_width": ["width-260", "width-1284", "width-4"],
    "add_omitted": ["add-260", "add-table-1284"],
    "add_row_not_looked_up": ["add-table-260", "add-table-1284"],
    "eps_outside_sqrt": ["numerics-eps1e-05", "numerics-eps1e-06"],
}


@pytest.mark.parametrize("mistake", K.MISTAKES)
def test_bound_tells_the_named_mistakes(mistake):
    """Six ways this kernel could be subtly wrong, as float32 host arithmetic in the kernel's order but for the mistake:
    each lands outside the bound on committed cases, while the right mimic is inside on all of them (above)."""
    assert set(_SHOWS_ON) == set(K.MISTAKES)
    for name in _SHOWS_ON[mistake]:
        c = K.CASE[name]
        x, add, plain, dead = c.inputs()
        wrong = K.layernorm_mimic(x, c.gamma, c.beta, c.eps, add=add, mistake=mistake, add_plain=plain).double()
        ref, tol = c.reference()
        over = (wrong - ref).abs() / tol
        over = torch.where(torch.isnan(over), torch.full_like(over, float("inf")), over)      # NaN (a negative variance) is outside
        print(f"{mistake} on {name}: worst / bound {over.max().item():.3g}, elements outside {(over > 1).double().mean().item():.2f}")
        assert over.max().item() > 10, (mistake, name, over.max().item())
    if mistake == "one_pass_variance":
        # it is the offset-1000 rows that show it
        c = K.CASE["numerics-eps1e-06"]
        wrong = K.layernorm_mimic(c.x, c.gamma, c.beta, c.eps, mistake=mistake).double()
        ref, tol = c.reference()
        assert not ((wrong - ref).abs()[:2] <= 10 * tol[:2]).all()


def test_gelu_bound_terms():
    """The approximant's bound: A-S 7.1.26 in float64 is within 1.5e-7 of erf, and gelu_err is that plus the f32
    arithmetic, never below it and never far above (under 1e-5 at |x| <= 8)."""
    x = torch.linspace(-8, 8, 64001, dtype=F64)
    ax = x.abs() / math.sqrt(2.0)
    t = 1.0 / (1.0 + K._AS_P * ax)
    e = sum(a * t ** (k + 1) for k, a in enumerate(K._AS)) * torch.exp(-ax * ax)
    assert ((1.0 - e) - torch.erf(ax)).abs().max().item() <= 1.5e-7
    approx = torch.clamp(x, min=0) - 0.5 * x.abs() * e
    err = K.gelu_err(x)
    assert ((approx - K.gelu_ref(x)).abs() <= err).all()
    assert (err >= 0.5 * x.abs() * 1.5e-7).all() and err.max().item() < 1e-5


def test_split_rule_accepts_the_reference_and_refuses_a_wrong_low_part():
    g = torch.Generator().manual_seed(3)
    v = torch.cat([torch.randn(4, 8, generator=g), torch.randn(4, 8, generator=g) * 1e-4,
                   torch.tensor([[0.0, -0.0, 1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11, 60001.3, -65519.0, 2.0 ** -25, 1e-8]])])
    s = K.split_ref(v)
    K.check_split_rule(s, v, "reference")
    bad = s.clone()
    bad[0, 8] = (bad[0, 8].float() * (1 + 2.0 ** -9)).half()          # one f16 ulp or so of the low part
    assert not torch.equal(K.bits(bad), K.bits(s))
    with pytest.raises(AssertionError):
        K.check_split_rule(bad, v, "low part off by an ulp")
    neg = s.clone()
    neg[8, 0] = -0.0                                                    # +0 stored as -0
    with pytest.raises(AssertionError):
        K.check_split_rule(neg, v, "sign of zero")


def test_add_refs_are_periodic_broadcasts():
    g = torch.Generator().manual_seed(4)
    a, row, blk = torch.randn(6, 8, generator=g), torch.randn(8, generator=g), torch.randn(2, 8, generator=g)
    assert torch.equal(K.add_f32_ref(a, row), a + row)
    assert torch.equal(K.add_f32_ref(a, blk), (a.view(3, 2, 8) + blk).view(6, 8))
    assert torch.equal(K.add_cvt_ref(a, blk), (a.view(3, 2, 8) + blk).view(6, 8).half())
    assert torch.equal(K.add_cvt_ref(a), a.half())
    s = K.add_split_ref(a, row)
    assert s.shape == (6, 24) and torch.equal(s[:, :8], (a + row).half())
