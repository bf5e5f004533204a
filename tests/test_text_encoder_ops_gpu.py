"""ops.text_embed_ln and ops.attn_text_f32 (inklayer_amd/csrc/text_bert.hip) against float64, each launch on its own.
GPU box only.  The references and the per-element bounds are tests/text_encoder_ref.py's (derived there from the kernels'
arithmetic); the split-f16 outputs are checked against the f32 outputs of the same launch:
  hi + lo / 64 reproduces the f32 value v to 2^-21 |v| (hi = f16(v) and v - hi are exact, the f16 rounding of
  (v - hi) * 64 is 2^-11 of a term below 2^-11 |v| * 64) plus 2^-31 absolute: where (v - hi) * 64 falls below f16's
  normal range (|v| under about 2^-9) its rounding is absolute, half of the subnormal spacing 2^-24, divided by 64;
  the third segment is f16(hi / 64) exactly."""
import pytest
import torch

import text_encoder_ref as R
from attn_few_ref import TOL_FEWQ
from row_kernels_ref import check_split as _check_split

pytestmark = pytest.mark.gpu

F16, F32, I32 = torch.float16, torch.float32, torch.int32


# ---------------------------------------------------------------------------------------------------------------
# ops.text_embed_ln
# ---------------------------------------------------------------------------------------------------------------
V, P, C = 64, 16, 768


def _embed_case(n_rows):
    g = torch.Generator().manual_seed(50 + n_rows)
    word, pos = 0.05 * torch.randn(V, C, generator=g), 0.05 * torch.randn(P, C, generator=g)
    type_row = 0.05 * torch.randn(C, generator=g)
    gamma, beta = 1 + 0.1 * torch.randn(C, generator=g), 0.05 * torch.randn(C, generator=g)
    ids = torch.randint(0, V, (n_rows,), generator=g)
    pid = torch.randint(0, P, (n_rows,), generator=g)
    ids[0], pid[0] = V - 1, P - 1                       # the tables' last rows ...
    if n_rows > 1:
        ids[-1], pid[-1] = 0, 0                         # ... and their first
    return ids, pid, word, pos, type_row, gamma, beta


@torch.no_grad()
@pytest.mark.parametrize("n_rows", [1, 5, 67])
def test_text_embed_ln(dev, n_rows):
    """One row, a partial workgroup (4 rows each), 17 workgroups; C = 768 is BERT's (three 16-byte vectors per lane)."""
    from inklayer_amd import ops
    ids, pid, *tabs = _embed_case(n_rows)
    ref, tol = R.embed_ln_ref(ids, pid, *tabs, 1e-12)
    out, split = ops.text_embed_ln(ids.tolist(), pid, *(t.to(dev) for t in tabs), 1e-12)
    assert out.shape == (n_rows, C) and out.dtype == F32 and split.shape == (n_rows, 3 * C) and split.dtype == F16
    err = (out.cpu().double() - ref).abs()
    print(f"R={n_rows}: max abs err {err.max().item():.3g}, worst / bound {(err / tol).max().item():.3f}, "
          f"bound max {tol.max().item():.3g}")
    assert (err <= tol).all()
    assert tol.max().item() < 2e-5 * max(1.0, ref.abs().max().item())       # the bound is an f32-grade one
    _check_split(split.cpu(), out.cpu(), n_rows)
    # device ids take the same path; out-of-range DEVICE ids are clamped into the tables
    dids, dpid = ids.to(I32).to(dev), pid.to(I32).to(dev)
    out2, split2 = ops.text_embed_ln(dids, dpid, *(t.to(dev) for t in tabs), 1e-12)
    assert torch.equal(out2, out) and torch.equal(split2, split)
    bad, badp = dids.clone(), dpid.clone()
    bad[0], badp[0] = V + 1000, P + 7
    if n_rows > 1:
        bad[-1], badp[-1] = -5, -1
    out3, _ = ops.text_embed_ln(bad, badp, *(t.to(dev) for t in tabs), 1e-12)
    assert torch.equal(out3, out)


def test_text_embed_ln_refuses_bad_host_ids(dev):
    from inklayer_amd import ops
    ids, pid, *tabs = _embed_case(5)
    tabs = [t.to(dev) for t in tabs]
    for bad_ids, bad_pid in (([0, V], [0, 0]), ([-1, 0], [0, 0]), ([0, 1], [0, P]), (torch.tensor([0, 1]), torch.tensor([-1, 0]))):
        with pytest.raises(ValueError):
            ops.text_embed_ln(bad_ids, bad_pid, *tabs, 1e-12)


# ---------------------------------------------------------------------------------------------------------------
# ops.attn_text_f32
# ---------------------------------------------------------------------------------------------------------------
LENGTHS = ((1, 9, 23), (4, 4, 4), (256,), (255, 17))
SCALE = 0.125
# q, k and v are half-normal rows.  The worst-case bound of an f32 dot product grows with |q|.|k| (64 terms here, 16 in
# the few-query kernel TOL_FEWQ was set for) and every term of the output bound with |v|, while TOL_FEWQ has an absolute
# floor at |ref|max <= 1: at these gains the derived bound stays under it for every case below, at unit gains it is a
# few times larger for any f32 kernel of this shape.
QK_GAIN = V_GAIN = 0.5


def _caption_blocked(n):
    if n == 1:
        return torch.zeros(1, 1, dtype=torch.uint8)
    allowed, _ = R.masks_and_pos(R.caption_ids(n))
    return (~allowed).to(torch.uint8)


def _random_blocked(n, seed):
    """Three pairs of four blocked at random, the diagonal kept: a row sees about a quarter of the caption, which is
    still far more keys than a phrase of a real caption has."""
    g = torch.Generator().manual_seed(seed)
    m = (torch.rand(n, n, generator=g) < 0.75).to(torch.uint8)
    m[torch.arange(n), torch.arange(n)] = 0
    return m


_CASES = {}


def _case(lens, H, kind):
    """q, k, v as the three column blocks of one packed projection [R, 3 H 64], the per-caption masks, the float64
    reference and bound: computed once per case and shared."""
    key = (lens, H, kind)
    if key not in _CASES:
        g = torch.Generator().manual_seed(1000 * len(lens) + 10 * sum(lens) + H)
        Rn = sum(lens)
        qkv = torch.randn(Rn, 3 * H * 64, generator=g)
        qkv[:, :2 * H * 64] *= QK_GAIN
        qkv[:, 2 * H * 64:] *= V_GAIN
        q, k, v = (qkv[:, i * H * 64:(i + 1) * H * 64].reshape(Rn, H, 64) for i in range(3))
        if kind == "caption":
            blocked = [_caption_blocked(n) for n in lens]
        elif kind == "random":
            blocked = [_random_blocked(n, 31 * n + b) for b, n in enumerate(lens)]
        else:
            blocked = None
        dead = None
        if kind == "random" and max(lens) >= 9:            # one caption with a row that sees nothing
            b = max(range(len(lens)), key=lambda i: lens[i])
            dead = (b, lens[b] // 2)
            blocked[b][dead[1]] = 1
        ref, tol = R.attn_text_ref(q, k, v, lens, blocked, SCALE)
        _CASES[key] = (qkv, q, k, v, blocked, dead, ref, tol)
    return _CASES[key]


def _batched_mask(lens, blocked):
    if blocked is None:
        return None
    Tmax = max(lens)
    m = torch.ones(len(lens), Tmax, Tmax, dtype=torch.uint8)
    for b, n in enumerate(lens):
        m[b, :n, :n] = blocked[b]
    return m


def _row_start(lens, dev):
    s = [0]
    for n in lens:
        s.append(s[-1] + n)
    return torch.tensor(s, dtype=I32).to(dev)


def _launch(dev, qkv_dev, lens, H, mask, rows=None):
    from inklayer_amd import ops
    E = H * 64
    x = qkv_dev if rows is None else qkv_dev[rows]
    return ops.attn_text_f32(x[:, :E], x[:, E:2 * E], x[:, 2 * E:], _row_start(lens, dev), Tmax=max(lens), n_heads=H,
                             scale=SCALE, blocked=None if mask is None else mask.to(dev), want_f32=True)


@torch.no_grad()
@pytest.mark.parametrize("kind", ["caption", "random", "none"])
@pytest.mark.parametrize("H", [12, 1])
@pytest.mark.parametrize("lens", LENGTHS, ids=lambda l: "-".join(map(str, l)))
def test_attn_text_f32(dev, lens, H, kind):
    """One token, captions below and across the 64-query / 64-key tiles (255, 256: four tiles, the last one partial),
    equal and mixed lengths; BERT's 12 heads and one; q / k / v read in place at ld = 3 H 64."""
    qkv, q, k, v, blocked, dead, ref, tol = _case(lens, H, kind)
    split, out = _launch(dev, qkv.to(dev), lens, H, _batched_mask(lens, blocked))
    Rn, E = sum(lens), H * 64
    assert split.shape == (Rn, 3 * E) and out.shape == (Rn, E)
    got = out.cpu().double().view(Rn, H, 64)
    assert torch.isfinite(got).all()
    err = (got - ref).abs()
    yard = TOL_FEWQ * max(1.0, ref.abs().max().item())
    print(f"lens={lens} H={H} {kind}: max abs err {err.max().item():.3g}, worst / bound {(err / tol).max().item():.3f}, "
          f"bound max {tol.max().item():.3g} (project figure {yard:.3g})")
    assert tol.max().item() <= yard                         # the derived bound is no looser than the project's figure
    assert (err <= tol).all()
    if dead is not None:
        r0 = sum(lens[:dead[0]]) + dead[1]
        assert (ref[r0] == 0).all() and (got[r0] == 0).all()
    _check_split(split.cpu(), out.cpu(), (lens, H, kind))


@torch.no_grad()
@pytest.mark.parametrize("kind", ["caption", "random"])
@pytest.mark.parametrize("lens", [l for l in LENGTHS if len(l) > 1], ids=lambda l: "-".join(map(str, l)))
def test_attn_text_f32_caption_alone_is_bitwise(dev, lens, kind):
    """Every caption's rows of the batched launch equal a B = 1 launch on that caption alone (its own Tmax and mask)."""
    H = 12
    qkv, q, k, v, blocked, dead, ref, tol = _case(lens, H, kind)
    qkv_dev = qkv.to(dev)
    split, out = _launch(dev, qkv_dev, lens, H, _batched_mask(lens, blocked))
    r0 = 0
    for b, n in enumerate(lens):
        rows = slice(r0, r0 + n)
        s1, o1 = _launch(dev, qkv_dev, (n,), H, blocked[b][None].contiguous(), rows=rows)
        assert torch.equal(o1, out[rows]) and torch.equal(s1, split[rows]), (lens, b)
        r0 += n


@torch.no_grad()
@pytest.mark.parametrize("lens", [(1, 9, 23), (255, 17)], ids=lambda l: "-".join(map(str, l)))
def test_attn_text_f32_bound_tells_the_named_mistakes(lens):
    """The two mistakes this kernel could make unnoticed by a loose check - ignoring the mask, and reading a neighbour
    caption's keys - land far outside the bound on the data of the cases above (host arithmetic only: the GPU result
    is within the bound of the right answer, test_attn_text_f32)."""
    for kind in ("caption", "random"):
        qkv, q, k, v, blocked, dead, ref, tol = _case(lens, 12, kind)
        unmasked, _ = R.attn_text_ref(q, k, v, lens, blocked, SCALE, ignore_mask=True)
        neighbour, _ = R.attn_text_ref(q, k, v, lens, blocked, SCALE, shift_keys=1)
        for name, wrong in (("mask ignored", unmasked), ("neighbour's keys", neighbour)):
            over = ((wrong - ref).abs() / tol)
            frac = (over > 100).double().mean().item()
            print(f"lens={lens} {kind} {name}: worst / bound {over.max().item():.3g}, elements over 100 bounds {frac:.2f}")
            assert over.max().item() > 1e4 and frac > 0.25
