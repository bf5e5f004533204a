"""float64 parity of ink_flash_attn on every dispatch path: each row of flash_attn_ref.CASES (every flash_attn_kernel
instance but <32, 3, 2>, which the Swin window test holds at production shape, and the dedicated win4 / glob4 kernels
away from SAM's own shapes) against the float64 reference, element by element within flash_attn_ref.tolerance.
Inputs are column slices of wider buffers filled with 65504; O is a view of a NaN-filled buffer with 64 guard rows
behind it and 64 guard columns beside it (68 in some cases: O rows then sit on 8-byte, not 16-byte boundaries).
Per case: every written element within its bound, every other element of the buffer (guards, and with tok_rows
nothing but real tokens is written) still NaN; the named mistakes that apply,
re-checked on the case's own data, land >= 100x outside the bound; entry 1 of the run equals, bit for bit, a
one-entry run on its rows; a run through shared row tables equals, bit for bit, the run on materialised copies.
tests/test_flash_attn_plan_cpu.py holds the plan these cases fulfil.  GPU box only."""
import pytest
import torch

import flash_attn_ref as R

pytestmark = pytest.mark.gpu

NAN = float("nan")
GUARD = 64


def _args(d):
    c = d.case
    kw = dict(n_batch=c.B, n_heads=c.H, head_dim=c.hd, scale=d.scale, n_q=c.n_q, n_k=c.n_k, grid_w=c.grid_w,
              q_batch_rows=d.q_rows, kv_batch_rows=d.kv_rows)
    if c.mode == 1:
        kw.update(rel_h=d.rel_h, rel_w=d.rel_w)
    if c.mode == 2:
        kw.update(rel_aug=d.rel_aug)
    if c.tok:
        kw.update(tok_rows=d.tok_rows, pad_k=d.pad_k, pad_v=d.pad_v)
    return kw


def _run(d, q, k, v, n_out, **kw):
    """ops.flash_attn into a [n_out, D] view of a NaN-filled [n_out + 64, D + 64 (or 68)] buffer; the guards are checked here."""
    from inklayer_amd import ops
    c = d.case
    D = c.H * c.hd
    assert R.instance_of(c.hd, c.mode, kw["n_batch"], c.n_q, c.n_k, c.grid_w, R.ldo_of(c), c.tok) == R.case_instance(c)
    buf = torch.full((n_out + GUARD, D + c.gcols), NAN, dtype=R.F16, device=q.device)
    assert buf.stride(0) == R.ldo_of(c)
    ops.flash_attn(q, k, v, out=buf[:n_out, :D], **kw)
    torch.cuda.synchronize()
    assert buf[n_out:].isnan().all() and buf[:, D:].isnan().all(), f"{c.name}: a guard row or column was written"
    return buf[:n_out, :D]


def _entry1(d, out):
    """Entry 1 alone, on views of its rows: bit for bit what the full run wrote for it."""
    c = d.case
    kw = _args(d)
    kw.update(n_batch=1, q_batch_rows=None, kv_batch_rows=None)
    per = c.H * c.n_q
    for name in ("rel_h", "rel_w", "rel_aug"):
        if name in kw:
            kw[name] = kw[name].view(c.B * per, -1)[per:2 * per]
    if c.tok:
        kw.update(tok_rows=d.tok_rows[1:2].contiguous())
        one = _run(d, d.q, d.k, d.v, d.n_out, **kw)
        rows = d.tok_rows[1].long()
        rows = rows[rows >= 0]
        assert torch.equal(one[rows], out[rows]), f"{c.name}: window 1 alone != window 1 of the full run"
        keep = torch.ones(d.n_out, dtype=torch.bool, device=out.device)
        keep[rows] = False
        assert one[keep].isnan().all()
        return
    q0 = R._starts(d.q_rows, c.B, c.n_q)[1]
    k0 = R._starts(d.kv_rows, c.B, c.n_k)[1]
    one = _run(d, d.q[q0:q0 + c.n_q], d.k[k0:k0 + c.n_k], d.v[k0:k0 + c.n_k], c.n_q, **kw)
    assert torch.equal(one, out[c.n_q:2 * c.n_q]), f"{c.name}: entry 1 alone != entry 1 of the full run"


def _materialised(d, out):
    """The shared row tables replaced by copies of the rows they name (same kernel, no table): bit for bit the same O."""
    c = d.case
    D = c.H * c.hd
    kw = _args(d)
    kw.update(q_batch_rows=None, kv_batch_rows=None)
    cat = lambda t, s, n: torch.cat([t[r:r + n] for r in s])               # noqa: E731
    q = R.strided(cat(d.q, R._starts(d.q_rows, c.B, c.n_q), c.n_q), D + 8, 0)
    k = R.strided(cat(d.k, R._starts(d.kv_rows, c.B, c.n_k), c.n_k), D + 16, 8)
    v = R.strided(cat(d.v, R._starts(d.kv_rows, c.B, c.n_k), c.n_k), D + 8, 8)
    assert torch.equal(_run(d, q, k, v, d.n_out, **kw), out), f"{c.name}: shared rows != materialised copies"


@torch.no_grad()
@pytest.mark.parametrize("case", R.CASES, ids=[c.name for c in R.CASES])
def test_flash_attn_case(dev, case):
    """One row of flash_attn_ref.CASES through ops.flash_attn; see the module docstring for what is checked."""
    from inklayer_amd import ops
    inst = R.case_instance(case)
    assert inst is not None
    br = R.branches(case)
    if br & {"persistent_multi_block", "window_change_in_walk"}:
        # more items than workgroups on THIS device too, or the case degrades into one item per workgroup
        n_cus = torch.cuda.get_device_properties(dev).multi_processor_count
        nqb = -(-case.n_q // 224) if isinstance(inst, tuple) else 1
        assert case.B * case.H * nqb > n_cus
        assert br & {"persistent_multi_block", "window_change_in_walk"} <= R.branches(case, n_cus)
    d = R.make_data(case, dev)
    launches = 1
    if case.mode == 2 and case.grid_w == 14 and case.n_q == 196 and not case.q_share:
        # S = 14: the rel_aug rows of the product's own kernel (padded queries' rows stay NaN)
        aug = torch.full_like(d.rel_aug, NAN)
        ops.relpos_bias(d.q, d.Rh, d.Rw, S=14, n_batch=case.B, n_heads=case.H, head_dim=case.hd, scale=d.scale, out=aug,
                        tok_rows=d.tok_rows)
        d.rel_aug = aug
    out = _run(d, d.q, d.k, d.v, d.n_out, **_args(d))
    ref, tol = R.expected(d)
    worst = R.buf_within(out.double(), ref, tol, case.name)
    for what, wrong in R.mistakes(d):
        m = R.buf_discrimination(wrong, ref, tol)
        assert m >= 100, f"{case.name}: the bound cannot tell '{what}' apart: {m:.1f}x"
    del ref, tol
    if case.B > 1:
        _entry1(d, out)
        launches += 1
    if case.q_share or case.kv_share:
        _materialised(d, out)
        launches += 1
    print(f"  FA_CASE {case.name} predicted={str(inst).replace(' ', '')} launches={launches} worst={worst:.3f}x the bound "
          f"branches={','.join(sorted(br))}")
