"""The device-table MSDA forward (f32 / f64, any C and L) and its backward against the float64 oracle
(oracle/gdino_ref.py:msda_core and torch.autograd through it), plus the groundingdino._C drop-in.  GPU box only."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

F32, F64 = torch.float32, torch.float64
# odd sizes and a 1x1 level; the first L of them are used
LEVELS = [(7, 5), (1, 1), (3, 9), (12, 10), (2, 2), (5, 1), (1, 6), (9, 9), (4, 3)]
MODEL_LEVELS = [(100, 100), (50, 50), (25, 25), (13, 13)]


def _starts(shapes):
    return [int(v) for v in np.cumsum([0] + [h * w for h, w in shapes])[:-1]]


def _tables(shapes, dev=None):
    return (torch.tensor(shapes, dtype=torch.int64, device=dev), torch.tensor(_starts(shapes), dtype=torch.int64, device=dev))


def _jitter(loc, shapes, gap=1e-3):
    """Moves every coordinate at least `gap` px away from the integer grid of its level's image coordinate
    (x*W - 0.5, y*H - 0.5): the oracle is piecewise linear there, so its gradient jumps across those lines."""
    loc = loc.copy()
    for l, (H, W) in enumerate(shapes):
        for axis, n in ((0, W), (1, H)):
            c = loc[:, :, :, l, :, axis]
            u = c * n - 0.5
            near = np.abs(u - np.round(u)) < 2 * gap
            c[near] += 4 * gap / n
    return loc


def _make(rs, B, Q, M, C, shapes, P, dtype, *, jitter, lo=-0.1, hi=1.1):
    S = sum(h * w for h, w in shapes)
    L = len(shapes)
    v = rs.standard_normal((B, S, M, C))
    loc = rs.uniform(lo, hi, size=(B, Q, M, L, P, 2))
    aw = rs.uniform(0, 1, size=(B, Q, M, L, P))
    if not jitter:               # exact 0, 1 and pixel centres
        loc[0, 0] = 0.0
        loc[0, 1 % Q] = 1.0
        for l, (H, W) in enumerate(shapes):
            loc[-1, 2 % Q, :, l, :, 0] = (np.arange(P) % W + 0.5) / W
            loc[-1, 2 % Q, :, l, :, 1] = (np.arange(P) % H + 0.5) / H
    else:
        loc = _jitter(loc, shapes)
    t = lambda a: torch.from_numpy(a.astype(np.float32)).to(dtype)   # f32 inputs are exact in the f64 oracle
    return t(v), t(loc), t(aw)


def _oracle(v, shapes, loc, aw, g=None, qchunk=None):
    """float64 forward (+ the three gradients of <out, g> by autograd through msda_core), chunked over queries."""
    from oracle import gdino_ref
    v, loc, aw = v.double().cpu(), loc.double().cpu(), aw.double().cpu()
    Q = loc.shape[1]
    qchunk = qchunk or Q
    outs, gls, gas = [], [], []
    gv = torch.zeros_like(v)
    for q0 in range(0, Q, qchunk):
        vv = v.clone().requires_grad_(g is not None)
        ll = loc[:, q0:q0 + qchunk].clone().requires_grad_(g is not None)
        aa = aw[:, q0:q0 + qchunk].clone().requires_grad_(g is not None)
        out = gdino_ref.msda_core(vv, shapes, ll, aa)
        if g is not None:
            out.backward(g[:, q0:q0 + qchunk].double().cpu())
            gv += vv.grad
            gls.append(ll.grad)
            gas.append(aa.grad)
        outs.append(out.detach())
    if g is None:
        return torch.cat(outs, 1)
    return torch.cat(outs, 1), gv, torch.cat(gls, 1), torch.cat(gas, 1)


def _assert_forward(got, v, shapes, loc, aw, dtype, what, qchunk=None):
    r = _oracle(v, shapes, loc, aw, qchunk=qchunk)
    ra = _oracle(v.abs(), shapes, loc, aw.abs(), qchunk=qchunk)
    tol = (1e-12 if dtype == F64 else 1e-5) * (1 + ra)
    err = (got.double().cpu() - r).abs()
    assert bool((err <= tol).all()), f"{what}: max err {err.max().item():.3e}, worst ratio {(err / tol).max().item():.3f}"
    return r, tol


def _assert_grad(got, ref, dtype, what):
    got = got.double().cpu()
    d = got - ref
    maxn = (d.abs().max() / ref.abs().max().clamp(min=1e-300)).item()
    if dtype == F64:
        assert maxn <= 1e-10, f"{what}: max-normalised error {maxn:.3e}"
    else:
        rel = (d.norm() / ref.norm().clamp(min=1e-300)).item()
        assert rel <= 1e-5 and maxn <= 1e-4, f"{what}: relative L2 {rel:.3e}, max-normalised {maxn:.3e}"


def _assert_grads(got, ref, dtype, what):
    for name, a, b in zip(("grad_value", "grad_sampling_loc", "grad_attn_weight"), got, ref):
        assert a.dtype == dtype and tuple(a.shape) == tuple(b.shape), (what, name, a.dtype, a.shape)
        _assert_grad(a, b, dtype, f"{what} {name}")


CONFIGS = [(C, L, P) for C in (1, 3, 32, 64, 256) for L in (1, 4, 5, 9) for P in (1, 4, 8)]


# ------------------------------------------------------------------------------------------------------------
# 1. general forward
@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
@pytest.mark.parametrize("C,L,P", CONFIGS)
def test_forward_general(dev, dtype, C, L, P):
    from inklayer_amd import ops
    rs = np.random.RandomState(C * 100 + L * 10 + P)
    shapes = LEVELS[:L]
    v, loc, aw = _make(rs, 2, 13, 2, C, shapes, P, dtype, jitter=False)
    ss, ls = _tables(shapes, dev)
    got = ops.ms_deform_attn_forward(v.to(dev), ss, ls, loc.to(dev), aw.to(dev), 64)
    assert got.dtype == dtype and tuple(got.shape) == (2, 13, 2 * C)
    r, tol = _assert_forward(got, v, shapes, loc, aw, dtype, f"forward C={C} L={L} P={P}")
    # the tolerance is tight enough to see x and y swapped
    swapped = _oracle(v, shapes, loc.flip(-1), aw)
    assert bool(((swapped - r).abs() > tol).any()), "x/y swap not discriminated"


# 2. the existing call is unchanged
def test_existing_call_unchanged(dev):
    from inklayer_amd import _lib, ops
    rs = np.random.RandomState(5)
    shapes = [(20, 20), (10, 10), (5, 5), (3, 3)]
    B, Q, M, L, P = 2, 50, 8, 4, 4
    v, loc, aw = _make(rs, B, Q, M, 32, shapes, P, F32, jitter=False)
    v, loc, aw = v.to(dev), loc.to(dev), aw.to(dev)
    S = v.shape[1]
    flat = [x for hw in shapes for x in hw]
    direct = torch.empty((B, Q, M * 32), device=dev)
    _lib.check(_lib.lib().ink_ms_deform_attn_forward(
        v.data_ptr(), (ctypes.c_int64 * 8)(*flat), (ctypes.c_int64 * 4)(*_starts(shapes)), loc.data_ptr(),
        aw.data_ptr(), B, S, M, 32, Q, L, P, 64, direct.data_ptr(), ops._stream()), "direct")
    host = ops.ms_deform_attn_forward(v, torch.tensor(shapes), torch.tensor(_starts(shapes)), loc, aw, 64)
    devt = ops.ms_deform_attn_forward(v, *_tables(shapes, dev), loc, aw, 64)
    # one kernel template: the host-table and device-table instances give the same bits
    assert torch.equal(host, direct)
    assert torch.equal(devt, direct)
    # a value tensor 4 bytes off 16-B alignment takes the scalar-gather instance: the same bits again
    buf = torch.empty(v.numel() + 1, device=dev)
    vm = buf[1:].view(v.shape)
    vm.copy_(v)
    assert torch.equal(ops.ms_deform_attn_forward(vm, *_tables(shapes, dev), loc, aw, 64), direct)
    _assert_forward(direct, v.cpu(), shapes, loc.cpu(), aw.cpu(), F32, "direct")


# 3. backward against the float64 oracle's autograd
@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
@pytest.mark.parametrize("C,L,P", CONFIGS)
def test_backward_general(dev, dtype, C, L, P):
    from inklayer_amd import ops
    rs = np.random.RandomState(C * 100 + L * 10 + P + 1)
    shapes = LEVELS[:L]
    v, loc, aw = _make(rs, 2, 13, 2, C, shapes, P, dtype, jitter=True)
    g = torch.from_numpy(rs.standard_normal((2, 13, 2 * C)).astype(np.float32)).to(dtype)
    _, *ref = _oracle(v, shapes, loc, aw, g)
    got = ops.ms_deform_attn_backward(v.to(dev), *_tables(shapes, dev), loc.to(dev), aw.to(dev), g.to(dev), 64)
    _assert_grads(got, ref, dtype, f"backward C={C} L={L} P={P}")


@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
def test_backward_all_outside_is_exactly_zero(dev, dtype):
    from inklayer_amd import _lib, ops
    rs = np.random.RandomState(11)
    shapes = LEVELS[:5]
    B, Q, M, C, P = 2, 9, 3, 32, 4
    v, loc, aw = _make(rs, B, Q, M, C, shapes, P, dtype, jitter=False)
    # x*W - 0.5 <= -1.1 or >= W + 0.1 on every level: outside (-1, W)
    loc = torch.where(torch.from_numpy(rs.uniform(size=tuple(loc.shape)) < 0.5), -0.6, 1.6).to(dtype)
    g = torch.randn(B, Q, M * C, dtype=dtype)
    ss, ls = _tables(shapes, dev)
    vd, ld, ad, gd = v.to(dev), loc.to(dev), aw.to(dev), g.to(dev)
    assert not ops.ms_deform_attn_forward(vd, ss, ls, ld, ad, 64).any()
    # the entry point writes every element of its three outputs, grad_value included: start them as NaN
    outs = [torch.full_like(t, float("nan")) for t in (vd, ld, ad)]
    _lib.check(_lib.lib().ink_ms_deform_attn_backward_dev(
        vd.data_ptr(), ss.data_ptr(), ls.data_ptr(), ld.data_ptr(), ad.data_ptr(), gd.data_ptr(),
        0 if dtype == F32 else 1, B, v.shape[1], M, C, Q, len(shapes), P, 64, *(o.data_ptr() for o in outs),
        ops._stream()), "backward_dev")
    for o in outs:
        assert not o.isnan().any() and not o.any()
    for o in ops.ms_deform_attn_backward(vd, ss, ls, ld, ad, gd, 64):
        assert not o.any()


def test_backward_writes_every_element(dev):
    """Uninitialised (NaN-filled) outputs come back equal to the wrapper's, on inputs with samples inside."""
    from inklayer_amd import _lib, ops
    rs = np.random.RandomState(12)
    shapes = LEVELS[:4]
    B, Q, M, C, P = 2, 11, 2, 3, 4
    v, loc, aw = _make(rs, B, Q, M, C, shapes, P, F64, jitter=True)
    g = torch.randn(B, Q, M * C, dtype=F64)
    ss, ls = _tables(shapes, dev)
    vd, ld, ad, gd = v.to(dev), loc.to(dev), aw.to(dev), g.to(dev)
    outs = [torch.full_like(t, float("nan")) for t in (vd, ld, ad)]
    _lib.check(_lib.lib().ink_ms_deform_attn_backward_dev(
        vd.data_ptr(), ss.data_ptr(), ls.data_ptr(), ld.data_ptr(), ad.data_ptr(), gd.data_ptr(), 1, B, v.shape[1],
        M, C, Q, len(shapes), P, 64, *(o.data_ptr() for o in outs), ops._stream()), "backward_dev")
    _, *ref = _oracle(v, shapes, loc, aw, g)
    _assert_grads(outs, ref, F64, "NaN-initialised outputs")


# 4. gradcheck of the autograd Function
def test_gradcheck_f64(dev):
    from inklayer_amd import ops
    rs = np.random.RandomState(13)
    shapes = [(3, 4), (1, 1), (2, 3)]
    v, loc, aw = _make(rs, 1, 3, 2, 3, shapes, 2, F64, jitter=True)
    ss, ls = _tables(shapes, dev)
    inputs = tuple(t.to(dev).requires_grad_() for t in (v, loc, aw))
    fn = lambda a, b, c: ops.ms_deform_attn(a, ss, ls, b, c, 64)
    # grad_value is an atomic sum: its last bits may differ between the two backward passes gradcheck compares
    assert torch.autograd.gradcheck(fn, inputs, eps=1e-6, atol=1e-8, rtol=1e-6, nondet_tol=1e-12)


# 5. model shapes, f32
@pytest.mark.parametrize("B,Q", [(1, 13294), (2, 900)], ids=["encoder", "decoder"])
def test_model_shapes_f32(dev, B, Q):
    from inklayer_amd import ops
    rs = np.random.RandomState(Q)
    shapes = MODEL_LEVELS
    v, loc, aw = _make(rs, B, Q, 8, 32, shapes, 4, F32, jitter=True)
    g = torch.from_numpy(rs.standard_normal((B, Q, 256)).astype(np.float32))
    ss, ls = _tables(shapes, dev)
    vd, ld, ad = v.to(dev), loc.to(dev), aw.to(dev)
    out = ops.ms_deform_attn_forward(vd, ss, ls, ld, ad, 64)
    _assert_forward(out, v, shapes, loc, aw, F32, "model-shape forward", qchunk=1024)
    got = ops.ms_deform_attn_backward(vd, ss, ls, ld, ad, g.to(dev), 64)
    _, *ref = _oracle(v, shapes, loc, aw, g, qchunk=1024)
    _assert_grads(got, ref, F32, f"model-shape backward B={B} Q={Q}")


# 6. im2col_step is validated only
def test_im2col_step(dev):
    from inklayer_amd import ops
    rs = np.random.RandomState(14)
    shapes = LEVELS[:4]
    v, loc, aw = _make(rs, 4, 10, 2, 32, shapes, 4, F32, jitter=True)
    g = torch.from_numpy(rs.standard_normal((4, 10, 64)).astype(np.float32))
    ss, ls = _tables(shapes, dev)
    vd, ld, ad, gd = v.to(dev), loc.to(dev), aw.to(dev), g.to(dev)
    base = ops.ms_deform_attn_forward(vd, ss, ls, ld, ad, 64)
    _, *ref = _oracle(v, shapes, loc, aw, g)
    for step in (1, 2, 4, 64):
        assert torch.equal(ops.ms_deform_attn_forward(vd, ss, ls, ld, ad, step), base), step
        _assert_grads(ops.ms_deform_attn_backward(vd, ss, ls, ld, ad, gd, step), ref, F32, f"step {step}")
    for step in (3, 0):
        with pytest.raises(ValueError):
            ops.ms_deform_attn_forward(vd, ss, ls, ld, ad, step)
        with pytest.raises(ValueError):
            ops.ms_deform_attn_backward(vd, ss, ls, ld, ad, gd, step)
    with pytest.raises(ValueError):      # B = 3, step 2: 3 % 2 != 0
        ops.ms_deform_attn_forward(vd[:3], ss, ls, ld[:3], ad[:3], 2)


def test_rejects_bad_inputs_on_gpu(dev):
    from inklayer_amd import ops
    rs = np.random.RandomState(15)
    shapes = LEVELS[:2]
    v, loc, aw = (t.to(dev) for t in _make(rs, 2, 5, 2, 8, shapes, 2, F32, jitter=True))
    ss, ls = _tables(shapes, dev)
    g = torch.zeros(2, 5, 16, device=dev)
    with pytest.raises(ValueError):      # non-contiguous
        ops.ms_deform_attn_forward(v.transpose(2, 3).contiguous().transpose(2, 3), ss, ls, loc, aw, 64)
    with pytest.raises(ValueError):
        ops.ms_deform_attn_backward(v, ss, ls, loc, aw, torch.zeros(2, 16, 5, device=dev).transpose(1, 2), 64)
    with pytest.raises(ValueError):      # mixed f32 / f64
        ops.ms_deform_attn_backward(v, ss, ls, loc, aw, g.double(), 64)
    with pytest.raises(ValueError):      # int32 tables
        ops.ms_deform_attn_forward(v, ss.int(), ls.int(), loc, aw, 64)
    with pytest.raises(ValueError):      # host tables that do not describe S rows
        ops.ms_deform_attn_forward(v.double(), torch.tensor([[7, 5], [2, 2]]), torch.tensor([0, 35]),
                                   loc.double(), aw.double(), 64)


# 7. no host synchronisation with device tables
def test_no_host_sync_with_device_tables(dev):
    from inklayer_amd import ops
    rs = np.random.RandomState(16)
    shapes = LEVELS[:5]
    v, loc, aw = (t.to(dev) for t in _make(rs, 2, 7, 2, 32, shapes, 4, F32, jitter=True))
    g = torch.randn(2, 7, 64, device=dev)
    ss, ls = _tables(shapes, dev)
    torch.cuda.synchronize()
    prev = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        out = ops.ms_deform_attn_forward(v, ss, ls, loc, aw, 64)
        grads = ops.ms_deform_attn_backward(v, ss, ls, loc, aw, g, 64)
    finally:
        torch.cuda.set_sync_debug_mode(prev)
    assert out.shape == (2, 7, 64) and len(grads) == 3


# 8. drop-in for groundingdino._C
class _MSDeformAttnFunctionStyle(torch.autograd.Function):
    """How GroundingDINO calls its extension (positional arguments, once-differentiable)."""

    @staticmethod
    def forward(ctx, value, shapes, starts, loc, aw, im2col_step):
        from inklayer_amd import ops as _C
        ctx.im2col_step = im2col_step
        out = _C.ms_deform_attn_forward(value, shapes, starts, loc, aw, ctx.im2col_step)
        ctx.save_for_backward(value, shapes, starts, loc, aw)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_output):
        from inklayer_amd import ops as _C
        value, shapes, starts, loc, aw = ctx.saved_tensors
        grad_value, grad_loc, grad_aw = _C.ms_deform_attn_backward(value, shapes, starts, loc, aw, grad_output,
                                                                   ctx.im2col_step)
        return grad_value, None, None, grad_loc, grad_aw, None


class _DeformAttn(torch.nn.Module):
    """A GroundingDINO-style multi-scale deformable attention layer: value / offset / weight / output linears,
    softmax over the L*P samples of a head, 2-d reference points plus offsets normalised by (W, H)."""

    def __init__(self, d=256, M=8, L=4, P=4):
        super().__init__()
        self.M, self.L, self.P = M, L, P
        self.sampling_offsets = torch.nn.Linear(d, M * L * P * 2)
        self.attention_weights = torch.nn.Linear(d, M * L * P)
        self.value_proj = torch.nn.Linear(d, d)
        self.output_proj = torch.nn.Linear(d, d)

    def locations(self, query, ref, shapes_t):
        B, Q, _ = query.shape
        off = self.sampling_offsets(query).view(B, Q, self.M, self.L, self.P, 2)
        norm = torch.stack([shapes_t[:, 1], shapes_t[:, 0]], -1).to(query.dtype)
        return ref[:, :, None, None, None, :] + off / norm[None, None, None, :, None, :]

    def forward(self, query, ref, value_in, shapes_t, core):
        B, Q, D = query.shape
        value = self.value_proj(value_in).view(B, value_in.shape[1], self.M, D // self.M)
        aw = self.attention_weights(query).view(B, Q, self.M, self.L * self.P).softmax(-1)
        out = core(value, self.locations(query, ref, shapes_t), aw.view(B, Q, self.M, self.L, self.P))
        return self.output_proj(out)


def test_groundingdino_style_dropin(dev):
    import copy
    from oracle import gdino_ref
    torch.manual_seed(17)
    shapes = [(32, 32), (16, 16), (8, 8), (4, 4)]
    B, Q, S, D = 2, 900, sum(h * w for h, w in shapes), 256
    mod = _DeformAttn()
    with torch.no_grad():
        mod.sampling_offsets.weight.normal_(0, 0.02)
        mod.sampling_offsets.bias.uniform_(-2, 2)
    ref64 = copy.deepcopy(mod).double()
    query = torch.randn(B, Q, D)
    value_in = torch.randn(B, S, D)
    ss_host = torch.tensor(shapes)
    # reference points drawn again for every query with a sample within 1e-3 px of a grid line (the oracle's
    # gradient jumps there, and the f32 and f64 locations differ by ~1e-5 px)
    ref = torch.rand(B, Q, 2) * 0.9 + 0.05
    for _ in range(200):
        with torch.no_grad():
            loc = ref64.locations(query.double(), ref.double(), ss_host)
        u = torch.stack([loc[..., l, :, 0] * w for l, (h, w) in enumerate(shapes)] +
                        [loc[..., l, :, 1] * h for l, (h, w) in enumerate(shapes)], -1) - 0.5
        bad = ((u - u.round()).abs() < 1e-3).flatten(2).any(-1)
        if not bad.any():
            break
        ref[bad] = torch.rand(int(bad.sum()), 2) * 0.9 + 0.05
    assert not bad.any()
    g = torch.randn(B, Q, D)

    modg = copy.deepcopy(mod).to(dev)
    ss, ls = _tables(shapes, dev)
    core = lambda v, l, a: _MSDeformAttnFunctionStyle.apply(v, ss, ls, l, a, 64)
    out = modg(query.to(dev), ref.to(dev), value_in.to(dev), ss, core)
    out.backward(g.to(dev))

    core64 = lambda v, l, a: gdino_ref.msda_core(v, shapes, l, a)
    out64 = ref64(query.double(), ref.double(), value_in.double(), ss_host, core64)
    out64.backward(g.double())
    _assert_grad(out.detach(), out64.detach(), F32, "module output")
    for (name, p), p64 in zip(modg.named_parameters(), ref64.parameters()):
        _assert_grad(p.grad, p64.grad, F32, f"d loss / d {name}")
