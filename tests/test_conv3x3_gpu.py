"""ops.conv3x3 (ink_conv3x3_f16, the direct 3x3 convolution of the DPT head) against the float64 statement in
tests/conv3x3_ref.py: every output element within the project's bound for the 16x16x32 MFMA GEMM at K = 9 C, at the
shapes of conv3x3_ref.CASES, each with the epilogue the engine uses.  The output is a view of a NaN-filled buffer with
64 guard rows; the input map is a view inside a NaN-filled buffer with at least (W + 2) C guard elements on both sides,
so that a padding tap read from memory instead of the zero row poisons its output without leaving the allocation.  The
named mistakes are re-checked on the full data (tests/test_depth_models_cpu.py shows the same on the CPU).  GPU box only."""
import pytest
import torch

import conv3x3_ref as R

pytestmark = pytest.mark.gpu

NAN = float("nan")
GUARD_ROWS = 64


def _run(dev, c, d):
    """ops.conv3x3 on the case's operands -> the whole NaN-prefilled output buffer [M + 64, N]."""
    from inklayer_amd import ops
    n = c.B * c.H * c.W * c.C
    guard = (c.W + 2) * c.C                                  # a multiple of 32 elements: the view stays 16-byte aligned
    buf = torch.full((guard + n + guard,), NAN, dtype=R.F16, device=dev)
    x = buf[guard:guard + n].view(-1, c.C)
    x.copy_(d["x"])
    assert x.data_ptr() % 16 == 0
    M = R.rows(c)
    out = torch.full((M + GUARD_ROWS, c.N), NAN, dtype=R.F16 if c.f16 else R.F32, device=dev)
    gpu = lambda t: None if t is None else t.to(dev)         # noqa: E731
    got = ops.conv3x3(x, c.B, c.H, c.W, gpu(d["w"]), gpu(d["b"]), stride=c.stride, relu_in=c.relu_in, act=c.act,
                      residual=gpu(d["r"]), out=out[:M])
    assert got.data_ptr() == out.data_ptr()
    torch.cuda.synchronize()
    assert torch.isnan(buf[:guard]).all() and torch.isnan(buf[guard + n:]).all()
    return out


@torch.no_grad()
@pytest.mark.parametrize("name", list(R.CASES))
def test_conv3x3_matches_float64(dev, name):
    c = R.CASES[name]
    d = R.conv_data(c, torch.Generator().manual_seed(900 + list(R.CASES).index(name)))
    M = R.rows(c)
    buf = _run(dev, c, d).cpu()
    assert torch.isnan(buf[M:]).all(), "guard rows written"
    got = buf[:M].double()
    ref, mag = R.conv_ref(c, d)
    tol = R.conv_tol(c, ref, mag)
    worst = R.assert_within(got, ref, tol, f"conv3x3 {name} {tuple(c)}")
    print(f"  conv3x3 {name}: M = {M}, worst error {worst:.3f}x the bound")
    for what, wrong in R.conv_mistakes(c, d):
        m = R.assert_discriminates(wrong, ref, tol, f"{name}: {what}")
        print(f"    '{what}' lands {m:.0f}x outside")


def test_conv3x3_rejects_bad_arguments(dev):
    """C = 48, stride = 3, a misaligned input and N = 6 return 1 (bad argument) with nothing launched: the output
    keeps its NaN prefill."""
    from inklayer_amd import _lib
    L = _lib.lib()
    B, H, W = 1, 4, 4
    xbuf = torch.zeros(B * H * W * 64 + 8, dtype=R.F16, device=dev)
    w = torch.zeros(8 * 9 * 64, dtype=R.F16, device=dev)
    out = torch.full((B * H * W, 8), NAN, dtype=R.F32, device=dev)

    def call(x=xbuf.data_ptr(), C=64, N=8, stride=1):
        return L.ink_conv3x3_f16(x, B, H, W, C, w.data_ptr(), N, None, stride, 0, 0, None, out.data_ptr(), 0, None)

    assert call(C=48) == 1 and call(stride=3) == 1 and call(stride=0) == 1 and call(N=6) == 1
    assert xbuf.data_ptr() % 16 == 0 and call(x=xbuf.data_ptr() + 8) == 1
    assert call(C=0) == 1 and call(N=0) == 1
    torch.cuda.synchronize()
    assert torch.isnan(out).all()
    assert call() == 0
    torch.cuda.synchronize()
    assert (out == 0).all()
