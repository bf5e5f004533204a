"""Op-level parity of the SAM / Depth pixel-side kernels against plain float64 references (oracle/sam_ref.py where it
restates the operation): exact equality for data movement, derived bounds elsewhere.  Outputs are pre-filled with NaN.
GPU box only."""
import contextlib

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

F16, F32, F64 = torch.float16, torch.float32, torch.float64
U = 2.0 ** -24
NAN = float("nan")


@contextlib.contextmanager
def _default_dtype(dt):
    old = torch.get_default_dtype()
    torch.set_default_dtype(dt)
    try:
        yield
    finally:
        torch.set_default_dtype(old)


# ---------------------------------------------------------------------------------------------------------------
# sam_patchify
# ---------------------------------------------------------------------------------------------------------------
def _sam_reference(img, L, P, chan_reverse):
    """sam_ref.preprocess in float64 (its mean / std tensors follow the default dtype; the u8 -> f32 cast is exact)
    on the channel-reversed or plain image, unfolded to [tokens, c*P*P + ky*P + kx]."""
    from oracle import sam_ref
    x = torch.from_numpy(np.ascontiguousarray(img[..., ::-1] if chan_reverse else img)).permute(2, 0, 1)
    with _default_dtype(F64):
        r = sam_ref.preprocess(sam_ref.SamConfig(img_size=L, patch_size=P), x)
    assert r.dtype == F64
    g = L // P
    return r.view(3, g, P, g, P).permute(1, 3, 0, 2, 4).reshape(g * g, 3 * P * P)


@torch.no_grad()
@pytest.mark.parametrize("split", [False, True], ids=["plain", "split"])
@pytest.mark.parametrize("chan_reverse", [False, True], ids=["rgb", "bgr"])
@pytest.mark.parametrize("case", [(1024, 16, 1024, 683), (64, 16, 40, 29)], ids=["L1024", "L64"])
def test_sam_patchify(dev, case, chan_reverse, split):
    """Sam.preprocess + the 16x16 patch gather.  Plain: the kernel multiplies by 1/std where the reference divides
    (two more f32 roundings, <= 2^-21 relative together with the subtraction), so it may differ from the float64 value
    rounded to f16 by one f16 ulp, and only where that value lies within 2^-21 relative of the rounding boundary.
    Split: hi + lo/64 is within 2^-21 |ref| + 1e-7 of the float64 value (f32 path 2^-22, f16 rounding of lo
    2^-11 * 2^-11), hs is exactly f16(hi / 64), and the padded area is 0 in all three segments."""
    from inklayer_amd import ops
    from oracle import sam_ref
    L, P, h, w = case
    rs = np.random.RandomState(h + w + int(chan_reverse))
    img = rs.randint(0, 256, (h, w, 3)).astype(np.uint8)
    r64 = _sam_reference(img, L, P, chan_reverse)
    pad = (_sam_reference(np.full((h, w, 3), 7, np.uint8), L, P, False) == 0)      # the zero-padded area
    tol = 2.0 ** -21 * r64.abs() + 1e-7
    m = ((_sam_reference(img, L, P, not chan_reverse) - r64).abs() / tol).max().item()
    assert m >= 100, "the bound cannot see the channel order"
    KP, T = 3 * P * P, (L // P) ** 2
    cfg = sam_ref.SamConfig()
    out = torch.full((T, 3 * KP if split else KP), NAN, dtype=F16, device=dev)
    ops.sam_patchify(torch.from_numpy(img).to(dev), L, P, cfg.pixel_mean, cfg.pixel_std, chan_reverse, out, split=split)
    got = out.cpu()
    hi = got[:, :KP]
    r16 = torch.from_numpy(r64.numpy().astype(np.float16))          # float64 -> f16, one rounding
    if not split:
        diff = hi.view(torch.int16) != r16.view(torch.int16)
        if diff.any():
            a, b = hi[diff].double(), r16[diff].double()
            assert ((a.view(-1).half().view(torch.int16).int() - b.half().view(torch.int16).int()).abs() == 1).all()
            mid = (a + b) / 2
            assert ((r64[diff] - mid).abs() <= 2.0 ** -21 * r64[diff].abs()).all(), "off by one ulp away from a tie"
        assert (hi[pad] == 0).all()
        return
    lo, hs = got[:, KP:2 * KP], got[:, 2 * KP:]
    recon = hi.double() + lo.double() / 64
    err = (recon - r64).abs()
    assert (err <= tol).all(), f"hi + lo/64 off by {err.max().item():.3g}"
    assert torch.equal(hs.view(torch.int16), (hi.float() / 64).half().view(torch.int16))
    for seg in (hi, lo, hs):
        assert (seg[pad] == 0).all()


# ---------------------------------------------------------------------------------------------------------------
# im2col3x3
# ---------------------------------------------------------------------------------------------------------------
def _im2col_reference(x, B, H, W, swap=False):
    """F.unfold(pad 1) rearranged to [(ky*3 + kx)*C + c]; swap: (kx*3 + ky) (a mistake)."""
    import torch.nn.functional as Fn
    C = x.shape[1]
    nchw = x.float().view(B, H, W, C).permute(0, 3, 1, 2)
    u = Fn.unfold(nchw, 3, padding=1).view(B, C, 3, 3, H * W)
    if swap:
        u = u.transpose(2, 3)
    return u.reshape(B, C, 9, H * W).permute(0, 3, 2, 1).reshape(B * H * W, 9 * C).half()


@torch.no_grad()
@pytest.mark.parametrize("C", [8, 256])
@pytest.mark.parametrize("HW", [(64, 64), (5, 3), (1, 1)])
@pytest.mark.parametrize("B", [1, 2])
def test_im2col3x3(dev, B, HW, C):
    """Pure data movement: bit-equal to F.unfold(pad=1) in the [(ky*3+kx)*C + c] column order."""
    from inklayer_amd import ops
    H, W = HW
    rs = np.random.RandomState(B * 1000 + H * 10 + C)
    x = torch.from_numpy(rs.standard_normal((B * H * W, C)).astype(np.float16))
    want = _im2col_reference(x, B, H, W)
    if H > 1:
        assert not torch.equal(_im2col_reference(x, B, H, W, swap=True), want)
    out = torch.full((B * H * W, 9 * C), NAN, dtype=F16, device=dev)
    ops.im2col3x3(x.to(dev), B, H, W, out=out)
    assert torch.equal(out.cpu().view(torch.int16), want.view(torch.int16))


# ---------------------------------------------------------------------------------------------------------------
# sam_pe_encode
# ---------------------------------------------------------------------------------------------------------------
@torch.no_grad()
@pytest.mark.parametrize("n_add", [0, 1, 2])
def test_sam_pe_encode(dev, n_add):
    """[sin, cos](2 pi (2c - 1) @ G) (+ add[n % n_add]) vs sam_ref._pe_encoding in float64.  Bound per element:
    the f32 argument is off by <= 2 u (2 pi (|cx G0| + |cy G1|)) + 2 u |arg| (2c - 1, two products, the sum, the f32 2pi
    and its product), sinf / cosf by <= 2 u and the add by u |out|:  4 u (2 pi (|cx G0| + |cy G1|) + 1) + u |out|,
    i.e. below 2e-6 for |arg| <= 8 and proportionally more for the |arg| ~ 30 a randn matrix reaches."""
    from inklayer_amd import ops
    from oracle import sam_ref
    Fd, N = 128, 4097                                       # N * F = 2049 workgroups of 256: the last one partial
    rs = np.random.RandomState(9 + n_add)
    G = torch.from_numpy(rs.standard_normal((2, Fd)).astype(np.float32))
    c = rs.uniform(0, 1, (N, 2)).astype(np.float32)
    c[:9] = [(0, 0), (0.5, 0.5), (1, 1), (0, 1), (1, 0), (0.5, 0), (0, 0.5), (1, 0.5), (0.5, 1)]
    c = torch.from_numpy(c)
    r = sam_ref._pe_encoding({"prompt_encoder.pe_layer.positional_encoding_gaussian_matrix": G.double()}, c.double())
    add = None
    if n_add:
        add = torch.from_numpy(rs.standard_normal((n_add, 2 * Fd)).astype(np.float32))
        r = r + add.double()[torch.arange(N) % n_add]
    cc = (2 * c.double() - 1).abs()
    arg = 2 * np.pi * (cc[:, :1] * G[0].double().abs() + cc[:, 1:] * G[1].double().abs())
    tol = 4 * U * (torch.cat([arg, arg], 1) + 1) + U * r.abs()
    if n_add == 2:
        wrong = r - add.double()[torch.arange(N) % 2] + add.double()[torch.arange(N) // (N // 2 + 1)]
        assert ((wrong - r).abs() / tol).max() >= 100
    out = torch.full((N, 2 * Fd), NAN, dtype=F32, device=dev)
    ops.sam_pe_encode(c.to(dev), G.to(dev), add=add.to(dev) if add is not None else None, out=out)
    got = out.double().cpu()
    err = (got - r).abs()
    assert (err <= tol).all(), f"{int((~(err <= tol)).sum())} elements out of bound, worst {err.max().item():.3g}"


# ---------------------------------------------------------------------------------------------------------------
# add_f32
# ---------------------------------------------------------------------------------------------------------------
@torch.no_grad()
@pytest.mark.parametrize("period", ["4", "C", "TC"])
def test_add_f32(dev, period):
    """a + b with b periodic in the flat index (the f32 output of the kernel add_cvt_f16 shares): exact, since both
    sides make one correctly rounded f32 addition.  n / 4 = 524800 float4 is past the 2048-workgroup grid-stride wrap."""
    from inklayer_amd import ops
    T, C = 8200, 256
    rs = np.random.RandomState(len(period))
    a = torch.from_numpy(rs.standard_normal((T, C)).astype(np.float32))
    nb = {"4": 4, "C": C, "TC": T * C}[period]
    b = torch.from_numpy(rs.standard_normal(nb).astype(np.float32) * 3)
    want = (a.view(-1, nb) + b).view(T, C)
    out = torch.full((T, C), NAN, device=dev)
    got = ops.add_f32(a.to(dev), b.to(dev), out=out)
    assert got.data_ptr() == out.data_ptr()
    assert torch.equal(out.cpu().view(torch.int32), want.view(torch.int32))


def test_add_f32_rejects_bad_sizes(dev):
    from inklayer_amd import ops
    from inklayer_amd._lib import InkLayerHipError
    with pytest.raises(InkLayerHipError):                 # n % 4 != 0
        ops.add_f32(torch.zeros(10, device=dev), torch.zeros(5, device=dev))
    with pytest.raises(InkLayerHipError):                 # period % 4 != 0
        ops.add_f32(torch.zeros(12, device=dev), torch.zeros(6, device=dev))
    with pytest.raises(AssertionError):                   # period does not divide n
        ops.add_f32(torch.zeros(12, device=dev), torch.zeros(8, device=dev))
    torch.cuda.synchronize()
