"""float64 statement of ink_conv3x3_f16 (the direct 3x3 / pad 1 convolution of the DPT head), its per-element bound, the
cases tests/test_conv3x3_gpu.py runs and the named mistakes the bound has to tell apart.  Shared by that GPU test and
tests/test_depth_models_cpu.py (which shows on the CPU that every mistake lands >= 100x outside the bound).

Two statements of the same convolution: conv_ref_conv2d is torch.nn.functional.conv2d in float64 on the f16-rounded
operands; conv_ref builds the [M, 9, C] tap matrix by index arithmetic, which is what lets a mistake be expressed as a
change of one index or one validity rule.  The CPU test requires the two to agree to float64 rounding."""
from collections import namedtuple

import torch
import torch.nn.functional as F

from vith_ref import F16, F32, F64, H16, SUB16, U, assert_discriminates, assert_within, discrimination  # noqa: F401

# relu_in: ResidualConvUnit's activation(x) in front of the conv; act: None / "relu"; res: f32 residual added after act;
# f16: f16 output rows
Case = namedtuple("Case", "B H W C N stride relu_in bias act res f16")
CASES = {
    # only the centre tap / a 2x2 block of taps is valid; one ragged tile
    "centre_only": Case(3, 1, 1, 32, 32, 1, False, False, None, False, False),
    "taps_2x2": Case(1, 2, 2, 64, 64, 1, False, False, None, False, False),
    # BK = 32, one K-tile per tap, M = 70 < 128, N < 128, the image boundary inside the tile: bias + ReLU, f16 out
    "bk32": Case(2, 5, 7, 32, 32, 1, False, True, "relu", False, True),
    # three K-tiles (of 32) per tap; ResidualConvUnit conv1: relu_in, bias + ReLU, f16 out
    "rcu_conv1": Case(2, 9, 11, 96, 64, 1, True, True, "relu", False, True),
    # BK = 64; ResidualConvUnit conv2: bias, f32 residual, f32 out - and the layer*_rn form without bias and residual
    "rcu_conv2": Case(2, 9, 11, 64, 64, 1, False, True, None, True, False),
    "layer_rn": Case(2, 9, 11, 64, 64, 1, False, False, None, False, False),
    # stride 2 at odd and even extents (OH x OW = 5x6 and 4x5): resize_layers.3's form, bias and f16 out
    "stride2_odd": Case(2, 9, 11, 128, 128, 2, False, True, None, False, True),
    "stride2_even": Case(1, 8, 10, 64, 32, 2, False, True, None, False, True),
    # 22 M-tiles, ragged last tile, an image boundary in mid-tile: conv1 of a ViT-B ResidualConvUnit
    "many_tiles": Case(2, 37, 37, 128, 128, 1, True, True, "relu", False, True),
    # two N-tiles, K = 2304: conv2 of a ViT-L ResidualConvUnit
    "vitl": Case(1, 19, 23, 256, 256, 1, False, True, None, True, False),
}


def out_hw(c):
    return (c.H - 1) // c.stride + 1, (c.W - 1) // c.stride + 1


def rows(c):
    oh, ow = out_hw(c)
    return c.B * oh * ow


def bk(c):
    """K step of the kernel instance: 64 when C % 64 == 0, else 32."""
    return 64 if c.C % 64 == 0 else 32


def conv_data(c, gen, dev="cpu"):
    """x f16 [B*H*W, C] ~ N(0, 1), w f16 [N, 9*C] ~ N(0, 1 / K) in (ky, kx, c) order, b ~ 0.1 N, r ~ N(0, 1)."""
    K = 9 * c.C
    d = {"x": torch.randn(c.B * c.H * c.W, c.C, generator=gen, device=dev).half(),
         "w": (torch.randn(c.N, K, generator=gen, device=dev) / K ** 0.5).half()}
    d["b"] = 0.1 * torch.randn(c.N, generator=gen, device=dev) if c.bias else None
    d["r"] = torch.randn(rows(c), c.N, generator=gen, device=dev) if c.res else None
    return d


def taps(x64, c, *, flat=False, tall=False, odd=False):
    """[M, 9, C] float64: tap (ky, kx) of every output pixel, zero outside the image.
    Mistakes: flat (no padding: the tap is the flat row neighbour centre + (ky-1) W + (kx-1) of the [B*H*W, C] matrix,
    so it wraps round row ends and images; zero only outside the matrix), tall (the batch is one image of B*H rows),
    odd (stride-2 centres on the odd pixels)."""
    oh, ow = out_hw(c)
    dev = x64.device
    b, oy, ox = torch.meshgrid(torch.arange(c.B, device=dev), torch.arange(oh, device=dev),
                               torch.arange(ow, device=dev), indexing="ij")
    b, iy, ix = b.reshape(-1), oy.reshape(-1) * c.stride + int(odd), ox.reshape(-1) * c.stride + int(odd)
    out = x64.new_zeros(b.numel(), 9, c.C)
    n = c.B * c.H * c.W
    for ky in range(3):
        for kx in range(3):
            yy, xx = iy + ky - 1, ix + kx - 1
            if flat:
                idx = (b * c.H + iy) * c.W + ix + (ky - 1) * c.W + (kx - 1)
                ok = (idx >= 0) & (idx < n)
            else:
                idx = (b * c.H + yy) * c.W + xx
                gy = b * c.H + yy
                ok = (xx >= 0) & (xx < c.W) & ((gy >= 0) & (gy < c.B * c.H) if tall else (yy >= 0) & (yy < c.H))
            out[:, ky * 3 + kx] = x64[idx.clamp(0, n - 1)] * ok[:, None]
    return out


def conv_ref(c, d, *, flat=False, tall=False, odd=False, swap_kykx=False, drop_relu_in=False, relu_after=False,
             skip_last_ktile=False, drop_bias=False, res_times=1):
    """float64 (out, mag): out = res_times * r + act(sum relu_in?(tap) * w + b); mag = sum |tap| |w| + |b| + |r|.
    Mistakes: see taps; swap_kykx (weight taps transposed), drop_relu_in, relu_after (the ReLU applied to the sum of
    products instead of the input), skip_last_ktile (the last bk(c) channels of tap 8 left out), drop_bias, res_times."""
    x64, w64 = d["x"].double(), d["w"].double()
    if c.relu_in and not drop_relu_in and not relu_after:
        x64 = x64.clamp(min=0)
    t = taps(x64, c, flat=flat, tall=tall, odd=odd)
    if skip_last_ktile:
        t[:, 8, c.C - bk(c):] = 0
    if swap_kykx:
        w64 = w64.view(c.N, 3, 3, c.C).transpose(1, 2).reshape(c.N, 9 * c.C)
    t = t.reshape(-1, 9 * c.C)
    lin = t @ w64.t()
    if c.relu_in and relu_after:
        lin = lin.clamp(min=0)
    mag = t.abs() @ w64.abs().t()
    if c.bias:
        mag = mag + d["b"].double().abs()
        if not drop_bias:
            lin = lin + d["b"].double()
    out = lin.clamp(min=0) if c.act == "relu" else lin
    if c.res:
        out = out + res_times * d["r"].double()
        mag = mag + d["r"].double().abs()
    return out, mag


def conv_ref_conv2d(c, d):
    """The same through torch.nn.functional.conv2d in float64 on the f16-rounded operands."""
    x = d["x"].double().view(c.B, c.H, c.W, c.C).permute(0, 3, 1, 2)
    if c.relu_in:
        x = x.clamp(min=0)
    w = d["w"].double().view(c.N, 3, 3, c.C).permute(0, 3, 1, 2)
    y = F.conv2d(x, w, d["b"].double() if c.bias else None, stride=c.stride, padding=1)
    y = y.permute(0, 2, 3, 1).reshape(-1, c.N)
    if c.act == "relu":
        y = y.clamp(min=0)
    return y + d["r"].double() if c.res else y


def conv_tol(c, out, mag):
    """The project's bound for the 16x16x32 MFMA GEMM (depth_ops_ref.gemm_tol) with K = 9 * C: the kernel is that GEMM
    with another A-address generator, K / 32 MFMA steps per output element, the same accumulator (residual preloaded)
    and the same epilogue: (K / 32 + 7) u mag, plus half an f16 ulp for f16 outputs.  The packed max of the input ReLU
    is exact."""
    t = (9 * c.C / 32 + 7) * U * mag
    if c.f16:
        t = t + H16 * out.abs() + SUB16
    return t


def conv_mistakes(c, d):
    """(what, wrong output) of the mistakes that can show on the case's shape and form."""
    out = [("no zero padding (flat neighbours)", conv_ref(c, d, flat=True)[0])]
    if c.B > 1:
        out.append(("batch stacked as one tall image", conv_ref(c, d, tall=True)[0]))
    if c.H > 1 and c.W > 1:          # a 1x1 image has the centre tap only
        out.append(("ky / kx exchanged", conv_ref(c, d, swap_kykx=True)[0]))
        out.append(("last K-tile skipped", conv_ref(c, d, skip_last_ktile=True)[0]))
    if c.relu_in:
        out.append(("input ReLU dropped", conv_ref(c, d, drop_relu_in=True)[0]))
        out.append(("input ReLU applied after the product", conv_ref(c, d, relu_after=True)[0]))
    if c.stride == 2:
        out.append(("stride-2 centres on the odd pixels", conv_ref(c, d, odd=True)[0]))
    if c.bias:
        out.append(("bias dropped", conv_ref(c, d, drop_bias=True)[0]))
    if c.res:
        out.append(("residual dropped", conv_ref(c, d, res_times=0)[0]))
        out.append(("residual added twice", conv_ref(c, d, res_times=2)[0]))
    return out
