"""Times the device-table MSDA forward and backward (f32, ops.ms_deform_attn_forward / _backward) at the GroundingDINO
encoder shape (batch 8, S = Q = 13294 tokens over 100², 50², 25², 13², M = 8, C = 32, L = P = 4) and the decoder shape
(batch 8, Q = 900), with HIP events after a warm-up.  Reports per call: µs; the bytes the backward adds into grad_value
(in-range corners only, and the all-corners figure the sizing uses) ÷ time against the ≈1.3 TB/s chip-wide rate of
global float atomics; and the same forward + backward through torch's F.grid_sample autograd as a yardstick.

    python tools/msda_time.py [--iters 50] [--warmup 5]
"""
import argparse
import sys
from pathlib import Path

import torch
import torch.nn.functional as F

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from inklayer_amd import ops  # noqa: E402

SHAPES = [(100, 100), (50, 50), (25, 25), (13, 13)]
ATOMIC_RATE = 1.3e12


def _time(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(iters):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) * 1e3 / iters


def _grid_sample_msda(value, shapes, loc, aw):
    """MSDA as one F.grid_sample per level (align_corners=False, zero padding: the oracle's semantics)."""
    B, S, M, C = value.shape
    _, Q, _, L, P, _ = loc.shape
    out = 0
    start = 0
    for l, (H, W) in enumerate(shapes):
        v = value[:, start:start + H * W].permute(0, 2, 3, 1).reshape(B * M, C, H, W)
        grid = (2 * loc[:, :, :, l] - 1).permute(0, 2, 1, 3, 4).reshape(B * M, Q, P, 2)
        s = F.grid_sample(v, grid, mode="bilinear", padding_mode="zeros", align_corners=False)     # [B*M, C, Q, P]
        w = aw[:, :, :, l].permute(0, 2, 1, 3).reshape(B * M, 1, Q, P)
        out = out + (s * w).sum(-1)
        start += H * W
    return out.view(B, M, C, Q).permute(0, 3, 1, 2).reshape(B, Q, M * C)


def _in_range_corners(loc, shapes):
    """Number of (sample, corner) pairs that land inside the map: each adds one C-channel row into grad_value."""
    n = 0
    for l, (H, W) in enumerate(shapes):
        x = loc[:, :, :, l, :, 0] * W - 0.5
        y = loc[:, :, :, l, :, 1] * H - 0.5
        inside = (x > -1) & (y > -1) & (x < W) & (y < H)
        x0, y0 = torch.floor(x), torch.floor(y)
        for dy in (0, 1):
            for dx in (0, 1):
                yy, xx = y0 + dy, x0 + dx
                n += int((inside & (yy >= 0) & (yy < H) & (xx >= 0) & (xx < W)).sum())
    return n


def run(name, B, Q, iters, warmup, dev):
    g = torch.Generator(device=dev).manual_seed(0)
    M, C, L, P = 8, 32, 4, 4
    S = sum(h * w for h, w in SHAPES)
    value = torch.randn(B, S, M, C, device=dev, generator=g)
    # reference point + small offsets, as the encoder samples: mostly inside, some past the border
    ref = torch.rand(B, Q, 1, 1, 1, 2, device=dev, generator=g)
    loc = (ref + 0.05 * torch.randn(B, Q, M, L, P, 2, device=dev, generator=g)).contiguous()
    aw = torch.rand(B, Q, M, L * P, device=dev, generator=g).softmax(-1).view(B, Q, M, L, P).contiguous()
    gout = torch.randn(B, Q, M * C, device=dev, generator=g)
    ss = torch.tensor(SHAPES, dtype=torch.int64, device=dev)
    ls = torch.tensor([0, 10000, 12500, 13125], dtype=torch.int64, device=dev)

    t_fwd = _time(lambda: ops.ms_deform_attn_forward(value, ss, ls, loc, aw, 64), iters, warmup)
    t_bwd = _time(lambda: ops.ms_deform_attn_backward(value, ss, ls, loc, aw, gout, 64), iters, warmup)
    used = _in_range_corners(loc, SHAPES) * C * 4
    nominal = B * Q * M * L * P * 4 * C * 4

    vr, lr, ar = (t.clone().requires_grad_() for t in (value, loc, aw))

    def gs_step():
        out = _grid_sample_msda(vr, SHAPES, lr, ar)
        torch.autograd.grad(out, (vr, lr, ar), gout)

    def gs_fwd():
        with torch.no_grad():
            _grid_sample_msda(value, SHAPES, loc, aw)

    t_gs = _time(gs_step, max(3, iters // 5), 2)
    t_gs_fwd = _time(gs_fwd, max(3, iters // 5), 2)
    floor_used, floor_nominal = used / ATOMIC_RATE * 1e6, nominal / ATOMIC_RATE * 1e6
    print(f"{name}: B={B} S={S} Q={Q} M={M} C={C} L={L} P={P} f32")
    print(f"  forward  {t_fwd:9.1f} us   (grid_sample forward {t_gs_fwd:9.1f} us)")
    print(f"  backward {t_bwd:9.1f} us   grad_value atomics {used / 1e9:.3f} GB in-range "
          f"({nominal / 1e9:.3f} GB all corners) -> {used / t_bwd / 1e6:.3f} TB/s = "
          f"{used / t_bwd / 1e6 / (ATOMIC_RATE / 1e12):.2f} of 1.3 TB/s; floor {floor_used:.1f} us "
          f"({floor_nominal:.1f} us all corners)")
    print(f"  fwd+bwd  {t_fwd + t_bwd:9.1f} us   grid_sample autograd fwd+bwd {t_gs:9.1f} us -> "
          f"{t_gs / (t_fwd + t_bwd):.1f}x")
    return dict(fwd=t_fwd, bwd=t_bwd, gs=t_gs)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    print(f"device: {torch.cuda.get_device_name(dev)}; {a.iters} timed calls after {a.warmup} warm-up calls")
    run("encoder", 8, 13294, a.iters, a.warmup, dev)
    run("decoder", 8, 900, a.iters, a.warmup, dev)


if __name__ == "__main__":
    main()
