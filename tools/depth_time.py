"""Times the DPT head's 3x3 convolutions and batched depth inference on the GPU (it fails without one).

  convolutions   every 3x3 convolution shape of the ViT-S / ViT-B / ViT-L heads at a 518 x 518 input (37 x 37 patches),
                 with the epilogue the engine uses: ops.conv3x3 (the direct kernel) against ops.im2col3x3 + ops.gemm
                 (the pair it replaces) on the same seeded operands.  The two are ALTERNATED call by call in one process
                 after --warmup calls of each, every call between two HIP events; one pass gives the median of --iters
                 calls of each, and the whole alternation is repeated --reps times: the report shows the lowest and the
                 highest pass median (the spread) and calls a shape slower on the kernel only when its LOWEST pass median
                 is above the pair's HIGHEST.  Their outputs are compared before anything is timed.  Next to the times:
                 the bytes each form has to move, from the shapes (input, weights, output, residual; for the pair the
                 im2col matrix written once and read once on top).
  inference      DepthEngine on random weights per model at B = 1 and B = 8 equal-size 750 x 750 sketches: patchify,
                 encode, head (with the final resize) and the total, per image, medians of --reps runs between HIP events.

    python tools/depth_time.py [--iters 20] [--warmup 5] [--reps 5] [--out profiles/depth_conv_times.txt]
"""
import argparse
import statistics
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
from inklayer_amd import depth, ops, synthetic, weights_init  # noqa: E402

F16, F32 = torch.float16, torch.float32
PH = PW = 37


def conv_shapes(cfg):
    """(name, H, W, C, N, stride, relu_in, bias, act, residual, f16 out) of every 3x3 convolution of the model's head
    (DepthEngine.head_batch) at PH x PW patches; one row per distinct shape and form."""
    Fe, ocp = cfg.features, [depth.pad_channels(c) for c in cfg.out_channels]
    s3 = (PH - 1) // 2 + 1
    sizes = [4 * PH, 2 * PH, PH, s3]
    rows = [("resize_layers.3", PH, PW, ocp[3], ocp[3], 2, False, True, None, False, True)]
    rows += [(f"layer{i + 1}_rn", sizes[i], sizes[i], ocp[i], Fe, 1, False, False, None, False, False) for i in range(4)]
    for r, s in ((4, s3), (3, PH), (2, 2 * PH), (1, 4 * PH)):
        rows.append((f"refinenet{r} RCU conv1", s, s, Fe, Fe, 1, True, True, "relu", False, True))
        rows.append((f"refinenet{r} RCU conv2", s, s, Fe, Fe, 1, False, True, None, True, False))
    rows.append(("output_conv1", 8 * PH, 8 * PW, Fe, Fe // 2, 1, False, True, None, False, False))
    rows.append(("output_conv2.0", 14 * PH, 14 * PW, Fe // 2, 32, 1, False, True, "relu", False, True))
    return rows


def time_pair(fa, fb, warmup, iters, reps):
    """Pass medians (us) of fa and fb, alternated call by call: ([reps], [reps])."""
    for _ in range(warmup):
        fa()
        fb()
    ma, mb = [], []
    for _ in range(reps):
        ev = [[torch.cuda.Event(enable_timing=True) for _ in range(4)] for _ in range(iters)]
        torch.cuda.synchronize()
        for e in ev:
            e[0].record()
            fa()
            e[1].record()
            e[2].record()
            fb()
            e[3].record()
        torch.cuda.synchronize()
        ma.append(statistics.median(e[0].elapsed_time(e[1]) for e in ev) * 1e3)
        mb.append(statistics.median(e[2].elapsed_time(e[3]) for e in ev) * 1e3)
    return ma, mb


def measure_convs(a, dev):
    lines = [f"{'model':5s} {'convolution':22s} {'H x W':>9s} {'C':>5s} {'N':>4s} {'s':>1s} | {'direct us (min..max)':>22s} "
             f"{'im2col+GEMM us (min..max)':>26s} {'ratio':>6s} | {'direct MB':>9s} {'pair MB':>9s} | {'same bits':>9s} verdict"]
    slower = []
    for name, cfg in depth.DEPTH_CONFIGS.items():
        for (what, H, W, C, N, stride, relu_in, bias, act, res, f16) in conv_shapes(cfg):
            g = torch.Generator(device=dev).manual_seed(7)
            OH, OW = (H - 1) // stride + 1, (W - 1) // stride + 1
            M, K = OH * OW, 9 * C
            x = torch.randn(H * W, C, generator=g, device=dev).half()
            w = (torch.randn(N, K, generator=g, device=dev) / K ** 0.5).half()
            b = 0.1 * torch.randn(N, generator=g, device=dev) if bias else None
            r = torch.randn(M, N, generator=g, device=dev) if res else None
            od = F16 if f16 else F32
            out_a, out_b = torch.empty((M, N), device=dev, dtype=od), torch.empty((M, N), device=dev, dtype=od)

            def direct():
                ops.conv3x3(x, 1, H, W, w, b, stride=stride, relu_in=relu_in, act=act, residual=r, out=out_a)

            def pair():
                ops.gemm(ops.im2col3x3(x, 1, H, W, stride=stride, relu=relu_in), w, b, act=act, residual=r, out=out_b)

            direct()
            pair()
            torch.cuda.synchronize()
            same = torch.equal(out_a, out_b)
            worst = (out_a.double() - out_b.double()).abs().max().item()
            ma, mb = time_pair(direct, pair, a.warmup, a.iters, a.reps)
            esz = 2 if f16 else 4
            common = H * W * C * 2 + N * K * 2 + M * N * esz + (M * N * 4 if res else 0)
            verdict = "kernel"
            if min(ma) > max(mb):
                verdict = "SLOWER on the kernel: stays on the pair"
                slower.append((name, what, (C, N, stride, relu_in), M, statistics.median(ma), statistics.median(mb)))
            lines.append(f"{name:5s} {what:22s} {H:4d}x{W:<4d} {C:5d} {N:4d} {stride:1d} | {min(ma):10.1f}..{max(ma):<10.1f} "
                         f"{min(mb):12.1f}..{max(mb):<12.1f} {statistics.median(ma) / statistics.median(mb):6.2f} | "
                         f"{common / 1e6:9.1f} {(common + 2 * M * K * 2) / 1e6:9.1f} | "
                         f"{'yes' if same else f'{worst:.1e}':>9s} {verdict}")
            del x, w, b, r, out_a, out_b
            torch.cuda.empty_cache()
    lines.append("")
    if slower:
        lines.append("slower on the direct kernel beyond the spread, as depth.CONV_ON_PAIR holds them: (C, N, stride, relu_in) "
                     "at M rows, median us direct / pair")
        lines += [f"  {n} {wh}: {key} at {M} rows  {da:.1f} / {pa:.1f}  "
                  f"{'(in CONV_ON_PAIR)' if depth.CONV_ON_PAIR.get(key, 0) >= M else '(NOT in CONV_ON_PAIR)'}"
                  for n, wh, key, M, da, pa in slower]
    else:
        lines.append("no shape is slower on the direct kernel beyond the spread")
    return lines


def stage_ms(eng, imgs, reps):
    """Medians (ms) of patchify, encode, head + final resize and the total for one batch of equal-size images."""
    cfg = eng.cfg
    B = len(imgs)
    h, w_ = int(imgs[0].shape[0]), int(imgs[0].shape[1])
    nh, nw = depth.resize_shape(h, w_, cfg.input_size, cfg.patch_size)
    ph, pw = nh // cfg.patch_size, nw // cfg.patch_size
    ts = []
    for rep in range(reps + 1):                                  # the first pass is the warm-up
        e = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
        torch.cuda.synchronize()
        e[0].record()
        pts = [ops.depth_patchify(im, nh, nw, cfg.patch_size, eng.KP, cfg.pixel_mean, cfg.pixel_std, chan_reverse=True)
               for im in imgs]
        e[1].record()
        feats = eng.encode(pts, ph, pw)
        e[2].record()
        d = eng.head_batch(feats, B, ph, pw)
        ops.resize_bilinear_ac(d.reshape(B * nh * nw, 1).contiguous(), B, nh, nw, h, w_)
        e[3].record()
        torch.cuda.synchronize()
        if rep:
            ts.append([e[i].elapsed_time(e[i + 1]) for i in range(3)] + [e[0].elapsed_time(e[3])])
        del pts, feats, d
    return [statistics.median(t[i] for t in ts) for i in range(4)]


def measure_inference(a, dev):
    lines = [f"infer_images on random weights, 750 x 750 sketches -> 518 x 518 (37 x 37 patches); ms PER IMAGE, medians of "
             f"{a.reps} runs after one warm-up run",
             f"{'model':5s} {'B':>2s} {'patchify':>9s} {'encode':>9s} {'head':>9s} {'total':>9s}"]
    imgs = [torch.from_numpy(np.ascontiguousarray(synthetic.synthetic_sketch(s, 750, 750)[..., ::-1])).to(dev) for s in range(8)]
    for name in depth.DEPTH_CONFIGS:
        cfg = depth.config_for(name)
        eng = depth.DepthEngine(weights_init.random_depth_state_dict(cfg, dev), cfg, dev)
        ref = eng.infer_image(imgs[0])
        assert torch.equal(eng.infer_images(imgs[:2])[0], ref)
        for B in (1, 8):
            t = stage_ms(eng, imgs[:B], a.reps)
            lines.append(f"{name:5s} {B:2d} " + " ".join(f"{x / B:9.3f}" for x in t))
        del eng
        torch.cuda.empty_cache()
    return lines


@torch.no_grad()
def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "depth_conv_times.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("tools/depth_time.py measures on the GPU: no device found")
    dev = torch.device("cuda:0")
    lines = [f"DPT head 3x3 convolutions and batched depth inference on one {torch.cuda.get_device_name(0)}",
             f"convolutions: B = 1; direct = ops.conv3x3, pair = ops.im2col3x3 + ops.gemm, alternated call by call; each "
             f"figure is the median of {a.iters} calls between two HIP events (wrapper and the pair's matrix allocation "
             f"included), lowest..highest over {a.reps} passes; ratio = direct / pair (medians of the pass medians); MB = "
             "bytes the form has to move, from the shapes", ""]
    lines += measure_convs(a, dev) + [""] + measure_inference(a, dev)
    text = "\n".join(lines) + "\n"
    print(text, end="")
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(text)


if __name__ == "__main__":
    main()
