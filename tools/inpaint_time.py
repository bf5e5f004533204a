"""Times the pre- and post-processing of the inpainting stage (inklayer_amd/inpaint.py, csrc/inpaint_ops.hip) on one
1024 x 1024 layer, the diffusion pipe excluded, and the numpy restatement tests/inpaint_ref.py on the same host:

  pre    contrast + bilateral, mask dilation + blur, the two Lanczos resizes to 768 x 768, the condition tensor
  again  the Lanczos resize of the first pass's image and its condition tensor (the second pass of ControlNet_inpaint)
  post   Lanczos back to 1024 x 1024, adaptive-threshold clean-up + soft blend, grey round trip + unsharp mask
  whole  controlnet_inpaint() around a pipe that returns its input: the three above plus every host crossing
         (upload of image and mask, PIL images and the CPU condition tensor for two pipe calls, the returned image)

GPU: device-resident tensors, HIP events, median of --iters runs after --warmup; `whole` is wall time.  The results of
both sides are compared before anything is timed.

    python tools/inpaint_time.py [--iters 20] [--warmup 3] [--out profiles/inpaint_times.txt]
"""
import argparse
import statistics
import sys
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
import inpaint_ref as R  # noqa: E402
from inklayer_amd import inpaint  # noqa: E402

SIDE = 1024


class EchoPipe:
    class Out:
        def __init__(self, image):
            self.images = [image]

    def __call__(self, **kw):
        return EchoPipe.Out(kw["image"])


def gpu_pre(rgb, mask):
    image, m = inpaint.preprocess_image(rgb), inpaint.preprocess_mask(mask)
    up, mup = inpaint.resize(image, (768, 768)), inpaint.resize(m, (768, 768))
    return up, mup, inpaint.condition(up, mup)


def gpu_again(result768, mup):
    up = inpaint.resize(result768, (768, 768))
    return up, inpaint.condition(up, mup)


def gpu_post(result768, rgb, mask):
    back = inpaint.resize(result768, (SIDE, SIDE))
    return inpaint.finish(inpaint.postprocess(back, rgb, mask))


def cpu_pre(rgb, mask):
    image, m = R.preprocess_image(rgb), R.mask_prepare(mask)
    up, mup = R.resize(image, 768, 768, "lanczos"), R.resize(m, 768, 768, "lanczos")
    return up, mup, R.condition(up, mup)


def cpu_again(result768, mup):
    up = R.resize(result768, 768, 768, "lanczos")
    return up, R.condition(up, mup)


def cpu_post(result768, rgb, mask):
    return R.finish(R.postprocess(R.resize(result768, SIDE, SIDE, "lanczos"), rgb, mask))


def _event_ms(fn):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0.record()
    out = fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1), out


def _wall_ms(fn):
    t = time.perf_counter()
    out = fn()
    return (time.perf_counter() - t) * 1e3, out


@torch.no_grad()
def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "inpaint_times.txt"))
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    rgb_h, mask_h = R.make_sketch((SIDE, SIDE))
    rgb, mask = torch.from_numpy(rgb_h).to(dev), torch.from_numpy(mask_h).to(dev)

    cpu = {}
    cpu["pre"], (up_h, mup_h, cond_h) = _wall_ms(lambda: cpu_pre(rgb_h, mask_h))
    cpu["again"], _ = _wall_ms(lambda: cpu_again(up_h, mup_h))
    cpu["post"], post_h = _wall_ms(lambda: cpu_post(up_h, rgb_h, mask_h))
    cpu["whole"], whole_h = _wall_ms(lambda: R.controlnet_inpaint(EchoPipe(), rgb_h, mask_h))

    up, mup, cond = gpu_pre(rgb, mask)
    assert np.array_equal(up.cpu().numpy(), up_h) and np.array_equal(mup.cpu().numpy(), mup_h)
    assert np.array_equal(cond.cpu().numpy(), cond_h)
    assert np.array_equal(gpu_post(up, rgb, mask).cpu().numpy(), post_h)
    from PIL import Image
    pil_rgb, pil_mask = Image.fromarray(rgb_h), Image.fromarray(mask_h)
    assert np.array_equal(np.asarray(inpaint.controlnet_inpaint(EchoPipe(), pil_rgb, pil_mask)), whole_h)

    calls = {"pre": lambda: gpu_pre(rgb, mask), "again": lambda: gpu_again(up, mup), "post": lambda: gpu_post(up, rgb, mask)}
    gpu = {k: [] for k in (*calls, "whole")}
    for it in range(a.warmup + a.iters):
        for k, fn in calls.items():
            ms, _ = _event_ms(fn)
            if it >= a.warmup:
                gpu[k].append(ms)
        torch.cuda.synchronize()
        ms, _ = _wall_ms(lambda: inpaint.controlnet_inpaint(EchoPipe(), pil_rgb, pil_mask))
        if it >= a.warmup:
            gpu["whole"].append(ms)

    names = {"pre": "pre-processing (to the first pipe call)", "again": "second pass (resize + condition)",
             "post": "post-processing (after the last pipe call)", "whole": "controlnet_inpaint, echo pipe, host crossings"}
    lines = [
        "inpainting pre- and post-processing per 1024 x 1024 layer (ControlNet_inpaint without the diffusion pipe; results equal)",
        f"GPU: inklayer_amd.inpaint on one {torch.cuda.get_device_name(0)}, median of {a.iters} runs after {a.warmup} warm-up runs "
        "(HIP events; the last row wall time)",
        "CPU: tests/inpaint_ref.py (numpy restatement), one run, same machine's host",
        f"{'step':48s} {'GPU ms':>9s} {'min':>8s} {'max':>8s} {'CPU ms':>9s}",
    ]
    for k in ("pre", "again", "post", "whole"):
        v = gpu[k]
        lines.append(f"{names[k]:48s} {statistics.median(v):9.3f} {min(v):8.3f} {max(v):8.3f} {cpu[k]:9.1f}")
    dev_sum = sum(statistics.median(gpu[k]) for k in ("pre", "again", "post"))
    lines.append(f"{'pre + second pass + post':48s} {dev_sum:9.3f} {'':8s} {'':8s} {cpu['pre'] + cpu['again'] + cpu['post']:9.1f}")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(text)


if __name__ == "__main__":
    main()
