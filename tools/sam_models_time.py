"""Times the SAM image encoder (SamEngine.encode: patch embedding, all blocks, neck) of the three registry models at
batch 1 and batch 8 with HIP events after a warm-up, full depth, random weights, 1024 x 1024 synthetic sketches.  Every
ViT-L / ViT-B figure is taken right next to a ViT-H figure of the same run (ViT-H, model, ViT-H, model, ... in turn), so
the ratio does not depend on which box of the pool the run landed on.  ViT-B / ViT-L run the templated attention of
csrc/attention.hip (head_dim 64, f32 rel tables); ViT-H its dedicated one-wave-per-SIMD kernels.

    python tools/sam_models_time.py [--iters 10] [--warmup 3] [--rounds 3] [--batches 1 8]
"""
import argparse
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from inklayer_amd import sam, synthetic, weights_init  # noqa: E402


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
    return t0.elapsed_time(t1) / iters


@torch.no_grad()
def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 8])
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    maxb = max(a.batches)
    engines = {}
    for name in ("vit_h", "vit_l", "vit_b"):
        cfg = sam.config_for(name)
        # (the bias correction changes bias values only: off, to keep the set-up short)
        engines[name] = sam.SamEngine(weights_init.random_sam_state_dict(cfg, dev), cfg, dev, max_batch=maxb,
                                      bias_correction=False)
    imgs = [torch.from_numpy(synthetic.synthetic_sketch(i)).to(dev) for i in range(maxb)]
    print(f"device: {torch.cuda.get_device_name(0)}; encoder ms per batch, median of {a.rounds} rounds of {a.iters} "
          f"timed encodes after {a.warmup} warm-up encodes; each model timed in turn with ViT-H")
    print("| model | blocks x width (heads) | B | encoder ms | ms per image | ViT-H ms, same run | ratio to ViT-H |")
    print("|---|---|---|---|---|---|---|")
    med = lambda v: sorted(v)[len(v) // 2]  # noqa: E731
    for B in a.batches:
        run = {n: (lambda e=e: e.encode(imgs[:B])) for n, e in engines.items()}
        rows = {}
        for name in ("vit_l", "vit_b"):
            th, tm = [], []
            for _ in range(a.rounds):
                th.append(_time(run["vit_h"], a.iters, a.warmup))
                tm.append(_time(run[name], a.iters, a.warmup))
            rows[name] = (med(tm), med(th))
        h = 0.5 * (rows["vit_l"][1] + rows["vit_b"][1])
        for name, (tm, th) in (("vit_h", (h, h)), ("vit_l", rows["vit_l"]), ("vit_b", rows["vit_b"])):
            c = engines[name].cfg
            print(f"| {name} | {c.depth} x {c.embed_dim} ({c.num_heads}) | {B} | {tm:.2f} | {tm / B:.2f} | {th:.2f} | "
                  f"{tm / th:.3f} |")


if __name__ == "__main__":
    main()
