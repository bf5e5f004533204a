"""Times one SAM mask decode (prompt encoder + mask decoder, low-res logits and IoU; SamEngine.decode_low_res /
decode_prompts) on one image embedding at 16 and 64 prompts, with HIP events after a warm-up, for four calls:
box prompts with a single mask (InkLayer's path), box prompts with multimask output, 4 points with multimask output,
and a box plus a mask input.  ViT-H decoder dimensions with seeded weights (the decoder does not depend on the encoder
depth, so a 2-block encoder keeps the set-up short).  Prints µs per decode and the ratio to the single-mask call.

    python tools/sam_prompt_time.py [--iters 30] [--warmup 5] [--prompts 16 64]
"""
import argparse
import sys
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from inklayer_amd import sam  # noqa: E402
from oracle import sam_ref  # noqa: E402


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


@torch.no_grad()
def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--prompts", type=int, nargs="+", default=[16, 64])
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    oc = sam_ref.SamConfig(depth=2, global_attn_indexes=(1,))
    sd = sam_ref.seeded_state_dict(sam_ref.sam_param_shapes(oc), 3)
    eng = sam.SamEngine(sd, sam.SamConfig(depth=2, global_attn_indexes=(1,)), dev)
    rs = np.random.RandomState(0)
    emb = torch.from_numpy(rs.standard_normal((1, 4096, 256)).astype(np.float32)).to(dev)
    print(f"device: {torch.cuda.get_device_name(0)}; {a.iters} timed decodes after {a.warmup} warm-up decodes; "
          f"1 image, ViT-H decoder (E = 256, 2 layers, 8 heads)")
    for P in a.prompts:
        xy = rs.uniform(0, 900, (P, 2))
        boxes = torch.from_numpy(np.concatenate([xy, xy + rs.uniform(20, 120, (P, 2))], 1).astype(np.float32))
        pts = torch.from_numpy(rs.uniform(0, 1000, (P, 4, 2)).astype(np.float32))
        lab = torch.from_numpy(rs.randint(0, 2, (P, 4)).astype(np.int32))
        img = [0] * P
        prev, _ = eng.decode_prompts(emb, img, None, None, boxes)
        mask = prev.contiguous()                                      # [P, 1, 256, 256]: a previous call's logits
        calls = [
            ("box, single mask", lambda: eng.decode_low_res(emb, boxes, img)),
            ("box, multimask", lambda: eng.decode_prompts(emb, img, None, None, boxes, multimask_output=True)),
            ("4 points, multimask", lambda: eng.decode_prompts(emb, img, pts, lab, multimask_output=True)),
            ("box + mask_input", lambda: eng.decode_prompts(emb, img, None, None, boxes, mask)),
        ]
        base = None
        print(f"{P} prompts:")
        for name, fn in calls:
            us = _time(fn, a.iters, a.warmup)
            base = base or us
            print(f"  {name:22s} {us:9.1f} us per decode  {us / P:7.2f} us per prompt  {us / base:5.2f}x")


if __name__ == "__main__":
    main()
