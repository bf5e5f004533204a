"""Times SamAutomaticMaskGenerator (inklayer_amd/amg.py) on one 1024 x 1024 synthetic sketch with the full-depth ViT-H
engine (seeded weights) and the reference's default settings (32 x 32 points, 16 batches of 64):

  * per batch, HIP events, medians over --iters repetitions after --warmup, A / B interleaved in one process:
    decode_prompts alone; the new tail (device IoU filter + ops.sam_amg_stats + the table copy + ops.mask_rle, i.e.
    SamAutomaticMaskGenerator._process_low_res); and the yardstick, the REFERENCE's tail written with torch ops on the
    same device: ops.sam_postprocess(want_logits=True) for the 192 full-resolution f32 logit images, then
    tests/amg_ref.py's filters, calculate_stability_score, threshold, batched_mask_to_box and mask_to_rle on device
    tensors.  Peak device memory of both (torch.cuda.max_memory_allocated);
  * whole generate() wall time of the new path and of amg_ref driven by SamPredictor.predict_torch(return_logits=True);
  * --trace-only: a few calls of the tail and of ops.sam_postprocess (byte masks only, postprocess_rows_kernel: the
    yardstick of the stats kernel) without any timing loop, for `rocprofv3 --kernel-trace --stats`.

Seeded weights predict IoUs around -0.4 and noise-like masks, which the default thresholds (0.88 / 0.95) reject to the
last candidate, so a timing on them would time an empty tail.  The per-batch tail is therefore timed on hand-made logits
(one steep or shallow cone per mask, the data of tests/test_amg_gpu.py::test_tail_seam_exact scaled to this frame:
about 70 % pass the IoU filter, a quarter of those fail the stability filter), and generate() runs with both
thresholds at the medians of the first batch, so that about half of the candidates pass each filter.

    python tools/amg_time.py [--iters 20] [--warmup 3] [--depth 32] [--trace-only]
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
import amg_ref  # noqa: E402
from inklayer_amd import amg, ops, sam, synthetic  # noqa: E402
from oracle import sam_ref  # noqa: E402

IOU_BIAS = "mask_decoder.iou_prediction_head.layers.2.bias"


def blob_batch(seed, n_side=8):
    """64 points x 3 masks: one cone per mask, radii R, 1.08 R, 1.16 R, slope 8 (stable) or 0.6 (unstable) per low-res
    pixel, IoU predictions uniform in 0.83 .. 1.0"""
    rs = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:256, 0:256].astype(np.float32)
    low = np.empty((64, 3, 256, 256), dtype=np.float32)
    for p in range(64):
        cy = (p // 8 + 0.5) / 8 * 256 + rs.uniform(-2, 2)
        cx = (p % 8 + 0.5) / 8 * 256 + rs.uniform(-2, 2)
        rad = rs.uniform(8, 14)
        for m in range(3):
            k = 8.0 if rs.uniform() < 0.8 else 0.6
            r = np.sqrt((yy - cy) ** 2 + (xx - cx) ** 2)
            low[p, m] = np.clip(k * (rad * (1.0, 1.08, 1.16)[m] - r), -8, 8)
    iou = (0.88 + rs.uniform(-0.05, 0.12, (64, 3))).astype(np.float32)
    return torch.from_numpy(low), torch.from_numpy(iou), amg_ref.build_point_grid(n_side) * 1024.0


def _event_ms(fn):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0.record()
    out = fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1), out


def _line(name, xs):
    xs = sorted(xs)
    q = statistics.quantiles(xs, n=4) if len(xs) >= 4 else [xs[0], xs[len(xs) // 2], xs[-1]]
    return (f"  {name:34s} median {statistics.median(xs):9.3f} ms   quartiles {q[0]:9.3f} .. {q[2]:9.3f}   "
            f"min {xs[0]:9.3f}  max {xs[-1]:9.3f}")


@torch.no_grad()
def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--depth", type=int, default=32)
    ap.add_argument("--trace-only", action="store_true")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    if a.depth == 32:
        oc, cfg = sam_ref.SamConfig(), sam.SamConfig()
    else:
        gi = tuple(range(1, a.depth, 2))
        oc, cfg = sam_ref.SamConfig(depth=a.depth, global_attn_indexes=gi), sam.SamConfig(depth=a.depth, global_attn_indexes=gi)
    sd = sam_ref.seeded_state_dict(sam_ref.sam_param_shapes(oc), 11)
    sd[IOU_BIAS] = sd[IOU_BIAS] + 1.0          # predictions around 0.6 instead of -0.4: a positive median threshold
    eng = sam.SamEngine(sd, cfg, dev, max_batch=1)
    pred = sam.SamPredictor(eng)
    image = synthetic.synthetic_sketch(4, 1024, 1024)
    hw, box = (1024, 1024), [0, 0, 1024, 1024]
    low, iou, points = blob_batch(40)
    low, iou = low.to(dev), iou.to(dev)
    gen = amg.SamAutomaticMaskGenerator(pred, output_mode="uncompressed_rle")
    ref = amg_ref.AmgRef(pred, output_mode="uncompressed_rle")

    def new_tail():
        return gen._process_low_res(low, iou, points, hw, box, hw)

    def torch_tail():
        logits = ops.sam_postprocess(low.reshape(192, 256, 256), 1024, hw, hw, 0.0, want_logits=True)[1]
        return ref.process_logits(logits.reshape(64, 3, *hw), iou, points, box, hw)

    def byte_masks():
        return ops.sam_postprocess(low.reshape(192, 256, 256), 1024, hw, hw, 0.0)

    a_part, b_part = new_tail(), torch_tail()
    assert a_part["rles"] == b_part["rles"] and torch.equal(a_part["boxes"], b_part["boxes"].cpu())
    if a.trace_only:
        for _ in range(5):
            new_tail()
            byte_masks()
        gen._nms(torch.cat([a_part["boxes"]] * 20).float(), torch.cat([a_part["iou_preds"]] * 20), 0.7)
        torch.cuda.synchronize()
        return
    print(f"device: {torch.cuda.get_device_name(0)}; ViT-H depth {a.depth}, seeded weights; 1024 x 1024 sketch; "
          f"{a.iters} timed repetitions after {a.warmup} warm-up, interleaved in one process")
    pred.set_image(image)
    emb = pred.features.reshape(1, eng.T, -1)
    tp = torch.as_tensor(pred.transform.apply_coords(points, hw), dtype=torch.float, device=dev)[:, None, :]
    lab = torch.ones(64, 1, dtype=torch.int, device=dev)

    def decode():
        return eng.decode_prompts(emb, [0] * 64, tp, lab, multimask_output=True)

    calls = {"decode_prompts (64 points, 3 masks)": decode, "new tail (_process_low_res)": new_tail,
             "torch composition of the reference": torch_tail, "sam_postprocess, byte masks only": byte_masks}
    times = {k: [] for k in calls}
    for it in range(a.warmup + a.iters):
        for k, fn in calls.items():
            ms, _ = _event_ms(fn)
            if it >= a.warmup:
                times[k].append(ms)
    print(f"per batch of 64 points (192 candidates; {len(a_part['rles'])} pass the three filters of the tail):")
    for k in calls:
        print(_line(k, times[k]))
    new, old = times["new tail (_process_low_res)"], times["torch composition of the reference"]
    print(f"  ratio of medians torch composition / new tail: {statistics.median(old) / statistics.median(new):.1f}x; "
          f"slowest new {max(new):.3f} ms, fastest composition {min(old):.3f} ms")
    for k in ("new tail (_process_low_res)", "torch composition of the reference"):
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        calls[k]()
        torch.cuda.synchronize()
        print(f"  peak device memory above the resident {base / 2**20:.0f} MiB, {k}: "
              f"{(torch.cuda.max_memory_allocated() - base) / 2**20:.1f} MiB")
    # generate(): thresholds at the medians of the first batch
    m, i, _ = pred.predict_torch(tp, lab, multimask_output=True, return_logits=True)
    t_iou = float(i.median())
    t_stab = float(amg_ref.calculate_stability_score(m.flatten(0, 1), 0.0, 1.0).median())
    del m
    pred.reset_image()
    kw = dict(pred_iou_thresh=t_iou, stability_score_thresh=t_stab, output_mode="uncompressed_rle")
    g_new, g_ref = amg.SamAutomaticMaskGenerator(pred, **kw), amg_ref.AmgRef(pred, **kw)
    wall = {"new": [], "amg_ref + predict_torch": []}
    for it in range(1 + 3):
        for k, g in (("new", g_new), ("amg_ref + predict_torch", g_ref)):
            torch.cuda.synchronize()
            t = time.perf_counter()
            recs = g.generate(image)
            torch.cuda.synchronize()
            if it:
                wall[k].append((time.perf_counter() - t) * 1e3)
            n_rec = len(recs)
    print(f"generate(), 32 x 32 points, thresholds {t_iou:.4f} / {t_stab:.4f} (medians of the first batch), "
          f"{n_rec} records, wall time of 3 runs after 1 warm-up:")
    for k, v in wall.items():
        print(f"  {k:34s} median {statistics.median(v):9.1f} ms   min {min(v):9.1f}  max {max(v):9.1f}")


if __name__ == "__main__":
    main()
