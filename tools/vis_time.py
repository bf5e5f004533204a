"""Times the coloured-sketch kernels (csrc/visualize.hip) on a 1024 x 1024 sketch with 16 masks resident on the GPU, the
host code they replace, and what the change does to the runner's "masks/ + detection visualisations" stage.

  kernels   ink_vis_gray_min and ink_vis_colour (stack form and label form): HIP events around --iters back-to-back
            launches after --warmup, per launch (at this size that is the host's launch rate, not the kernel: the kernel
            times in DESIGN.md come from `rocprofv3 --kernel-trace --stats -- python tools/vis_time.py --kernels-only`);
            next to the bytes each has to move (sketch, the mask bytes its lanes really ask for counted in 64-byte
            lines, output) over the achievable HBM rate.  --tile T: the same sketch tiled T x T (4: 4096 x 4096)
  host      the tint the runner drew before (label image + half/half look-up, kept below as `old_colour`), and this
            build's numpy path of the reference's picture, one thread of the same machine's host
  stage     the runner's stage block (bboxes.json, masks/, segmented_sketch.png, bboxes.png) with the old and the new
            visualisations, alternating: the tick (until the jobs are handed to the I/O threads and the device is idle)
            and the time until every file is written

The sketch is the 1024 x 1024 input of the mario_bunny fixture with its 13 masks and 3 seeded rectangles; every result
is compared with the host path before anything is timed.

    python tools/vis_time.py [--iters 200] [--warmup 20] [--out profiles/vis_times.txt]
"""
import argparse
import statistics
import sys
import tempfile
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
from inklayer_amd import ops, visualize  # noqa: E402

HBM_TBS = 6.3          # achievable streaming rate of the MI355X's HBM3E (8 TB/s peak)


def old_colour(rgb, masks):
    """The runner's former segmented_sketch.png: every mask tints its pixels half / half in a golden-ratio hue."""
    base = np.asarray(rgb)
    label = np.zeros(base.shape[:2], np.uint16)
    half = np.zeros((len(masks) + 1, 3), np.uint8)
    for i, m in enumerate(masks):
        hue = (i * 0.61803398875) % 1.0
        half[i + 1] = [int(127.5 * (0.6 + 0.4 * abs(((hue * 6 + k) % 6) / 3 - 1))) for k in (0, 4, 2)]
        label[np.asarray(m) != 0] = i + 1
    out = base.copy()
    sel = label > 0
    out[sel] = (base[sel] >> 1) + half[label[sel]]
    return out


def old_boxes(pil, boxes):
    from PIL import ImageDraw
    im = pil.copy()
    d = ImageDraw.Draw(im)
    for b in boxes:
        d.rectangle([b[0], b[1], b[2], b[3]], outline=(220, 40, 40), width=2)
    return im


def inputs():
    z = np.load(ROOT / "tests" / "golden" / "refine_mario_bunny.npz")
    rgb = z["input"]
    H, W = rgb.shape[:2]
    masks = np.unpackbits(z["masks"], axis=-1)[..., :W].astype(bool)
    rs = np.random.RandomState(0)
    extra = np.zeros((16 - len(masks), H, W), bool)
    for m in extra:
        y, x = rs.randint(0, H // 2), rs.randint(0, W // 2)
        m[y:y + H // 3, x:x + W // 3] = True
    boxes = [[int(v) for v in b * [W, H, W, H]] for b in z["bboxes"]]
    return np.ascontiguousarray(rgb), np.concatenate([masks, extra]), boxes, z["scores"].tolist()


def mask_bytes(rgb, masks):
    """Bytes of the mask stack the colour kernel asks for, in 64-byte lines: a lane (4 pixels) walks the planes from the
    last one down to the deepest "last mask" of its stroke pixels, all of them when a stroke pixel is in no mask."""
    gray = visualize.gray_host(rgb).reshape(-1)
    n = len(masks)
    last = np.full(gray.shape, -1, np.int64)
    for k, m in enumerate(masks):
        last[m.reshape(-1)] = k
    depth = np.where(gray < 250, n - np.maximum(last, 0), 0)            # planes down to the pixel's last mask
    lanes = np.minimum(n, (depth.reshape(-1, 4).max(1) + 3) // 4 * 4)   # the kernel reads them four at a time
    lines = lanes.reshape(-1, 16).max(1)                                # 16 lanes x 4 bytes = one 64-byte line per plane
    return int(lines.sum()) * 64


def per_launch_us(fn, warmup, iters):
    for _ in range(warmup):
        fn()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0.record()
    for _ in range(iters):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) * 1e3 / iters


def wall_ms(fn, reps=5):
    ts = []
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t) * 1e3)
    return statistics.median(ts)


def stage(new, out_dir, pil, rgb, boxes, scores, masks_np, masks_dev):
    """The first block of InkLayer.runner.finish_sketch -> (tick ms, ms until the files are written)."""
    import os
    from InkLayer.utils.io import flush, save_all
    from InkLayer.utils.processing import save_norm_bboxes
    from InkLayer.utils.visualization import draw_norm_bbox_on_image
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    save_norm_bboxes(bboxes_list=boxes, scores_list=scores, input_pil=pil, out_path=os.path.join(out_dir, "bboxes.json"))
    os.makedirs(os.path.join(out_dir, "masks"), exist_ok=True)
    jobs = [(np.asarray(m, dtype=bool), os.path.join(out_dir, "masks", f"mask_{i}.png")) for i, m in enumerate(masks_np)]
    if new:
        coloured = visualize.colour_sketch(rgb, masks_dev).cpu().numpy()
        jobs += [(coloured, os.path.join(out_dir, "segmented_sketch.png")),
                 (lambda: draw_norm_bbox_on_image(pil, boxes, ["object"] * len(boxes)), os.path.join(out_dir, "bboxes.png"))]
    else:
        jobs += [(lambda: old_colour(rgb, masks_np), os.path.join(out_dir, "segmented_sketch.png")),
                 (lambda: old_boxes(pil, boxes), os.path.join(out_dir, "bboxes.png"))]
    save_all(jobs, wait=False)
    torch.cuda.synchronize()
    tick = (time.perf_counter() - t0) * 1e3
    flush()
    return tick, (time.perf_counter() - t0) * 1e3


@torch.no_grad()
def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "vis_times.txt"))
    ap.add_argument("--tile", type=int, default=1)
    ap.add_argument("--kernels-only", action="store_true")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    rgb, masks, boxes, scores = inputs()
    n = len(masks)
    want = torch.from_numpy(visualize.colour_sketch(rgb, list(masks), use_gpu=False)).to(dev).repeat(a.tile, a.tile, 1)
    sk = torch.from_numpy(rgb).to(dev).repeat(a.tile, a.tile, 1).contiguous()
    m = torch.from_numpy(masks.view(np.uint8)).to(dev).repeat(1, a.tile, a.tile).contiguous()
    H, W = (int(v) for v in sk.shape[:2])
    label = torch.from_numpy(visualize.label_image(list(masks), rgb.shape[:2])).to(dev).repeat(a.tile, a.tile).contiguous()
    tables = torch.from_numpy(visualize.colour_tables(visualize.pastel_colors(n))).to(dev)
    mn = ops.vis_gray_min(sk)
    assert torch.equal(ops.vis_colour(sk, m, tables, mn), want)
    assert torch.equal(ops.vis_colour(sk, label, tables, mn, by_label=True), want)

    px = H * W
    asked = mask_bytes(rgb, masks) * a.tile * a.tile          # rows of 1024 pixels are whole 64-byte lines: tiling repeats them
    rows = [("ink_vis_gray_min", lambda: ops.vis_gray_min(sk, out=mn), 3 * px),
            ("ink_vis_colour, stack of 16 masks", lambda: ops.vis_colour(sk, m, tables, mn), 6 * px + asked),
            ("ink_vis_colour, label image", lambda: ops.vis_colour(sk, label, tables, mn, by_label=True), 7 * px)]
    lines = [f"coloured sketch, {W} x {H}, {n} masks resident on one {torch.cuda.get_device_name(0)}; results equal the host path",
             f"kernels: HIP events around {a.iters} back-to-back launches after {a.warmup} warm-up launches (wrapper and output "
             "allocation included; the data stays in the caches between launches)",
             f"{'kernel':40s} {'us/launch':>10s} {'MB moved':>9s} {'us at ' + str(HBM_TBS) + ' TB/s':>16s} {'fraction':>9s}"]
    for name, fn, nbytes in rows:
        us = per_launch_us(fn, a.warmup, a.iters)
        floor = nbytes / (HBM_TBS * 1e12) * 1e6
        lines.append(f"{name:40s} {us:10.2f} {nbytes / 1e6:9.2f} {floor:16.2f} {floor / us:9.2f}")
    lines.append(f"mask stack: {n * px / 1e6:.2f} MB, of which the lanes ask for {asked / 1e6:.2f} MB "
                 "(planes behind the last mask of a lane's stroke pixels, and lanes without strokes, are never read)")
    if a.kernels_only or a.tile != 1:
        print("\n".join(lines))
        return

    lines.append("host, one thread, median of 5 runs:")
    lines.append(f"  {'former tint (label image + half/half look-up)':56s} {wall_ms(lambda: old_colour(rgb, list(masks))):9.2f} ms")
    lines.append(f"  {'numpy path of the reference picture (use_gpu=False)':56s} "
                 f"{wall_ms(lambda: visualize.colour_sketch(rgb, list(masks), use_gpu=False)):9.2f} ms")
    lines.append(f"  {'colour_sketch(host sketch, resident masks) + copy back':56s} "
                 f"{wall_ms(lambda: visualize.colour_sketch(rgb, m).cpu().numpy()):9.2f} ms")

    from PIL import Image
    pil = Image.fromarray(rgb)
    masks_np = list(masks)
    ticks = {False: [], True: []}
    with tempfile.TemporaryDirectory() as tmp:
        for rep in range(12):
            for new in (False, True):
                t = stage(new, tmp, pil, rgb, boxes, scores, masks_np, m)
                if rep >= 2:
                    ticks[new].append(t)
    lines.append('runner stage "masks/ + detection visualisations" (bboxes.json, 16 mask files, the two pictures), median of 10, '
                 "old and new alternating:")
    for new in (False, True):
        tk = statistics.median(t[0] for t in ticks[new])
        done = statistics.median(t[1] for t in ticks[new])
        lines.append(f"  {'new' if new else 'old'}: tick {tk:8.2f} ms   every file written after {done:8.2f} ms")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(text)


if __name__ == "__main__":
    main()
