"""Times the evaluation kernels (csrc/evaluate.hip) on a 1024 x 1024 sketch with 16 masks resident on the GPU and on the
same tiled 4 x 4 (4096 x 4096), next to the numpy path of inklayer_amd/evaluate.py on the host of the same machine.

  kernels   every entry point (label ranks = 2 clears + 3 kernels, contingency in stack and label form, all pixels and
            stroke-only, label boxes = init + kernel, paint): the median of --iters launches, each between two HIP events,
            launched back to back after --warmup; next to the bytes the call has to move and the share of the achievable
            HBM rate that is.  The per-kernel device times come from a run of its own,
            `rocprofv3 --kernel-trace --stats -- python tools/eval_time.py --kernels-only --tile 1` (and 4), whose
            kernel-stats CSVs --kernel-stats folds into the report.
  end to end   contingency + iou_matrix + Evaluator.add from resident tensors (wall time, median of 5, includes the
            synchronising read of the number of distinct values and the copy of the table)
  host      the numpy path (use_gpu=False) on the same arrays, one thread

The ground truth is the label image of the 16 masks (the last mask holding a pixel wins); every result is compared with
the numpy path before anything is timed.

    python tools/eval_time.py [--iters 100] [--warmup 10] [--out profiles/eval_times.txt] [--kernel-stats CSV1 CSV4]
"""
import argparse
import csv
import statistics
import sys
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
from inklayer_amd import evaluate, ops, visualize  # noqa: E402

HBM_TBS = 6.3          # achievable streaming rate of the MI355X's HBM3E (8 TB/s peak), as in tools/vis_time.py


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
    masks = np.concatenate([masks, extra])
    return np.ascontiguousarray(rgb), masks, visualize.label_image(list(masks), (H, W))


def median_us(fn, warmup, iters):
    for _ in range(warmup):
        fn()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)]
    torch.cuda.synchronize()
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    return statistics.median(a.elapsed_time(b) for a, b in ev) * 1e3


def wall_ms(fn, reps=5):
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t) * 1e3)
    return statistics.median(ts)


def measure(tile, rgb, masks, label, a, with_host):
    dev = torch.device("cuda:0")
    sk = torch.from_numpy(rgb).to(dev).repeat(tile, tile, 1).contiguous()
    m = torch.from_numpy(masks.view(np.uint8)).to(dev).repeat(1, tile, tile).contiguous()
    lab = torch.from_numpy(label).to(dev).repeat(tile, tile).contiguous()
    n, (H, W) = len(masks), lab.shape
    px = H * W
    rank, values, info = ops.eval_label_ranks(lab)
    U = int(info[0])
    T_host, v_host = evaluate.contingency(masks, label, rgb, True, use_gpu=False)
    for so in (False, True):
        Th = evaluate.contingency(masks, label, rgb, so, use_gpu=False)[0] * tile * tile
        assert np.array_equal(ops.eval_contingency(m, rank, U, sketch_u8=sk if so else None).cpu().numpy(), Th)
        assert np.array_equal(ops.eval_contingency(lab, rank, U, n_labels=n, sketch_u8=sk if so else None).cpu().numpy(),
                              evaluate.contingency(label, label, rgb, so, use_gpu=False, n_labels=n)[0] * tile * tile)
    colors = torch.from_numpy(np.array([(255, 255, 255)] + visualize.pastel_colors(U - 1), np.uint8)).to(dev)
    assert np.array_equal(ops.eval_paint_labels(rank, colors).cpu().numpy()[:label.shape[0], :label.shape[1]],
                          evaluate.label_picture(label, use_gpu=False))
    strokes = int((visualize.gray_host(rgb) < 250).sum()) * tile * tile
    rows = [("ink_eval_label_ranks (uint8 labels)", lambda: ops.eval_label_ranks(lab), 2 * px + 2 * px),
            ("ink_eval_contingency, stack of 16", lambda: ops.eval_contingency(m, rank, U), (n + 2) * px),
            ("ink_eval_contingency, stack, stroke-only", lambda: ops.eval_contingency(m, rank, U, sketch_u8=sk), 3 * px),
            ("ink_eval_contingency, label image", lambda: ops.eval_contingency(lab, rank, U, n_labels=n), 3 * px),
            ("ink_eval_contingency, label, stroke-only", lambda: ops.eval_contingency(lab, rank, U, n_labels=n, sketch_u8=sk), 3 * px),
            ("ink_eval_label_boxes", lambda: ops.eval_label_boxes(rank, U), 2 * px),
            ("ink_eval_paint_labels", lambda: ops.eval_paint_labels(rank, colors), 5 * px)]
    lines = [f"{W} x {H}, {n} masks, {U} distinct ground-truth values, {strokes} stroke pixels",
             f"{'entry point':44s} {'us/call':>10s} {'MB moved':>9s} {'us at ' + str(HBM_TBS) + ' TB/s':>16s} {'share':>7s}"]
    for name, fn, nbytes in rows:
        us = median_us(fn, a.warmup, a.iters)
        floor = nbytes / (HBM_TBS * 1e12) * 1e6
        lines.append(f"{name:44s} {us:10.2f} {nbytes / 1e6:9.2f} {floor:16.2f} {floor / us:7.2f}")
    lines.append("bytes: the label image is read twice and the rank image written (ranks); rank image + every mask plane (stack; "
                 "stroke-only lanes without a stroke read neither: the sketch alone is counted), or + label image / sketch; "
                 "rank image (boxes); rank image + picture (paint)")
    if a.kernels_only:
        return lines

    def end_to_end():
        ev = evaluate.Evaluator()
        T, v = evaluate.contingency(m, lab, sk, True)
        ev.add(evaluate.iou_matrix(T, v), np.linspace(1.0, 0.5, n))
        return ev

    lines.append(f"  {'contingency + iou_matrix + Evaluator.add, resident tensors':60s} {wall_ms(end_to_end):9.2f} ms")
    if with_host:
        lines.append(f"  {'numpy path (use_gpu=False), all pixels':60s} "
                     f"{wall_ms(lambda: evaluate.contingency(masks, label, rgb, False, use_gpu=False)):9.2f} ms")
        lines.append(f"  {'numpy path (use_gpu=False), stroke-only':60s} "
                     f"{wall_ms(lambda: evaluate.contingency(masks, label, rgb, True, use_gpu=False)):9.2f} ms")
        lines.append(f"  {'host arrays in: upload + kernels + copy back, stroke-only':60s} "
                     f"{wall_ms(lambda: evaluate.contingency(masks, label, rgb, True)):9.2f} ms")
    return lines


def kernel_stats(path, tile):
    """Lines of a rocprofv3 kernel-stats CSV (Name, Calls, TotalDurationNs, AverageNs, ...) for the eval_ kernels."""
    out = [f"kernel times of `rocprofv3 --kernel-trace --stats -- python tools/eval_time.py --kernels-only --tile {tile}` "
           f"({1024 * tile} x {1024 * tile}; the contingency kernel's row is all four of its forms together):",
           f"  {'kernel':34s} {'calls':>7s} {'average us':>11s} {'min us':>9s} {'max us':>9s}"]
    with open(path, newline="") as fh:
        for row in csv.DictReader(fh):
            name = row.get("Name", "")
            if "eval_" not in name:
                continue
            short = name.split("eval_")[1].split("(")[0]
            out.append(f"  {'eval_' + short:34s} {int(row['Calls']):7d} {float(row['AverageNs']) / 1e3:11.2f} "
                       f"{float(row['MinNs']) / 1e3:9.2f} {float(row['MaxNs']) / 1e3:9.2f}")
    return out


@torch.no_grad()
def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "eval_times.txt"))
    ap.add_argument("--kernels-only", action="store_true")
    ap.add_argument("--tile", type=int, default=0, help="1 or 4: only that size (default: both)")
    ap.add_argument("--kernel-stats", nargs=2, default=None, metavar=("CSV_TILE1", "CSV_TILE4"),
                    help="kernel-stats CSVs of rocprofv3 runs of --kernels-only --tile 1 and --tile 4")
    a = ap.parse_args()
    rgb, masks, label = inputs()
    lines = [f"evaluation kernels on one {torch.cuda.get_device_name(0)}; results equal the numpy path",
             f"median of {a.iters} calls, each between two HIP events, back to back after {a.warmup} warm-up calls (wrapper, "
             "output allocation and the calls' own clears included; the data stays in the caches between calls)"]
    for tile in ((a.tile,) if a.tile else (1, 4)):
        lines += [""] + measure(tile, rgb, masks, label, a, with_host=tile == 1)
    if a.kernel_stats:
        for tile, path in zip((1, 4), a.kernel_stats):
            lines += [""] + kernel_stats(path, tile)
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if not a.kernels_only and not a.tile:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(text)


if __name__ == "__main__":
    main()
