"""Scores an output tree of tools/run_dir.py (or of the reference) against ground truth.

For every <name>/ of the tree that has a ground truth of the same stem in --gt (a <name>.mat / .npy / .png label image, or
a directory <name>/ that holds mask_<i>.png itself or in its masks_final/ - the tree of another run), four figure sets:
  masks        AP / AR of masks/mask_<i>.png scored with scores[i] of bboxes.json
  masks_final  AP / AR of masks_final/mask_<i>.png; mask_<i>.png scores scores[kept_indices.index(i)] of bboxes_final.json,
               a mask whose index is not kept (the appended mask of the unlabeled strokes) scores 0
  panoptic     PQ / SQ / RQ, pixel accuracy and mean best IoU of the final masks (disjoint: their table is the table of
               their label image)
  boxes        AP / AR of the boxes of bboxes_final.json against the ground-truth instances' bounding boxes
One JSON line per sketch, then one summary line over the data set.  With --stroke-only only the stroke pixels of
<name>/input.png (grey < 250) are counted in the mask figures.  Runs on the GPU when there is one, in numpy otherwise.

    python tools/eval_dir.py --pred output --gt data/InkScenes/GT [--stroke-only] [--type INSTANCE_GT] [--json FILE]
"""
import argparse
import json
import os
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
from inklayer_amd import evaluate  # noqa: E402


def find_gt(gt_dir, name):
    for ext in (".mat", ".npy", ".png"):
        p = os.path.join(gt_dir, name + ext)
        if os.path.isfile(p):
            return p
    d = os.path.join(gt_dir, name)
    if os.path.isdir(os.path.join(d, "masks_final")):
        return os.path.join(d, "masks_final")
    return d if os.path.isdir(d) else None


def _one(ev_all, iou, scores, keep=None):
    if keep is not None:                         # a mask without a counted pixel is no detection
        iou, scores = iou[keep], np.asarray(scores, np.float64)[keep]
    ev_all.add(iou, scores)
    one = evaluate.Evaluator()
    one.add(iou, scores)
    return one.summary()


def score_sketch(pred_dir, gt_path, key, stroke_only, use_gpu, totals):
    from PIL import Image
    labels = evaluate.load_labels(gt_path, key=key)
    H, W = labels.shape
    sketch = np.asarray(Image.open(os.path.join(pred_dir, "input.png")).convert("RGB")) if stroke_only else None
    count = lambda masks: evaluate.contingency(masks, labels, sketch, stroke_only, use_gpu=use_gpu)
    out = {}
    if os.path.isdir(os.path.join(pred_dir, "masks")) and os.path.isfile(os.path.join(pred_dir, "bboxes.json")):
        idx, masks = evaluate.load_mask_dir(os.path.join(pred_dir, "masks"))
        scores = json.load(open(os.path.join(pred_dir, "bboxes.json")))["scores"]
        T, values = count(masks)
        out["masks"] = _one(totals["masks"], evaluate.iou_matrix(T, values), [scores[i] for i in idx], T[:-1].sum(1) > 0)
    if os.path.isdir(os.path.join(pred_dir, "masks_final")) and os.path.isfile(os.path.join(pred_dir, "bboxes_final.json")):
        final = json.load(open(os.path.join(pred_dir, "bboxes_final.json")))
        kept = list(final["kept_indices"])
        idx, masks = evaluate.load_mask_dir(os.path.join(pred_dir, "masks_final"))
        T, values = count(masks)
        scores = [final["scores"][kept.index(i)] if i in kept else 0.0 for i in idx]
        out["masks_final"] = _one(totals["masks_final"], evaluate.iou_matrix(T, values), scores, T[:-1].sum(1) > 0)
        pq = evaluate.panoptic(T, values)
        totals["panoptic"].append(pq)
        out["panoptic"] = {k: pq[k] for k in ("PQ", "SQ", "RQ", "accuracy", "mean_best_iou")}
        gt_boxes, gt_values = evaluate.label_boxes(labels, use_gpu=use_gpu)
        gt_boxes = gt_boxes[gt_values != 0].astype(np.float64)
        gt_boxes[:, 2:] += 1                                         # inclusive pixel bounds -> corner coordinates
        boxes = np.asarray(final["bboxes"], np.float64).reshape(-1, 4) * [W, H, W, H]
        out["boxes"] = _one(totals["boxes"], evaluate.box_iou(boxes, gt_boxes), final["scores"])
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--pred", required=True, help="output tree: one directory per sketch")
    ap.add_argument("--gt", required=True, help="ground truth: <name>.mat/.npy/.png or <name>/ directories")
    ap.add_argument("--stroke-only", action="store_true", help="count only the stroke pixels of input.png")
    ap.add_argument("--type", default="INSTANCE_GT", help="matrix of a .mat ground truth (INSTANCE_GT or CLASS_GT)")
    ap.add_argument("--json", default=None, help="also write all lines into this file as one JSON document")
    ap.add_argument("--cpu", action="store_true", help="count in numpy even when a GPU is there")
    a = ap.parse_args(argv)
    use_gpu = False if a.cpu else None
    totals = {"masks": evaluate.Evaluator(), "masks_final": evaluate.Evaluator(), "boxes": evaluate.Evaluator(), "panoptic": []}
    per_sketch = []
    for name in sorted(os.listdir(a.pred)):
        pred_dir = os.path.join(a.pred, name)
        gt_path = find_gt(a.gt, name) if os.path.isdir(pred_dir) else None
        if gt_path is None:
            continue
        line = {"name": name, **score_sketch(pred_dir, gt_path, a.type, a.stroke_only, use_gpu, totals)}
        per_sketch.append(line)
        print(json.dumps(line), flush=True)
    pooled = evaluate.panoptic_pool(totals["panoptic"]) if totals["panoptic"] else None
    summary = {"summary": True, "sketches": len(per_sketch), "stroke_only": bool(a.stroke_only),
               "masks": totals["masks"].summary(), "masks_final": totals["masks_final"].summary(),
               "panoptic": None if pooled is None else {k: pooled[k] for k in ("PQ", "SQ", "RQ", "accuracy", "mean_best_iou")},
               "boxes": totals["boxes"].summary()}
    print(json.dumps(summary), flush=True)
    if a.json:
        Path(a.json).write_text(json.dumps({"sketches": per_sketch, "summary": summary}, indent=1) + "\n")
    return 0 if per_sketch else 1


if __name__ == "__main__":
    sys.exit(main())
