"""Evaluation stage: score a run against a ground-truth label image - InkScenes' INSTANCE_GT / CLASS_GT
matrices, or the masks_final/ of another run.

  contingency     T[i, u] = pixels inside prediction i with the u-th distinct ground-truth value, row n = all counted
                  pixels: csrc/evaluate.hip on the GPU, np.unique + one bincount per mask without one
  iou_matrix      prediction x instance IoU from T
  match_coco, Evaluator    COCO's published AP / AR procedure (score order, greedy matching per IoU threshold 0.50:0.05:0.95,
                  monotone precision envelope, 101 recall points, at most 100 detections per image)
  panoptic        PQ / SQ / RQ, pixel accuracy and mean best IoU of a disjoint prediction
  box_iou, label_boxes     the same AP / AR over boxes
  load_labels     .mat / .npy / .png / a directory of mask_i.png
  label_picture   the reference's ground-truth viewer (InkScenes/read_GT_mat_file.py:40-70) as arrays

Everything after the counting is float64 arithmetic on small integer tables on the host.  The metrics restate the
published procedures; they are not pinned to pycocotools or panopticapi.  Nothing under oracle/ or tests/ is imported.
"""
from __future__ import annotations

import os
import re
from typing import Optional

import numpy as np

from .visualize import STROKE_BELOW, gray_host, pastel_colors

MAX_VALUES = 256            # distinct ground-truth values of one contingency table (columns of the kernel's LDS table)
MAX_LABEL = 65535           # label values are 0 .. 65535 (the presence bitmap of the rank kernel)
THRESHOLDS = np.arange(50, 100, 5) / 100.0          # COCO's IoU thresholds 0.50:0.05:0.95
RECALL_GRID = np.arange(101) / 100.0                # COCO's 101 recall points
MAX_DETS = 100                                      # COCO's detections per image


def _is_cuda(t) -> bool:
    return hasattr(t, "is_cuda") and bool(t.is_cuda)


def _gpu_available() -> bool:
    try:
        import torch
        return bool(torch.cuda.is_available())
    except ImportError:
        return False


def _host_labels(labels) -> np.ndarray:
    """A host label image as an integer array; ValueError for non-integral floats or values outside 0 .. 65535."""
    a = np.asarray(labels)
    if a.ndim != 2:
        raise ValueError(f"label image: [H, W] expected, got shape {a.shape}")
    if a.dtype == np.bool_:
        a = a.astype(np.uint8)
    if a.dtype.kind == "f":
        if not np.array_equal(a, np.round(a)):          # NaN and inf fail here too
            raise ValueError("label image: float labels must be integral")
    elif a.dtype.kind not in "iu":
        raise ValueError(f"label image: integer labels expected, got {a.dtype}")
    if a.size and (a.min() < 0 or a.max() > MAX_LABEL):
        raise ValueError(f"label image: label values must be 0 .. {MAX_LABEL} (got {a.min()} .. {a.max()})")
    if a.dtype in (np.uint8, np.uint16, np.int32):
        return a
    return a.astype(np.uint16 if a.dtype.kind == "f" or a.dtype.itemsize <= 2 else np.int32)


def _device_labels(labels, dev):
    """The label image as a contiguous uint8 / uint16 / int32 tensor on dev (values out of range stay out of range, so
    that the kernel's flag reports them)."""
    import torch
    if not torch.is_tensor(labels):
        a = np.ascontiguousarray(_host_labels(labels))
        return torch.from_numpy(a if a.flags.writeable else a.copy()).to(dev)
    t = labels
    if t.dim() != 2:
        raise ValueError(f"label image: [H, W] expected, got shape {tuple(t.shape)}")
    if t.dtype == torch.bool:
        t = t.view(torch.uint8)
    if t.is_floating_point():
        if not bool((t == t.round()).all()):
            raise ValueError("label image: float labels must be integral")
    if t.dtype not in (torch.uint8, torch.uint16, torch.int32):
        t = t.clamp(-1, MAX_LABEL + 1).to(torch.int32)
    return t.to(dev).contiguous()


def _ranks_on_device(lab, limit=MAX_VALUES):
    """(rank, values[:U], U) of a device label image; ValueError through the kernel's flag or for U above `limit`."""
    from . import ops
    rank, values, info = ops.eval_label_ranks(lab, values_cap=MAX_VALUES)
    U, bad = (int(v) for v in info.cpu().tolist())
    if bad:
        raise ValueError(f"label image: label values must be 0 .. {MAX_LABEL}")
    if limit is not None and U > limit:
        raise ValueError(f"label image: {U} distinct values, at most {limit} are supported")
    return rank, values[:min(U, MAX_VALUES)], U


def _pred_form(pred, n_labels):
    """-> (by_label, n or None, (H, W) or None) of a prediction argument: a 2-D array is a label image."""
    if isinstance(pred, (list, tuple)):
        if len(pred) == 0:
            return False, 0, None
        return False, len(pred), tuple(np.shape(pred[0]) if not hasattr(pred[0], "shape") else pred[0].shape)
    nd = pred.dim() if hasattr(pred, "dim") else np.ndim(pred)
    if nd == 2:
        return True, (None if n_labels is None else int(n_labels)), tuple(pred.shape)
    if nd == 3:
        return False, int(pred.shape[0]), tuple(pred.shape[1:])
    raise ValueError(f"predictions: a stack [n, H, W], a sequence of [H, W] masks or a label image [H, W] expected, got {nd} dimensions")


def _contingency_host(pred, by_label, n, labels, sketch):
    lab = _host_labels(labels)
    values, rank = np.unique(lab, return_inverse=True)
    rank = rank.reshape(-1)
    U = len(values)
    if U > MAX_VALUES:
        raise ValueError(f"label image: {U} distinct values, at most {MAX_VALUES} are supported")
    counted = None if sketch is None else (gray_host(np.asarray(sketch)) < STROKE_BELOW).reshape(-1)
    if by_label:
        pl = np.asarray(pred).reshape(-1)
        if n is None:
            n = int(pl.max()) if pl.size else 0
        planes = [(pl == l) for l in range(1, n + 1)]
    else:
        planes = [(np.asarray(m) != 0).reshape(-1) for m in pred]
    T = np.zeros((n + 1, U), np.int64)
    for i, m in enumerate(planes):
        T[i] = np.bincount(rank[m if counted is None else (m & counted)], minlength=U)
    T[n] = np.bincount(rank if counted is None else rank[counted], minlength=U)
    return T, values.astype(np.int64)


def contingency(pred, gt_labels, sketch=None, stroke_only=False, use_gpu: Optional[bool] = None, n_labels: Optional[int] = None):
    """-> (T, values).  values: the sorted distinct values of the ground-truth label image gt_labels [H, W] (integers
    0 .. 65535, at most 256 distinct).  T [n + 1, len(values)]: T[i, u] = number of counted pixels inside prediction i whose
    ground-truth value is values[u]; row n counts every counted pixel (the ground-truth areas).
    pred: a stack [n, H, W] or a sequence of [H, W] masks (non-zero = inside, masks may overlap), or a label image [H, W]
    (l = mask l - 1; n = n_labels, by default the largest label; labels above n count as 0; n <= 255 on the GPU).
    stroke_only: only the pixels of `sketch` (uint8 [H, W, 3] R, G, B or [H, W]) whose grey is below 250 count.
    CUDA tensors in: the kernels run on the current stream and int32 tensors come back.  Host arrays in: numpy arrays come
    back; with a GPU the arrays are uploaded and the kernels run, without one (or with use_gpu=False) numpy counts."""
    by_label, n, shape = _pred_form(pred, n_labels)
    gshape = tuple(gt_labels.shape) if hasattr(gt_labels, "shape") else np.shape(gt_labels)
    if len(gshape) != 2:
        raise ValueError(f"label image: [H, W] expected, got shape {gshape}")
    if shape is not None and shape != gshape:
        raise ValueError(f"predictions {shape} and ground truth {gshape} differ in shape")
    if stroke_only:
        if sketch is None:
            raise ValueError("stroke_only needs the sketch")
        sshape = tuple(sketch.shape)
        if sshape[:2] != gshape or not (len(sshape) == 2 or (len(sshape) == 3 and sshape[2] == 3)):
            raise ValueError(f"sketch {sshape} does not fit the ground truth {gshape}")
    else:
        sketch = None
    on_dev = _is_cuda(pred) or _is_cuda(gt_labels) or _is_cuda(sketch) or \
        (isinstance(pred, (list, tuple)) and any(_is_cuda(m) for m in pred))
    if on_dev:
        if use_gpu is False:
            raise ValueError("contingency: CUDA tensors cannot take the host path")
        use_gpu = True
    elif use_gpu is None:
        use_gpu = _gpu_available()
    if not use_gpu:
        return _contingency_host(pred, by_label, n, gt_labels, sketch)

    import torch
    from . import ops
    dev = next((t.device for t in (pred, gt_labels, sketch) if _is_cuda(t)), None)
    if dev is None and isinstance(pred, (list, tuple)):
        dev = next((m.device for m in pred if _is_cuda(m)), None)
    dev = dev or torch.device("cuda")

    def up(a, nonzero):
        if isinstance(a, (list, tuple)):
            a = torch.stack(list(a)) if torch.is_tensor(a[0]) else np.stack([np.asarray(m) for m in a])
        if not torch.is_tensor(a):
            a = np.asarray(a)
            a = np.ascontiguousarray(a.view(np.uint8) if a.dtype == np.bool_ else a)
            a = torch.from_numpy(a if a.flags.writeable else a.copy())
        if a.dtype == torch.bool:
            a = a.view(torch.uint8)
        if a.dtype != torch.uint8:
            a = (a != 0).to(torch.uint8) if nonzero else a.clamp(0, 255).to(torch.uint8)
        return a.to(dev).contiguous()

    rank, values, U = _ranks_on_device(_device_labels(gt_labels, dev))
    if by_label:
        p = pred if torch.is_tensor(pred) else torch.from_numpy(np.ascontiguousarray(np.asarray(pred)))
        if n is None:
            n = int(p.max()) if p.numel() else 0
        if n > 255:
            raise ValueError(f"label-image predictions hold at most 255 masks on the GPU (got {n}); pass the mask stack")
        p = up(p, nonzero=False)
    elif n == 0:
        p = torch.zeros((0,) + gshape, dtype=torch.uint8, device=dev)
    else:
        p = up(pred, nonzero=True)
    sk = None if sketch is None else up(sketch, nonzero=False)
    T = ops.eval_contingency(p, rank, U, n_labels=n if by_label else None, sketch_u8=sk)
    if on_dev:
        return T, values
    return T.cpu().numpy().astype(np.int64), values.cpu().numpy().astype(np.int64)


def _np(a) -> np.ndarray:
    return a.detach().cpu().numpy() if hasattr(a, "detach") else np.asarray(a)


def _instances(T: np.ndarray, values: np.ndarray) -> np.ndarray:
    """Columns that are ground-truth instances: value != 0 and area in the counted domain > 0."""
    return np.flatnonzero((values != 0) & (T[-1] > 0))


def iou_matrix(T, values) -> np.ndarray:
    """float64 [n, G]: IoU of every prediction with every ground-truth instance (the columns whose value is not 0 and
    whose area in the counted domain is positive, in the order of `values`); 0 where the union is 0."""
    T = _np(T).astype(np.int64)
    cols = _instances(T, _np(values))
    inter = T[:-1][:, cols]
    union = T[:-1].sum(1, keepdims=True) + T[-1][None, cols] - inter
    return np.where(union > 0, inter / np.maximum(union, 1), 0.0).astype(np.float64)


def box_iou(a, b) -> np.ndarray:
    """float64 [n, m]: IoU of boxes (x0, y0, x1, y1); 0 where the union is 0."""
    a = np.asarray(a, np.float64).reshape(-1, 4)
    b = np.asarray(b, np.float64).reshape(-1, 4)
    w = np.clip(np.minimum(a[:, None, 2], b[None, :, 2]) - np.maximum(a[:, None, 0], b[None, :, 0]), 0, None)
    h = np.clip(np.minimum(a[:, None, 3], b[None, :, 3]) - np.maximum(a[:, None, 1], b[None, :, 1]), 0, None)
    inter = w * h
    area = lambda r: np.clip(r[:, 2] - r[:, 0], 0, None) * np.clip(r[:, 3] - r[:, 1], 0, None)
    union = area(a)[:, None] + area(b)[None, :] - inter
    return np.where(union > 0, inter / np.where(union > 0, union, 1.0), 0.0)


def match_coco(iou, scores, thr: float) -> np.ndarray:
    """int64 [n]: the instance every prediction is matched to, -1 for none.  Predictions go in descending score (stable on
    the index); each takes the still-unmatched instance of highest IoU >= thr, the lowest index among equals."""
    iou = np.asarray(iou, np.float64)
    n, G = iou.shape
    out = np.full(n, -1, np.int64)
    if G == 0:
        return out
    taken = np.zeros(G, bool)
    for d in np.argsort(-np.asarray(scores, np.float64), kind="stable"):
        row = np.where(taken, -1.0, iou[d])
        g = int(np.argmax(row))
        if row[g] >= thr:
            out[d] = g
            taken[g] = True
    return out


class Evaluator:
    """COCO's AP / AR over a data set: add(iou, scores) per image, summary() at the end."""

    def __init__(self, thresholds=THRESHOLDS, max_dets: int = MAX_DETS):
        self.thresholds = np.asarray(thresholds, np.float64)
        self.max_dets = int(max_dets)
        self.scores, self.hits = [], []
        self.instances = 0
        self.images = 0

    def add(self, iou, scores) -> None:
        """iou: float [n, G] of one image's n predictions and G instances; scores: [n]."""
        iou = np.asarray(iou, np.float64)
        scores = np.asarray(scores, np.float64).reshape(-1)
        if iou.ndim != 2 or iou.shape[0] != len(scores):
            raise ValueError(f"Evaluator.add: IoU matrix {iou.shape} does not fit {len(scores)} scores")
        keep = np.argsort(-scores, kind="stable")[:self.max_dets]
        iou, scores = iou[keep], scores[keep]
        self.scores.append(scores)
        self.hits.append(np.stack([match_coco(iou, scores, t) >= 0 for t in self.thresholds]).reshape(len(self.thresholds), -1))
        self.instances += iou.shape[1]
        self.images += 1

    def summary(self) -> dict:
        """AP (mean over the thresholds), AP50, AP75, AR (mean over the thresholds of matched / instances); -1, COCO's
        "undefined", when the data set has no instance."""
        nd = int(sum(len(s) for s in self.scores))
        out = {"images": self.images, "instances": self.instances, "detections": nd}
        if self.instances == 0:
            out.update(AP=-1.0, AP50=-1.0, AP75=-1.0, AR=-1.0)
            return out
        scores = np.concatenate(self.scores) if self.scores else np.zeros(0)
        hits = np.concatenate(self.hits, axis=1) if self.hits else np.zeros((len(self.thresholds), 0), bool)
        order = np.argsort(-scores, kind="stable")
        ap, ar = [], []
        for k in range(len(self.thresholds)):
            tp = np.cumsum(hits[k][order])
            fp = np.cumsum(~hits[k][order])
            recall = tp / self.instances
            precision = tp / np.maximum(tp + fp, 1)
            envelope = np.maximum.accumulate(precision[::-1])[::-1]
            at = np.searchsorted(recall, RECALL_GRID, side="left")
            q = np.zeros(len(RECALL_GRID))                      # precision 0 at recalls that are never reached
            q[at < nd] = envelope[at[at < nd]]
            ap.append(float(np.mean(q)))
            ar.append(float(recall[-1]) if nd else 0.0)
        at_thr = lambda t: ap[int(np.argmin(np.abs(self.thresholds - t)))]
        out.update(AP=float(np.mean(ap)), AP50=at_thr(0.5), AP75=at_thr(0.75), AR=float(np.mean(ar)))
        return out


def panoptic(T, values) -> dict:
    """Panoptic quality of a disjoint prediction (the final label image).  A prediction (a row with pixels) and an
    instance match when their IoU is above 0.5, which makes the match unique.  PQ = sum of matched IoUs / (TP + FP / 2 +
    FN / 2) = SQ x RQ; accuracy = matched intersection pixels / instance pixels; mean_best_iou = mean over the instances
    of their best IoU with any prediction.  The raw sums are returned too so that a data set can be pooled
    (panoptic_pool).  Without predictions and without instances every figure is 0."""
    T = _np(T).astype(np.int64)
    cols = _instances(T, _np(values))
    rows = np.flatnonzero(T[:-1].sum(1) > 0)
    iou = iou_matrix(T, values)[rows]
    hit = iou > 0.5
    inter = T[:-1][rows][:, cols]
    raw = {"tp": int(hit.sum()), "fp": int((~hit.any(1)).sum()), "fn": int((~hit.any(0)).sum()),
           "iou_sum": float(iou[hit].sum()), "matched_pixels": int(inter[hit].sum()), "instance_pixels": int(T[-1][cols].sum()),
           "best_iou_sum": float(iou.max(0).sum()) if len(rows) else 0.0, "instances": int(len(cols))}
    return panoptic_pool([raw])


def panoptic_pool(parts) -> dict:
    """The figures of `panoptic` over the pooled raw sums of several images."""
    keys = ("tp", "fp", "fn", "iou_sum", "matched_pixels", "instance_pixels", "best_iou_sum", "instances")
    s = {k: sum(p[k] for p in parts) for k in keys}
    den = s["tp"] + 0.5 * s["fp"] + 0.5 * s["fn"]
    s.update(PQ=s["iou_sum"] / den if den else 0.0, SQ=s["iou_sum"] / s["tp"] if s["tp"] else 0.0,
             RQ=s["tp"] / den if den else 0.0,
             accuracy=s["matched_pixels"] / s["instance_pixels"] if s["instance_pixels"] else 0.0,
             mean_best_iou=s["best_iou_sum"] / s["instances"] if s["instances"] else 0.0)
    return s


def label_boxes(labels, use_gpu: Optional[bool] = None):
    """-> (boxes [U, 4] = xmin, ymin, xmax, ymax inclusive, values [U]) of a label image; tensors for a CUDA tensor,
    numpy arrays otherwise (kernels when a GPU is there, numpy without one or with use_gpu=False)."""
    on_dev = _is_cuda(labels)
    if on_dev or (use_gpu is None and _gpu_available()) or use_gpu:
        import torch
        from . import ops
        dev = labels.device if on_dev else torch.device("cuda")
        rank, values, U = _ranks_on_device(_device_labels(labels, dev))
        boxes = ops.eval_label_boxes(rank, U)
        return (boxes, values) if on_dev else (boxes.cpu().numpy().astype(np.int64), values.cpu().numpy().astype(np.int64))
    lab = _host_labels(labels)
    values = np.unique(lab)
    boxes = np.zeros((len(values), 4), np.int64)
    for u, v in enumerate(values):
        ys, xs = np.nonzero(lab == v)
        boxes[u] = xs.min(), ys.min(), xs.max(), ys.max()
    return boxes, values.astype(np.int64)


def label_picture(labels, use_gpu: Optional[bool] = None):
    """The reference's visualize_label_matrix (InkScenes/read_GT_mat_file.py:40-70) as arrays: uint8 [H, W, 3], the idx-th
    distinct value painted colors[idx] with colors = [white] + pastel_colors(U - 1), value 0 left white.  As in the
    reference, when 0 is absent the smallest label has index 0 and is white too.  A CUDA tensor goes through the
    kernels (at most 256 distinct values 0 .. 65535) and a tensor comes back; host arrays give a numpy array, through the
    kernels when a GPU is there and the image is within those limits, through numpy otherwise."""
    on_dev = _is_cuda(labels)
    lab = None
    if not on_dev:
        a = np.asarray(labels)
        if a.ndim != 2:
            raise ValueError(f"label image: [H, W] expected, got shape {a.shape}")
        values, rank = np.unique(a, return_inverse=True)            # the reference's own statement, any dtype
        in_limits = len(values) <= MAX_VALUES and a.dtype.kind in "iuf" and \
            np.array_equal(values, np.round(values)) and values.min() >= 0 and values.max() <= MAX_LABEL
        if use_gpu is None:
            use_gpu = _gpu_available() and in_limits
        if not use_gpu:
            table = np.array([(255, 255, 255)] + pastel_colors(len(values) - 1), np.uint8)
            table[values == 0] = 255
            return table[rank.reshape(a.shape)]
        lab = a
    import torch
    from . import ops
    dev = labels.device if on_dev else torch.device("cuda")
    rank, values, U = _ranks_on_device(_device_labels(labels if on_dev else lab, dev))
    table = np.array([(255, 255, 255)] + pastel_colors(U - 1), np.uint8)
    out = ops.eval_paint_labels(rank, torch.from_numpy(table).to(dev))
    return out if on_dev else out.cpu().numpy()


def _mask_files(path):
    found = []
    for f in os.listdir(path):
        m = re.fullmatch(r"mask_(\d+)\.png", f)
        if m:
            found.append((int(m.group(1)), os.path.join(path, f)))
    return sorted(found)


def load_mask_dir(path):
    """-> (indices, masks bool [n, H, W]) of a directory of mask_<i>.png, in the order of i."""
    from PIL import Image
    files = _mask_files(path)
    if not files:
        raise ValueError(f"{path}: no mask_<i>.png found")
    masks = np.stack([np.asarray(Image.open(f).convert("L")) > 127 for _, f in files])
    return [i for i, _ in files], masks


def load_labels(path, key: str = "INSTANCE_GT") -> np.ndarray:
    """A ground-truth label image from a .mat file (`key`: INSTANCE_GT or CLASS_GT), a .npy file, an 8- or 16-bit .png, or
    a directory of mask_<i>.png (label i + 1 for mask_<i>.png, the last mask holding a pixel wins: the masks_final/ of
    another run as ground truth)."""
    path = os.fspath(path)
    if os.path.isdir(path):
        indices, masks = load_mask_dir(path)
        if indices[-1] + 1 > MAX_LABEL:
            raise ValueError(f"{path}: mask index {indices[-1]} is above the largest label {MAX_LABEL}")
        label = np.zeros(masks.shape[1:], np.uint16 if indices[-1] + 1 > 255 else np.uint8)
        for i, m in zip(indices, masks):
            label[m] = i + 1
        return label
    ext = os.path.splitext(path)[1].lower()
    if ext == ".mat":
        try:
            from scipy.io import loadmat
        except ImportError as e:
            raise ImportError(f"{path}: reading .mat ground truth needs scipy (scipy.io.loadmat); convert the file to .npy or "
                              ".png, or install scipy") from e
        data = loadmat(path)
        if key not in data:
            raise KeyError(f"{path}: no matrix {key!r} (it has {sorted(k for k in data if not k.startswith('__'))})")
        return np.asarray(data[key])
    if ext == ".npy":
        return np.load(path)
    if ext == ".png":
        from PIL import Image
        im = Image.open(path)
        if im.mode not in ("L", "I;16", "I;16L", "I;16B", "I", "P", "1"):
            raise ValueError(f"{path}: a single-channel 8- or 16-bit label image expected, got mode {im.mode}")
        a = np.asarray(im)
        return a.astype(np.uint8) if a.dtype == np.bool_ else a
    raise ValueError(f"{path}: .mat, .npy, .png or a directory of mask_<i>.png expected")
