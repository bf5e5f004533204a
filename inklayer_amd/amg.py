"""SamAutomaticMaskGenerator (SA/automatic_mask_generator.py) on the HIP engine: "segment everything" - a grid of
single-point prompts, three masks per point, filtered by predicted IoU and stability score, de-duplicated by box NMS,
returned as the reference's records.

The reference asks the predictor for full-resolution f32 LOGITS of every candidate (192 images per batch of 64 points,
805 MB at 1024^2) and walks them six to eight times.  Here the tail starts from the low-res logits: the predicted-IoU
filter runs on the device into an index list, ops.sam_amg_stats makes stability counts, area, box and a bit-packed mask
of the survivors in one pass (the floats it thresholds are bit for bit those of ops.sam_postprocess), ONE small table
comes back to the host for the two remaining filters, and ops.mask_rle writes the RLE of what is left.  Box NMS
(ops.box_nms) and, for min_mask_region_area > 0, remove_small_regions (ops.remove_small_regions) are kernels too.  Filter
order and comparison operators are the reference's, so the records are the reference's.

Host-side pieces (point grids, crop boxes, the crop-edge test on the m x 4 box table, RLE decoding) restate
SA/utils/amg.py; tests/test_amg_cpu.py holds them to values recorded from the reference's own functions.
"""
from __future__ import annotations

import math
from copy import deepcopy
from itertools import product
from typing import Any, Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import ops
from .sam import SamPredictor


# ------------------------------------------------------------------------------------------------ SA/utils/amg.py
def build_point_grid(n_per_side: int) -> np.ndarray:
    """amg.py:179-186: n x n points evenly spaced in [0, 1]^2, as [n^2, 2] (x, y)."""
    offset = 1 / (2 * n_per_side)
    side = np.linspace(offset, 1 - offset, n_per_side)
    px = np.tile(side[None, :], (n_per_side, 1))
    py = np.tile(side[:, None], (1, n_per_side))
    return np.stack([px, py], axis=-1).reshape(-1, 2)


def build_all_layer_point_grids(n_per_side: int, n_layers: int, scale_per_layer: int) -> List[np.ndarray]:
    """amg.py:189-197."""
    return [build_point_grid(int(n_per_side / (scale_per_layer ** i))) for i in range(n_layers + 1)]


def generate_crop_boxes(im_size: Tuple[int, ...], n_layers: int, overlap_ratio: float) -> Tuple[List[List[int]], List[int]]:
    """amg.py:200-234: the whole image, then (2^i)^2 overlapping crops for layer i, as XYXY boxes."""
    crop_boxes, layer_idxs = [], []
    im_h, im_w = im_size
    short_side = min(im_h, im_w)
    crop_boxes.append([0, 0, im_w, im_h])
    layer_idxs.append(0)

    def crop_len(orig_len, n_crops, overlap):
        return int(math.ceil((overlap * (n_crops - 1) + orig_len) / n_crops))

    for i_layer in range(n_layers):
        n_side = 2 ** (i_layer + 1)
        overlap = int(overlap_ratio * short_side * (2 / n_side))
        crop_w = crop_len(im_w, n_side, overlap)
        crop_h = crop_len(im_h, n_side, overlap)
        xs = [int((crop_w - overlap) * i) for i in range(n_side)]
        ys = [int((crop_h - overlap) * i) for i in range(n_side)]
        for x0, y0 in product(xs, ys):
            crop_boxes.append([x0, y0, min(x0 + crop_w, im_w), min(y0 + crop_h, im_h)])
            layer_idxs.append(i_layer + 1)
    return crop_boxes, layer_idxs


def uncrop_boxes_xyxy(boxes: torch.Tensor, crop_box: Sequence[int]) -> torch.Tensor:
    x0, y0 = crop_box[0], crop_box[1]
    return boxes + torch.tensor([[x0, y0, x0, y0]], device=boxes.device)


def uncrop_points(points: torch.Tensor, crop_box: Sequence[int]) -> torch.Tensor:
    x0, y0 = crop_box[0], crop_box[1]
    return points + torch.tensor([[x0, y0]], device=points.device)


def is_box_near_crop_edge(boxes: torch.Tensor, crop_box: Sequence[int], orig_box: Sequence[int],
                          atol: float = 20.0) -> torch.Tensor:
    """amg.py:78-88: a box side within atol of a crop side that is not also a side of the image."""
    crop_t = torch.as_tensor(crop_box, dtype=torch.float, device=boxes.device)
    orig_t = torch.as_tensor(orig_box, dtype=torch.float, device=boxes.device)
    boxes = uncrop_boxes_xyxy(boxes, crop_box).float()
    near_crop = torch.isclose(boxes, crop_t[None, :], atol=atol, rtol=0)
    near_image = torch.isclose(boxes, orig_t[None, :], atol=atol, rtol=0)
    return torch.any(torch.logical_and(near_crop, ~near_image), dim=1)


def box_xyxy_to_xywh(box_xyxy):
    box_xywh = deepcopy(box_xyxy)
    box_xywh[2] = box_xywh[2] - box_xywh[0]
    box_xywh[3] = box_xywh[3] - box_xywh[1]
    return box_xywh


def rle_to_mask(rle: Dict[str, Any]) -> np.ndarray:
    """amg.py:138-149: uncompressed RLE (column-major runs, zeros first) -> bool [h, w]."""
    h, w = rle["size"]
    mask = np.empty(h * w, dtype=bool)
    idx, parity = 0, False
    for count in rle["counts"]:
        mask[idx: idx + count] = parity
        idx += count
        parity ^= True
    return mask.reshape(w, h).transpose()


def area_from_rle(rle: Dict[str, Any]) -> int:
    return sum(rle["counts"][1::2])


def coco_encode_rle(uncompressed_rle: Dict[str, Any]) -> Dict[str, Any]:
    from pycocotools import mask as mask_utils  # type: ignore

    h, w = uncompressed_rle["size"]
    rle = mask_utils.frPyObjects(uncompressed_rle, h, w)
    rle["counts"] = rle["counts"].decode("utf-8")
    return rle


def batched_mask_to_box(masks: torch.Tensor) -> torch.Tensor:
    """amg.py:303-346 for bool [c, h, w]: int64 XYXY with inclusive maxima, [0, 0, 0, 0] for an empty mask."""
    if torch.numel(masks) == 0:
        return torch.zeros(*masks.shape[:-2], 4, device=masks.device)
    h, w = masks.shape[-2:]
    in_h, _ = torch.max(masks, dim=-1)
    hc = in_h * torch.arange(h, device=masks.device)[None, :]
    bottom, _ = torch.max(hc, dim=-1)
    top, _ = torch.min(hc + h * (~in_h), dim=-1)
    in_w, _ = torch.max(masks, dim=-2)
    wc = in_w * torch.arange(w, device=masks.device)[None, :]
    right, _ = torch.max(wc, dim=-1)
    left, _ = torch.min(wc + w * (~in_w), dim=-1)
    empty = (right < left) | (bottom < top)
    return torch.stack([left, top, right, bottom], dim=-1) * (~empty).unsqueeze(-1)


def unpack_col_planes(planes: torch.Tensor, H: int) -> torch.Tensor:
    """column-major bit planes int64 [k, W, ceil(H / 64)] -> bool [k, H, W] (host-side bookkeeping, not a hot path)"""
    k, W, hp = planes.shape
    sh = torch.arange(64, device=planes.device)
    out = torch.empty((k, H, W), device=planes.device, dtype=torch.bool)
    for a in range(0, k, 16):                            # the shifted words are 8 bytes per pixel: a few planes at a time
        bits = (planes[a:a + 16].unsqueeze(-1) >> sh) & 1
        out[a:a + 16] = bits.reshape(-1, W, hp * 64)[:, :, :H].transpose(1, 2).bool()
    return out


def box_area(boxes: torch.Tensor) -> torch.Tensor:
    return (boxes[:, 2] - boxes[:, 0]) * (boxes[:, 3] - boxes[:, 1])


_FIELDS = ("iou_preds", "points", "stability_score", "boxes", "cand")


def _empty_data() -> Dict[str, Any]:
    return dict(rles=[], iou_preds=torch.zeros(0), points=torch.zeros(0, 2, dtype=torch.float64),
                stability_score=torch.zeros(0), boxes=torch.zeros(0, 4, dtype=torch.int64),
                cand=torch.zeros(0, dtype=torch.int64))


def _cat(parts: List[Dict[str, Any]], extra: Sequence[str] = ()) -> Dict[str, Any]:
    if not parts:
        return _empty_data()
    out = {k: torch.cat([p[k] for p in parts], dim=0) for k in (*_FIELDS, *extra)}
    out["rles"] = [r for p in parts for r in p["rles"]]
    return out


def _filter(data: Dict[str, Any], keep: torch.Tensor) -> Dict[str, Any]:
    keep = keep.cpu()
    out = {k: v[keep] for k, v in data.items() if k != "rles"}
    out["rles"] = [data["rles"][int(i)] for i in keep]
    return out


# ------------------------------------------------------------------------------------------------ the generator
class SamAutomaticMaskGenerator:
    """SA/automatic_mask_generator.py:35-372 with the reference's arguments, defaults, assertions, record keys and record
    order.  `model` is a SamEngine or a SamPredictor.  min_mask_region_area > 0 runs remove_small_regions on the GPU
    (no cv2); output_mode="coco_rle" needs pycocotools, imported lazily as the reference does."""

    def __init__(self, model, points_per_side: Optional[int] = 32, points_per_batch: int = 64,
                 pred_iou_thresh: float = 0.88, stability_score_thresh: float = 0.95,
                 stability_score_offset: float = 1.0, box_nms_thresh: float = 0.7, crop_n_layers: int = 0,
                 crop_nms_thresh: float = 0.7, crop_overlap_ratio: float = 512 / 1500,
                 crop_n_points_downscale_factor: int = 1, point_grids: Optional[List[np.ndarray]] = None,
                 min_mask_region_area: int = 0, output_mode: str = "binary_mask") -> None:
        assert (points_per_side is None) != (point_grids is None), \
            "Exactly one of points_per_side or point_grid must be provided."
        if points_per_side is not None:
            self.point_grids = build_all_layer_point_grids(points_per_side, crop_n_layers,
                                                           crop_n_points_downscale_factor)
        else:
            self.point_grids = point_grids
        assert output_mode in ["binary_mask", "uncompressed_rle", "coco_rle"], f"Unknown output_mode {output_mode}."
        if output_mode == "coco_rle":
            from pycocotools import mask as mask_utils  # type: ignore # noqa: F401
        self.predictor = model if isinstance(model, SamPredictor) else SamPredictor(model)
        self.points_per_batch = points_per_batch
        self.pred_iou_thresh = pred_iou_thresh
        self.stability_score_thresh = stability_score_thresh
        self.stability_score_offset = stability_score_offset
        self.box_nms_thresh = box_nms_thresh
        self.crop_n_layers = crop_n_layers
        self.crop_nms_thresh = crop_nms_thresh
        self.crop_overlap_ratio = crop_overlap_ratio
        self.crop_n_points_downscale_factor = crop_n_points_downscale_factor
        self.min_mask_region_area = min_mask_region_area
        self.output_mode = output_mode

    @torch.no_grad()
    def generate(self, image: np.ndarray) -> List[Dict[str, Any]]:
        """image HWC uint8 -> records {segmentation, area, bbox XYWH, predicted_iou, point_coords, stability_score,
        crop_box XYWH} (automatic_mask_generator.py:137-195)."""
        data = self._generate_masks(image)
        if self.min_mask_region_area > 0:
            data = self._postprocess_small_regions(data, self.min_mask_region_area,
                                                   max(self.box_nms_thresh, self.crop_nms_thresh))
        return self._records(data)

    def _postprocess_small_regions(self, data: Dict[str, Any], min_area: int, nms_thresh: float) -> Dict[str, Any]:
        """automatic_mask_generator.py:323-372: holes, then islands, below min_area out of every mask; box NMS again with
        score 1 for the masks that needed no change and 0 for the others; new RLE and box for the changed ones kept."""
        if len(data["rles"]) == 0:
            return data
        dev = self.predictor.engine.dev
        h, w = data["rles"][0]["size"]
        masks = torch.from_numpy(np.stack([rle_to_mask(rle) for rle in data["rles"]])).to(dev)
        planes, changed = ops.remove_small_regions(ops.pack_col_planes(masks), h, w, int(min_area))
        del masks
        boxes = batched_mask_to_box(unpack_col_planes(planes, h)).cpu()
        changed = changed.cpu()
        keep = self._nms(boxes, (~changed).float(), nms_thresh)
        redo = [int(i) for i in keep if changed[i]]
        if redo:
            counts = ops.mask_rle(planes, h, w, torch.tensor(redo, dtype=torch.int32, device=dev))
            for i, c in zip(redo, counts):
                data["rles"][i] = {"size": [h, w], "counts": c}
                data["boxes"][i] = boxes[i]
        return _filter(data, keep)

    def _records(self, data: Dict[str, Any]) -> List[Dict[str, Any]]:
        if self.output_mode == "coco_rle":
            segs = [coco_encode_rle(rle) for rle in data["rles"]]
        elif self.output_mode == "binary_mask":
            segs = [rle_to_mask(rle) for rle in data["rles"]]
        else:
            segs = data["rles"]
        boxes, crops = data["boxes"].numpy(), data["crop_boxes"].numpy()
        iou, stab, pts = data["iou_preds"].numpy(), data["stability_score"].numpy(), data["points"].numpy()
        return [{
            "segmentation": segs[i],
            "area": area_from_rle(data["rles"][i]),
            "bbox": box_xyxy_to_xywh(boxes[i]).tolist(),
            "predicted_iou": iou[i].item(),
            "point_coords": [pts[i].tolist()],
            "stability_score": stab[i].item(),
            "crop_box": box_xyxy_to_xywh(crops[i]).tolist(),
        } for i in range(len(segs))]

    def _generate_masks(self, image: np.ndarray) -> Dict[str, Any]:
        orig_size = tuple(image.shape[:2])
        crop_boxes, layer_idxs = generate_crop_boxes(orig_size, self.crop_n_layers, self.crop_overlap_ratio)
        parts = [self._process_crop(image, cb, li, orig_size) for cb, li in zip(crop_boxes, layer_idxs)]
        data = _cat(parts, extra=("crop_boxes",))
        if len(crop_boxes) > 1:                              # between crops: prefer masks from smaller crops
            scores = 1 / box_area(data["crop_boxes"])
            data = _filter(data, self._nms(data["boxes"], scores, self.crop_nms_thresh))
        return data

    def _nms(self, boxes: torch.Tensor, scores: torch.Tensor, thresh: float) -> torch.Tensor:
        dev = self.predictor.engine.dev
        return ops.box_nms(boxes.float().contiguous().to(dev), scores.float().contiguous().to(dev), thresh).cpu()

    def _process_crop(self, image: np.ndarray, crop_box: List[int], crop_layer_idx: int,
                      orig_size: Tuple[int, int]) -> Dict[str, Any]:
        x0, y0, x1, y1 = crop_box
        self.predictor.set_image(image[y0:y1, x0:x1, :])
        try:
            return self._process_crop_features(self.predictor.features, self.predictor.input_size, crop_box, orig_size,
                                               crop_layer_idx)
        finally:
            self.predictor.reset_image()

    def _process_crop_features(self, features: torch.Tensor, input_hw: Tuple[int, int], crop_box: List[int],
                               orig_hw: Tuple[int, int], crop_layer_idx: int = 0) -> Dict[str, Any]:
        """_process_crop after set_image (automatic_mask_generator.py:238-264): the point batches through the decoder and
        the tail, the NMS inside the crop, the return to the image frame.  features: [4096, 256] of the crop."""
        pred, eng = self.predictor, self.predictor.engine
        x0, y0, x1, y1 = crop_box
        crop_hw = (y1 - y0, x1 - x0)
        points_for_image = self.point_grids[crop_layer_idx] * np.array(crop_hw)[None, ::-1]
        emb = features.reshape(1, eng.T, -1)
        parts = []
        for b in range(0, len(points_for_image), self.points_per_batch):
            points = points_for_image[b: b + self.points_per_batch]
            in_points = torch.as_tensor(pred.transform.apply_coords(points, crop_hw), dtype=torch.float, device=eng.dev)
            in_labels = torch.ones(in_points.shape[0], dtype=torch.int, device=eng.dev)
            low, iou = eng.decode_prompts(emb, [0] * len(points), in_points[:, None, :], in_labels[:, None],
                                          multimask_output=True)
            part = self._process_low_res(low, iou, points, input_hw, crop_box, orig_hw)
            part["cand"] += 3 * b
            parts.append(part)
        data = _cat(parts)
        data = _filter(data, self._nms(data["boxes"], data["iou_preds"], self.box_nms_thresh))
        data["boxes"] = uncrop_boxes_xyxy(data["boxes"], crop_box)
        data["points"] = uncrop_points(data["points"], crop_box)
        data["crop_boxes"] = torch.tensor([crop_box for _ in range(len(data["rles"]))], dtype=torch.int64).reshape(-1, 4)
        return data

    def _process_low_res(self, low: torch.Tensor, iou: torch.Tensor, points: np.ndarray, input_hw: Tuple[int, int],
                         crop_box: List[int], orig_hw: Tuple[int, int]) -> Dict[str, Any]:
        """_process_batch after the decoder (automatic_mask_generator.py:286-321): low [n, 3, S, S] f32 low-res logits and
        iou [n, 3] predictions on the device, points [n, 2] in crop pixels.  -> the batch's surviving candidates on the
        host: rles, boxes (crop frame), iou_preds, stability_score, points, and cand = 3 * point + mask index."""
        cfg = self.predictor.cfg
        n, M, S = low.shape[0], low.shape[1], low.shape[-1]
        x0, y0, x1, y1 = crop_box
        orig_h, orig_w = orig_hw
        low = low.reshape(n * M, S, S)
        iou = iou.reshape(n * M).contiguous()
        # predicted-IoU filter on the device: kept candidates first, in their order; no size comes back to the host
        keep = iou > self.pred_iou_thresh if self.pred_iou_thresh > 0.0 else torch.ones_like(iou, dtype=torch.bool)
        order = torch.argsort(~keep, stable=True).to(torch.int32)
        count = keep.sum().to(torch.int32).reshape(1)
        table, planes = ops.sam_amg_stats(low, cfg.img_size, input_hw, (y1 - y0, x1 - x0), cfg.mask_threshold,
                                          self.stability_score_offset, (x0, y0), orig_hw, index=order, count=count)
        host = torch.cat([table.reshape(-1), count, order, iou.view(torch.int32)]).cpu()      # the one copy
        m = int(host[8 * n * M])
        table = host[:8 * n * M].reshape(n * M, 8)[:m]
        cand = host[8 * n * M + 1: 9 * n * M + 1][:m].long()
        iou_h = host[9 * n * M + 1:].view(torch.float32)[cand]
        # calculate_stability_score: int32 / int32, the reference's float
        stability = table[:, 0] / table[:, 1]
        sel = torch.arange(m)
        if self.stability_score_thresh > 0.0:
            sel = sel[stability >= self.stability_score_thresh]
        boxes = table[:, 3:7].long()
        near = is_box_near_crop_edge(boxes[sel], crop_box, [0, 0, orig_w, orig_h])
        if not torch.all(~near):
            sel = sel[~near]
        counts = ops.mask_rle(planes, orig_h, orig_w, sel.to(torch.int32).to(low.device)) if len(sel) else []
        pts = torch.as_tensor(points.repeat(M, axis=0))
        return dict(rles=[{"size": [orig_h, orig_w], "counts": c} for c in counts], iou_preds=iou_h[sel],
                    points=pts[cand[sel]], stability_score=stability[sel], boxes=boxes[sel], cand=cand[sel])
