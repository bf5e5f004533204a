"""Plain torch / numpy restatement of the reference's automatic mask generator (SA/automatic_mask_generator.py and
SA/utils/amg.py), the yardstick of tests/test_amg_cpu.py (which pins it to tests/golden/amg_small.npz, recorded from the
reference's own functions) and tests/test_amg_gpu.py.  Every function states the reference's arithmetic on the
reference's dtypes; nothing here calls the project's kernels.  Two pieces have no recorded golden because the reference
takes them from libraries that are not installed (torchvision, cv2), so they are restated from their definitions:
  * nms: torchvision.ops.nms for one category, ties in score to the lower index (see include/inklayer_hip.h);
  * remove_small_regions: over scipy.ndimage.label with a 3 x 3 structure, labels renumbered in raster order of each
    component's first pixel, which is cv2.connectedComponentsWithStats' order.
The model is any object with SamPredictor's set_image / reset_image / predict_torch / transform / cfg.mask_threshold."""
import math
from copy import deepcopy
from itertools import product

import numpy as np
import torch


# ------------------------------------------------------------------------------------------------ SA/utils/amg.py
def uncrop_boxes_xyxy(boxes, crop_box):
    x0, y0, _, _ = crop_box
    return boxes + torch.tensor([[x0, y0, x0, y0]], device=boxes.device)


def uncrop_points(points, crop_box):
    x0, y0, _, _ = crop_box
    return points + torch.tensor([[x0, y0]], device=points.device)


def is_box_near_crop_edge(boxes, crop_box, orig_box, atol=20.0):
    crop_t = torch.as_tensor(crop_box, dtype=torch.float, device=boxes.device)
    orig_t = torch.as_tensor(orig_box, dtype=torch.float, device=boxes.device)
    boxes = uncrop_boxes_xyxy(boxes, crop_box).float()
    near_crop = torch.isclose(boxes, crop_t[None, :], atol=atol, rtol=0)
    near_image = torch.isclose(boxes, orig_t[None, :], atol=atol, rtol=0)
    return torch.any(torch.logical_and(near_crop, ~near_image), dim=1)


def box_xyxy_to_xywh(box):
    out = deepcopy(box)
    out[2] = out[2] - out[0]
    out[3] = out[3] - out[1]
    return out


def mask_to_rle(masks):
    """mask_to_rle_pytorch: bool [b, h, w] -> [{"size": [h, w], "counts": [...]}] (column-major runs)."""
    b, h, w = masks.shape
    flat = masks.permute(0, 2, 1).flatten(1)
    out = []
    for i in range(b):
        cur = flat[i]
        change = (cur[1:] ^ cur[:-1]).nonzero()[:, 0]
        idxs = torch.cat([torch.zeros(1, dtype=change.dtype, device=change.device), change + 1,
                          torch.full((1,), h * w, dtype=change.dtype, device=change.device)])
        counts = [] if cur[0] == 0 else [0]
        counts.extend((idxs[1:] - idxs[:-1]).cpu().tolist())
        out.append({"size": [h, w], "counts": counts})
    return out


def rle_to_mask(rle):
    h, w = rle["size"]
    mask = np.empty(h * w, dtype=bool)
    idx, parity = 0, False
    for count in rle["counts"]:
        mask[idx: idx + count] = parity
        idx += count
        parity ^= True
    return mask.reshape(w, h).transpose()


def area_from_rle(rle):
    return sum(rle["counts"][1::2])


def calculate_stability_score(masks, mask_threshold, threshold_offset):
    inter = (masks > (mask_threshold + threshold_offset)).sum(-1, dtype=torch.int16).sum(-1, dtype=torch.int32)
    union = (masks > (mask_threshold - threshold_offset)).sum(-1, dtype=torch.int16).sum(-1, dtype=torch.int32)
    return inter / union


def stability_counts(masks, mask_threshold, threshold_offset):
    """The two integers calculate_stability_score divides (what the stats kernel's table holds)."""
    inter = (masks > (mask_threshold + threshold_offset)).sum(-1, dtype=torch.int16).sum(-1, dtype=torch.int32)
    union = (masks > (mask_threshold - threshold_offset)).sum(-1, dtype=torch.int16).sum(-1, dtype=torch.int32)
    return inter, union


def build_point_grid(n_per_side):
    offset = 1 / (2 * n_per_side)
    side = np.linspace(offset, 1 - offset, n_per_side)
    px = np.tile(side[None, :], (n_per_side, 1))
    py = np.tile(side[:, None], (1, n_per_side))
    return np.stack([px, py], axis=-1).reshape(-1, 2)


def build_all_layer_point_grids(n_per_side, n_layers, scale_per_layer):
    return [build_point_grid(int(n_per_side / (scale_per_layer ** i))) for i in range(n_layers + 1)]


def generate_crop_boxes(im_size, n_layers, overlap_ratio):
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


def uncrop_masks(masks, crop_box, orig_h, orig_w):
    x0, y0, x1, y1 = crop_box
    if x0 == 0 and y0 == 0 and x1 == orig_w and y1 == orig_h:
        return masks
    pad_x, pad_y = orig_w - (x1 - x0), orig_h - (y1 - y0)
    return torch.nn.functional.pad(masks, (x0, pad_x - x0, y0, pad_y - y0), value=0)


def batched_mask_to_box(masks):
    """bool [c, h, w] -> int64 [c, 4] xyxy, inclusive maxima, [0, 0, 0, 0] for an empty mask."""
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
    out = torch.stack([left, top, right, bottom], dim=-1)
    return out * (~empty).unsqueeze(-1)


def remove_small_regions(mask, area_thresh, mode):
    from scipy import ndimage
    assert mode in ("holes", "islands")
    correct_holes = mode == "holes"
    working = (correct_holes ^ mask).astype(np.uint8)
    lab, n = ndimage.label(working, structure=np.ones((3, 3), dtype=np.int32))
    # cv2 numbers components in raster order of their first pixel
    flat = lab.ravel()
    first = np.full(n + 1, flat.size, dtype=np.int64)
    np.minimum.at(first, flat, np.arange(flat.size))
    order = np.argsort(first[1:], kind="stable")
    remap = np.zeros(n + 1, dtype=np.int64)
    remap[order + 1] = np.arange(1, n + 1)
    regions = remap[lab]
    n_labels = n + 1
    sizes = np.bincount(regions.ravel(), minlength=n_labels)[1:]
    small = [i + 1 for i, s in enumerate(sizes) if s < area_thresh]
    if len(small) == 0:
        return mask, False
    fill = [0] + small
    if not correct_holes:
        fill = [i for i in range(n_labels) if i not in fill]
        if len(fill) == 0:
            fill = [int(np.argmax(sizes)) + 1]
    return np.isin(regions, fill), True


# ------------------------------------------------------------------------------------------------ torchvision.ops.nms
def nms(boxes, scores, iou_threshold):
    """boxes f32 [n, 4] xyxy, scores f32 [n] -> int64 kept indices in descending score order (stable: ties to the lower
    index).  iou = inter / (a_i + a_j - inter) in f32; suppressed when iou > iou_threshold."""
    boxes = boxes.detach().cpu().float().numpy()
    scores = scores.detach().cpu().float().numpy()
    n = boxes.shape[0]
    if n == 0:
        return torch.empty((0,), dtype=torch.int64)
    order = np.argsort(-scores.astype(np.float64), kind="stable")
    b = boxes[order]
    area = (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
    removed = np.zeros(n, dtype=bool)
    keep = []
    with np.errstate(invalid="ignore", divide="ignore"):
        for i in range(n):
            if removed[i]:
                continue
            keep.append(order[i])
            xx1 = np.maximum(b[i, 0], b[i + 1:, 0])
            yy1 = np.maximum(b[i, 1], b[i + 1:, 1])
            xx2 = np.minimum(b[i, 2], b[i + 1:, 2])
            yy2 = np.minimum(b[i, 3], b[i + 1:, 3])
            w = np.maximum(np.float32(0), xx2 - xx1)
            h = np.maximum(np.float32(0), yy2 - yy1)
            inter = w * h
            iou = inter / (area[i] + area[i + 1:] - inter)
            removed[i + 1:] |= iou > np.float32(iou_threshold)
    return torch.as_tensor(np.asarray(keep, dtype=np.int64))


def box_area(boxes):
    return (boxes[:, 2] - boxes[:, 0]) * (boxes[:, 3] - boxes[:, 1])


# ------------------------------------------------------------------------------------------------ MaskData
class MaskData:
    def __init__(self, **kw):
        self._stats = dict(**kw)

    def __setitem__(self, k, v):
        self._stats[k] = v

    def __delitem__(self, k):
        del self._stats[k]

    def __getitem__(self, k):
        return self._stats[k]

    def __contains__(self, k):
        return k in self._stats

    def items(self):
        return self._stats.items()

    def filter(self, keep):
        for k, v in self._stats.items():
            if v is None:
                self._stats[k] = None
            elif isinstance(v, torch.Tensor):
                self._stats[k] = v[torch.as_tensor(keep, device=v.device)]
            elif isinstance(v, np.ndarray):
                self._stats[k] = v[keep.detach().cpu().numpy()]
            elif isinstance(v, list) and keep.dtype == torch.bool:
                self._stats[k] = [a for i, a in enumerate(v) if keep[i]]
            elif isinstance(v, list):
                self._stats[k] = [v[i] for i in keep]
            else:
                raise TypeError(k)

    def cat(self, new):
        for k, v in new.items():
            if k not in self._stats or self._stats[k] is None:
                self._stats[k] = deepcopy(v)
            elif isinstance(v, torch.Tensor):
                self._stats[k] = torch.cat([self._stats[k], v], dim=0)
            elif isinstance(v, np.ndarray):
                self._stats[k] = np.concatenate([self._stats[k], v], axis=0)
            elif isinstance(v, list):
                self._stats[k] = self._stats[k] + deepcopy(v)
            else:
                raise TypeError(k)

    def to_numpy(self):
        for k, v in self._stats.items():
            if isinstance(v, torch.Tensor):
                self._stats[k] = v.detach().cpu().numpy()


# ------------------------------------------------------------------------------------------------ the generator
class AmgRef:
    """SamAutomaticMaskGenerator restated.  `stats` (a dict) collects what the tests count: candidates seen and the
    number each filter rejected."""

    def __init__(self, predictor, points_per_side=32, points_per_batch=64, pred_iou_thresh=0.88,
                 stability_score_thresh=0.95, stability_score_offset=1.0, box_nms_thresh=0.7, crop_n_layers=0,
                 crop_nms_thresh=0.7, crop_overlap_ratio=512 / 1500, crop_n_points_downscale_factor=1, point_grids=None,
                 min_mask_region_area=0, output_mode="binary_mask", mask_threshold=0.0):
        assert (points_per_side is None) != (point_grids is None)
        if points_per_side is not None:
            self.point_grids = build_all_layer_point_grids(points_per_side, crop_n_layers, crop_n_points_downscale_factor)
        else:
            self.point_grids = point_grids
        assert output_mode in ("binary_mask", "uncompressed_rle", "coco_rle")
        self.predictor = predictor
        self.points_per_batch = points_per_batch
        self.pred_iou_thresh = pred_iou_thresh
        self.stability_score_thresh = stability_score_thresh
        self.stability_score_offset = stability_score_offset
        self.box_nms_thresh = box_nms_thresh
        self.crop_n_layers = crop_n_layers
        self.crop_nms_thresh = crop_nms_thresh
        self.crop_overlap_ratio = crop_overlap_ratio
        self.min_mask_region_area = min_mask_region_area
        self.output_mode = output_mode
        self.mask_threshold = mask_threshold
        self.stats = {"candidates": 0, "rej_iou": 0, "rej_stability": 0, "rej_edge": 0, "rej_nms": 0}

    @torch.no_grad()
    def generate(self, image):
        data = self._generate_masks(image)
        return self.records(data)

    def records(self, data):
        if self.min_mask_region_area > 0:
            data = self.postprocess_small_regions(data, self.min_mask_region_area,
                                                  max(self.box_nms_thresh, self.crop_nms_thresh))
        if self.output_mode == "binary_mask":
            segs = [rle_to_mask(r) for r in data["rles"]]
        else:
            segs = data["rles"]
        out = []
        for i in range(len(segs)):
            out.append({
                "segmentation": segs[i],
                "area": area_from_rle(data["rles"][i]),
                "bbox": box_xyxy_to_xywh(data["boxes"][i]).tolist(),
                "predicted_iou": data["iou_preds"][i].item(),
                "point_coords": [data["points"][i].tolist()],
                "stability_score": data["stability_score"][i].item(),
                "crop_box": box_xyxy_to_xywh(data["crop_boxes"][i]).tolist(),
            })
        return out

    def _generate_masks(self, image):
        orig_size = image.shape[:2]
        crop_boxes, layer_idxs = generate_crop_boxes(orig_size, self.crop_n_layers, self.crop_overlap_ratio)
        data = MaskData()
        for crop_box, layer_idx in zip(crop_boxes, layer_idxs):
            data.cat(self._process_crop(image, crop_box, layer_idx, orig_size))
        return self.merge_crops(data, len(crop_boxes))

    def merge_crops(self, data, n_crops):
        if n_crops > 1 and len(data["rles"]) > 0:
            scores = 1 / box_area(data["crop_boxes"])
            keep = nms(data["boxes"].float(), scores.float(), self.crop_nms_thresh)
            data.filter(keep)
        data.to_numpy()
        return data

    def _process_crop(self, image, crop_box, crop_layer_idx, orig_size):
        x0, y0, x1, y1 = crop_box
        cropped = image[y0:y1, x0:x1, :]
        cropped_size = cropped.shape[:2]
        self.predictor.set_image(cropped)
        points_scale = np.array(cropped_size)[None, ::-1]
        points_for_image = self.point_grids[crop_layer_idx] * points_scale
        batches = []
        for b in range(0, len(points_for_image), self.points_per_batch):
            points = points_for_image[b: b + self.points_per_batch]
            tp = self.predictor.transform.apply_coords(points, cropped_size)
            in_points = torch.as_tensor(tp, device=self.predictor.engine.dev, dtype=torch.float)
            in_labels = torch.ones(in_points.shape[0], dtype=torch.int, device=in_points.device)
            masks, iou_preds, _ = self.predictor.predict_torch(in_points[:, None, :], in_labels[:, None],
                                                               multimask_output=True, return_logits=True)
            batches.append(self.process_logits(masks, iou_preds, points, crop_box, orig_size))
        self.predictor.reset_image()
        return self.finish_crop(batches, crop_box)

    def process_logits(self, masks, iou_preds, points, crop_box, orig_size):
        """_process_batch after the model: masks f32 [n, 3, h, w] full-resolution logits of the crop, iou_preds [n, 3]."""
        orig_h, orig_w = orig_size
        data = MaskData(masks=masks.flatten(0, 1), iou_preds=iou_preds.flatten(0, 1),
                        points=torch.as_tensor(points.repeat(masks.shape[1], axis=0)))
        self.stats["candidates"] += len(data["iou_preds"])
        if self.pred_iou_thresh > 0.0:
            keep = data["iou_preds"] > self.pred_iou_thresh
            self.stats["rej_iou"] += int((~keep).sum())
            data.filter(keep)
        data["stability_score"] = calculate_stability_score(data["masks"], self.mask_threshold,
                                                            self.stability_score_offset)
        if self.stability_score_thresh > 0.0:
            keep = data["stability_score"] >= self.stability_score_thresh
            self.stats["rej_stability"] += int((~keep).sum())
            data.filter(keep)
        data["masks"] = data["masks"] > self.mask_threshold
        data["boxes"] = batched_mask_to_box(data["masks"])
        keep = ~is_box_near_crop_edge(data["boxes"], crop_box, [0, 0, orig_w, orig_h])
        if not torch.all(keep):
            self.stats["rej_edge"] += int((~keep).sum())
            data.filter(keep)
        data["masks"] = uncrop_masks(data["masks"], crop_box, orig_h, orig_w)
        data["rles"] = mask_to_rle(data["masks"])
        del data["masks"]
        return data

    def finish_crop(self, batches, crop_box):
        data = MaskData()
        for b in batches:
            data.cat(b)
        keep = nms(data["boxes"].float(), data["iou_preds"], self.box_nms_thresh)
        self.stats["rej_nms"] += len(data["rles"]) - len(keep)
        data.filter(keep)
        data["boxes"] = uncrop_boxes_xyxy(data["boxes"], crop_box)
        data["points"] = uncrop_points(data["points"], crop_box)
        data["crop_boxes"] = torch.tensor([crop_box for _ in range(len(data["rles"]))]).reshape(-1, 4)
        return data

    @staticmethod
    def postprocess_small_regions(mask_data, min_area, nms_thresh):
        if len(mask_data["rles"]) == 0:
            return mask_data
        new_masks, scores = [], []
        for rle in mask_data["rles"]:
            mask = rle_to_mask(rle)
            mask, changed = remove_small_regions(mask, min_area, mode="holes")
            unchanged = not changed
            mask, changed = remove_small_regions(mask, min_area, mode="islands")
            unchanged = unchanged and not changed
            new_masks.append(torch.as_tensor(mask).unsqueeze(0))
            scores.append(float(unchanged))
        masks = torch.cat(new_masks, dim=0)
        boxes = batched_mask_to_box(masks)
        keep = nms(boxes.float(), torch.as_tensor(scores), nms_thresh)
        for i in keep:
            if scores[i] == 0.0:
                mask_data["rles"][i] = mask_to_rle(masks[i].unsqueeze(0))[0]
                mask_data["boxes"][i] = boxes[i].numpy()
        mask_data.filter(keep)
        return mask_data
