"""Generate tests/golden/amg_small.npz: the REFERENCE's own segment_anything/utils/amg.py
(/root/reference/InkLayer/third_party/segment-anything/segment_anything/utils/amg.py) on the CPU, on seeded random logits
of odd sizes, with the inputs and outputs of calculate_stability_score, batched_mask_to_box, mask_to_rle_pytorch,
rle_to_mask, area_from_rle, build_all_layer_point_grids, generate_crop_boxes, is_box_near_crop_edge, uncrop_masks,
uncrop_boxes_xyxy, uncrop_points and box_xyxy_to_xywh.  Build-container only, data only.

utils/amg.py imports numpy and torch at module level and cv2 / pycocotools inside the functions that need them, so the
file is loaded by path without any stub.  NOT pinned here, because the reference takes them from libraries that are not
installed: batched_nms (torchvision) and remove_small_regions (cv2.connectedComponentsWithStats) - tests/amg_ref.py
restates both from their definitions and tests/test_amg_cpu.py checks the restatements on hand-made cases.
"""
import importlib.util
from pathlib import Path

import numpy as np
import torch

HERE = Path(__file__).resolve().parent
AMG = "/root/reference/InkLayer/third_party/segment-anything/segment_anything/utils/amg.py"
SEED = 2024


def _smooth(rs, n, h, w):
    x = torch.from_numpy(rs.standard_normal((n, 1, h, w)).astype(np.float32))
    k = torch.ones(1, 1, 5, 5) / 25
    return torch.nn.functional.conv2d(x, k, padding=2)[:, 0] * 6.0


def main():
    spec = importlib.util.spec_from_file_location("ref_amg", AMG)
    A = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(A)
    rs = np.random.RandomState(SEED)
    h, w = 37, 53
    logits = _smooth(rs, 6, h, w)
    logits[1] = -3.0                       # empty at every threshold
    logits[2] = 3.0                        # full at every threshold
    logits[3, 0, 0] = 2.5                  # starts with a one
    logits[4, :, :] = -2.0
    logits[4, h - 1, w - 1] = 2.0          # ends with a one, nothing else
    out = dict(seed=np.int64(SEED), logits=logits.numpy())
    out["stability"] = A.calculate_stability_score(logits, 0.0, 1.0).numpy()
    out["stability_off03"] = A.calculate_stability_score(logits, 0.25, 0.3).numpy()
    masks = logits > 0.0
    out["boxes"] = A.batched_mask_to_box(masks).numpy()
    rles = A.mask_to_rle_pytorch(masks)
    out["rle_sizes"] = np.array([r["size"] for r in rles])
    out["rle_lens"] = np.array([len(r["counts"]) for r in rles])
    out["rle_counts"] = np.concatenate([np.asarray(r["counts"], dtype=np.int64) for r in rles])
    out["rle_masks"] = np.stack([A.rle_to_mask(r) for r in rles])
    out["rle_areas"] = np.array([A.area_from_rle(r) for r in rles])
    grids = A.build_all_layer_point_grids(8, 2, 2)
    for i, g in enumerate(grids):
        out[f"grid{i}"] = g
    cb, li = A.generate_crop_boxes((600, 801), 2, 512 / 1500)
    out["crop_boxes"], out["crop_layers"] = np.array(cb), np.array(li)
    crop = cb[6]
    bx = torch.from_numpy(rs.randint(0, 150, (40, 4)).astype(np.int64))
    bx[:, 2:] += bx[:, :2]
    bx[:8] = torch.tensor([0, 0, crop[2] - crop[0] - 1, crop[3] - crop[1] - 1])
    bx[8:16, 0] = torch.arange(15, 23)      # around the 20-pixel tolerance
    out["edge_crop"], out["edge_orig"], out["edge_boxes"] = np.array(crop), np.array([0, 0, 801, 600]), bx.numpy()
    out["edge_near"] = A.is_box_near_crop_edge(bx, crop, [0, 0, 801, 600]).numpy()
    out["edge_near_full"] = A.is_box_near_crop_edge(bx, [0, 0, 801, 600], [0, 0, 801, 600]).numpy()
    out["uncrop_box"] = np.array([11, 7, 11 + w, 7 + h])
    out["uncrop_masks"] = A.uncrop_masks(masks, [11, 7, 11 + w, 7 + h], 60, 70).numpy()
    out["uncrop_boxes"] = A.uncrop_boxes_xyxy(bx, crop).numpy()
    pts = torch.from_numpy(rs.uniform(0, 100, (5, 2)))
    out["points"], out["uncrop_points"] = pts.numpy(), A.uncrop_points(pts, crop).numpy()
    out["xywh"] = np.stack([A.box_xyxy_to_xywh(b).numpy() for b in bx[:5]])
    path = HERE / "amg_small.npz"
    np.savez_compressed(path, **out)
    print("wrote", path, path.stat().st_size >> 10, "KiB")


if __name__ == "__main__":
    main()
