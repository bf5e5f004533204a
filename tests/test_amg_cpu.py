"""tests/amg_ref.py (the restatement of the reference's automatic mask generator that tests/test_amg_gpu.py compares the
GPU path against) is the reference: exact equality with tests/golden/amg_small.npz, which make_amg_golden.py recorded
from the reference's own segment_anything/utils/amg.py; and the two restatements that have no recorded golden (box NMS,
remove_small_regions) on hand-made cases.  The host-side pieces of inklayer_amd/amg.py are held to the same golden."""
from pathlib import Path

import numpy as np
import pytest
import torch

import amg_ref as R

G = np.load(Path(__file__).resolve().parent / "golden" / "amg_small.npz")


def _rles():
    out, o = [], 0
    for size, n in zip(G["rle_sizes"], G["rle_lens"]):
        out.append({"size": size.tolist(), "counts": G["rle_counts"][o:o + n].tolist()})
        o += n
    return out


def _host_modules():
    from inklayer_amd import amg
    return [R, amg]


def test_stability_boxes_match_reference():
    logits = torch.from_numpy(G["logits"])
    assert np.array_equal(R.calculate_stability_score(logits, 0.0, 1.0).numpy(), G["stability"], equal_nan=True)
    assert np.array_equal(R.calculate_stability_score(logits, 0.25, 0.3).numpy(), G["stability_off03"], equal_nan=True)
    i, u = R.stability_counts(logits, 0.0, 1.0)
    assert np.array_equal((i / u).numpy(), G["stability"], equal_nan=True)
    boxes = R.batched_mask_to_box(logits > 0.0)
    assert boxes.dtype == torch.int64 and np.array_equal(boxes.numpy(), G["boxes"])
    assert G["boxes"][1].tolist() == [0, 0, 0, 0] and G["boxes"][2].tolist() == [0, 0, 52, 36]


def test_rle_matches_reference():
    masks = torch.from_numpy(G["logits"]) > 0.0
    assert R.mask_to_rle(masks) == _rles()
    rles = _rles()
    assert rles[1]["counts"] == [37 * 53] and rles[2]["counts"] == [0, 37 * 53] and rles[3]["counts"][0] == 0
    for mod in _host_modules():
        for i, r in enumerate(rles):
            assert np.array_equal(mod.rle_to_mask(r), G["rle_masks"][i])
            assert np.array_equal(mod.rle_to_mask(r), masks[i].numpy())
            assert mod.area_from_rle(r) == G["rle_areas"][i] == int(masks[i].sum())


def test_grids_and_crop_boxes_match_reference():
    for mod in _host_modules():
        grids = mod.build_all_layer_point_grids(8, 2, 2)
        assert len(grids) == 3
        for i, g in enumerate(grids):
            assert np.array_equal(g, G[f"grid{i}"])
        cb, li = mod.generate_crop_boxes((600, 801), 2, 512 / 1500)
        assert np.array_equal(np.array(cb), G["crop_boxes"]) and np.array_equal(np.array(li), G["crop_layers"])


def test_edge_filter_and_uncrop_match_reference():
    bx = torch.from_numpy(G["edge_boxes"])
    crop, orig = G["edge_crop"].tolist(), G["edge_orig"].tolist()
    assert G["edge_near"].any() and not G["edge_near"].all()
    for mod in _host_modules():
        assert np.array_equal(mod.is_box_near_crop_edge(bx, crop, orig).numpy(), G["edge_near"])
        assert np.array_equal(mod.is_box_near_crop_edge(bx, orig, orig).numpy(), G["edge_near_full"])
        assert np.array_equal(mod.uncrop_boxes_xyxy(bx, crop).numpy(), G["uncrop_boxes"])
        assert np.array_equal(mod.uncrop_points(torch.from_numpy(G["points"]), crop).numpy(), G["uncrop_points"])
        assert np.array_equal(np.stack([mod.box_xyxy_to_xywh(b).numpy() for b in bx[:5]]), G["xywh"])
    masks = torch.from_numpy(G["logits"]) > 0.0
    assert np.array_equal(R.uncrop_masks(masks, G["uncrop_box"].tolist(), 60, 70).numpy(), G["uncrop_masks"])


# ------------------------------------------------------------------------------------------------ NMS restatement
def test_nms_hand_made():
    f = torch.tensor
    # two identical boxes and a distant one: the higher score wins, order is descending score
    b = f([[0., 0., 10., 10.], [0., 0., 10., 10.], [20., 20., 30., 30.]])
    assert R.nms(b, f([0.5, 0.9, 0.1]), 0.5).tolist() == [1, 2]
    # ties in score go to the lower index
    assert R.nms(b, f([0.5, 0.5, 0.5]), 0.5).tolist() == [0, 2]
    assert R.nms(b.flip(0), f([1.0, 0.0, 0.0]), 0.5).tolist() == [0, 1]
    # iou == thr is kept: [0,0,2,1] and [0,0,1,1] have inter 1, union 2 -> 0.5 exactly
    c = f([[0., 0., 2., 1.], [0., 0., 1., 1.]])
    assert R.nms(c, f([0.9, 0.8]), 0.5).tolist() == [0, 1]
    assert R.nms(c, f([0.9, 0.8]), 0.49).tolist() == [0]
    # zero-area boxes: iou with themselves is 0 / 0 = nan, never > thr, so nothing is suppressed ([0,0,0,0] of empty masks)
    z = f([[0., 0., 0., 0.], [0., 0., 0., 0.], [5., 5., 5., 9.]])
    assert R.nms(z, f([0.3, 0.2, 0.1]), 0.0).tolist() == [0, 1, 2]
    # threshold 1.0 keeps everything (iou <= 1)
    assert R.nms(b, f([0.1, 0.2, 0.3]), 1.0).tolist() == [2, 1, 0]
    # chains: a suppressed box suppresses nobody
    d = f([[0., 0., 10., 10.], [4., 0., 14., 10.], [8., 0., 18., 10.]])
    assert R.nms(d, f([0.9, 0.8, 0.7]), 0.4).tolist() == [0, 2]
    assert R.nms(torch.zeros(0, 4), torch.zeros(0), 0.7).tolist() == []
    assert R.nms(b[:1], f([0.3]), 0.7).tolist() == [0]


# ------------------------------------------------------------------------------------------------ small regions
def test_remove_small_regions_hand_made():
    m = np.zeros((12, 16), dtype=bool)
    m[1:9, 1:9] = True
    m[4, 4] = False                     # a hole of area 1
    m[10, 12:14] = True                 # an island of area 2
    out, changed = R.remove_small_regions(m, 2, "holes")
    assert changed and out[4, 4] and out.sum() == m.sum() + 1
    out2, changed = R.remove_small_regions(m, 1, "holes")
    assert not changed and out2 is m
    out3, changed = R.remove_small_regions(m, 3, "islands")
    assert changed and not out3[10, 12:14].any() and out3[1:9, 1:9].sum() == 63
    out4, changed = R.remove_small_regions(m, 2, "islands")
    assert not changed and out4 is m
    # 8-connectivity: a diagonal neighbour belongs to the island
    d = np.zeros((6, 6), dtype=bool)
    d[1, 1] = d[2, 2] = d[3, 3] = True
    d[0, 5] = True
    out5, changed = R.remove_small_regions(d, 2, "islands")
    assert changed and out5.sum() == 3 and not out5[0, 5]


def test_remove_small_regions_all_small_keeps_first_largest():
    m = np.zeros((8, 20), dtype=bool)
    m[5, 0:3] = True                    # area 3, first pixel later in raster order than the next one
    m[1, 10:13] = True                  # area 3, first in raster order: label 1
    m[7, 17] = True
    out, changed = R.remove_small_regions(m, 100, "islands")
    assert changed and out[1, 10:13].all() and out.sum() == 3
    # label order is raster order of the first pixel, not scipy's (identical here) nor size order
    m2 = np.zeros((8, 20), dtype=bool)
    m2[2, 5:7] = True
    m2[4, 0:4] = True                   # the largest
    out, changed = R.remove_small_regions(m2, 100, "islands")
    assert changed and out[4, 0:4].all() and out.sum() == 4
    e = np.zeros((4, 4), dtype=bool)
    out, changed = R.remove_small_regions(e, 5, "islands")
    assert not changed and not out.any()


def test_generator_argument_checks():
    from inklayer_amd import amg
    with pytest.raises(AssertionError):
        amg.SamAutomaticMaskGenerator(None, points_per_side=8, point_grids=[np.zeros((1, 2))])
    with pytest.raises(AssertionError):
        amg.SamAutomaticMaskGenerator(None, points_per_side=None, point_grids=None)
    with pytest.raises(AssertionError, match="Unknown output_mode"):
        amg.SamAutomaticMaskGenerator(None, output_mode="polygons")
    import importlib.util
    if importlib.util.find_spec("pycocotools") is None:          # imported lazily, as the reference does
        with pytest.raises(ImportError):
            amg.SamAutomaticMaskGenerator(None, output_mode="coco_rle")


def test_new_entry_points_reject_bad_arguments_without_launch():
    """argument validation happens before any HIP call, so it is testable without a GPU"""
    import ctypes
    from inklayer_amd import _lib
    l = _lib.lib()
    assert l.ink_sam_amg_stats(None, 1, None, 1, None, 256, 1024, 768, 1024, 600, 800, 0.0, 1.0, 0, 0, 600, 800,
                               None, None, None, None) == 1
    # a crop that does not fit into the frame
    assert l.ink_sam_amg_stats(16, 1, None, 1, None, 256, 1024, 768, 1024, 600, 800, 0.0, 1.0, 10, 0, 600, 800,
                               16, 16, None, None) == 1
    assert l.ink_mask_rle_counts(None, None, 1, 600, 800, None, None) == 1
    assert l.ink_mask_rle_write(16, None, 0, 600, 800, 16, 16, None) == 1
    assert l.ink_box_nms(16, 16, 4097, 0.7, 16, 16, 16, None) == 1           # more than the documented bound
    assert l.ink_box_nms(16, 16, -1, 0.7, 16, 16, 16, None) == 1
    assert l.ink_mask_small_regions(None, 1, 600, 800, 100, 1, None, None, None, None, None) == 1
    need = ctypes.c_int64(0)
    assert l.ink_mask_small_regions_workspace_ints(2, 600, 800, ctypes.byref(need)) == 0
    assert need.value == 4 + 8 + 2 * (800 + 7 * 800 * 300)
    assert l.ink_mask_small_regions_workspace_ints(0, 600, 800, ctypes.byref(need)) == 1
