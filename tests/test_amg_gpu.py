"""SamAutomaticMaskGenerator on the GPU (inklayer_amd/amg.py, csrc/amg.hip) against tests/amg_ref.py, the restatement
of the reference's generator that tests/test_amg_cpu.py pins to values recorded from the reference's own functions.
Everything after the decoder is integer logic on floats that are bit for bit those of ops.sam_postprocess, so every
comparison here is exact, except the float64 tier at the end, which checks the whole chain from the embeddings.
ViT-H decoder dimensions, a 4-block encoder (the engine of test_sam_prompts_gpu.py)."""
import numpy as np
import pytest
import torch

import amg_ref as R
from amg_cases import pack_planes, smooth_noise, unpack_planes
import sam_prompt_ref as PR

pytestmark = pytest.mark.gpu


IOU_BIAS = "mask_decoder.iou_prediction_head.layers.2.bias"


def seeded_weights(oc):
    """The weights of test_sam_prompts_gpu.py's engine (seed 11) with +1.0 on the last bias of the IoU head.  Seeded
    weights predict IoUs of -1.12 .. 0.36 (median -0.36), and the reference skips the predicted-IoU filter for a
    threshold <= 0 (`if self.pred_iou_thresh > 0.0`), so a median threshold would switch the filter off instead of
    splitting the candidates.  The constant moves every prediction, on the GPU and in the float64 restatement alike, to
    -0.12 .. 1.36 and changes nothing else."""
    from oracle import sam_ref
    sd = sam_ref.seeded_state_dict(sam_ref.sam_param_shapes(oc), 11)
    sd[IOU_BIAS] = sd[IOU_BIAS] + 1.0
    return sd


@pytest.fixture(scope="module")
def eng_sd(dev):
    from oracle import sam_ref
    from inklayer_amd import sam
    oc = sam_ref.SamConfig(depth=4, global_attn_indexes=(1, 3))
    sd = seeded_weights(oc)
    eng = sam.SamEngine(sd, sam.SamConfig(depth=4, global_attn_indexes=(1, 3)), dev, max_batch=1)
    return eng, oc, PR.to64(sd)


@pytest.fixture(scope="module")
def embs():
    rs = np.random.RandomState(5)
    return torch.from_numpy(rs.standard_normal((2, 4096, 256)).astype(np.float32))


# ------------------------------------------------------------------------------------------------ data
def stats_logits(seed, n=6):
    """low-res logits [n + 2, 256, 256]: blobs kept away from the frame border (interior boxes that differ per mask),
    one all-negative and one all-positive mask."""
    low = smooth_noise(seed, n, 256, 256)
    yy, xx = torch.meshgrid(torch.arange(256.0), torch.arange(256.0), indexing="ij")
    for i in range(n):
        cy, cx, ry, rx = 60 + 12 * i, 110 - 6 * i, 30 + 5 * i, 40 + 6 * i
        inside = ((yy - cy).abs() < ry) & ((xx - cx).abs() < rx)
        low[i][~inside] = -4.0
    return torch.cat([low, torch.full((1, 256, 256), -3.0), torch.full((1, 256, 256), 3.0)]).contiguous()


def blob_batch(seed, low_hw, crop_hw):
    """64 points x 3 masks of hand-made low-res logits for the tail seam: one cone per mask (slope k per low-res pixel,
    clipped to +-8) centred near the point; the three radii of a point are R, 1.08 R and 1.16 R, so its masks have
    boxes of IoU 0.74 .. 0.86 (all but one of the survivors fall to the NMS); shallow cones fail the stability filter; big cones of the outer
    ring reach the crop edge; IoU "predictions" are uniform around 0.88.  low_hw: the part of the 256 x 256 frame that
    the crop occupies."""
    rs = np.random.RandomState(seed)
    lh, lw = low_hw
    yy, xx = np.mgrid[0:256, 0:256].astype(np.float32)
    low = np.empty((64, 3, 256, 256), dtype=np.float32)
    for p in range(64):
        cy = (p // 8 + 0.5) / 8 * lh + rs.uniform(-2, 2)
        cx = (p % 8 + 0.5) / 8 * lw + rs.uniform(-2, 2)
        rad = rs.uniform(8, 14)
        for m in range(3):
            k = 8.0 if rs.uniform() < 0.8 else 0.6
            r = np.sqrt((yy - cy) ** 2 + (xx - cx) ** 2)
            low[p, m] = np.clip(k * (rad * (1.0, 1.08, 1.16)[m] - r), -8, 8)
    iou = (0.88 + rs.uniform(-0.05, 0.12, (64, 3))).astype(np.float32)
    points = R.build_point_grid(8) * np.array(crop_hw)[None, ::-1]
    return torch.from_numpy(low), torch.from_numpy(iou), points


def ref_table(logits, thr, off):
    """what the stats table must hold, from amg_ref on the full-resolution logits"""
    hi, lo = R.stability_counts(logits, thr, off)
    masks = logits > thr
    area = masks.flatten(1).sum(1)
    boxes = R.batched_mask_to_box(masks)
    return torch.cat([hi[:, None].long(), lo[:, None].long(), area[:, None], boxes,
                      torch.zeros(len(logits), 1, dtype=torch.long)], 1), masks


# ------------------------------------------------------------------------------------------------ 1. stats op
CASES = [  # input_hw, crop_hw, xy0, orig_hw
    ((1024, 768), (1500, 1125), (0, 0), None),             # width % 4 != 0: the one-pixel form
    ((768, 1024), (600, 800), (0, 0), None),               # the rows form
    ((768, 1024), (600, 800), (37, 101), (777, 901)),      # a crop at a non-zero, non-multiple-of-64 offset
    ((1024, 768), (530, 397), (130, 75), (700, 640)),      # the same on the one-pixel form
]


@torch.no_grad()
@pytest.mark.parametrize("use_index", [False, True])
@pytest.mark.parametrize("case", range(len(CASES)))
def test_stats_op_exact(dev, case, use_index):
    from inklayer_amd import ops
    input_hw, crop_hw, xy0, orig_hw = CASES[case]
    low = stats_logits(100 + case).to(dev)
    n = low.shape[0]
    index = torch.tensor([6, 1, 7, 4, 3], dtype=torch.int32, device=dev) if use_index else None
    src = low[index.long()].contiguous() if use_index else low
    thr, off = 0.0, 1.0
    table, planes, lg = ops.sam_amg_stats(low, 1024, input_hw, crop_hw, thr, off, xy0, orig_hw, index=index,
                                          want_logits=True)
    _, want = ops.sam_postprocess(src, 1024, input_hw, crop_hw, thr, want_logits=True)
    assert torch.equal(lg, want), "the stats kernel's floats are not those of ink_sam_postprocess"
    ref, masks = ref_table(want.cpu(), thr, off)
    print(table.cpu().tolist())
    assert torch.equal(table.cpu().long(), ref)
    oh, ow = orig_hw or crop_hw
    full = R.uncrop_masks(masks, [xy0[0], xy0[1], xy0[0] + crop_hw[1], xy0[1] + crop_hw[0]], oh, ow)
    assert torch.equal(unpack_planes(planes, oh), full)
    # the data do what the test needs: both thresholds cut, boxes interior and different
    t = ref[:-2] if not use_index else ref[[1, 3, 4]]
    assert (t[:, 0] < t[:, 2]).all() and (t[:, 2] < t[:, 1]).all() and (t[:, 0] > 0).all()
    assert (t[:, 3] > 0).all() and (t[:, 5] < crop_hw[1] - 1).all() and len({tuple(r[3:7].tolist()) for r in t}) == len(t)
    # a device-side count: only the first `count` masks are processed, the other table rows stay zero
    if use_index:
        cnt = torch.tensor([3], dtype=torch.int32, device=dev)
        t2, p2 = ops.sam_amg_stats(low, 1024, input_hw, crop_hw, thr, off, xy0, orig_hw, index=index, count=cnt)
        assert torch.equal(t2[:3], table[:3]) and not t2[3:].any() and torch.equal(p2[:3], planes[:3])
    # another threshold / offset pair (thr + off and thr - off are not representable sums of each other)
    table3, _ = ops.sam_amg_stats(low, 1024, input_hw, crop_hw, 0.3, 0.7, xy0, orig_hw, index=index)
    ref3, _ = ref_table(want.cpu(), 0.3, 0.7)
    assert torch.equal(table3.cpu().long(), ref3)


# ------------------------------------------------------------------------------------------------ 2. RLE op
def _check_rle(masks, planes, H, W, select=None):
    from inklayer_amd import amg, ops
    got = ops.mask_rle(planes, H, W, select)
    want = R.mask_to_rle(masks if select is None else masks[select.cpu().long()])
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert g == w["counts"]
        rle = {"size": [H, W], "counts": g}
        assert amg.area_from_rle(rle) == R.area_from_rle(w)
    for i, g in enumerate(got):
        src = masks[i] if select is None else masks[int(select[i])]
        assert np.array_equal(amg.rle_to_mask({"size": [H, W], "counts": g}), src.numpy())


@torch.no_grad()
def test_rle_op_exact(dev):
    from inklayer_amd import ops
    # on the planes of the stats op (a crop inside a larger frame: long zero runs, column wrap-around)
    input_hw, crop_hw, xy0, orig_hw = CASES[2]
    low = stats_logits(7).to(dev)
    table, planes, lg = ops.sam_amg_stats(low, 1024, input_hw, crop_hw, 0.0, 1.0, xy0, orig_hw, want_logits=True)
    masks = unpack_planes(planes, orig_hw[0])
    assert masks.any()
    _check_rle(masks, planes, orig_hw[0], orig_hw[1])
    _check_rle(masks, planes, orig_hw[0], orig_hw[1], torch.tensor([7, 0, 3], dtype=torch.int32, device=dev))
    # full frame, all-positive mask included (starts with a one)
    t2, p2 = ops.sam_amg_stats(low, 1024, (768, 1024), (600, 800), 0.0, 1.0)
    _check_rle(unpack_planes(p2, 600), p2, 600, 800)
    # hand-made planes; heights that are not a multiple of 64, below 64, exactly 64
    for H, W in ((37, 53), (64, 5), (130, 70), (200, 3)):
        hand = torch.zeros(9, H, W, dtype=torch.bool)
        hand[1] = True
        hand[2, 0, 0] = True
        hand[3, 0, W - 1] = True
        hand[4, H - 1, 0] = True
        hand[5, H - 1, W - 1] = True
        hand[6, H - 1, :] = True                      # the last row: a run that ends each column
        hand[6, 0, 1:] = True                         # ... and continues into the next one
        hand[7] = torch.from_numpy(np.random.RandomState(H).uniform(size=(H, W)) < 0.5)
        hand[8, :, ::2] = True                        # whole columns
        _check_rle(hand, pack_planes(hand, dev), H, W)
    assert ops.mask_rle(p2, 600, 800, torch.zeros(0, dtype=torch.int32, device=dev)) == []


# ------------------------------------------------------------------------------------------------ 3. NMS op
def _boxes(rs, n):
    """heavy overlap: a few dozen clusters of jittered copies"""
    c = rs.uniform(0, 800, (40, 2))
    s = rs.uniform(20, 200, (40, 2))
    k = rs.randint(0, 40, n)
    xy = c[k] + rs.uniform(-6, 6, (n, 2))
    wh = s[k] * rs.uniform(0.85, 1.15, (n, 2))
    return torch.from_numpy(np.concatenate([xy, xy + wh], 1).astype(np.float32))


@torch.no_grad()
def test_nms_op_exact(dev):
    from inklayer_amd import ops
    rs = np.random.RandomState(3)
    boxes = _boxes(rs, 3000)
    scores = torch.from_numpy((rs.randint(0, 200, 3000) / 200.0).astype(np.float32))     # deliberate ties
    assert len(scores.unique()) <= 200
    boxes[17] = boxes[5]
    scores[17] = scores[5]
    boxes[100:104] = torch.tensor([3.0, 3.0, 3.0, 3.0])                                   # zero-area boxes
    for thr in (0.7, 0.3, 1.0):
        got = ops.box_nms(boxes.to(dev), scores.to(dev), thr)
        want = R.nms(boxes, scores, thr)
        print(f"thr {thr}: kept {len(want)} of 3000")
        assert got.dtype == torch.int64 and torch.equal(got.cpu(), want)
    assert len(R.nms(boxes, scores, 1.0)) == 3000 and 100 < len(R.nms(boxes, scores, 0.7)) < 2900
    # 0 / 1 scores (postprocess_small_regions), sizes around the 64-box words, the bound
    for n in (0, 1, 2, 63, 64, 65, 129, 4096):
        b, s = _boxes(rs, n), torch.from_numpy((rs.uniform(size=n) < 0.5).astype(np.float32))
        assert torch.equal(ops.box_nms(b.to(dev), s.to(dev), 0.7).cpu(), R.nms(b, s, 0.7))
    with pytest.raises(ValueError):
        ops.box_nms(_boxes(rs, 4097).to(dev), torch.zeros(4097, device=dev), 0.7)
    # iou == thr is kept
    c = torch.tensor([[0., 0., 2., 1.], [0., 0., 1., 1.]], device=dev)
    assert ops.box_nms(c, torch.tensor([0.9, 0.8], device=dev), 0.5).tolist() == [0, 1]


# ------------------------------------------------------------------------------------------------ 4. small regions
@torch.no_grad()
@pytest.mark.parametrize("min_area", [1, 100, 10 ** 6])
def test_small_regions_exact(dev, min_area):
    """holes then islands on thresholded smoothed noise at 600 x 800 (hundreds of components per mask), plus an empty, a
    full and a one-pixel mask, a checkerboard (the run bound: every second pixel of every column starts a run) and two
    equal largest islands; 10^6 makes every island small: the first largest stays."""
    from inklayer_amd import ops
    H, W = 600, 800
    masks = smooth_noise(21, 4, H, W, k=5, scale=8.0, bias=0.3) > 0
    extra = torch.zeros(6, H, W, dtype=torch.bool)
    extra[1] = True
    extra[2, 300, 400] = True
    yy, xx = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    extra[3] = (yy + xx) % 2 == 0
    extra[4, 100:110, 500:520] = True            # two islands of area 200: the upper one comes first in raster order
    extra[4, 50:60, 700:720] = True
    extra[4, 400:405, 10:20] = True
    extra[5] = (yy % 2 == 0) & (xx % 3 != 0)     # many short runs per column, 4-connected rows
    masks = torch.cat([masks, extra])
    planes = pack_planes(masks, dev)
    assert torch.equal(ops.pack_col_planes(masks.to(dev)), planes)
    out, changed = ops.remove_small_regions(planes, H, W, min_area)
    got = unpack_planes(out, H)
    n_changed = 0
    for i in range(len(masks)):
        m, c1 = R.remove_small_regions(masks[i].numpy(), min_area, "holes")
        m, c2 = R.remove_small_regions(m, min_area, "islands")
        assert np.array_equal(got[i].numpy(), m), i
        assert bool(changed[i]) == (c1 or c2), i
        n_changed += c1 or c2
    print(f"min_area {min_area}: {n_changed} of {len(masks)} masks changed")
    assert (n_changed == 0) == (min_area == 1)
    # the islands pass alone (after the holes pass 10^6 leaves nothing but full masks): "keep the largest" with its tie
    # rule - mask 8 has two islands of area 200, the upper one comes first in raster order
    out2, changed2 = ops.remove_small_regions(planes, H, W, min_area, modes=("islands",))
    got2 = unpack_planes(out2, H)
    for i in range(len(masks)):
        m, c = R.remove_small_regions(masks[i].numpy(), min_area, "islands")
        assert np.array_equal(got2[i].numpy(), m) and bool(changed2[i]) == c, i
    if min_area == 10 ** 6:
        assert got2[8, 50:60, 700:720].all() and got2[8].sum() == 200
        assert got2[:4].flatten(1).sum(1).min() > 0
    # a workspace limit that forces one plane per chunk gives the same result
    out1, changed1 = ops.remove_small_regions(planes, H, W, min_area, max_workspace_bytes=1)
    assert torch.equal(out1, out) and torch.equal(changed1, changed)


# ------------------------------------------------------------------------------------------------ 5. tail seam
def _records_equal(got, want):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert set(g) == set(w)
        for k in w:
            if isinstance(w[k], np.ndarray):
                assert np.array_equal(g[k], w[k]), k
            else:
                assert g[k] == w[k], (k, g[k], w[k])


class _StubPredictor:
    def __init__(self, eng):
        from inklayer_amd import sam
        self.engine, self.cfg = eng, eng.cfg
        self.transform = sam.ResizeLongestSide(eng.cfg.img_size)


SEAM = [  # crop_box, orig_hw: the full frame, an interior crop at an odd offset (one-pixel form: width % 4 != 0)
    ([0, 0, 800, 600], (600, 800)),
    ([123, 77, 123 + 501, 77 + 376], (600, 800)),
]


def seam_inputs(case):
    from oracle import sam_ref
    crop_box, orig_hw = SEAM[case]
    crop_hw = (crop_box[3] - crop_box[1], crop_box[2] - crop_box[0])
    input_hw = sam_ref.preprocess_shape(crop_hw[0], crop_hw[1], 1024)
    low, iou, points = blob_batch(40 + case, (input_hw[0] // 4, input_hw[1] // 4), crop_hw)
    return crop_box, orig_hw, crop_hw, input_hw, low, iou, points


@torch.no_grad()
@pytest.mark.parametrize("case", range(len(SEAM)))
def test_tail_seam_exact(dev, eng_sd, case):
    """_process_low_res + the NMS of _process_crop_features on hand-made blobs at the reference's default thresholds
    against amg_ref on ops.sam_postprocess's logits of the same low-res logits.  The data (seeds 40 / 41, tuned with
    amg_ref on the CPU) make every stage do work: >= 10 rejected by the IoU filter, the stability filter and the NMS,
    >= 10 by the crop-edge filter on the interior crop (on the full frame that filter cannot reject: crop == image),
    >= 10 survivors."""
    from inklayer_amd import amg, ops
    eng = eng_sd[0]
    crop_box, orig_hw, crop_hw, input_hw, low, iou, points = seam_inputs(case)
    gen = amg.SamAutomaticMaskGenerator(eng, points_per_side=8, output_mode="uncompressed_rle")
    part = gen._process_low_res(low.to(dev), iou.to(dev), points, input_hw, crop_box, orig_hw)
    logits = ops.sam_postprocess(low.reshape(192, 256, 256).to(dev), 1024, input_hw, crop_hw, 0.0, want_logits=True)[1]
    ref = R.AmgRef(_StubPredictor(eng), points_per_side=8, output_mode="uncompressed_rle")
    rpart = ref.process_logits(logits.cpu().reshape(64, 3, *crop_hw), iou, points, crop_box, orig_hw)
    assert part["rles"] == rpart["rles"]
    for k in ("iou_preds", "stability_score", "boxes", "points"):
        assert torch.equal(part[k], rpart[k]), k
    rdata = ref.finish_crop([rpart], crop_box)
    st = ref.stats
    print(st, "survivors", len(rdata["rles"]))
    assert st["candidates"] == 192 and st["rej_iou"] >= 10 and st["rej_stability"] >= 10 and st["rej_nms"] >= 10
    assert st["rej_edge"] >= (10 if case else 0) and len(rdata["rles"]) >= 10
    # the crop's NMS and the return to the image frame: the generator's own code on the same batch
    data = amg._cat([part])
    data = amg._filter(data, gen._nms(data["boxes"], data["iou_preds"], gen.box_nms_thresh))
    data["boxes"] = amg.uncrop_boxes_xyxy(data["boxes"], crop_box)
    data["points"] = amg.uncrop_points(data["points"], crop_box)
    data["crop_boxes"] = torch.tensor([crop_box] * len(data["rles"]), dtype=torch.int64).reshape(-1, 4)
    rdata.to_numpy()
    _records_equal(gen._records(data), ref.records(rdata))


# ------------------------------------------------------------------------------------------------ 6. generator, exact
def _medians(eng, image, **kw):
    """medians of predicted IoU and stability score over ALL reference-side candidates (no filter)"""
    from inklayer_amd import sam
    probe = R.AmgRef(sam.SamPredictor(eng), pred_iou_thresh=0.0, stability_score_thresh=0.0, box_nms_thresh=1.0,
                     crop_nms_thresh=1.0, **kw)
    iou, stab = [], []
    orig = probe.process_logits

    def spy(masks, iou_preds, points, crop_box, orig_size):
        iou.append(iou_preds.flatten())
        stab.append(R.calculate_stability_score(masks.flatten(0, 1), 0.0, 1.0))
        return orig(masks, iou_preds, points, crop_box, orig_size)

    probe.process_logits = spy
    probe.generate(image)
    return float(torch.cat(iou).median()), float(torch.cat(stab).median())


@torch.no_grad()
def test_generator_exact(dev, eng_sd):
    """generate() with one crop layer against amg_ref driven by the project's own SamPredictor.predict_torch(...,
    return_logits=True) on the same engine: record lists equal, floats included.  Thresholds = medians over the
    reference-side candidates, so each filter splits them about in half."""
    from inklayer_amd import amg, sam, synthetic
    eng = eng_sd[0]
    image = synthetic.synthetic_sketch(4, 600, 800)
    kw = dict(points_per_side=8, points_per_batch=64, crop_n_layers=1)
    t_iou, t_stab = _medians(eng, image, **kw)
    print(f"median predicted IoU {t_iou:.4f}, median stability {t_stab:.4f}")
    assert t_iou > 0.0 and t_stab > 0.0, "thresholds <= 0 would switch the filters off"
    for nms_thr, mode in ((1.0, "uncompressed_rle"), (0.7, "uncompressed_rle"), (0.7, "binary_mask")):
        kw2 = dict(kw, pred_iou_thresh=t_iou, stability_score_thresh=t_stab, box_nms_thresh=nms_thr,
                   crop_nms_thresh=nms_thr, output_mode=mode)
        ref = R.AmgRef(sam.SamPredictor(eng), **kw2)
        want = ref.generate(image)
        got = amg.SamAutomaticMaskGenerator(eng, **kw2).generate(image)
        print(f"nms {nms_thr} {mode}: {len(want)} records, {ref.stats}")
        _records_equal(got, want)
        if nms_thr == 1.0:
            assert len(want) >= 10 and ref.stats["rej_iou"] >= 10 and ref.stats["rej_stability"] >= 10
    # small regions on top (noise-like masks: many small islands and holes per column, the stress case of the run bound)
    kw3 = dict(kw, pred_iou_thresh=t_iou, stability_score_thresh=t_stab, min_mask_region_area=100, box_nms_thresh=1.0,
               crop_nms_thresh=1.0, output_mode="binary_mask")
    ref = R.AmgRef(sam.SamPredictor(eng), **kw3)
    want = ref.generate(image)
    print(f"min_mask_region_area 100: {len(want)} records")
    assert len(want) >= 10
    _records_equal(amg.SamAutomaticMaskGenerator(eng, **kw3).generate(image), want)
    # through the re-export next to SamPredictor, on a predictor
    gen = sam.SamAutomaticMaskGenerator(sam.SamPredictor(eng), points_per_side=4, pred_iou_thresh=t_iou,
                                        stability_score_thresh=t_stab)
    recs = gen.generate(image)
    assert all(r["segmentation"].shape == (600, 800) and r["segmentation"].dtype == np.bool_ for r in recs)


# ------------------------------------------------------------------------------------------------ 7. float64 tier
F64_IMAGE = 0        # embs[0]


def f64_reference(oc, sd64, embs, orig_hw=(600, 800)):
    """Reference side of the float64 tier, CPU only: sam_prompt_ref.decode_all + float64 postprocess_masks on the 8 x 8
    grid -> (logits f64 [192, H, W], iou f64 [192], points [64, 2], input_hw)."""
    from oracle import sam_ref
    input_hw = sam_ref.preprocess_shape(orig_hw[0], orig_hw[1], 1024)
    points = R.build_point_grid(8) * np.array(orig_hw)[None, ::-1]
    tp = torch.from_numpy(PR.apply_coords(points, orig_hw, 1024)).float()[:, None, :]
    lab = torch.ones(64, 1, dtype=torch.int32)
    emb = embs[F64_IMAGE].t().reshape(1, 256, 64, 64).double().expand(64, -1, -1, -1)
    low, iou = [], []
    for s in range(0, 64, 16):
        l, i = PR.decode_all(sd64, oc, emb[s:s + 16], PR.embed_sparse(sd64, oc, tp[s:s + 16], lab[s:s + 16], None))
        low.append(l[:, 1:])
        iou.append(i[:, 1:])
    low, iou = torch.cat(low), torch.cat(iou)
    logits = sam_ref.postprocess_masks(oc, low.reshape(192, 1, 256, 256), input_hw, orig_hw)[:, 0]
    return logits, iou.reshape(192), points, input_hw


def f64_decisive(logits, iou, t_iou, t_stab, off=1.0):
    """(passes both filters, decisive) per candidate, rules (i) and (ii) of the test below"""
    band = 1e-2 * logits.std().item()
    flat = logits.flatten(1)
    I = (flat > off).sum(1).double()
    U = (flat > -off).sum(1).double()
    bp = ((flat - off).abs() <= band).sum(1).double()
    bm = ((flat + off).abs() <= band).sum(1).double()
    lo, hi = (I - bp) / (U + bm), (I + bp) / (U - bm).clamp_min(1)
    dec = ((iou - t_iou).abs() > 1e-3 * abs(t_iou)) & ~((lo <= t_stab) & (t_stab <= hi))
    passes = (iou > t_iou) & (I / U >= t_stab)
    return passes, dec, I / U


@torch.no_grad()
def test_generator_float64_tier(dev, eng_sd, embs):
    """The whole chain from random embeddings (no encoder): _process_crop_features on the GPU against float64 decode +
    float64 postprocess_masks + amg_ref on the CPU, 8 x 8 points, full-frame crop of 600 x 800, box_nms_thresh = 1.0,
    thresholds = medians over the 192 reference candidates, stability offset 1.0.  A reference candidate is decisive
    when (i) its predicted IoU is more than 1e-3 relative from the threshold, (ii) the interval of stability scores
    reachable by flipping the pixels within 1e-2 std(logits) of thr +- offset excludes the threshold and (iii) its box
    is not within a pixel of flipping is_box_near_crop_edge (never the case on a full-frame crop).  Every decisive
    reference survivor must be in the GPU output with mask IoU >= 0.999, no GPU record may be a decisive reject, and at
    most 10 % of the candidates may be non-decisive.
    Observed on the CPU for this fixture (seeded_weights above, RandomState(5) embeddings, image 0): thresholds 0.6423
    and 0.1226, 9 of 192 candidates (4.7 %) non-decisive, 68 reference survivors."""
    from inklayer_amd import amg
    eng, oc, sd64 = eng_sd
    orig_hw = (600, 800)
    logits, iou, points, input_hw = f64_reference(oc, sd64, embs, orig_hw)
    stab_all = R.calculate_stability_score(logits, 0.0, 1.0)
    t_iou, t_stab = float(iou.median()), float(stab_all.median())
    passes, dec, _ = f64_decisive(logits, iou, t_iou, t_stab)
    assert t_iou > 0.0 and t_stab > 0.0, "thresholds <= 0 would switch the filters off"
    print(f"thresholds {t_iou:.4f} {t_stab:.4f}: non-decisive {int((~dec).sum())} of 192, survivors {int(passes.sum())}")
    assert (~dec).sum().item() <= 0.10 * 192
    assert passes.sum().item() >= 10
    gen = amg.SamAutomaticMaskGenerator(eng, points_per_side=8, pred_iou_thresh=t_iou, stability_score_thresh=t_stab,
                                        box_nms_thresh=1.0, output_mode="binary_mask")
    data = gen._process_crop_features(embs[F64_IMAGE].to(dev), input_hw, [0, 0, 800, 600], orig_hw)
    got = {int(c): i for i, c in enumerate(data["cand"])}
    assert len(got) == len(data["rles"])
    for c in range(192):
        if not dec[c]:
            continue
        if passes[c]:
            assert c in got, f"decisive reference survivor {c} missing"
            g = torch.from_numpy(amg.rle_to_mask(data["rles"][got[c]]).copy())
            r = logits[c] > 0.0
            assert (g & r).sum().item() / max((g | r).sum().item(), 1) >= 0.999
            assert data["points"][got[c]].tolist() == points[c // 3].tolist()
        else:
            assert c not in got, f"decisive reference reject {c} is in the GPU output"


# ------------------------------------------------------------------------------------------------ 8. edges
@torch.no_grad()
def test_argument_checks_and_empty_result(dev, eng_sd):
    from inklayer_amd import amg, synthetic
    eng = eng_sd[0]
    with pytest.raises(AssertionError):
        amg.SamAutomaticMaskGenerator(eng, points_per_side=8, point_grids=[R.build_point_grid(2)])
    with pytest.raises(AssertionError):
        amg.SamAutomaticMaskGenerator(eng, points_per_side=None)
    with pytest.raises(AssertionError, match="Unknown output_mode"):
        amg.SamAutomaticMaskGenerator(eng, output_mode="png")
    image = synthetic.synthetic_sketch(4, 300, 400)
    # explicit grids; a predicted-IoU threshold nothing reaches: every candidate filtered, on one crop layer too
    gen = amg.SamAutomaticMaskGenerator(eng, points_per_side=None, point_grids=[R.build_point_grid(3)] * 2,
                                        pred_iou_thresh=1e6, crop_n_layers=1)
    assert gen.generate(image) == []
    gen = amg.SamAutomaticMaskGenerator(eng, points_per_side=3, stability_score_thresh=2.0)
    assert gen.generate(image) == []
