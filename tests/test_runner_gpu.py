"""BASELINE config 1 on the HIP path (rows D0, D17, G, S0): the plugin entry points exactly as the reference's
main.py drives them - InkLayer.runner.run_inklayer_pipeline -> InkLayer.detector.gdino.run_ft_dino_on_sketch ->
InkLayer.utils.processing -> InkLayer.segmentor.sam.run_SAM - on a GENERATED sketch PNG, full-depth models (6+6 DINO
layers, 32 ViT-H blocks) with seeded random weights (INKLAYER_RANDOM_WEIGHTS=1: no checkpoints exist offline),
checked against the CPU oracle run on the same weights: output tree, bboxes.json, masks.  GPU box only."""
import json
import os
from pathlib import Path

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent


@torch.no_grad()
def test_runner_plugins_full_depth_against_oracle(dev, tmp_path, monkeypatch):
    from PIL import Image
    monkeypatch.setenv("INKLAYER_RANDOM_WEIGHTS", "1")
    monkeypatch.syspath_prepend(str(ROOT))
    import InkLayer.detector.gdino as DET
    import InkLayer.segmentor.sam as SEG
    import InkLayer.runner as R
    from InkLayer.utils import processing as P
    from inklayer_amd import gdino, sam, synthetic, weights_init
    from oracle import gdino_ref, sam_ref

    # a generated 750x750 RGBA sketch (the size/mode of the reference's data/bunny_cook_sketch.png)
    W = H = 750
    rgb = synthetic.synthetic_sketch(5, H, W)
    png = tmp_path / "generated.sketch.png"
    Image.fromarray(np.dstack([rgb, np.full((H, W), 255, np.uint8)]), "RGBA").save(png)

    # ---- oracle detector on the weights the shim will generate (same seeds, same device generator)
    gcfg = gdino.GDinoConfig()
    gsd = {k: v.cpu() for k, v in weights_init.random_gdino_state_dict(gcfg, "cuda").items()}
    text = weights_init.random_text_features(gcfg, "cuda").cpu()
    # random weights saturate every score at 1.0 (|logit| ~ 40): the decoder's final LayerNorm is scaled by 0.05 in
    # BOTH the oracle's and the engine's weights so that the scores spread out and a threshold can separate them
    for leaf in ("weight", "bias"):
        gsd[f"transformer.decoder.norm.{leaf}"] = gsd[f"transformer.decoder.norm.{leaf}"] * 0.05
    sm, pid = gdino_ref.text_masks_and_position_ids(list(gdino.DEFAULT_TOKEN_IDS))
    torch.set_num_threads(min(16, os.cpu_count() or 16))
    x = gdino_ref.load_image(np.asarray(Image.open(png).convert("RGB")))
    # ---- the product engine, through the plugin module's own singleton
    DET.model = None
    SEG._engine = None
    eng = DET.get_model()
    eng.w["dec.norm.w"].mul_(0.05)
    eng.w["dec.norm.b"].mul_(0.05)
    eng._graphs.clear()
    # the oracle is pinned to the two-stage SELECTION the HIP path makes for this image (its order is numerically
    # arbitrary between f16 and fp32, see tests/test_gdino_gpu.py::test_detect_threshold_path_matches_oracle_postprocess)
    from inklayer_amd import ops
    rgb_dev = torch.from_numpy(np.ascontiguousarray(np.asarray(Image.open(png).convert("RGB")))).to(eng.dev)
    oh, ow = gdino.resize_shape(W, H)
    st = {}
    eng._forward_eager([ops.resize_bilinear_u8(rgb_dev, oh, ow)], stages=st)
    ref_logits, ref_boxes = gdino_ref.detector_forward(gsd, gdino_ref.GDinoConfig(), x[None], text, sm, pid,
                                                       stages={"force_topk": st["topk"].cpu()})
    score = ref_logits[0].sigmoid().max(-1)[0]
    srt = torch.sort(score, descending=True)[0]
    gaps = srt[3:12] - srt[4:13]                 # keep 4..12 boxes: the widest score gap decides (random weights put
    k = int(gaps.argmax()) + 4                   # hundreds of queries above the reference's 0.2)
    thr = float((srt[k - 1] + srt[k]) / 2)
    print(f"oracle: threshold {thr:.4f} keeps {k} boxes (gap {gaps.max().item():.4f}); top scores {srt[:13].tolist()}")
    want_xyxy, want_sc = gdino_ref.postprocess_detections(ref_logits[0], ref_boxes[0], thr)

    # ---- the product path, through the plugin surfaces
    eng.cfg.box_threshold = thr
    try:
        # the call the reference's main.py makes for `--img png --out_dir out` (main.py:24)
        out_dir = Path(R.run_inklayer_pipeline(str(png), str(tmp_path / "out"), no_intermediate=False, inpaint=False))
        dino_out = DET.run_ft_dino_on_sketch(str(png))
    finally:
        eng.cfg.box_threshold = gcfg.box_threshold
    assert out_dir == tmp_path / "out" / "generated"            # name = basename before the FIRST dot
    assert sorted(p.name for p in out_dir.iterdir()) == ["bboxes.json", "bboxes.png", "bboxes_final.json",
                                                         "bboxes_final.png", "depth_map.png", "input.png", "masks",
                                                         "masks_cleaned", "masks_disjoint", "masks_final",
                                                         "segmented_sketch.png", "segmented_sketch_final.png"]
    # D0 / D17: detector plugin output vs the oracle.  Random weights leave an ill-conditioned tail of queries whose
    # score can cross any threshold (tests/test_gdino_gpu.py), so the kept boxes are MATCHED to the oracle's 900
    # queries (nearest box) instead of being compared by position: every kept box must be an oracle query, every
    # oracle query clearly above the threshold must be kept, none clearly below it.
    got_xyxy = np.asarray(dino_out["bboxes"], dtype=np.float64).reshape(-1, 4)
    n = len(got_xyxy)
    assert abs(n - k) <= 2 and dino_out["labels"] == ["object"] * n, (n, k)
    all_xyxy, all_sc = gdino_ref.postprocess_detections(ref_logits[0], ref_boxes[0], -1.0)      # all 900 queries
    dist = np.abs(got_xyxy[:, None, :] - all_xyxy[None, :, :]).max(-1)                            # [n, 900]
    match = dist.argmin(1)
    e = dist[np.arange(n), match]
    se = np.abs(np.asarray(dino_out["scores"]) - all_sc[match])
    print("plugin boxes vs matched oracle queries: err", e.tolist(), "score err", se.tolist())
    # bounds = 10x the errors this test logs on the MI355X (boxes 1.4e-3, scores 3e-4)
    assert len(set(match.tolist())) == n and np.median(e) < 3e-3 and e.max() < 1.4e-2
    assert np.median(se) < 5e-3 and se.max() < 3e-3
    clear = 0.03
    assert set(np.nonzero(all_sc > thr + clear)[0].tolist()) <= set(match.tolist())
    assert (all_sc[match] > thr - clear).all()
    k = n
    # G: bboxes.json = int()-truncated pixel boxes re-normalised (runner.py:36-44): exact given the plugin's boxes
    pil = Image.open(png).convert("RGB")
    boxes_tensor, _ = P.process_dino_output(dino_out, pil)
    saved = json.loads((out_dir / "bboxes.json").read_text())
    assert saved["bboxes"] == [[int(v[0]) / W, int(v[1]) / H, int(v[2]) / W, int(v[3]) / H] for v in boxes_tensor.tolist()]
    assert saved["scores"] == dino_out["scores"]
    # S0: masks/mask_i.png (PIL mode "1") vs the full-depth SAM oracle prompted with the same boxes
    ssd = {k_: v.cpu() for k_, v in weights_init.random_sam_state_dict(sam.SamConfig(), "cuda").items()}
    ref_masks = sam_ref.run_sam(ssd, sam_ref.SamConfig(), np.asarray(pil), boxes_tensor)
    ious = []
    for i, r in enumerate(ref_masks):
        m = Image.open(out_dir / "masks" / f"mask_{i}.png")
        assert m.mode == "1" and m.size == (W, H)
        g = np.asarray(m, dtype=bool)
        ious.append(float((g & r).sum() / max(1, (g | r).sum())))
    print("runner masks vs oracle IoU:", [round(v, 5) for v in ious])
    assert len(ious) == k and min(ious) >= 0.999
    # §8(f)-1 through the runner: masks_cleaned/ and bboxes_final.json vs the refinement oracle on the SAME raw masks
    from oracle import refine_ref
    raw = [np.asarray(Image.open(out_dir / "masks" / f"mask_{i}.png").convert("L")) for i in range(k)]
    want_clean = [refine_ref.clean_up_mask(m) for m in raw]
    for i, wc in enumerate(want_clean):
        assert np.array_equal(np.asarray(Image.open(out_dir / "masks_cleaned" / f"mask_{i}.png")), wc)
    want_final = refine_ref.process_json_with_sketch_nms(np.asarray(pil), saved, want_clean, 0.2)
    assert json.loads((out_dir / "bboxes_final.json").read_text()) == want_final
    # §8(f)-2 / -4 through the runner (config 5's stages): the depth map of the GPU engine against the depth oracle
    # on the same random weights, then masks_disjoint / masks_final against the host stage re-run on the ORACLE's depth
    from oracle import depth_ref
    from inklayer_amd import depth as hip_depth
    from oracle import refine4_ref as refine_host
    import InkLayer.refinement.depth_sort as DS
    dcfg = depth_ref.DepthConfig()
    dsd = {k_: v.cpu() for k_, v in weights_init.random_depth_state_dict(hip_depth.DepthConfig(), "cuda").items()}
    bgr = np.ascontiguousarray(np.asarray(pil)[..., ::-1])
    ref_depth = depth_ref.infer_image(dsd, dcfg, bgr)
    got_depth = DS.get_depth_map(str(out_dir / "input.png"))
    rel = np.abs(got_depth - ref_depth).max() / np.abs(ref_depth).max()
    print("runner depth map vs oracle: max-rel", rel)
    assert got_depth.shape == (H, W) and rel < 1e-2
    kept = want_final["kept_indices"]
    boxes_px = refine_host.unnormalize_bboxes(want_final["bboxes"], H, W)

    def host_stage(depth):
        dis, sboxes, _ = refine_host.parse_masks_to_disjoint_masks([want_clean[i] for i in kept], boxes_px, np.asarray(pil), depth)
        return dis, refine_host.improve_sam_masks(np.asarray(pil), dis, sboxes)

    def tree_equals(sub, want):
        files = sorted((out_dir / sub).iterdir(), key=lambda p_: int(p_.stem.split("_")[1]))
        return len(files) == len(want) and all(
            np.array_equal(np.asarray(Image.open(f)) > 0, np.asarray(m) > 0) for f, m in zip(files, want))

    # the runner's trees are EXACTLY the refinement stage applied to the oracle-cleaned masks under the depth map the
    # runner computed ...
    dis, fin = host_stage(got_depth)
    assert tree_equals("masks_disjoint", dis), "masks_disjoint/ differs from the refinement stage on the runner's depth map"
    assert tree_equals("masks_final", fin), "masks_final/ differs from the refinement stage on the runner's depth map"
    # ... and the same under the ORACLE's depth map whenever the two depth maps order the masks identically (the depth
    # scores are histogram modes of a map that agrees to 1e-2: an order swap between near-equal scores is legitimate)
    order_of = lambda depth: refine_host.sort_sketch_masks([want_clean[i] for i in kept], boxes_px, np.asarray(pil), depth)[0]
    o_got, o_ref = [int(i) for i in order_of(got_depth)], [int(i) for i in order_of(ref_depth)]
    print("depth order under the runner's / the oracle's depth map:", o_got, o_ref)
    if o_got == o_ref:
        dis_r, fin_r = host_stage(ref_depth)
        assert tree_equals("masks_disjoint", dis_r) and tree_equals("masks_final", fin_r)
    DS._engine = None
    DET.model = None
    SEG._engine = None
    torch.cuda.empty_cache()
