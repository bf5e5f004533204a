"""Generate tests/golden/sam_prompts_small.npz: the REFERENCE's own PromptEncoder + MaskDecoder
(/root/reference/InkLayer/third_party/segment-anything/segment_anything/modeling) on CPU for point, point + box and
box + mask prompts, with all four masks and IoU predictions, and ResizeLongestSide.apply_coords for a non-square image.

Build-container only, like make_sam_golden.py (same SMALL config, same seeded weights loaded with strict=True).  The
low-res masks are stored at every 4th pixel to keep the file small; the dense mask embedding likewise.
"""
import sys
import types
from pathlib import Path

import numpy as np
import torch

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))
from make_sam_golden import SA, SEED, SMALL, build_reference, sam_ref  # noqa: E402

SEED_PROMPTS = 4321


def _reference_transform():
    """utils/transforms.py imports torchvision for its image half only: stub that import, use the coordinate half."""
    tv = types.ModuleType("torchvision")
    tv.transforms = types.ModuleType("torchvision.transforms")
    tv.transforms.functional = types.ModuleType("torchvision.transforms.functional")
    tv.transforms.functional.resize = tv.transforms.functional.to_pil_image = None
    sys.modules.update({"torchvision": tv, "torchvision.transforms": tv.transforms,
                        "torchvision.transforms.functional": tv.transforms.functional})
    sys.path.insert(0, str(Path(SA) / "utils"))
    import transforms  # noqa: E402  (the reference's utils/transforms.py)
    return transforms.ResizeLongestSide


@torch.no_grad()
def main():
    cfg = SMALL
    sd = sam_ref.seeded_state_dict(sam_ref.sam_param_shapes(cfg), SEED)
    model = build_reference(cfg)
    model.load_state_dict(sd, strict=True)
    pe, md = model.prompt_encoder, model.mask_decoder
    g, L = cfg.grid, cfg.img_size
    rs = np.random.RandomState(SEED_PROMPTS)
    emb = torch.from_numpy(rs.standard_normal((1, cfg.prompt_embed_dim, g, g)).astype(np.float32))
    out = dict(seed=np.int64(SEED), image_embedding=emb.numpy())
    cases = {
        # points only (the encoder appends the pad point); labels -1 / 0 / 1 and one label outside them (PE alone)
        "pts": dict(points=rs.uniform(0, L, (2, 3, 2)), labels=np.array([[1, 0, -1], [1, 2, 0]])),
        "ptsbox": dict(points=rs.uniform(0, L, (2, 4, 2)), labels=np.array([[1, 1, 0, -1], [0, 1, 1, 1]]),
                       boxes=np.array([[30.5, 40.25, 300.0, 410.75], [100.0, 17.0, 140.5, 90.0]])),
        "boxmask": dict(boxes=np.array([[10.0, 20.0, 500.0, 400.0], [200.0, 100.0, 260.0, 300.0]]),
                        masks=rs.standard_normal((2, 1, 4 * g, 4 * g)) * 4.0),
    }
    for name, c in cases.items():
        pts = torch.tensor(c["points"], dtype=torch.float) if "points" in c else None
        lab = torch.tensor(c["labels"], dtype=torch.int) if "labels" in c else None
        box = torch.tensor(c["boxes"], dtype=torch.float) if "boxes" in c else None
        msk = torch.tensor(c["masks"], dtype=torch.float) if "masks" in c else None
        sparse, dense = pe(points=(pts, lab) if pts is not None else None, boxes=box, masks=msk)
        low, iou = md.predict_masks(image_embeddings=emb, image_pe=pe.get_dense_pe(),
                                    sparse_prompt_embeddings=sparse, dense_prompt_embeddings=dense)
        for k, v in (("points", pts), ("labels", lab), ("boxes", box), ("masks", msk)):
            if v is not None:
                out[f"{name}_{k}"] = v.numpy()
        out[f"{name}_sparse"] = sparse.numpy()
        out[f"{name}_low_sub"] = low[:, :, ::4, ::4].numpy()
        out[f"{name}_iou"] = iou.numpy()
        if msk is not None:
            out[f"{name}_dense_sub"] = dense[:, :, ::4, ::4].numpy()
    tr = _reference_transform()(1024)
    coords = rs.uniform(0, 700, (5, 2))
    out["coords_orig"], out["coords_orig_hw"] = coords, np.array([700, 525])
    out["coords_applied"] = tr.apply_coords(coords, (700, 525))
    path = HERE / "sam_prompts_small.npz"
    np.savez_compressed(path, **out)
    print("wrote", path, path.stat().st_size >> 10, "KiB")


if __name__ == "__main__":
    main()
