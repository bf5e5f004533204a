"""Packs the reference's OWN committed visualisations into small fixtures (tests/golden/vis_<set>.npz, vis_colors.npz).

Six of the reference's output sets (custom_interface/static/outputs/*) hold segmented_sketch.png,
segmented_sketch_final.png, bboxes.png and bboxes_final.png next to the input.png, masks/, masks_final/, bboxes.json and
bboxes_final.json they were drawn from (inputs and masks are already in refine_<set>.npz).  This script only COPIES
PIXELS AND NUMBERS:
  seg_xor, seg_final_xor, bboxes_xor, bboxes_final_xor   uint8 [H, W, 3]: the picture XOR input.png (mostly zeros)
  bboxes, scores, final_bboxes, final_scores             the numbers of the two JSON files
  n_masks, n_masks_final                                 how many mask files each stage has
vis_colors.npz holds what the reference's generate_pastel_colors returns for n = 0 .. 64 and 255 (`ns`, `colors_<n>`);
the reference module is loaded from its file with cv2 stubbed, since only that function is called.

    python tests/golden/make_vis_golden.py          # build container only (/root/reference)
"""
import glob
import importlib.util
import io
import json
import os
import sys
import types
from pathlib import Path

import numpy as np
from PIL import Image

REF = Path("/root/reference")
OUT = Path(__file__).resolve().parent
SETS = sorted(Path(p) for p in glob.glob(str(REF / "custom_interface/static/outputs/*/"))
              if os.path.exists(os.path.join(p, "segmented_sketch_final.png")))
LIMIT = 1000 * 1024
PICTURES = {"seg_xor": "segmented_sketch.png", "seg_final_xor": "segmented_sketch_final.png",
            "bboxes_xor": "bboxes.png", "bboxes_final_xor": "bboxes_final.png"}


def _rgb(p):
    return np.asarray(Image.open(p).convert("RGB"))


def _npz(**arrays) -> bytes:
    buf = io.BytesIO()
    np.savez_compressed(buf, **arrays)
    return buf.getvalue()


def _colors():
    sys.modules.setdefault("cv2", types.ModuleType("cv2"))
    spec = importlib.util.spec_from_file_location("_ref_visualization", REF / "InkLayer/utils/visualization.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    ns = list(range(65)) + [255]
    out = {"ns": np.asarray(ns, np.int64)}
    for n in ns:
        out[f"colors_{n}"] = np.asarray(mod.generate_pastel_colors(n), np.int64).reshape(n, 3)
    (OUT / "vis_colors.npz").write_bytes(_npz(**out))
    print("vis_colors.npz", (OUT / "vis_colors.npz").stat().st_size >> 10, "KiB")


def main():
    _colors()
    for d in SETS:
        inp = _rgb(d / "input.png")
        bj = json.loads((d / "bboxes.json").read_text())
        fj = json.loads((d / "bboxes_final.json").read_text())
        out = {k: _rgb(d / f) ^ inp for k, f in PICTURES.items()}
        out.update(bboxes=np.asarray(bj["bboxes"], np.float64).reshape(-1, 4), scores=np.asarray(bj["scores"], np.float64),
                   final_bboxes=np.asarray(fj["bboxes"], np.float64).reshape(-1, 4),
                   final_scores=np.asarray(fj["scores"], np.float64),
                   n_masks=np.int64(len(glob.glob(str(d / "masks" / "mask_*.png")))),
                   n_masks_final=np.int64(len(glob.glob(str(d / "masks_final" / "mask_*.png")))))
        data = _npz(**out)
        if len(data) <= LIMIT:
            (OUT / f"vis_{d.name}.npz").write_bytes(data)
            print(d.name, len(data) >> 10, "KiB")
        else:                       # two files: the coloured sketches / the box drawings and numbers
            a = {k: v for k, v in out.items() if k.startswith("seg")}
            b = {k: v for k, v in out.items() if not k.startswith("seg")}
            for suffix, part in (("", a), ("_boxes", b)):
                data = _npz(**part)
                assert len(data) <= LIMIT, (d.name, suffix, len(data))
                (OUT / f"vis_{d.name}{suffix}.npz").write_bytes(data)
                print(d.name + suffix, len(data) >> 10, "KiB")


if __name__ == "__main__":
    main()
