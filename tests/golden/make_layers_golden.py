"""Packs the reference's OWN committed layer-assembly outputs into small fixtures (tests/golden/layers_<set>.npz).

Six of the reference's output sets (custom_interface/static/outputs/*) hold complete_layers/,
complete_layers_process/ and complete_layers_rgba/, including the inpainted_image.png that the diffusion model
returned.  With that file taken as data, every other file of the stage is a function of input.png and masks_final/
(both already in refine_<set>.npz).  This script only COPIES PIXELS, bit-packed where they are binary:
  n_layers, need_inpaint[n], edit_mask[n, H, ceil(W/8)] (bits), sketch_layer[n, H, W, 3] (as saved),
  inpainted[k, H, W, 3] and final_xor[k, H, W, 3] (final_composited = inpainted ^ final_xor) for the k layers in
  inpaint_index, rgba_alpha[n, H, ceil(W/8)] (bits), rgba_rgb[n, H, W] (R of the RGBA file; rgba_gray_ok tells
  that R == G == B everywhere).
A set whose file would pass LIMIT bytes keeps the inpainted images of its first layers only (inpaint_index).

    python tests/golden/make_layers_golden.py          # build container only (/root/reference)
"""
import glob
import io
import os
from pathlib import Path

import numpy as np
from PIL import Image

REF = Path("/root/reference")
OUT = Path(__file__).resolve().parent
SETS = sorted(Path(p) for p in glob.glob(str(REF / "custom_interface/static/outputs/*/"))
              if os.path.isdir(os.path.join(p, "complete_layers_rgba")))
LIMIT = 1000 * 1024


def _rgb(p):
    return np.asarray(Image.open(p).convert("RGB"))


def _pack(d, name, keep):
    n = len(glob.glob(str(d / "masks_final" / "mask_*.png")))
    proc = d / "complete_layers_process"
    H, W = _rgb(d / "input.png").shape[:2]
    need = np.zeros(n, bool)
    edit = np.zeros((n, H, W), bool)
    sketch = np.zeros((n, H, W, 3), np.uint8)
    alpha = np.zeros((n, H, W), bool)
    rgb1 = np.zeros((n, H, W), np.uint8)
    gray_ok = True
    inp_idx, inp, fx = [], [], []
    for i in range(n):
        m = proc / f"mask_{i}"
        sketch[i] = _rgb(m / "sketch_layer.png")
        if (m / "edit_mask.png").exists():
            need[i] = True
            e = np.asarray(Image.open(m / "edit_mask.png").convert("L"))
            assert set(np.unique(e).tolist()) <= {0, 255}
            edit[i] = e > 0
            if len(inp_idx) < keep:
                a, f = _rgb(m / "inpainted_image.png"), _rgb(m / "final_composited.png")
                inp_idx.append(i)
                inp.append(a)
                fx.append(a ^ f)
                assert np.array_equal(_rgb(d / "complete_layers" / f"layer_{i}.png"), f)
        else:
            assert np.array_equal(_rgb(d / "complete_layers" / f"layer_{i}.png"), sketch[i])
        r = np.asarray(Image.open(d / "complete_layers_rgba" / f"layer_{i}.png").convert("RGBA"))
        assert set(np.unique(r[..., 3]).tolist()) <= {0, 255}
        alpha[i] = r[..., 3] > 0
        rgb1[i] = r[..., 0]
        gray_ok &= bool((r[..., 0] == r[..., 1]).all() and (r[..., 1] == r[..., 2]).all())
    out = dict(n_layers=np.int64(n), need_inpaint=need, edit_mask=np.packbits(edit, axis=-1), sketch_layer=sketch,
               inpaint_index=np.asarray(inp_idx, np.int64),
               inpainted=np.stack(inp) if inp else np.zeros((0, H, W, 3), np.uint8),
               final_xor=np.stack(fx) if fx else np.zeros((0, H, W, 3), np.uint8),
               rgba_alpha=np.packbits(alpha, axis=-1), rgba_rgb=rgb1, rgba_gray_ok=np.bool_(gray_ok))
    buf = io.BytesIO()
    np.savez_compressed(buf, **out)
    return buf.getvalue(), int(need.sum()), len(inp_idx)


def main():
    for d in SETS:
        keep = 10 ** 6
        while True:
            data, n_need, n_kept = _pack(d, d.name, keep)
            if len(data) <= LIMIT or n_kept == 0:
                break
            keep = n_kept - 1
        (OUT / f"layers_{d.name}.npz").write_bytes(data)
        print(d.name, len(data) >> 10, "KiB; inpainted layers", n_need, "stored", n_kept)


if __name__ == "__main__":
    main()
