"""Layer assembly: the reference's inpainting stage around the diffusion model, on the GPU.

  background_masks   get_mask (InkLayer/inpainting/fill_object_bg_mask.py:50-114) for a batch of grey images
  assemble_layers    assemble_inpaint_input_at_index (util.py:22-106) for every layer of a sketch at once; the
                     background mask of an overlapped object is computed ONCE (the reference recomputes it per pair)
  composite          composite_original_sketch_onto_inpainted (util.py:109-133)
  rgba_layers        create_rgba_with_background_mask (fill_object_bg_mask.py:117-185)

The kernels are csrc/layers.hip; the host code here only orders them, reads the few per-plane decisions back (branch
of get_mask, shrink_by, overlap table) and resolves the rare hole that the component pass leaves undecided.  Nothing
under oracle/ or tests/ is imported.
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import ops
from ._lib import InkLayerHipError

# get_mask's defaults, and the values assemble_inpaint_input_at_index passes (util.py:77-84)
DEFAULT_PARAMS = dict(dilate_iter=5, kernel_size=3, safety_margin=0, stroke_thick=1, border_band=2)
OVERLAP_PARAMS = dict(dilate_iter=10, kernel_size=5, safety_margin=1, stroke_thick=2, border_band=3)
OPEN, CLOSED = "open-curve", "closed-silhouette"


def unpack_planes(planes: torch.Tensor, W: int) -> np.ndarray:
    """int64 [n, H, Wp] bit planes -> bool [n, H, W] on the host."""
    a = planes.cpu().numpy().view(np.uint8)
    return np.unpackbits(a, axis=-1, bitorder="little")[..., :W].astype(bool)


def pack_planes(bits: np.ndarray, dev) -> torch.Tensor:
    """bool [n, H, W] -> int64 [n, H, Wp] bit planes on `dev`."""
    n, H, W = bits.shape
    Wp = (W + 63) // 64
    padded = np.zeros((n, H, Wp * 64), np.uint8)
    padded[..., :W] = bits
    words = np.packbits(padded, axis=-1, bitorder="little").view(np.int64)
    return torch.from_numpy(np.ascontiguousarray(words)).to(dev)


# ---- undecided holes: a hole of fewer than 50 own cells that surrounds foreground islands ---------------------------------
def _grow(seed: np.ndarray, allowed: np.ndarray, conn8: bool) -> np.ndarray:
    cur = seed & allowed
    while True:
        nxt = cur.copy()
        nxt[1:] |= cur[:-1]
        nxt[:-1] |= cur[1:]
        nxt[:, 1:] |= cur[:, :-1]
        nxt[:, :-1] |= cur[:, 1:]
        if conn8:
            nxt[1:, 1:] |= cur[:-1, :-1]
            nxt[1:, :-1] |= cur[:-1, 1:]
            nxt[:-1, 1:] |= cur[1:, :-1]
            nxt[:-1, :-1] |= cur[1:, 1:]
        nxt &= allowed
        if np.array_equal(nxt, cur):
            return cur
        cur = nxt


def _hole_with_islands(mask: np.ndarray, rec: Sequence[int]) -> Tuple[np.ndarray, Tuple[slice, slice], int]:
    """The hole through (rec's first pixel) with everything it surrounds, inside its box grown by one, and twice its
    contour area by the same 2x2-cell rule as the kernel (two or more corners: 1, one corner: 1/2)."""
    _, x0, x1, y0, y1, _, sy, sx = (int(v) for v in rec)
    win = (slice(y0 - 1, y1 + 2), slice(x0 - 1, x1 + 2))       # the box is off the image edge by at least 2
    crop = mask[win]
    seed = np.zeros_like(crop)
    seed[sy - y0 + 1, sx - x0 + 1] = True
    hole = _grow(seed, ~crop, conn8=False)
    ring = np.zeros_like(crop)
    ring[0] = ring[-1] = ring[:, 0] = ring[:, -1] = True
    outside = _grow(ring, ~hole, conn8=True)
    region = ~outside
    r = np.pad(region.astype(np.int64), 1)
    c = r[:-1, :-1] + r[:-1, 1:] + r[1:, :-1] + r[1:, 1:]
    return region, win, int(2 * (c >= 2).sum() + (c == 1).sum())


def _resolve_undecided(dilated: torch.Tensor, filled: torch.Tensor, W: int, hdr: np.ndarray) -> torch.Tensor:
    count = int(hdr[1])
    if count == 0:
        return filled
    if count > 64:
        raise InkLayerHipError(f"ink_layers_components: {count} undecided holes, more than the 64 it records")
    recs = hdr[2:2 + 8 * count].reshape(count, 8)
    planes = sorted({int(r[0]) for r in recs})
    src = unpack_planes(dilated[planes], W)
    dst = unpack_planes(filled[planes], W)
    for r in recs:
        k = planes.index(int(r[0]))
        region, win, area2 = _hole_with_islands(src[k], r)
        if area2 >= 100:
            dst[k][win] |= region
    filled = filled.clone()
    filled[planes] = pack_planes(dst, filled.device)
    return filled


def _header(hdr: torch.Tensor, what: str) -> np.ndarray:
    h = hdr.cpu().numpy()
    if h[0] != 0:
        raise InkLayerHipError(f"ink_layers_components ({what}): run table overflow")
    return h


@torch.no_grad()
def background_masks(gray_u8: torch.Tensor, params: Optional[dict] = None, *, strokes_bright: bool = False):
    """get_mask for n grey images uint8 [n, H, W] on the GPU (as cv2.imread(IMREAD_GRAYSCALE) gives them: dark strokes
    on white; strokes_bright: the strokes are the bright pixels, e.g. a 0 / 255 object mask).
    -> (bit planes int64 [n, H, Wp], branch name per plane, shrink_by per plane)."""
    p = {**DEFAULT_PARAMS, **(params or {})}
    assert gray_u8.dtype == torch.uint8 and gray_u8.is_cuda and gray_u8.dim() == 3
    gray_u8 = gray_u8.contiguous()
    n, H, W = (int(v) for v in gray_u8.shape)
    strokes, _, _ = ops.layers_otsu_planes(gray_u8, invert=not strokes_bright)
    thick = ops.layers_dilate(strokes, W, p["kernel_size"], p["dilate_iter"])
    touches = ops.layers_border_band(thick, W, p["border_band"]).cpu().numpy() != 0
    out = torch.empty_like(strokes)
    branch = [OPEN if t else CLOSED for t in touches]
    shrink = [0] * n
    idx_open = [i for i in range(n) if touches[i]]
    idx_closed = [i for i in range(n) if not touches[i]]
    if idx_open:
        s = strokes[idx_open].contiguous()
        dil = ops.layers_dilate(s, W, p["kernel_size"], p["stroke_thick"])
        filled, hdr = ops.layers_components(dil, W, "fill_rule")
        out[idx_open] = _resolve_undecided(dil, filled, W, _header(hdr, "fill_rule"))
    if idx_closed:
        t = thick[idx_closed].contiguous()
        sil, h0 = ops.layers_components(t, W, "flood")
        big, h1 = ops.layers_components(sil, W, "largest")
        _, _, shrink_dev, shrunk = ops.layers_chamfer(big, strokes[idx_closed].contiguous(), W, p["safety_margin"])
        final, h2 = ops.layers_components(shrunk, W, "fill_all")
        for h, what in ((h0, "flood"), (h1, "largest"), (h2, "fill_all")):
            _header(h, what)
        out[idx_closed] = final
        for i, v in zip(idx_closed, shrink_dev.cpu().tolist()):
            shrink[i] = int(v)
    return out, branch, shrink


@dataclass
class Layer:
    sketch_layer: torch.Tensor                 # uint8 [H, W, 3] in the order the reference holds it: (B, G, R)
    edit_mask: Optional[torch.Tensor]          # uint8 [H, W] 0 / 255, None when the layer needs no inpainting
    debug_vis: Optional[torch.Tensor]          # uint8 [H, W, 3]; uint8 [H, W] mask when nothing overlaps; None for layer 0
    overlaps: List[int] = field(default_factory=list)


@torch.no_grad()
def assemble_layers(sketch_rgb, final_masks_dev: torch.Tensor) -> List[Layer]:
    """sketch_rgb: uint8 [H, W, 3] (R, G, B), host array or GPU tensor; final_masks_dev: uint8 [n, H, W] on the GPU in
    masks_final order (> 0 inside).  One pass for all layers."""
    masks = final_masks_dev.contiguous()
    assert masks.dtype == torch.uint8 and masks.is_cuda and masks.dim() == 3
    n, H, W = (int(v) for v in masks.shape)
    dev = masks.device
    rgb = sketch_rgb if torch.is_tensor(sketch_rgb) else torch.from_numpy(np.array(sketch_rgb, np.uint8))
    rgb = rgb.to(dev).contiguous()
    bbox, overlap = ops.layers_mask_tables(masks)
    ov = overlap.cpu().numpy() != 0
    used = [j for j in range(n) if ov[:, j].any()]
    bg = torch.zeros((n, H, (W + 63) // 64), device=dev, dtype=torch.int64)
    if used:
        planes, _, _ = background_masks(masks[used], OVERLAP_PARAMS, strokes_bright=True)
        bg[used] = planes
    sketch, edit, debug = ops.layers_assemble(rgb, masks, bg, bbox, overlap)
    out = []
    for i in range(n):
        js = [int(j) for j in np.nonzero(ov[i])[0]]
        if i == 0:
            out.append(Layer(sketch[i], None, None, []))
        elif not js:
            out.append(Layer(sketch[i], None, debug[i, :, :, 0], []))
        else:
            out.append(Layer(sketch[i], edit[i], debug[i], js))
    return out


@torch.no_grad()
def composite(inpainted_rgb, sketch_layer: torch.Tensor) -> torch.Tensor:
    """inpainted_rgb: uint8 [H, W, 3] (R, G, B), host array or GPU tensor; sketch_layer as assemble_layers returns it.
    -> uint8 [H, W, 3] (R, G, B) on the GPU."""
    a = inpainted_rgb if torch.is_tensor(inpainted_rgb) else torch.from_numpy(np.array(inpainted_rgb, np.uint8))
    return ops.layers_composite(a.to(sketch_layer.device).contiguous(), sketch_layer.contiguous())


@torch.no_grad()
def rgba_layers(layers_rgb: torch.Tensor):
    """uint8 [n, H, W, 3] (the pixels of complete_layers/layer_i.png, on the GPU) -> (uint8 [n, H, W, 4], branch names,
    shrink_by)."""
    gray = ops.layers_gray(layers_rgb.contiguous())
    bg, branch, shrink = background_masks(gray, DEFAULT_PARAMS)
    return ops.layers_rgba(gray, bg), branch, shrink
