"""Visualisation stage: the reference's coloured sketch, pixel for pixel.

  pastel_colors    generate_pastel_colors (InkLayer/utils/visualization.py:30-60) without matplotlib
  colour_tables    everything color_sketch_by_masks (visualization.py:63-167) computes per pixel, as uint8 tables
  colour_sketch    the picture itself: csrc/visualize.hip on the GPU, a numpy label look-up without one

The reference paints every mask with a Python loop over H x W.  Its output pixel depends only on the pixel's grey
value, on the LAST mask that holds the pixel and on one image-wide flag (is some stroke pixel darker than grey 230,
i.e. max_stroke_opacity > 0.1), so the picture is a [n + 1, 256, 3] table look-up; the table is evaluated here with the
reference's own float32 / float64 steps.  Nothing under oracle/ or tests/ is imported.
"""
from __future__ import annotations

from typing import Optional, Sequence

import numpy as np

STROKE_BELOW = 250          # visualization.py:92: a stroke pixel has grey < 250
FAINT_ABOVE = 229           # max_stroke_opacity > 0.1  <=>  some stroke pixel has grey <= 229  (26 / 255 > 0.1 >= 25 / 255)


def _hsv_to_rgb(h: float, s: float, v: float):
    """matplotlib.colors.hsv_to_rgb for one colour, in the same float64 steps."""
    i = int(h * 6.0)
    f = (h * 6.0) - i
    p = v * (1.0 - s)
    q = v * (1.0 - s * f)
    t = v * (1.0 - s * (1.0 - f))
    return ((v, t, p), (q, v, p), (p, v, t), (p, q, v), (t, p, v), (v, p, q))[i % 6]


def pastel_colors(n_colors: int):
    """visualization.py:30-60: n evenly spaced hues in the interleaved order, S = 0.7, V = 0.88, int(c * 255)."""
    hues = [x / n_colors for x in range(n_colors)]
    result, queue = [], [hues]
    while queue:
        current = queue.pop(0)
        if len(current) <= 1:
            result += current
        else:
            queue.append(current[::2])
            queue.append(current[1::2])
    return [tuple(int(c * 255) for c in _hsv_to_rgb(h, 0.7, 0.88)) for h in result]


def colour_tables(colors: Sequence, enhance_factor: float = 1.5, min_opacity: float = 0.2) -> np.ndarray:
    """uint8 [2, n + 1, 256, 3]: [v, i, g] = the output pixel of a stroke pixel of grey g whose last mask is i (row n:
    in no mask, the black "background stroke"), v = 0 for an image with a stroke pixel of grey <= 229 (power law,
    visualization.py:109-118), v = 1 for a faint one (raw * 3, :119-125).  Entries with g >= 250 are white."""
    g = np.arange(256, dtype=np.uint8)
    stroke = g < STROKE_BELOW
    raw = (255 - g) / 255.0                                                  # float64
    power = np.power(raw, 1.0 / enhance_factor)
    power = np.where(stroke & (raw > 0.02), np.maximum(power, min_opacity), power)
    faint = np.where(stroke, np.maximum(raw * 3, min_opacity), raw)
    rows = np.array([tuple(c) for c in colors] + [(0, 0, 0)], dtype=np.float32).reshape(-1, 3)
    opacity = np.stack([power, faint])[:, :STROKE_BELOW]                     # float64 [2, 250]
    # :146-150: float32 colour x float32(opacity) + float32(255) x float32(1 - opacity), the subtraction in float64
    weighted = rows[None, :, None, :] * opacity.astype(np.float32)[:, None, :, None]
    white = np.float32(255) * (1 - opacity).astype(np.float32)
    out = np.full((2, len(rows), 256, 3), 255, np.uint8)
    out[:, :, :STROKE_BELOW] = (weighted + white[:, None, :, None]).astype(np.uint8)
    return out


def gray_host(sketch: np.ndarray) -> np.ndarray:
    """cv2.cvtColor(COLOR_RGB2GRAY) of uint8 pixels; a single-channel sketch is taken as it is (visualization.py:82-85)."""
    a = np.asarray(sketch)
    if a.ndim == 2:
        return a.astype(np.uint8, copy=False)
    r, g, b = (a[..., k].astype(np.uint32) for k in range(3))
    return ((4899 * r + 9617 * g + 1868 * b + 8192) >> 14).astype(np.uint8)


def label_image(masks, shape) -> np.ndarray:
    """[H, W] label image of a sequence of masks: l = the last mask (index l - 1) holding the pixel, 0 = none."""
    label = np.zeros(shape, np.uint16 if len(masks) > 255 else np.uint8)
    for i, m in enumerate(masks):
        label[np.asarray(m) != 0] = i + 1
    return label


def _is_cuda(t) -> bool:
    return hasattr(t, "is_cuda") and bool(t.is_cuda)


def colour_sketch(sketch, masks_or_label, colors=None, enhance_factor: float = 1.5, min_opacity: float = 0.2,
                  n_labels: Optional[int] = None, use_gpu: Optional[bool] = None):
    """color_sketch_by_masks as arrays.  sketch: uint8 [H, W, 3] (R, G, B) or [H, W]; masks_or_label: a stack [n, H, W]
    or a sequence of [H, W] masks (bool or integer, non-zero = inside, the last mask holding a pixel wins), or - with
    n_labels given - a uint8 label image [H, W] (0: no mask, l: mask l - 1, l <= n_labels <= 255).
    CUDA tensors in: the kernels run on the current stream and the picture stays on the device (uint8 [H, W, 3] tensor).
    Host arrays in: a numpy array comes back; with a GPU the sketch and the masks are uploaded and the kernels run,
    without one (or with use_gpu=False) the same tables go through a numpy label look-up."""
    by_label = n_labels is not None
    n = int(n_labels) if by_label else len(masks_or_label)
    if colors is None:
        colors = pastel_colors(n)
    if len(colors) < n:
        raise IndexError(f"colour_sketch: {n} masks but only {len(colors)} colours")
    tables = colour_tables(list(colors)[:n], enhance_factor, min_opacity)
    on_dev = _is_cuda(sketch) or _is_cuda(masks_or_label)
    if on_dev:
        assert use_gpu is not False, "colour_sketch: CUDA tensors cannot take the host path"
        use_gpu = True
    elif use_gpu is None:
        try:
            import torch
            use_gpu = torch.cuda.is_available() and (not by_label or n <= 255)
        except ImportError:
            use_gpu = False
    if not use_gpu:
        sk = np.asarray(sketch)
        gray = gray_host(sk)
        label = np.asarray(masks_or_label) if by_label else label_image(masks_or_label, gray.shape)
        stroke = gray < STROKE_BELOW
        variant = 0 if (stroke.any() and int(gray[stroke].min()) <= FAINT_ABOVE) else 1
        row = np.where((label == 0) | (label > n), n, label.astype(np.int64) - 1)      # a label above n counts as 0
        return tables[variant][row, gray]

    import torch
    from . import ops
    dev = sketch.device if _is_cuda(sketch) else (masks_or_label.device if _is_cuda(masks_or_label) else torch.device("cuda"))

    def up(a, bool_ok=False):
        if torch.is_tensor(a):
            t = a
        else:
            a = np.asarray(a)
            t = torch.from_numpy(np.ascontiguousarray(a.view(np.uint8) if a.dtype == np.bool_ else a))
        if t.dtype == torch.bool:
            t = t.view(torch.uint8)
        if t.dtype != torch.uint8:
            t = (t != 0).to(torch.uint8) if bool_ok else t.to(torch.uint8)
        return t.to(dev).contiguous()

    sk = up(sketch)
    if by_label:
        second = up(masks_or_label)
    elif torch.is_tensor(masks_or_label):
        second = up(masks_or_label, bool_ok=True)
    elif n == 0:
        second = torch.zeros((0,) + tuple(sk.shape[:2]), dtype=torch.uint8, device=dev)
    else:
        second = up(np.stack([np.asarray(m) for m in masks_or_label]), bool_ok=True)
    out = ops.vis_colour(sk, second, torch.from_numpy(tables).to(dev), ops.vis_gray_min(sk), by_label=by_label)
    return out if on_dev else out.cpu().numpy()
