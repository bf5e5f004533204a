"""Checker for the visualisation stage: color_sketch_by_masks (InkLayer/utils/visualization.py:63-167) restated step by
step with its per-pixel loops, for TINY images only.  It deliberately does not use the table form of
inklayer_amd/visualize.py - it is what checks those tables.  numpy only (cv2's grey conversion is its integer formula).
"""
import numpy as np


def gray_rgb2gray(rgb):
    """cv2.cvtColor(COLOR_RGB2GRAY) for uint8: (4899 R + 9617 G + 1868 B + 8192) >> 14."""
    a = np.asarray(rgb).astype(np.int64)
    return ((4899 * a[..., 0] + 9617 * a[..., 1] + 1868 * a[..., 2] + 8192) >> 14).astype(np.uint8)


def color_sketch_by_masks(sketch, seg_masks, colors, enhance_factor=1.5, min_opacity=0.2):
    """sketch: uint8 [H, W, 3] or [H, W]; seg_masks: list of [H, W] arrays; colors: one (r, g, b) per mask.
    -> uint8 [H, W, 3]."""
    sketch = np.array(sketch)
    gray = gray_rgb2gray(sketch) if sketch.ndim == 3 else sketch
    h, w = gray.shape
    canvas = np.ones((h, w, 3), dtype=np.float32) * 255
    stroke = gray < 250
    covered = np.zeros((h, w), dtype=bool)
    for m in seg_masks:
        covered = np.logical_or(covered, m)
    raw = (255 - gray) / 255.0
    values = raw[stroke]
    if len(values) > 0:
        if np.max(values) > 0.1:
            opacity = np.power(raw, 1.0 / enhance_factor)
            opacity = np.where(stroke & (raw > 0.02), np.maximum(opacity, min_opacity), opacity)
        else:
            opacity = np.where(stroke, np.maximum(raw * 3, min_opacity), raw)
    else:
        opacity = raw
    white = np.array([255, 255, 255], dtype=np.float32)
    layers = [(np.array(colors[i], dtype=np.float32), np.logical_and(stroke, m)) for i, m in enumerate(seg_masks)]
    layers.append((np.array([0, 0, 0], dtype=np.float32), np.logical_and(stroke, ~covered)))
    for color, where in layers:
        for y in range(h):
            for x in range(w):
                if where[y, x]:
                    o = float(opacity[y, x])
                    canvas[y, x] = color * o + white * (1 - o)
    return canvas.astype(np.uint8)
