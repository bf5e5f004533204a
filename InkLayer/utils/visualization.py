"""Visualisation plugin (reference surface: InkLayer/utils/visualization.py), the reference's pictures pixel for pixel.

  generate_pastel_colors(n_colors)                      -> [(r, g, b)] in the interleaved hue order (no matplotlib)
  color_sketch_by_masks(sketch_image_pil, seg_masks, colors=None, enhance_factor=1.5, min_opacity=0.2) -> PIL image;
      the per-pixel Python loops of the reference are one table look-up (inklayer_amd/visualize.py), on the GPU when
      there is one
  get_background_idxs(sketch, seg_masks)                -> bool [H, W]: in no mask
  draw_norm_bbox_on_image / draw_boxes                  vector drawing and font rasterisation: Pillow calls on the host,
      in the reference's order and with its fall-backs (the text pixels depend on the font Pillow finds)"""
from typing import List, Union

import numpy as np
from PIL import Image, ImageDraw, ImageFont

from inklayer_amd.visualize import colour_sketch, pastel_colors


def generate_pastel_colors(n_colors):
    return pastel_colors(n_colors)


def color_sketch_by_masks(sketch_image_pil, seg_masks, colors=None, enhance_factor=1.5, min_opacity=0.2):
    """seg_masks: PIL images of mode "1" or "L", or bool / uint8 arrays (non-zero = inside); later masks paint over
    earlier ones, strokes in no mask turn black."""
    sketch = np.array(sketch_image_pil)
    if sketch.ndim == 3 and sketch.shape[2] != 3:
        sketch = sketch[..., :3]                                  # RGBA: cv2's RGB2GRAY reads the first three channels
    masks = [np.asarray(m) for m in seg_masks]
    return Image.fromarray(colour_sketch(sketch, masks, colors, enhance_factor, min_opacity))


def get_background_idxs(sketch, seg_masks):
    covered = np.zeros(np.shape(sketch)[:2], dtype=bool)
    for mask in seg_masks:
        covered = np.logical_or(covered, mask)
    return ~covered


def draw_norm_bbox_on_image(image_pil, bboxes, pred_phrases=None, color=(255, 0, 0), thickness=5):
    """Boxes in pastel colours (the `color` argument is overridden per box, as in the reference); a box whose largest
    coordinate is <= 1 is taken as normalised; the phrase is drawn at the box's corner in the box colour."""
    out = image_pil.copy()
    pen = ImageDraw.Draw(out)
    width, height = image_pil.size
    palette = generate_pastel_colors(len(bboxes))
    for i, (x1, y1, x2, y2) in enumerate(bboxes):
        if max(x1, y1, x2, y2) <= 1:
            x1, y1, x2, y2 = x1 * width, y1 * height, x2 * width, y2 * height
        pen.rectangle([x1, y1, x2, y2], outline=palette[i], width=thickness)
        if pred_phrases is not None and i < len(pred_phrases):
            pen.text((x1, y1), pred_phrases[i], fill=palette[i])
    return out


def draw_boxes(image: Union[str, Image.Image], boxes: List[List[float]], scores: List[float] = None,
               labels: List[str] = None, line_width: int = 3, font_size: int = 16, show_scores: bool = True,
               output_path: str = None) -> Image.Image:
    """Normalised boxes with a filled label tab ("label : 0.87") above each; arial.ttf when Pillow finds it, its
    default font otherwise; the tab is len(text) * font_size wide when the font has no getsize (Pillow >= 10)."""
    if isinstance(image, str):
        image = Image.open(image)
    out = image.copy()
    pen = ImageDraw.Draw(out)
    width, height = image.size
    try:
        font = ImageFont.truetype("arial.ttf", font_size)
    except Exception:
        font = ImageFont.load_default()
    palette = generate_pastel_colors(len(boxes))
    for i, box in enumerate(boxes):
        x1, y1, x2, y2 = box[0] * width, box[1] * height, box[2] * width, box[3] * height
        pen.rectangle([(x1, y1), (x2, y2)], outline=palette[i], width=line_width)
        parts = []
        if labels and i < len(labels):
            parts.append(labels[i])
        if show_scores and scores and i < len(scores):
            parts.append(f"{scores[i]:.2f}")
        if not parts:
            continue
        text = " : ".join(parts)
        text_w = font.getsize(text)[0] if hasattr(font, "getsize") else len(text) * font_size
        text_h = font_size + 4
        pen.rectangle([(x1, y1 - text_h), (x1 + text_w + 4, y1)], fill=palette[i])
        pen.text((x1 + 2, y1 - text_h + 2), text, fill="white", font=font)
    if output_path:
        out.save(output_path)
    return out
