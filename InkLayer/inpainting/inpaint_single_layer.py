"""Reference surface: InkLayer/inpainting/inpaint_single_layer.py with the registered inpainting function in place of
the ControlNet pipeline (the text prompt is not passed on: the registered signature has no prompt)."""
import os

import numpy as np
from PIL import Image

import InkLayer.inpainting as _reg


def inpaint_single_layer(image_path: str, mask_path: str, output_dir: str, prompt: str, layer_id: str,
                         position_data=None):
    fn = _reg.require_inpaint_func("InkLayer.inpainting.inpaint_single_layer.inpaint_single_layer")
    image = Image.open(image_path).convert("RGB")
    mask = Image.open(mask_path).convert("L")
    if position_data:
        mask = _move_mask(mask, position_data, image.size)
    result = fn(input_image=image, mask_image=mask).convert("RGB")
    if result.size != image.size:
        result = result.resize(image.size, Image.LANCZOS)
    result.save(os.path.join(output_dir, f"inpainted_layer_{layer_id}.png"))
    result_np, mask_np = np.array(result), np.array(mask)
    rgba = np.zeros(result_np.shape[:2] + (4,), np.uint8)
    inside = mask_np > 128
    rgba[..., :3][inside] = result_np[inside]
    rgba[..., 3][inside] = 255
    layer_rgba_path = os.path.join(output_dir, f"layer_{layer_id}_rgba.png")
    Image.fromarray(rgba, "RGBA").save(layer_rgba_path)
    return layer_rgba_path


def _move_mask(mask_img, position_data, canvas_size):
    if isinstance(position_data, list):
        position_data = position_data[0]
    x, y = int(position_data.get("x", 0)), int(position_data.get("y", 0))
    w, h = int(position_data.get("width", mask_img.width)), int(position_data.get("height", mask_img.height))
    canvas = Image.new("L", canvas_size, 0)
    canvas.paste(mask_img.resize((w, h)), (x, y))
    return canvas
