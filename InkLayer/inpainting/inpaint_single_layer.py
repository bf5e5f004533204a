"""Reference surface: InkLayer/inpainting/inpaint_single_layer.py.  With a ControlNet pipe registered
(InkLayer.inpainting.set_diffusion_pipe) it is the reference's path, text prompt included, around that pipe
(inklayer_amd/inpaint.py).  With a function registered (set_inpaint_func, which has priority) the function stands in for
the whole model call and the text prompt is not passed on: the registered signature has no prompt."""
import os

import numpy as np
from PIL import Image

import InkLayer.inpainting as _reg


def inpaint_single_layer(image_path: str, mask_path: str, output_dir: str, prompt: str, layer_id: str,
                         position_data=None):
    me = "InkLayer.inpainting.inpaint_single_layer.inpaint_single_layer"
    fn = _reg.get_inpaint_func()
    pipe = _reg.get_diffusion_pipe("controlnet") if fn is None else None
    if fn is None and pipe is None:
        fn = _reg.require_inpaint_func(me)       # raises, unless an SDXL pipe is all there is: then it stands in as a function
    image = Image.open(image_path).convert("RGB")
    mask = Image.open(mask_path).convert("L")
    if position_data:
        mask = _move_mask(mask, position_data, image.size)
    if pipe is not None:                                      # inpaint_single_layer.py:34-85
        from inklayer_amd import inpaint
        result, rgba = inpaint.single_layer_inpaint(pipe, image, mask, prompt)
        result.save(os.path.join(output_dir, f"inpainted_layer_{layer_id}.png"))
        layer_rgba_path = os.path.join(output_dir, f"layer_{layer_id}_rgba.png")
        rgba.save(layer_rgba_path)
        return layer_rgba_path
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
