"""Inpainting around a diffusion pipe: everything ControlNet_inpaint, inpaint_single_layer and
SDXL_inpaint do to the image and the mask before and after the model call, on the GPU.

  preprocess_image / preprocess_mask   InkLayer/inpainting/inpaint_ControlNet.py:49-75
  condition                            make_inpaint_condition, inpaint_ControlNet.py:77-90
  postprocess                          postprocess_result / _adaptive_threshold_blend, inpaint_ControlNet.py:92-124
  finish                               the grey round trip and the unsharp mask, inpaint_ControlNet.py:181-182
  controlnet_inpaint                   ControlNet_inpaint, inpaint_ControlNet.py:126-184
  single_layer_inpaint                 inpaint_single_layer.py:34-78
  sdxl_inpaint                         SDXL_inpaint, inpaint_SDXL.py:13-33

The diffusion model itself is not part of this build: `pipe` is the user's diffusers pipeline (any callable that takes
the reference's keyword arguments and returns an object with `.images`).  The kernels are csrc/inpaint_ops.hip; this
module computes their small tables in double precision, orders the launches, and moves the image to the host only for
the pipe call and for the value it returns.  The Pillow stages equal Pillow bit for bit; the OpenCV stages restate
OpenCV's published algorithm (DESIGN §9 says what that does and does not pin)."""
from __future__ import annotations

import math
from typing import Dict, Tuple

import numpy as np
import torch

from . import ops

PROMPT = ("high quality black and white line drawing, clean precise lines, detailed sketch, professional illustration, "
          "sharp edges")
NEGATIVE_PROMPT = "blurry, smudged, messy lines, low quality, artifacts, noise, distorted, pixelated"
SDXL_PROMPT = "black and white sketch, complete lines"
TARGET_SIZE = 768            # inpaint_ControlNet.py:149
SDXL_SIZE = 1024             # inpaint_SDXL.py:23
SEED = 3

# the taps of cv2.bilateralFilter(d=5): the radius-2 disc in row-major order
BILATERAL_TAPS = [(i, j) for i in range(-2, 3) for j in range(-2, 3) if i * i + j * j <= 4]

_TABLES: Dict[tuple, torch.Tensor] = {}


def _cached(key, dev, make) -> torch.Tensor:
    k = (key, str(dev))
    if k not in _TABLES:
        _TABLES[k] = make().to(dev)
    return _TABLES[k]


def bilateral_tables(dev, sigma_color: float = 50.0, sigma_space: float = 50.0) -> torch.Tensor:
    """f32 [13 + 768]: exp(-(i^2 + j^2) / (2 sigma_space^2)) per tap, then exp(-d^2 / (2 sigma_color^2)), d = 0..767."""
    def make():
        sw = [math.exp(-(i * i + j * j) / (2.0 * sigma_space * sigma_space)) for i, j in BILATERAL_TAPS]
        cw = [math.exp(-(d * d) / (2.0 * sigma_color * sigma_color)) for d in range(768)]
        return torch.from_numpy(np.array(sw + cw, np.float32))
    return _cached(("bilateral", sigma_color, sigma_space), dev, make)


def gauss11_taps(dev) -> torch.Tensor:
    """f32 [11]: cv2.getGaussianKernel(11, 2) as adaptiveThreshold uses it: c_i = exp(-0.125 (i - 5)^2), k = c / sum."""
    def make():
        c = [math.exp(-0.125 * (i - 5) * (i - 5)) for i in range(11)]
        s = 0.0
        for v in c:
            s += v
        return torch.from_numpy(np.array([v * (1.0 / s) for v in c], np.float32))
    return _cached("gauss11", dev, make)


def gauss3_taps(dev) -> torch.Tensor:
    """f64 [2]: centre and side weight of cv2.getGaussianKernel(3, 1)."""
    def make():
        c = [math.exp(-0.5), 1.0, math.exp(-0.5)]
        inv = 1.0 / (c[0] + c[1] + c[2])
        return torch.tensor([c[1] * inv, c[0] * inv], dtype=torch.float64)
    return _cached("gauss3", dev, make)


def box_weights(radius: float = 0.5, passes: int = 3) -> Tuple[int, int]:
    """Pillow's Gaussian-to-box rule (BoxBlur.c _gaussian_blur_radius, evaluated in float as there) and the two
    fixed-point weights of a box pass, for a box radius below 1."""
    f = np.float32
    sigma2 = f(f(radius) * f(radius) / f(passes))
    L = f(math.sqrt(12.0 * float(sigma2) + 1.0))
    l = f(math.floor((float(L) - 1.0) / 2.0))
    a = f(f(2 * l + 1) * f(f(l * f(l + 1)) - f(f(3) * sigma2)))
    a = f(a / f(f(6) * f(sigma2 - f(f(l + 1) * f(l + 1)))))
    r = f(l + a)
    if int(r) != 0:
        raise ValueError(f"unsharp mask: blur radius {radius} needs a box radius of {float(r):.3f}; only box radii below 1 "
                         "are built (the reference uses radius 0.5)")
    ww = int(f(1 << 24) / f(f(r * f(2)) + f(1)))
    return ww, ((1 << 24) - ww) // 2


# ---- host <-> device ---------------------------------------------------------------------------------------------------
def _device() -> torch.device:
    return torch.device("cuda", torch.cuda.current_device())


def to_device(image, mode: str) -> torch.Tensor:
    """A PIL image (converted to `mode`, "RGB" or "L"), a host array or a tensor -> contiguous uint8 tensor on the GPU."""
    if torch.is_tensor(image):
        t = image
    elif isinstance(image, np.ndarray):
        t = torch.from_numpy(np.ascontiguousarray(image))
    else:
        t = torch.from_numpy(np.array(image if image.mode == mode else image.convert(mode), np.uint8))
    assert t.dtype == torch.uint8 and t.dim() == (3 if mode == "RGB" else 2), f"expected an 8-bit {mode} image"
    if t.shape[0] < 3 or t.shape[1] < 3:                      # reflect-101 at radius 2 has no such neighbour
        raise ValueError(f"inpainting: images smaller than 3 pixels on a side are not supported (got {t.shape[1]}x{t.shape[0]})")
    return t.to(_device()).contiguous()


def to_pil(t: torch.Tensor):
    from PIL import Image
    return Image.fromarray(t.cpu().numpy())


# ---- stages ------------------------------------------------------------------------------------------------------------
def preprocess_image(rgb: torch.Tensor, enhance_contrast: bool = True, denoise: bool = True) -> torch.Tensor:
    if enhance_contrast:
        rgb = ops.inp_contrast(rgb, 1.2)
    if denoise:
        rgb = ops.inp_bilateral(rgb, bilateral_tables(rgb.device))
    return rgb


def preprocess_mask(mask: torch.Tensor, dilate_iterations: int = 1, blur_radius: int = 1) -> torch.Tensor:
    if blur_radius not in (0, 1):
        raise NotImplementedError("preprocess_mask: blur_radius 0 or 1 (the reference's value) only")
    return ops.inp_mask_prepare(mask, dilate_iterations, blur_radius > 0)


def resize(image: torch.Tensor, size: Tuple[int, int], filter: str = "lanczos") -> torch.Tensor:
    """Image.resize(size, filter); size is (width, height) as in Pillow."""
    return ops.inp_resize_u8(image, int(size[1]), int(size[0]), filter)


def condition(rgb: torch.Tensor, mask: torch.Tensor) -> torch.Tensor:
    return ops.inp_condition(rgb, mask)


def postprocess(result: torch.Tensor, original: torch.Tensor, mask: torch.Tensor) -> torch.Tensor:
    clean, _ = ops.inp_cleanup(result, gauss11_taps(result.device))
    return ops.inp_soft_blend(clean, original, mask, gauss3_taps(result.device))


def gray_round_trip(rgb: torch.Tensor) -> torch.Tensor:
    return ops.inp_luma(rgb, 3)


def unsharp(image: torch.Tensor, radius: float = 0.5, percent: int = 150, threshold: int = 3) -> torch.Tensor:
    ww, fw = box_weights(radius)
    return ops.inp_unsharp(image, ww, fw, percent, threshold)


def finish(rgb: torch.Tensor) -> torch.Tensor:
    return unsharp(gray_round_trip(rgb))


# ---- the pipe ----------------------------------------------------------------------------------------------------------
def _generator() -> torch.Generator:
    return torch.Generator(device="cuda").manual_seed(SEED)


def _pipe_image(pipe, **kwargs) -> "PIL.Image.Image":
    out = pipe(**kwargs)
    return out.images[0]


def _controlnet_call(pipe, inp: torch.Tensor, mask: torch.Tensor, generator, prompt: str, guidance_scale: float,
                     scale: float) -> torch.Tensor:
    image = _pipe_image(pipe, prompt=prompt, negative_prompt=NEGATIVE_PROMPT, image=to_pil(inp), mask_image=to_pil(mask),
                        control_image=condition(inp, mask).cpu(), guidance_scale=guidance_scale, num_inference_steps=30,
                        controlnet_conditioning_scale=scale, generator=generator)
    return to_device(image, "RGB")


@torch.no_grad()
def controlnet_inpaint(pipe, input_image, mask_image, preprocess_input: bool = True, postprocess_output: bool = True):
    """ControlNet_inpaint with `pipe` in place of get_controlnet_pipeline() -> PIL image of the input's size."""
    original_input = to_device(input_image, "RGB")
    original_mask = to_device(mask_image, "L")
    assert original_input.shape[:2] == original_mask.shape, "image and mask must have the same dimensions"
    image, mask = original_input, original_mask
    if preprocess_input:
        image, mask = preprocess_image(image), preprocess_mask(mask)
    generator = _generator()
    side = (TARGET_SIZE, TARGET_SIZE)
    input_resized, mask_resized = resize(image, side), resize(mask, side)
    result = None
    for pass_num in range(2):
        if pass_num > 0:                                     # the second pass starts from the first one's image
            input_resized = resize(result, side)
        result = _controlnet_call(pipe, input_resized, mask_resized, generator, PROMPT, 9.0, 1.2)
    result = resize(result, (original_input.shape[1], original_input.shape[0]))
    if postprocess_output:
        result = postprocess(result, original_input, original_mask)
    return to_pil(finish(result))


@torch.no_grad()
def single_layer_inpaint(pipe, image, mask, prompt: str):
    """inpaint_single_layer.py:34-78 -> (result PIL "RGB", layer PIL "RGBA" cut with the preprocessed mask > 128)."""
    from PIL import Image
    rgb = preprocess_image(to_device(image, "RGB"))
    m = preprocess_mask(to_device(mask, "L"))
    assert rgb.shape[:2] == m.shape, "image and mask must have the same dimensions"
    side = (TARGET_SIZE, TARGET_SIZE)
    result = _controlnet_call(pipe, resize(rgb, side), resize(m, side), _generator(), prompt, 7.0, 0.6)
    result = resize(result, (rgb.shape[1], rgb.shape[0]))
    rgba = ops.inp_rgba_cut(result, m)
    return to_pil(result), Image.fromarray(rgba.cpu().numpy(), "RGBA")


@torch.no_grad()
def sdxl_inpaint(pipe, input_image, mask_image):
    """SDXL_inpaint with `pipe` in place of the pipeline it loads -> PIL image of the input's size."""
    rgb, mask = to_device(input_image, "RGB"), to_device(mask_image, "L")
    side = (SDXL_SIZE, SDXL_SIZE)
    image = _pipe_image(pipe, prompt=SDXL_PROMPT, image=to_pil(resize(rgb, side, "bicubic")),
                        mask_image=to_pil(resize(mask, side, "bicubic")), guidance_scale=8.0, num_inference_steps=20,
                        strength=0.99, generator=_generator())
    result = resize(to_device(image, "RGB"), (rgb.shape[1], rgb.shape[0]))
    return to_pil(gray_round_trip(result))
