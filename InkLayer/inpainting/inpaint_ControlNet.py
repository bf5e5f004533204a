"""Reference surface: InkLayer/inpainting/inpaint_ControlNet.py.  The ControlNet pipeline itself (diffusers) is not part
of this build: it is the pipe registered with InkLayer.inpainting.set_diffusion_pipe (or, for the directory entry point,
the callable registered with set_inpaint_func).  Everything around the model call runs on the GPU
(inklayer_amd/inpaint.py); these functions take and return PIL images as the reference's do."""
import InkLayer.inpainting as _reg
from InkLayer.inpainting.util import run_inpainting_on_sketch_dir_template


def preprocess_image(image, enhance_contrast=True, denoise=True):
    from inklayer_amd import inpaint
    if image.mode != "RGB":
        raise ValueError(f"preprocess_image: an RGB image is expected, not mode {image.mode!r}")
    return inpaint.to_pil(inpaint.preprocess_image(inpaint.to_device(image, "RGB"), enhance_contrast, denoise))


def preprocess_mask(mask, dilate_iterations=1, blur_radius=1):
    from inklayer_amd import inpaint
    return inpaint.to_pil(inpaint.preprocess_mask(inpaint.to_device(mask, "L"), dilate_iterations, blur_radius))


def make_inpaint_condition(init_image, mask_image):
    """-> float32 tensor [1, 3, H, W] on the host, as the reference returns it."""
    from inklayer_amd import inpaint
    rgb, mask = inpaint.to_device(init_image, "RGB"), inpaint.to_device(mask_image, "L")
    assert rgb.shape[:2] == mask.shape, "image and mask must have the same dimensions"
    return inpaint.condition(rgb, mask).cpu()


def postprocess_result(result_image, original_image, mask_image):
    from inklayer_amd import inpaint
    result, original = inpaint.to_device(result_image, "RGB"), inpaint.to_device(original_image, "RGB")
    return inpaint.to_pil(inpaint.postprocess(result, original, inpaint.to_device(mask_image, "L")))


def ControlNet_inpaint(input_image, mask_image, preprocess_input=True, postprocess_output=True):
    pipe = _reg.require_diffusion_pipe("InkLayer.inpainting.inpaint_ControlNet.ControlNet_inpaint", "controlnet")
    from inklayer_amd import inpaint
    return inpaint.controlnet_inpaint(pipe, input_image, mask_image, preprocess_input, postprocess_output)


def run_inpainting_on_sketch_dir(sketch_dir):
    fn = _reg.require_inpaint_func("InkLayer.inpainting.inpaint_ControlNet.run_inpainting_on_sketch_dir")
    return run_inpainting_on_sketch_dir_template(fn)(sketch_dir)
