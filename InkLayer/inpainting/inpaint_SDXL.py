"""Reference surface: InkLayer/inpainting/inpaint_SDXL.py.  The SDXL pipeline (diffusers) is the pipe registered with
InkLayer.inpainting.set_diffusion_pipe(pipe, kind="sdxl"); the resizes and the grey round trip run on the GPU."""
import InkLayer.inpainting as _reg
from InkLayer.inpainting.util import run_inpainting_on_sketch_dir_template


def SDXL_inpaint(input_image, mask_image):
    pipe = _reg.require_diffusion_pipe("InkLayer.inpainting.inpaint_SDXL.SDXL_inpaint", "sdxl")
    from inklayer_amd import inpaint
    return inpaint.sdxl_inpaint(pipe, input_image, mask_image)


def run_inpainting_on_sketch_dir(sketch_dir):
    _reg.require_diffusion_pipe("InkLayer.inpainting.inpaint_SDXL.run_inpainting_on_sketch_dir", "sdxl")
    return run_inpainting_on_sketch_dir_template(SDXL_inpaint)(sketch_dir)
