"""Reference surface: InkLayer/inpainting/inpaint_ControlNet.py.  The ControlNet pipeline itself (diffusers) is not part
of this build: the model is the callable registered with InkLayer.inpainting.set_inpaint_func."""
import InkLayer.inpainting as _reg
from InkLayer.inpainting.util import run_inpainting_on_sketch_dir_template


def run_inpainting_on_sketch_dir(sketch_dir):
    fn = _reg.require_inpaint_func("InkLayer.inpainting.inpaint_ControlNet.run_inpainting_on_sketch_dir")
    return run_inpainting_on_sketch_dir_template(fn)(sketch_dir)
