"""Layer assembly and inpainting plugin (reference surface: InkLayer/inpainting/), MI355X kernels underneath.

Everything of the reference's inpainting stage except the diffusion model runs here (inklayer_amd/layers.py for the
layers, inklayer_amd/inpaint.py for what ControlNet_inpaint does around the model call).  The model is registered in
one of two ways:

    import InkLayer.inpainting
    InkLayer.inpainting.set_diffusion_pipe(pipe)  # the diffusers pipeline object; kind="controlnet" (default) or "sdxl"
    InkLayer.inpainting.set_inpaint_func(fn)      # fn(input_image: PIL.Image, mask_image: PIL.Image) -> PIL.Image

With a pipe, the reference's pre- and post-processing (contrast, denoise, mask dilation, Lanczos resizes, condition
tensor, clean-up, unsharp mask) runs on the GPU around `pipe(...)`, which is called with the reference's keyword
arguments.  A function does all of that itself: `input_image` is the sketch layer, `mask_image` the 0 / 255 edit mask
(mode "L"); the result has the same size.  A registered function has priority over a registered pipe.  With neither,
the entry points that need the model raise InkLayerHipError."""

_INPAINT_FUNC = None
_PIPE = None
_PIPE_KIND = None
PIPE_KINDS = ("controlnet", "sdxl")


def set_inpaint_func(fn):
    """Register (or, with None, remove) the inpainting model: fn(input_image, mask_image) -> PIL.Image."""
    global _INPAINT_FUNC
    if fn is not None and not callable(fn):
        raise TypeError("set_inpaint_func: expected a callable (input_image, mask_image) -> PIL.Image, or None")
    _INPAINT_FUNC = fn


def get_inpaint_func():
    return _INPAINT_FUNC


def set_diffusion_pipe(pipe, kind="controlnet"):
    """Register (or, with None, remove) the diffusion pipeline: a callable taking the keyword arguments the reference
    passes (StableDiffusionControlNetInpaintPipeline for kind "controlnet", AutoPipelineForInpainting for "sdxl") and
    returning an object whose `.images[0]` is a PIL image."""
    global _PIPE, _PIPE_KIND
    if pipe is None:
        _PIPE = _PIPE_KIND = None
        return
    if not callable(pipe):
        raise TypeError("set_diffusion_pipe: expected a callable diffusers pipeline, or None")
    if kind not in PIPE_KINDS:
        raise ValueError(f"set_diffusion_pipe: kind must be one of {PIPE_KINDS}, not {kind!r}")
    _PIPE, _PIPE_KIND = pipe, kind


def get_diffusion_pipe(kind=None):
    """The registered pipe (None without one); with `kind`, only a pipe registered as that kind."""
    return _PIPE if kind is None or kind == _PIPE_KIND else None


def get_diffusion_pipe_kind():
    return _PIPE_KIND


def _no_model(caller, what="inpainting function or diffusion pipe"):
    from inklayer_amd._lib import InkLayerHipError
    return InkLayerHipError(
        f"{caller}: no {what} is registered - the diffusion model is not part of this build; "
        "register one with InkLayer.inpainting.set_inpaint_func(fn), fn(input_image, mask_image) -> PIL.Image, "
        "or hand the diffusers pipeline to InkLayer.inpainting.set_diffusion_pipe(pipe, kind='controlnet' | 'sdxl')")


def require_diffusion_pipe(caller, kind):
    pipe = get_diffusion_pipe(kind)
    if pipe is None:
        raise _no_model(caller, f"{kind} diffusion pipe")
    return pipe


def resolve_inpaint_func():
    """What inpaints a layer: the registered function if there is one, else the reference's ControlNet_inpaint /
    SDXL_inpaint around the registered pipe, else None."""
    if _INPAINT_FUNC is not None:
        return _INPAINT_FUNC
    if _PIPE is None:
        return None
    pipe, kind = _PIPE, _PIPE_KIND

    def inpaint_with_pipe(input_image, mask_image):
        from inklayer_amd import inpaint
        fn = inpaint.controlnet_inpaint if kind == "controlnet" else inpaint.sdxl_inpaint
        return fn(pipe, input_image, mask_image)

    return inpaint_with_pipe


def require_inpaint_func(caller):
    """resolve_inpaint_func(), or a clear error naming the call that needed it."""
    fn = resolve_inpaint_func()
    if fn is None:
        raise _no_model(caller)
    return fn
