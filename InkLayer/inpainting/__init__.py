"""Layer assembly plugin (reference surface: InkLayer/inpainting/), MI355X kernels underneath.

Everything of the reference's inpainting stage except the diffusion model runs here (inklayer_amd/layers.py).  The
model is a callable the user registers:

    import InkLayer.inpainting
    InkLayer.inpainting.set_inpaint_func(fn)      # fn(input_image: PIL.Image, mask_image: PIL.Image) -> PIL.Image

`input_image` is the sketch layer, `mask_image` the 0 / 255 edit mask (mode "L"); the result has the same size.
Without a registered function the entry points that need the model raise InkLayerHipError."""

_INPAINT_FUNC = None


def set_inpaint_func(fn):
    """Register (or, with None, remove) the inpainting model: fn(input_image, mask_image) -> PIL.Image."""
    global _INPAINT_FUNC
    if fn is not None and not callable(fn):
        raise TypeError("set_inpaint_func: expected a callable (input_image, mask_image) -> PIL.Image, or None")
    _INPAINT_FUNC = fn


def get_inpaint_func():
    return _INPAINT_FUNC


def require_inpaint_func(caller):
    """The registered function, or a clear error naming the call that needed it."""
    if _INPAINT_FUNC is None:
        from inklayer_amd._lib import InkLayerHipError
        raise InkLayerHipError(
            f"{caller}: no inpainting function is registered - the diffusion model is not part of this build; "
            "register one with InkLayer.inpainting.set_inpaint_func(fn), fn(input_image, mask_image) -> PIL.Image")
    return _INPAINT_FUNC
