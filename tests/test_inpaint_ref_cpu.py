"""The numpy restatement of the inpainting pre- and post-processing (tests/inpaint_ref.py) against Pillow itself, hand
cases for the stages restated from OpenCV (which is not installed: they are not pinned to cv2), the package's table
builders against the restatement's, and the pipe registry.  No GPU."""
import functools

import numpy as np
import pytest

import inpaint_ref as R

SHAPES = [(70, 130), (130, 70), (97, 61)]


@functools.lru_cache(maxsize=None)
def sketch(shape):
    rgb, mask = R.make_sketch(shape)
    rgb.setflags(write=False)
    mask.setflags(write=False)
    return rgb, mask


def _pil(a):
    from PIL import Image
    return Image.fromarray(a)


@pytest.mark.parametrize("shape", SHAPES)
def test_contrast_equals_pillow_and_clips_at_both_ends(shape):
    from PIL import ImageEnhance
    rgb, _ = sketch(shape)
    want = np.asarray(ImageEnhance.Contrast(_pil(rgb)).enhance(1.2))
    assert np.array_equal(R.contrast(rgb), want)
    assert (want == 0).mean() > 0.01 and (want == 255).mean() > 0.01 and ((want > 0) & (want < 255)).mean() > 0.1


@pytest.mark.parametrize("shape", SHAPES)
def test_lanczos_equals_pillow_up_down_and_along_one_axis(shape):
    from PIL import Image
    rgb, mask = sketch(shape)
    H, W = shape
    for a in (rgb, mask):
        up = np.asarray(_pil(a).resize((768, 768), Image.LANCZOS))
        assert np.array_equal(R.resize(a, 768, 768, "lanczos"), up)
        assert np.array_equal(R.resize(up, H, W, "lanczos"), np.asarray(_pil(up).resize((W, H), Image.LANCZOS)))
        assert np.array_equal(R.resize(a, 200, W, "lanczos"), np.asarray(_pil(a).resize((W, 200), Image.LANCZOS)))
        assert np.array_equal(R.resize(a, H, 33, "lanczos"), np.asarray(_pil(a).resize((33, H), Image.LANCZOS)))
        assert np.array_equal(R.resize(a, H, W, "lanczos"), a)


@pytest.mark.parametrize("shape", SHAPES)
def test_default_bicubic_equals_pillow_up_and_down(shape):
    from PIL import Image
    rgb, mask = sketch(shape)
    H, W = shape
    for a in (rgb, mask):
        up = np.asarray(_pil(a).resize((1024, 1024)))                  # the default filter of these modes: bicubic
        assert np.array_equal(R.resize(a, 1024, 1024, "bicubic"), up)
        assert np.array_equal(R.resize(up, H, W, "bicubic"), np.asarray(_pil(up).resize((W, H), Image.BICUBIC)))
    assert np.array_equal(R.resize(rgb, 40, 50, "bilinear"), np.asarray(_pil(rgb).resize((50, 40), Image.BILINEAR)))


@pytest.mark.parametrize("shape", SHAPES)
def test_grey_round_trip_blur_and_unsharp_equal_pillow(shape):
    from PIL import ImageFilter
    rgb, _ = sketch(shape)
    grey = _pil(rgb).convert("L").convert("RGB")
    assert np.array_equal(R.gray_rgb(rgb), np.asarray(grey))
    assert np.array_equal(R.luma(rgb), np.asarray(_pil(rgb).convert("L")))
    assert np.array_equal(R.box_blur(rgb), np.asarray(_pil(rgb).filter(ImageFilter.GaussianBlur(0.5))))
    want = np.asarray(grey.filter(ImageFilter.UnsharpMask(radius=0.5, percent=150, threshold=3)))
    assert np.array_equal(R.finish(rgb), want)
    assert (want != np.asarray(grey)).mean() > 0.1                     # the comparison is not vacuous
    assert np.array_equal(R.unsharp(rgb), np.asarray(_pil(rgb).filter(ImageFilter.UnsharpMask(0.5, 150, 3))))


def test_mask_blur_of_a_single_pixel():
    one = np.zeros((9, 11), np.uint8)
    one[4, 5] = 255
    got = R.mask_prepare(one, dilate_iterations=0)
    assert got[3:6, 4:7].tolist() == [[16, 32, 16], [32, 64, 32], [16, 32, 16]] and got.sum() == 64 + 4 * 32 + 4 * 16
    d = R.mask_prepare(one, dilate_iterations=1, blur=False)
    assert d[3:6, 4:7].min() == 255 and d.sum() == 9 * 255
    corner = np.zeros((9, 11), np.uint8)
    corner[0, 0] = 200                                                 # pixels outside the image do not take part
    assert R.dilate3(corner).sum() == 4 * 200


def test_constant_images_are_fixed_points():
    const = np.full((9, 11, 3), 77, np.uint8)
    assert np.array_equal(R.bilateral(const), const)
    clean, thresh = R.cleanup(const)
    assert (thresh == 255).all() and (clean == 255).all()
    assert np.array_equal(R.contrast(const), const)


@pytest.mark.parametrize("shape", SHAPES)
def test_cleanup_and_soft_blend_on_the_sketch(shape):
    rgb, mask = sketch(shape)
    clean, thresh = R.cleanup(rgb)
    assert set(np.unique(thresh).tolist()) == {0, 255}
    assert (thresh == 255).mean() >= 0.05 and (thresh == 0).mean() >= 0.05
    assert np.array_equal(clean[thresh == 0], rgb[thresh == 0]) and (clean[thresh == 255] == 255).all()
    assert np.array_equal(R.soft_blend(rgb, rgb, mask), rgb)           # clean == original: unchanged
    soft = R.soft_mask(mask)
    assert soft.min() == 0.0 and soft.max() == 1.0 and ((soft > 0) & (soft < 1)).any()
    out = R.soft_blend(clean, rgb, mask)
    inside, outside = soft == 1.0, soft == 0.0
    assert np.array_equal(out[inside], clean[inside]) and np.array_equal(out[outside], rgb[outside])
    assert (R.bilateral(rgb) != rgb).mean() > 0.05                     # the colour weights matter on this input


def test_condition_tensor():
    rgb, mask = sketch((70, 130))
    m = R.mask_prepare(mask)
    c = R.condition(rgb, m)
    assert c.shape == (1, 3, 70, 130) and c.dtype == np.float32
    want = np.array(rgb).astype(np.float32) / 255.0
    want[m.astype(np.float32) / 255.0 > 0.5] = -1.0                    # the reference's own statement of it
    assert np.array_equal(c[0].transpose(1, 2, 0), want) and (c == -1).any() and set(np.unique(m)) - {0, 255}


# ---- the package's host-side tables ------------------------------------------------------------------------------------
@pytest.mark.parametrize("filt", ["bilinear", "bicubic", "lanczos"])
def test_package_coefficient_tables_equal_the_restatement(filt):
    from inklayer_amd.resize import pil_resize_coeffs
    for n_in, n_out in ((70, 768), (768, 130), (97, 61), (61, 97), (130, 33), (1024, 70)):
        bounds, coef = pil_resize_coeffs(n_in, n_out, filt)
        dense = np.zeros((n_out, n_in), np.int64)
        for o in range(n_out):
            lo, n = bounds[o]
            assert 0 <= lo and lo + n <= n_in and n <= coef.shape[1]
            dense[o, lo:lo + n] = coef[o, :n]
            assert not coef[o, n:].any()
        assert np.array_equal(dense, R.resize_coeffs(n_in, n_out, filt))


def test_package_tables_equal_the_restatement():
    from inklayer_amd import inpaint
    assert inpaint.box_weights(0.5) == R.box_weights(0.5)
    ww, fw = inpaint.box_weights(0.5)
    assert ww + 2 * fw in ((1 << 24), (1 << 24) - 1) and 0 < fw < ww
    with pytest.raises(ValueError):
        inpaint.box_weights(2.0)                                       # a box radius of 1 or more is not built
    assert inpaint.BILATERAL_TAPS == R.BILATERAL_TAPS and len(R.BILATERAL_TAPS) == 13
    sw, cw = R.bilateral_tables()
    assert np.array_equal(inpaint.bilateral_tables("cpu").numpy(), np.concatenate([sw, cw]))
    assert np.array_equal(inpaint.gauss11_taps("cpu").numpy(), R.gauss11())
    assert tuple(inpaint.gauss3_taps("cpu").tolist()) == R.gauss3_f64()
    assert (inpaint.PROMPT, inpaint.NEGATIVE_PROMPT, inpaint.SDXL_PROMPT) == (R.PROMPT, R.NEGATIVE, R.SDXL_PROMPT)


def test_inpaint_entry_points_reject_bad_arguments_without_launch():
    from inklayer_amd import _lib
    l = _lib.lib()
    p, q, r = 256, 512, 768
    assert l.ink_inp_contrast(None, 8, 8, 1.2, q, r, None) == 1
    assert l.ink_inp_contrast(p, 2, 8, 1.2, q, r, None) == 1                     # no reflect-101 neighbour at distance 2
    assert l.ink_inp_bilateral(p, 8, 8, q, p, None) == 1                         # in place
    assert l.ink_inp_bilateral(p, 8, 2, q, r, None) == 1
    assert l.ink_inp_mask_prepare(p, 8, 8, 0, 0, q, r, None) == 1                # nothing to do
    assert l.ink_inp_mask_prepare(p, 8, 8, 1, 2, q, r, None) == 1
    assert l.ink_inp_mask_prepare(p, 8, 8, -1, 1, q, r, None) == 1
    assert l.ink_resize_u8(p, 8, 8, 2, q, 4, 4, r, r, 3, r, r, 3, r, None) == 1          # 1 or 3 channels
    assert l.ink_resize_u8(p, 8, 8, 3, q, 4, 4, None, r, 3, r, r, 3, r, None) == 1
    assert l.ink_resize_u8(p, 8, 8, 3, q, 4, 4, r, r, 3, r, r, 3, None, None) == 1       # both passes need tmp
    assert l.ink_inp_condition(p, None, 8, 8, q, None) == 1
    assert l.ink_inp_cleanup(p, 8, 8, None, q, r, 1024, None) == 1
    assert l.ink_inp_cleanup(p, 8, 8, q, r, 1024, p, None) == 1                  # in place
    assert l.ink_inp_soft_blend(p, p, p, 8, 8, q, None, r, None) == 1
    assert l.ink_inp_luma(p, 8, 8, 2, q, None) == 1
    assert l.ink_inp_unsharp(p, 8, 8, 3, 15379114, 1, 150, 3, q, r, None) == 1   # fw is not (2^24 - ww) / 2
    assert l.ink_inp_unsharp(p, 8, 8, 2, 15379114, 699051, 150, 3, q, r, None) == 1
    assert l.ink_inp_rgba_cut(p, p, 0, 8, q, None) == 1
    assert l.ink_abi_version() == 10


def test_small_images_raise_value_error():
    from PIL import Image
    from inklayer_amd import inpaint, ops
    with pytest.raises(ValueError, match="smaller than 3"):
        inpaint.to_device(Image.new("RGB", (9, 2)), "RGB")             # refused before anything touches the device
    with pytest.raises(ValueError, match="smaller than 3"):
        inpaint.to_device(np.zeros((9, 2), np.uint8), "L")
    with pytest.raises(ValueError):
        ops._stencil_size(2, 9, "x")


# ---- registry ----------------------------------------------------------------------------------------------------------
@pytest.fixture
def registry():
    import InkLayer.inpainting as reg
    old_fn, old_pipe, old_kind = reg.get_inpaint_func(), reg.get_diffusion_pipe(), reg.get_diffusion_pipe_kind()
    reg.set_inpaint_func(None)
    reg.set_diffusion_pipe(None)
    yield reg
    reg.set_inpaint_func(old_fn)
    reg.set_diffusion_pipe(old_pipe, old_kind or "controlnet")


def test_registry_without_anything_raises_and_names_both_ways(registry):
    from PIL import Image
    from inklayer_amd._lib import InkLayerHipError
    from InkLayer.inpainting.inpaint_ControlNet import ControlNet_inpaint, run_inpainting_on_sketch_dir
    from InkLayer.inpainting.inpaint_SDXL import SDXL_inpaint
    im, m = Image.new("RGB", (8, 8)), Image.new("L", (8, 8))
    with pytest.raises(InkLayerHipError, match=r"ControlNet_inpaint.*set_diffusion_pipe"):
        ControlNet_inpaint(im, m)
    with pytest.raises(InkLayerHipError, match=r"SDXL_inpaint.*set_diffusion_pipe"):
        SDXL_inpaint(im, m)
    with pytest.raises(InkLayerHipError, match=r"run_inpainting_on_sketch_dir.*set_inpaint_func.*set_diffusion_pipe"):
        run_inpainting_on_sketch_dir("nowhere")
    assert registry.resolve_inpaint_func() is None and registry.get_diffusion_pipe() is None


def test_registered_function_wins_over_a_pipe_and_none_removes_the_pipe(registry):
    from inklayer_amd._lib import InkLayerHipError
    pipe = lambda **kw: None
    fn = lambda input_image, mask_image: input_image
    registry.set_diffusion_pipe(pipe)
    assert registry.get_diffusion_pipe() is pipe and registry.get_diffusion_pipe_kind() == "controlnet"
    assert registry.get_diffusion_pipe("controlnet") is pipe and registry.get_diffusion_pipe("sdxl") is None
    closure = registry.resolve_inpaint_func()
    assert callable(closure) and closure is not pipe and registry.require_inpaint_func("x") is not None
    registry.set_inpaint_func(fn)
    assert registry.resolve_inpaint_func() is fn and registry.require_inpaint_func("x") is fn
    registry.set_inpaint_func(None)
    registry.set_diffusion_pipe(pipe, kind="sdxl")
    assert registry.get_diffusion_pipe("sdxl") is pipe and registry.get_diffusion_pipe("controlnet") is None
    with pytest.raises(InkLayerHipError, match="controlnet"):
        registry.require_diffusion_pipe("x", "controlnet")
    registry.set_diffusion_pipe(None)
    assert registry.get_diffusion_pipe() is None and registry.resolve_inpaint_func() is None
    with pytest.raises(TypeError):
        registry.set_diffusion_pipe(3)
    with pytest.raises(ValueError):
        registry.set_diffusion_pipe(pipe, kind="other")


def test_runner_keeps_its_error_and_message_without_a_model(registry, tmp_path):
    from InkLayer.runner import run_inpaint_single_layer
    with pytest.raises(NotImplementedError):
        run_inpaint_single_layer({"image_name": "x", "layer_path": "layer_1.png", "prompt": "p"}, str(tmp_path), str(tmp_path))
