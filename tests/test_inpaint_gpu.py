"""The inpainting pre- and post-processing on the GPU (csrc/inpaint_ops.hip, inklayer_amd/inpaint.py,
InkLayer/inpainting) against the numpy restatement tests/inpaint_ref.py, bit for bit at 70 x 130 and 130 x 70 (more
than one workgroup, ragged last one, both orientations of every border), the resampler against Pillow itself, and the
three compositions and the directory entry points around a deterministic stand-in for the diffusion pipe."""
import functools
import os

import numpy as np
import pytest
import torch

import inpaint_ref as R

pytestmark = pytest.mark.gpu

SHAPES = [(70, 130), (130, 70)]


@functools.lru_cache(maxsize=None)
def case(shape):
    """The generated sketch and every stage of the restatement on it, computed once."""
    rgb, mask = R.make_sketch(shape)
    c = dict(rgb=rgb, mask=mask)
    c["contrast"] = R.contrast(rgb)
    c["bilateral"] = R.bilateral(c["contrast"])
    c["mask_p"] = R.mask_prepare(mask)
    c["up"] = R.resize(c["bilateral"], 768, 768, "lanczos")
    c["mask_up"] = R.resize(c["mask_p"], 768, 768, "lanczos")
    c["clean"], c["thresh"] = R.cleanup(rgb)
    for v in c.values():
        v.setflags(write=False)
    return c


def _eq(got, want):
    got = got.cpu() if torch.is_tensor(got) else torch.from_numpy(np.ascontiguousarray(got))
    want = want.cpu() if torch.is_tensor(want) else torch.from_numpy(np.ascontiguousarray(want))
    return got.dtype == want.dtype and got.shape == want.shape and torch.equal(got, want)


def _dev(a, dev):
    return torch.from_numpy(np.array(a)).to(dev)                       # (a copy: the shared cases are read-only)


class StandInPipe:
    """Deterministic stand-in for the diffusers pipeline: records its keyword arguments and returns grey strokes drawn
    where the mask is >= 128, over a dimmed copy of the image there."""

    class Out:
        def __init__(self, image):
            self.images = [image]

    def __init__(self):
        self.calls = []

    def __call__(self, *args, **kw):
        from PIL import Image
        assert not args, "the reference calls the pipe with keyword arguments only"
        self.calls.append(kw)
        image, mask = np.array(kw["image"]), np.array(kw["mask_image"])
        yy, xx = np.mgrid[0:image.shape[0], 0:image.shape[1]]
        sel, strokes = mask >= 128, (yy + 2 * xx) % 23 < 3
        out = image.copy()
        out[sel & ~strokes] = out[sel & ~strokes] // 2 + 120
        out[sel & strokes] = (60, 70, 50)
        return StandInPipe.Out(Image.fromarray(out))


@pytest.fixture
def registry():
    import InkLayer.inpainting as reg
    old_fn, old_pipe, old_kind = reg.get_inpaint_func(), reg.get_diffusion_pipe(), reg.get_diffusion_pipe_kind()
    reg.set_inpaint_func(None)
    reg.set_diffusion_pipe(None)
    yield reg
    reg.set_inpaint_func(old_fn)
    reg.set_diffusion_pipe(old_pipe, old_kind or "controlnet")


# ---- every wrapper against the restatement ---------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES)
def test_contrast_and_bilateral(dev, shape):
    from inklayer_amd import inpaint, ops
    c = case(shape)
    got = ops.inp_contrast(_dev(c["rgb"], dev), 1.2)
    assert _eq(got, c["contrast"])
    assert _eq(ops.inp_bilateral(got, inpaint.bilateral_tables(dev)), c["bilateral"])
    const = np.full(shape + (3,), 77, np.uint8)
    assert _eq(ops.inp_bilateral(_dev(const, dev), inpaint.bilateral_tables(dev)), const)
    assert _eq(ops.inp_contrast(_dev(const, dev)), const)
    assert _eq(inpaint.preprocess_image(_dev(c["rgb"], dev)), c["bilateral"])
    assert _eq(inpaint.preprocess_image(_dev(c["rgb"], dev), enhance_contrast=False), R.bilateral(c["rgb"]))


@pytest.mark.parametrize("shape", SHAPES)
def test_mask_preparation(dev, shape):
    from inklayer_amd import ops
    c = case(shape)
    m = _dev(c["mask"], dev)
    assert _eq(ops.inp_mask_prepare(m), c["mask_p"])
    assert _eq(ops.inp_mask_prepare(m, 0, True), R.mask_prepare(c["mask"], 0, True))
    assert _eq(ops.inp_mask_prepare(m, 1, False), R.mask_prepare(c["mask"], 1, False))
    assert _eq(ops.inp_mask_prepare(m, 3, True), R.mask_prepare(c["mask"], 3, True))
    assert _eq(ops.inp_mask_prepare(m, 2, False), R.mask_prepare(c["mask"], 2, False))
    one = np.zeros(shape, np.uint8)
    one[0, 0] = one[shape[0] - 1, shape[1] - 1] = one[20, 30] = 255     # corners: the border rules of both steps
    for it in (0, 1):
        assert _eq(ops.inp_mask_prepare(_dev(one, dev), it, True), R.mask_prepare(one, it, True))
    assert ops.inp_mask_prepare(_dev(one, dev), 0, True)[19:22, 29:32].cpu().tolist() == [[16, 32, 16], [32, 64, 32], [16, 32, 16]]


FILTERS = {"bilinear": "BILINEAR", "bicubic": "BICUBIC", "lanczos": "LANCZOS"}


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("filt", sorted(FILTERS))
def test_resampler_equals_pillow(dev, shape, filt):
    from PIL import Image
    from inklayer_amd import ops
    c = case(shape)
    H, W = shape
    pil_filter = getattr(Image, FILTERS[filt])
    for a in (c["rgb"], c["mask_p"]):                                   # three channels and one
        src = _dev(a, dev)
        for oh, ow in ((768, 768), (33, 41), (H, 200), (31, W), (H, W), (2 * H + 1, W // 3)):
            got = ops.inp_resize_u8(src, oh, ow, filt)
            want = np.asarray(Image.fromarray(a).resize((ow, oh), pil_filter))
            assert _eq(got, want), (filt, a.ndim, oh, ow)
        assert ops.inp_resize_u8(src, H, W, filt).data_ptr() != src.data_ptr()      # the same size: a copy


@pytest.mark.parametrize("filt", sorted(FILTERS))
def test_resampler_small_edges(dev, filt):
    """The one resampler behind both wrappers at 37 x 53, one channel and three: one axis shrinks while the other grows
    (two kernel widths, the intermediate image in use), one axis only (no intermediate, no table for the other axis),
    down to a single pixel, and the same size through both wrappers."""
    from PIL import Image
    from inklayer_amd import ops
    from inklayer_amd.resize import plan_for
    H, W = 37, 53
    rng = np.random.default_rng(37 * 53)
    rgb = rng.integers(0, 256, size=(H, W, 3), dtype=np.uint8)
    rgb[:9] = 255                                                       # saturated areas: the clipping of overshoots
    rgb[9:14, ::5] = 0
    pil_filter = getattr(Image, FILTERS[filt])
    for a in (rgb, np.ascontiguousarray(rgb[..., 1])):
        src, ch = _dev(a, dev), (3 if a.ndim == 3 else 1)
        for oh, ow in ((19, 71), (H, 20), (64, W), (1, 1)):
            pl = plan_for(H, W, oh, ow, dev, filt, ch)
            assert (pl.tmp is None) == (oh == H or ow == W) and (pl.xb is None) == (ow == W) and (pl.yb is None) == (oh == H)
            if (oh, ow) == (19, 71):
                assert pl.kx != pl.ky
            want = np.asarray(Image.fromarray(a).resize((ow, oh), pil_filter))
            assert _eq(ops.inp_resize_u8(src, oh, ow, filt), want), (filt, ch, oh, ow)
            if ch == 3 and filt == "bilinear":
                assert _eq(ops.resize_bilinear_u8(src, oh, ow), want), (ch, oh, ow)
                out = torch.zeros((oh, ow, 3), dtype=torch.uint8, device=dev)
                assert ops.resize_bilinear_u8(src, oh, ow, out=out) is out and _eq(out, want)
        same = ops.inp_resize_u8(src, H, W, filt)                       # the same size: a copy ...
        assert same.data_ptr() != src.data_ptr() and _eq(same, a)
        if ch == 3:
            assert ops.resize_bilinear_u8(src, H, W) is src             # ... or the input itself


@pytest.mark.parametrize("shape", SHAPES)
def test_lanczos_round_trip_and_condition(dev, shape):
    from PIL import Image
    from inklayer_amd import ops
    c = case(shape)
    H, W = shape
    up = ops.inp_resize_u8(_dev(c["bilateral"], dev), 768, 768, "lanczos")
    mup = ops.inp_resize_u8(_dev(c["mask_p"], dev), 768, 768, "lanczos")
    assert _eq(up, c["up"]) and _eq(mup, c["mask_up"])
    assert _eq(ops.inp_resize_u8(up, H, W, "lanczos"), np.asarray(Image.fromarray(c["up"]).resize((W, H), Image.LANCZOS)))
    big = ops.inp_resize_u8(_dev(c["rgb"], dev), 1024, 1024, "bicubic")
    assert _eq(big, np.asarray(Image.fromarray(c["rgb"]).resize((1024, 1024))))
    cond = ops.inp_condition(up, mup)
    assert _eq(cond, R.condition(c["up"], c["mask_up"])) and cond.dtype == torch.float32
    assert tuple(cond.shape) == (1, 3, 768, 768) and bool((cond == -1).any()) and bool((cond >= 0).any())


@pytest.mark.parametrize("shape", SHAPES)
def test_cleanup_and_soft_blend(dev, shape):
    from inklayer_amd import inpaint, ops
    c = case(shape)
    rgb = _dev(c["rgb"], dev)
    clean, thresh = ops.inp_cleanup(rgb, inpaint.gauss11_taps(dev))
    assert _eq(thresh, c["thresh"]) and _eq(clean, c["clean"])
    frac = float((thresh == 255).float().mean())
    assert 0.05 <= frac <= 0.95
    const = _dev(np.full(shape + (3,), 77, np.uint8), dev)
    assert bool((ops.inp_cleanup(const, inpaint.gauss11_taps(dev))[1] == 255).all())
    taps2 = inpaint.gauss3_taps(dev)
    mask = _dev(c["mask"], dev)
    other = _dev(c["bilateral"], dev)
    assert _eq(ops.inp_soft_blend(clean, other, mask, taps2), R.soft_blend(c["clean"], c["bilateral"], c["mask"]))
    assert _eq(ops.inp_soft_blend(rgb, rgb, mask, taps2), c["rgb"])
    soft_mask = _dev(c["mask_p"], dev)                                  # a mask with grey levels
    assert _eq(ops.inp_soft_blend(clean, other, soft_mask, taps2), R.soft_blend(c["clean"], c["bilateral"], c["mask_p"]))
    assert _eq(inpaint.postprocess(rgb, other, mask), R.postprocess(c["rgb"], c["bilateral"], c["mask"]))


@pytest.mark.parametrize("shape", SHAPES)
def test_luma_unsharp_and_rgba_cut(dev, shape):
    from PIL import Image, ImageFilter
    from inklayer_amd import inpaint, ops
    c = case(shape)
    rgb = _dev(c["rgb"], dev)
    assert _eq(ops.inp_luma(rgb, 1), R.luma(c["rgb"])) and _eq(ops.inp_luma(rgb, 3), R.gray_rgb(c["rgb"]))
    ww, fw = inpaint.box_weights(0.5)
    pil = Image.fromarray(c["rgb"])
    assert _eq(ops.inp_unsharp(rgb, ww, fw, 150, 3), np.asarray(pil.filter(ImageFilter.UnsharpMask(0.5, 150, 3))))
    assert _eq(ops.inp_unsharp(rgb, ww, fw, 150, 3), R.unsharp(c["rgb"]))
    grey = ops.inp_luma(rgb, 1)
    assert _eq(ops.inp_unsharp(grey, ww, fw, 150, 3), R.unsharp(R.luma(c["rgb"])))
    assert _eq(ops.inp_unsharp(grey, ww, fw, 70, 0), np.asarray(pil.convert("L").filter(ImageFilter.UnsharpMask(0.5, 70, 0))))
    want = np.asarray(pil.convert("L").convert("RGB").filter(ImageFilter.UnsharpMask(radius=0.5, percent=150, threshold=3)))
    assert _eq(inpaint.finish(rgb), want) and _eq(inpaint.finish(rgb), R.finish(c["rgb"]))
    rgba = np.zeros(shape + (4,), np.uint8)
    inside = c["mask_p"] > 128
    rgba[..., :3][inside] = c["rgb"][inside]
    rgba[..., 3][inside] = 255
    assert _eq(ops.inp_rgba_cut(rgb, _dev(c["mask_p"], dev)), rgba)


# ---- the compositions around the stand-in pipe -----------------------------------------------------------------------
CONTROLNET_KEYS = {"prompt", "negative_prompt", "image", "mask_image", "control_image", "guidance_scale",
                   "num_inference_steps", "controlnet_conditioning_scale", "generator"}


def _same_calls(got, want, side):
    """The recorded keyword arguments of two pipes, generator apart."""
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert set(g) == set(w)
        for k in w:
            if k == "generator":
                continue
            if k in ("image", "mask_image"):
                assert g[k].mode == ("RGB" if k == "image" else "L") and g[k].size == (side, side)
                assert np.array_equal(np.asarray(g[k]), np.asarray(w[k])), k
            elif k == "control_image":
                assert g[k].device.type == "cpu" and g[k].dtype == torch.float32 and torch.equal(g[k], w[k])
            else:
                assert type(g[k]) is type(w[k]) and g[k] == w[k], k


def _seeded(gen):
    return isinstance(gen, torch.Generator) and gen.device.type == "cuda" and gen.initial_seed() == 3


@pytest.mark.parametrize("shape", SHAPES)
def test_controlnet_inpaint_equals_the_restatement_chain(dev, shape, registry):
    from PIL import Image
    from InkLayer.inpainting.inpaint_ControlNet import ControlNet_inpaint
    c = case(shape)
    pipe, ref_pipe = StandInPipe(), StandInPipe()
    registry.set_diffusion_pipe(pipe)
    got = ControlNet_inpaint(Image.fromarray(c["rgb"]), Image.fromarray(c["mask"]))
    want = R.controlnet_inpaint(ref_pipe, c["rgb"], c["mask"])
    assert got.mode == "RGB" and got.size == (shape[1], shape[0]) and np.array_equal(np.asarray(got), want)
    assert (want != R.finish(c["rgb"])).mean() > 0.02                   # the pipe's strokes reached the result
    _same_calls(pipe.calls, ref_pipe.calls, 768)
    assert len(pipe.calls) == 2 and all(set(k) == CONTROLNET_KEYS for k in pipe.calls)
    first, second = pipe.calls
    assert first["prompt"] == R.PROMPT and first["negative_prompt"] == R.NEGATIVE
    assert (first["guidance_scale"], first["num_inference_steps"], first["controlnet_conditioning_scale"]) == (9.0, 30, 1.2)
    assert _seeded(first["generator"]) and second["generator"] is first["generator"]
    assert np.array_equal(np.asarray(first["image"]), c["up"]) and np.array_equal(np.asarray(first["mask_image"]), c["mask_up"])
    assert np.array_equal(np.asarray(second["mask_image"]), c["mask_up"])
    assert not np.array_equal(np.asarray(second["image"]), c["up"])     # the second pass starts from the first one's image


def test_controlnet_inpaint_shorter_paths(dev, registry):
    from PIL import Image
    from InkLayer.inpainting.inpaint_ControlNet import ControlNet_inpaint
    c = case(SHAPES[0])
    image, mask = Image.fromarray(c["rgb"]), Image.fromarray(c["mask"])
    outs = {}
    for pre, post in ((False, True), (True, False), (False, False)):
        pipe, ref_pipe = StandInPipe(), StandInPipe()
        registry.set_diffusion_pipe(pipe)
        got = np.asarray(ControlNet_inpaint(image, mask, preprocess_input=pre, postprocess_output=post))
        want = R.controlnet_inpaint(ref_pipe, c["rgb"], c["mask"], preprocess_input=pre, postprocess_output=post)
        assert np.array_equal(got, want), (pre, post)
        _same_calls(pipe.calls, ref_pipe.calls, 768)
        if not pre:                                                     # the raw image and mask went to the resize
            assert np.array_equal(np.asarray(pipe.calls[0]["image"]), R.resize(c["rgb"], 768, 768, "lanczos"))
            assert np.array_equal(np.asarray(pipe.calls[0]["mask_image"]), R.resize(c["mask"], 768, 768, "lanczos"))
        outs[(pre, post)] = got
    assert not np.array_equal(outs[(False, True)], outs[(False, False)])
    assert not np.array_equal(outs[(True, False)], outs[(False, False)])


def test_reference_surface_functions(dev, registry):
    """preprocess_image, preprocess_mask, make_inpaint_condition and postprocess_result with the reference's signatures."""
    from PIL import Image
    from InkLayer.inpainting import inpaint_ControlNet as M
    c = case(SHAPES[1])
    image, mask = Image.fromarray(c["rgb"]), Image.fromarray(c["mask"])
    assert np.array_equal(np.asarray(M.preprocess_image(image)), c["bilateral"])
    assert np.array_equal(np.asarray(M.preprocess_image(image, denoise=False)), c["contrast"])
    pm = M.preprocess_mask(mask)
    assert pm.mode == "L" and np.array_equal(np.asarray(pm), c["mask_p"])
    assert np.array_equal(np.asarray(M.preprocess_mask(mask, dilate_iterations=0, blur_radius=0)), c["mask"])
    cond = M.make_inpaint_condition(image, pm)
    assert cond.device.type == "cpu" and torch.equal(cond, torch.from_numpy(R.condition(c["rgb"], c["mask_p"])))
    post = M.postprocess_result(Image.fromarray(c["bilateral"]), image, mask)
    assert post.mode == "RGB" and np.array_equal(np.asarray(post), R.postprocess(c["bilateral"], c["rgb"], c["mask"]))
    with pytest.raises(ValueError):
        M.preprocess_mask(Image.new("L", (9, 2)))


def test_sdxl_inpaint_equals_the_restatement_chain(dev, registry):
    from PIL import Image
    from InkLayer.inpainting.inpaint_SDXL import SDXL_inpaint
    from inklayer_amd._lib import InkLayerHipError
    c = case(SHAPES[0])
    image, mask = Image.fromarray(c["rgb"]), Image.fromarray(c["mask"])
    pipe, ref_pipe = StandInPipe(), StandInPipe()
    registry.set_diffusion_pipe(pipe)                                   # a ControlNet pipe is not an SDXL pipe
    with pytest.raises(InkLayerHipError, match="sdxl"):
        SDXL_inpaint(image, mask)
    registry.set_diffusion_pipe(pipe, kind="sdxl")
    got = SDXL_inpaint(image, mask)
    want = R.sdxl_inpaint(ref_pipe, c["rgb"], c["mask"])
    assert got.mode == "RGB" and np.array_equal(np.asarray(got), want)
    _same_calls(pipe.calls, ref_pipe.calls, 1024)
    (call,) = pipe.calls
    assert set(call) == {"prompt", "image", "mask_image", "guidance_scale", "num_inference_steps", "strength", "generator"}
    assert (call["prompt"], call["guidance_scale"], call["num_inference_steps"], call["strength"]) == (R.SDXL_PROMPT, 8.0, 20, 0.99)
    assert _seeded(call["generator"])
    assert np.array_equal(np.asarray(registry.resolve_inpaint_func()(image, mask)), want)      # the closure over the pipe


# ---- the entry points ------------------------------------------------------------------------------------------------
def test_single_layer_passes_the_prompt_on(dev, registry, tmp_path):
    from PIL import Image
    from InkLayer.runner import run_inpaint_single_layer
    c = case(SHAPES[0])
    H, W = SHAPES[0]
    base = tmp_path / "static" / "outputs" / "pic"
    (base / "masks_disjoint").mkdir(parents=True)
    out_dir = tmp_path / "out"
    out_dir.mkdir()
    Image.fromarray(c["rgb"]).save(base / "input.png")
    small = np.zeros((H, W), np.uint8)
    small[30:40, 50:70] = 255
    Image.fromarray(small).save(base / "masks_disjoint" / "mask_2.png")
    pipe, ref_pipe = StandInPipe(), StandInPipe()
    registry.set_diffusion_pipe(pipe)
    request = {"image_name": "pic", "layer_path": "layers/layer_2.png", "prompt": "a cat with a hat"}
    path = run_inpaint_single_layer(request, str(tmp_path), str(out_dir))
    assert path == os.path.join(str(out_dir), "layer_2_rgba.png")
    grown = np.asarray(Image.open(out_dir / "mask_expanded_2.png").convert("L"))
    box = np.zeros((H, W), np.uint8)
    box[20:51, 40:81] = 255                                             # the runner's rule: the mask's box grown by 10
    assert np.array_equal(grown, box)
    want, want_rgba = R.single_layer_inpaint(ref_pipe, c["rgb"], grown, "a cat with a hat")
    _same_calls(pipe.calls, ref_pipe.calls, 768)
    (call,) = pipe.calls
    assert set(call) == CONTROLNET_KEYS and call["prompt"] == "a cat with a hat" and call["negative_prompt"] == R.NEGATIVE
    assert (call["guidance_scale"], call["num_inference_steps"], call["controlnet_conditioning_scale"]) == (7.0, 30, 0.6)
    assert _seeded(call["generator"])
    assert np.array_equal(np.asarray(Image.open(out_dir / "inpainted_layer_2.png").convert("RGB")), want)
    layer = Image.open(path)
    assert layer.mode == "RGBA" and np.array_equal(np.asarray(layer), want_rgba)
    alpha = np.asarray(layer)[..., 3]
    assert set(np.unique(alpha).tolist()) == {0, 255} and np.array_equal(alpha > 0, R.mask_prepare(grown) > 128)
    # a registered function keeps its priority, and the prompt is then not passed on (the signature has none)
    seen = []
    registry.set_inpaint_func(lambda input_image, mask_image: seen.append(1) or input_image)
    run_inpaint_single_layer(request, str(tmp_path), str(out_dir))
    assert seen == [1] and len(pipe.calls) == 1


def test_directory_entry_point_runs_through_the_pipe(dev, registry, tmp_path):
    from PIL import Image
    from test_layers_ref_cpu import load_set
    from InkLayer.inpainting.inpaint_ControlNet import run_inpainting_on_sketch_dir
    from InkLayer.utils.io import flush
    S = load_set("fscoco_animals")
    d = tmp_path / "fscoco_animals"
    (d / "masks_final").mkdir(parents=True)
    Image.fromarray(S["input"]).save(d / "input.png")
    for i, m in enumerate(S["masks"]):
        Image.fromarray(m).save(d / "masks_final" / f"mask_{i}.png")
    pipe = StandInPipe()
    registry.set_diffusion_pipe(pipe)
    out = run_inpainting_on_sketch_dir(str(d))
    flush()
    need = [i for i in range(S["n"]) if S["need"][i]]
    assert need and len(pipe.calls) == 2 * len(need)                    # two passes per layer that needs inpainting
    assert all(k["prompt"] == R.PROMPT and k["image"].size == (768, 768) for k in pipe.calls)
    assert sorted(os.listdir(out)) == sorted(f"layer_{i}.png" for i in range(S["n"]))
    i = need[0]
    edit = S["edit"][i].astype(np.uint8) * 255
    want = R.controlnet_inpaint(StandInPipe(), S["sketch"][i], edit)
    proc = d / "complete_layers_process" / f"mask_{i}"
    assert np.array_equal(np.asarray(Image.open(proc / "inpainted_image.png").convert("RGB")), want)
    layer = np.asarray(Image.open(d / "complete_layers" / f"layer_{i}.png").convert("RGB"))
    own = (S["sketch"][i] < 255).any(axis=2)                            # the layer's own strokes are put back
    assert np.array_equal(layer[~own], want[~own]) and np.array_equal(layer[own], S["sketch"][i][own][:, ::-1])
    for j in range(S["n"]):
        if j not in need:
            assert np.array_equal(np.asarray(Image.open(d / "complete_layers" / f"layer_{j}.png").convert("RGB")), S["sketch"][j])
