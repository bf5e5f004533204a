"""The plugin surface of the layer-assembly stage: every function of the reference's InkLayer/inpainting modules this
build provides exists with the reference's parameter names, and the entry points that need the diffusion model say so
when none is registered.  No GPU."""
import inspect

import pytest

SURFACE = {
    "InkLayer.inpainting.util": {
        "assemble_inpaint_input_at_index": ["masks_dir", "mask_index"],
        "composite_original_sketch_onto_inpainted": ["inpainted_image", "original_sketch_image", "original_sketch_mask"],
        "mask_within_bbox": ["mask", "bbox"],
        "mask_transparent_region": ["img_rgb", "mask"],
        "combine_masks": ["masks"],
        "mask_to_bbox": ["mask"],
        "create_background_mask_from_sketch": ["sketch_image_path", "mask_params"],
        "create_red_masked_region": ["base_mask", "overlay_mask"],
        "run_inpainting_on_sketch_dir_template": ["inpaint_func"],
    },
    "InkLayer.inpainting.fill_object_bg_mask": {
        "fill_enclosed_regions": ["mask_binary"],
        "fill_holes_not_touching_border": ["mask_binary", "min_area"],
        "get_mask": ["input_path", "output_path", "mask_color", "dilate_iter", "kernel_size", "safety_margin",
                     "stroke_thick", "border_band"],
        "create_rgba_with_background_mask": ["input_path", "output_path", "mask_params"],
        "create_rgba_with_background_mask_on_dir": ["input_dir", "output_dir"],
    },
    "InkLayer.inpainting.inpaint_ControlNet": {"run_inpainting_on_sketch_dir": ["sketch_dir"]},
    "InkLayer.inpainting.inpaint_single_layer": {
        "inpaint_single_layer": ["image_path", "mask_path", "output_dir", "prompt", "layer_id", "position_data"]},
}
CASES = [(m, f) for m, fs in SURFACE.items() for f in fs]


@pytest.mark.parametrize("module,func", CASES)
def test_reference_function_exists_with_its_parameters(module, func):
    import importlib
    fn = getattr(importlib.import_module(module), func)
    assert list(inspect.signature(fn).parameters) == SURFACE[module][func]


def test_get_mask_defaults_are_the_reference_ones():
    from InkLayer.inpainting.fill_object_bg_mask import fill_holes_not_touching_border, get_mask
    d = {k: v.default for k, v in inspect.signature(get_mask).parameters.items() if v.default is not inspect.Parameter.empty}
    assert d == dict(mask_color=(255, 0, 0), dilate_iter=5, kernel_size=3, safety_margin=0, stroke_thick=1, border_band=2)
    assert inspect.signature(fill_holes_not_touching_border).parameters["min_area"].default == 50


@pytest.fixture
def unregistered():
    import InkLayer.inpainting as reg
    old = reg.get_inpaint_func()
    reg.set_inpaint_func(None)
    yield reg
    reg.set_inpaint_func(old)


def test_unregistered_function_errors_name_the_call(unregistered, tmp_path):
    from inklayer_amd._lib import InkLayerHipError
    from InkLayer.inpainting.inpaint_ControlNet import run_inpainting_on_sketch_dir
    from InkLayer.inpainting.inpaint_single_layer import inpaint_single_layer
    with pytest.raises(InkLayerHipError, match=r"run_inpainting_on_sketch_dir.*set_inpaint_func"):
        run_inpainting_on_sketch_dir(str(tmp_path))
    with pytest.raises(InkLayerHipError, match=r"inpaint_single_layer.*set_inpaint_func"):
        inpaint_single_layer("a.png", "b.png", str(tmp_path), "a prompt", "1")
    assert not list(tmp_path.iterdir())                      # nothing was written before the error


def test_single_layer_runner_keeps_its_error_without_a_function(unregistered, tmp_path):
    from InkLayer.runner import run_inpaint_single_layer
    with pytest.raises(NotImplementedError):
        run_inpaint_single_layer({"image_name": "x", "layer_path": "layer_1.png", "prompt": "p"}, str(tmp_path), str(tmp_path))


def test_registration_takes_callables_only(unregistered):
    fn = lambda input_image, mask_image: input_image
    unregistered.set_inpaint_func(fn)
    assert unregistered.get_inpaint_func() is fn and unregistered.require_inpaint_func("x") is fn
    with pytest.raises(TypeError):
        unregistered.set_inpaint_func(3)


def test_array_helpers_keep_the_reference_rules():
    import numpy as np
    from InkLayer.inpainting import util
    m = np.zeros((8, 9), np.uint8)
    m[2:5, 3:7] = 255
    assert [int(v) for v in util.mask_to_bbox(m)] == [3, 2, 6, 4]                      # inclusive maxima
    inside = util.mask_within_bbox(m > 0, util.mask_to_bbox(m))
    assert inside[2:4, 3:6].all() and inside.sum() == 6                                # last row and column drop out
    assert util.combine_masks([m > 0, np.eye(8, 9, dtype=bool)])[0, 0]
    with pytest.raises(ValueError):
        util.combine_masks([])
    assert util.mask_transparent_region(np.zeros((8, 9, 3), np.uint8), m > 0)[3, 4, 3] == 0
    assert util.create_red_masked_region(m, np.eye(8, 9, dtype=bool))[0, 0].tolist() == [0, 0, 255]


def test_layer_entry_points_reject_bad_arguments_without_launch():
    """Every ink_layers_* entry point returns 1 before any HIP call for null pointers and sizes it has no kernel for."""
    import ctypes
    from inklayer_amd import _lib
    l = _lib.lib()
    p = 256
    assert l.ink_layers_otsu_planes(None, 1, 8, 8, 1, p, p, p, None) == 1
    assert l.ink_layers_otsu_planes(p, 255, 8, 8, 1, p, p, p, None) == 1            # more planes than a label image holds
    assert l.ink_layers_otsu_planes(p, 1, 8, 16384, 1, p, p, p, None) == 1          # run coordinates are 14-bit
    assert l.ink_layers_dilate(p, 1, 8, 8, 4, 1, 512, 768, None) == 1               # 3x3 and 5x5 ellipses only
    assert l.ink_layers_dilate(p, 1, 8, 8, 5, 0, 512, 768, None) == 1
    assert l.ink_layers_dilate(p, 1, 8, 8, 5, 1, p, 768, None) == 1                 # in place
    assert l.ink_layers_border_band(p, 1, 8, 8, 0, p, None) == 1
    assert l.ink_layers_components(p, 1, 8, 8, 4, 512, 768, 1024, None) == 1        # modes 0..3
    assert l.ink_layers_components(p, 1, 8, 8, 1, 512, 768, p, None) == 1           # in place
    assert l.ink_layers_chamfer(p, p, 1, 8, 8, -1, 0, p, p, p, p, p, None) == 1
    assert l.ink_layers_chamfer(p, None, 1, 8, 8, 0, 0, p, p, p, p, p, None) == 1
    assert l.ink_layers_mask_tables(p, 0, 8, 8, p, p, None) == 1
    assert l.ink_layers_assemble(p, p, p, p, p, 1, 8, 8, p, p, None, None) == 1
    assert l.ink_layers_composite(p, p, 0, 8, p, None) == 1
    assert l.ink_layers_gray(p, 1, 8, 8, None, None) == 1
    assert l.ink_layers_rgba(p, None, 1, 8, 8, p, None) == 1
    need = ctypes.c_int64(0)
    assert l.ink_layers_components_workspace_ints(2, 70, 130, ctypes.byref(need)) == 0
    rm = 130 // 2 + 1
    assert need.value == 2048 + 2 * (70 + 7 * 70 * rm + 70 * rm)
    assert l.ink_layers_chamfer_workspace_ints(2, 70, 130, ctypes.byref(need)) == 0 and need.value == 2 * (2 * 18 + 1)
    assert l.ink_layers_chamfer_workspace_ints(2, 0, 130, ctypes.byref(need)) == 1
