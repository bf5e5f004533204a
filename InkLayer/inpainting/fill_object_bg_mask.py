"""Reference surface: InkLayer/inpainting/fill_object_bg_mask.py, computed on the GPU (inklayer_amd/layers.py)."""
import glob
import os

import numpy as np
from PIL import Image


def _planes(mask_binary):
    import torch
    from inklayer_amd import layers
    m = np.asarray(mask_binary)
    return layers.pack_planes((m > 0)[None], "cuda"), m.shape[1]


def fill_enclosed_regions(mask_binary):
    """Fills every interior hole; uint8 0 / 255 in, uint8 0 / 255 out."""
    from inklayer_amd import layers, ops
    planes, W = _planes(mask_binary)
    out, hdr = ops.layers_components(planes, W, "fill_all")
    layers._header(hdr, "fill_all")
    return layers.unpack_planes(out, W)[0].astype(np.uint8) * 255


def fill_holes_not_touching_border(mask_binary, min_area=50):
    """Fills every hole whose contour stays off the image border and has a contour area of at least min_area."""
    from inklayer_amd import layers, ops
    if min_area != 50:
        from inklayer_amd._lib import InkLayerHipError
        raise InkLayerHipError("fill_holes_not_touching_border: the kernel is built for min_area = 50, the only value "
                               "the reference uses")
    planes, W = _planes(mask_binary)
    out, hdr = ops.layers_components(planes, W, "fill_rule")
    out = layers._resolve_undecided(planes, out, W, layers._header(hdr, "fill_rule"))
    return layers.unpack_planes(out, W)[0].astype(np.uint8) * 255


def _read_gray(path):
    """cv2.imread(path, IMREAD_GRAYSCALE): an 8-bit grey file as it is, a colour file through ink_layers_gray."""
    import torch
    from inklayer_amd import ops
    im = Image.open(path)
    if im.mode in ("L", "1"):
        return torch.from_numpy(np.array(im.convert("L"), np.uint8)).to("cuda")[None]
    rgb = torch.from_numpy(np.array(im.convert("RGB"), np.uint8)).to("cuda")
    return ops.layers_gray(rgb[None])


def _type_string(branch, shrink_by):
    return branch if branch == "open-curve" else f"closed-silhouette (shrunk by {shrink_by}px)"


def _get_mask_arrays(input_path, **params):
    from inklayer_amd import layers
    gray = _read_gray(input_path)
    planes, branch, shrink = layers.background_masks(gray, params)
    return layers.unpack_planes(planes, int(gray.shape[2]))[0], _type_string(branch[0], shrink[0])


def get_mask(input_path, output_path, mask_color=(255, 0, 0), dilate_iter=5, kernel_size=3, safety_margin=0,
             stroke_thick=1, border_band=2):
    """A filled silhouette when the drawing is closed, the thickened strokes when it touches the image border.
    Writes the coloured mask (mask_color is B, G, R as in the reference) and returns (array, mask type)."""
    from InkLayer.utils.io import save_all
    mask, mask_type = _get_mask_arrays(input_path, dilate_iter=dilate_iter, kernel_size=kernel_size,
                                       safety_margin=safety_margin, stroke_thick=stroke_thick, border_band=border_band)
    coloured = np.zeros(mask.shape + (3,), np.uint8)
    coloured[mask] = mask_color
    save_all([(np.ascontiguousarray(coloured[..., ::-1]), output_path)], wait=True)
    return coloured, mask_type


def _rgba_batch(paths, **mask_params):
    import torch
    from inklayer_amd import layers, ops
    rgb = np.stack([np.asarray(Image.open(p).convert("RGB")) for p in paths])
    gray = ops.layers_gray(torch.from_numpy(np.ascontiguousarray(rgb)).to("cuda"))
    bg, branch, shrink = layers.background_masks(gray, mask_params)
    rgba = ops.layers_rgba(gray, bg).cpu().numpy()
    return rgba, [_type_string(b, s) for b, s in zip(branch, shrink)]


def create_rgba_with_background_mask(input_path, output_path, **mask_params):
    """Sketch pixels keep their grey, the background mask becomes white, everything else is transparent."""
    from InkLayer.utils.io import save_all
    rgba, types = _rgba_batch([input_path], **mask_params)
    if not output_path.lower().endswith(".png"):
        output_path = os.path.splitext(output_path)[0] + ".png"
    save_all([(rgba[0], output_path)], wait=True)
    return rgba[0], types[0]


def rgba_layers_to_dir(layer_pixels, output_dir):
    """The runner's hand-off: the pixels of complete_layers/layer_i.png still in memory (uint8 [n, H, W, 3]) ->
    output_dir/layer_i.png, without reading the files back."""
    import torch
    from inklayer_amd import layers
    from InkLayer.utils.io import save_all
    os.makedirs(output_dir, exist_ok=True)
    if len(layer_pixels):
        rgba = layers.rgba_layers(torch.from_numpy(np.ascontiguousarray(layer_pixels)).to("cuda"))[0].cpu().numpy()
        save_all([(rgba[i], os.path.join(output_dir, f"layer_{i}.png")) for i in range(len(rgba))], wait=None)
    print(f"Saved RGBA images to {output_dir}")
    return output_dir


def create_rgba_with_background_mask_on_dir(input_dir, output_dir):
    """RGBA versions of all PNGs of input_dir, computed in one batch per image size."""
    from InkLayer.utils.io import save_all
    os.makedirs(output_dir, exist_ok=True)
    input_images = sorted(glob.glob(os.path.join(input_dir, "*.png")))
    if not os.path.exists(os.path.join(input_dir, "../input.png")):
        raise ValueError(f"Original sketch image not found at {os.path.join(input_dir, '../input.png')}")
    by_size = {}
    for p in input_images:
        by_size.setdefault(Image.open(p).size, []).append(p)
    jobs = []
    for paths in by_size.values():
        rgba, _ = _rgba_batch(paths)
        jobs += [(rgba[k], os.path.join(output_dir, os.path.basename(p))) for k, p in enumerate(paths)]
    save_all(jobs, wait=None)
    print(f"Saved RGBA images to {output_dir}")
    return output_dir
