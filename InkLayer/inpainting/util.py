"""Reference surface: InkLayer/inpainting/util.py.  The path-based functions read the PNGs and run the GPU path
(inklayer_amd/layers.py); the small array helpers are the reference's numpy arithmetic."""
import glob
import os
import shutil

import numpy as np
from PIL import Image


def _gray(path):
    return np.asarray(Image.open(path).convert("L"))


def _load_masks(masks_dir):
    n = len(glob.glob(f"{masks_dir}/mask_*"))
    return np.stack([_gray(f"{masks_dir}/mask_{i}.png") for i in range(n)]) if n else np.zeros((0, 0, 0), np.uint8)


def _assemble_all(sketch_rgb, masks_u8):
    """All layers of a sketch in one GPU pass -> list of (edit_mask, rgb_image, debug_vis, need_inpaint,
    original_sketch_mask) as assemble_inpaint_input_at_index returns them (host arrays)."""
    import torch
    from inklayer_amd import layers
    masks_dev = torch.from_numpy(np.ascontiguousarray(masks_u8)).to("cuda")
    out = []
    for i, l in enumerate(layers.assemble_layers(sketch_rgb, masks_dev)):
        layer = l.sketch_layer.cpu().numpy()
        mask = masks_u8[i].astype(bool)
        if i == 0:
            out.append((None, layer, None, False, None))
        elif l.edit_mask is None:
            out.append((mask, layer, mask, False, None))
        else:
            out.append((l.edit_mask.cpu().numpy() > 0, layer, l.debug_vis.cpu().numpy(), True, (layer < 255).any(axis=2)))
    return out


def assemble_inpaint_input_at_index(masks_dir, mask_index):
    sketch = np.asarray(Image.open(f"{masks_dir}/../input.png").convert("RGB"))
    masks = _load_masks(masks_dir)
    return _assemble_all(sketch, masks[:mask_index + 1])[mask_index]


def composite_original_sketch_onto_inpainted(inpainted_image, original_sketch_image, original_sketch_mask):
    """inpainted_image: PIL (R, G, B); original_sketch_image: array in (B, G, R); -> PIL image."""
    final_image = np.array(inpainted_image).copy()
    original_sketch_rgb = np.asarray(original_sketch_image)[..., ::-1]
    final_image[original_sketch_mask] = original_sketch_rgb[original_sketch_mask]
    return Image.fromarray(final_image)


def mask_within_bbox(mask, bbox):
    x1, y1, x2, y2 = bbox
    modified_mask = mask.copy()
    modified_mask[:y1, :] = False
    modified_mask[y2:, :] = False
    modified_mask[:, :x1] = False
    modified_mask[:, x2:] = False
    return modified_mask


def mask_transparent_region(img_rgb, mask):
    alpha = (~mask).astype(np.uint8) * 255
    return np.dstack((img_rgb, alpha))


def combine_masks(masks):
    if not masks:
        raise ValueError("Empty list of masks provided")
    height, width = masks[0].shape
    combined_mask = np.zeros((height, width), dtype=bool)
    for mask in masks:
        if mask.shape != (height, width):
            raise ValueError(f"Mask shape mismatch. Expected {(height, width)}, got {mask.shape}")
        combined_mask |= mask
    return combined_mask


def mask_to_bbox(mask):
    indices = np.where(np.asarray(mask) > 127)
    x1, x2 = np.min(indices[1]), np.max(indices[1])
    y1, y2 = np.min(indices[0]), np.max(indices[0])
    return [x1, y1, x2, y2]


def create_background_mask_from_sketch(sketch_image_path, **mask_params):
    """-> (bool background mask, mask type string) of the sketch image at the path, computed on the GPU."""
    from InkLayer.inpainting.fill_object_bg_mask import _get_mask_arrays
    mask, mask_type = _get_mask_arrays(sketch_image_path, **mask_params)
    return mask, mask_type


def create_red_masked_region(base_mask, overlay_mask):
    height, width = base_mask.shape
    rgb_image = np.zeros((height, width, 3), dtype=np.uint8)
    rgb_image[base_mask > 0] = [255, 255, 255]
    rgb_image[overlay_mask > 0] = [0, 0, 255]
    return rgb_image


def write_layers(sketch_dir, sketch_rgb, masks_u8, inpaint_func):
    """complete_layers/ and complete_layers_process/ of one sketch from masks held in memory (uint8 [n, H, W]); the PNGs
    go through InkLayer.utils.io.save_all.  -> (layers_out_dir, the pixels of every layer_i.png as uint8 [n, H, W, 3])."""
    import torch
    from inklayer_amd import layers
    from InkLayer.utils.io import save_all
    layers_out_dir = f"{sketch_dir}/complete_layers"
    debug_out_dir = f"{sketch_dir}/complete_layers_process"
    for d in (layers_out_dir, debug_out_dir):
        shutil.rmtree(d, ignore_errors=True)
        os.makedirs(d, exist_ok=True)
    jobs, layer_pixels = [], []
    if len(masks_u8):
        masks_dev = masks_u8 if torch.is_tensor(masks_u8) else torch.from_numpy(np.ascontiguousarray(masks_u8)).to("cuda")
        assembled = layers.assemble_layers(sketch_rgb, masks_dev)
    else:
        assembled = []
    for i, l in enumerate(assembled):
        print(f"Processing mask {i}")
        cur = f"{debug_out_dir}/mask_{i}"
        os.makedirs(cur, exist_ok=True)
        sketch_layer = l.sketch_layer.cpu().numpy()
        jobs.append((sketch_layer, f"{cur}/sketch_layer.png"))
        final = sketch_layer
        if l.debug_vis is not None:
            vis = l.debug_vis.cpu().numpy()
            jobs.append((vis > 0 if vis.ndim == 2 else vis, f"{cur}/debug_vis.png"))
        if l.edit_mask is not None:
            print(f"Processing overlaps for mask {i}: {l.overlaps}")
            edit = l.edit_mask.cpu().numpy()
            jobs.append((edit, f"{cur}/edit_mask.png"))
            inpainted = inpaint_func(input_image=Image.fromarray(sketch_layer), mask_image=Image.fromarray(edit))
            inpainted_rgb = np.ascontiguousarray(np.asarray(inpainted.convert("RGB")))
            if inpainted_rgb.shape != sketch_layer.shape:
                raise ValueError(f"the inpainting function returned {inpainted_rgb.shape[:2]} pixels for a layer of "
                                 f"{sketch_layer.shape[:2]}")
            final = layers.composite(inpainted_rgb, l.sketch_layer).cpu().numpy()
            jobs.append((inpainted_rgb, f"{cur}/inpainted_image.png"))
            jobs.append((final, f"{cur}/final_composited.png"))
        jobs.append((final, f"{layers_out_dir}/layer_{i}.png"))
        layer_pixels.append(final)
    save_all(jobs, wait=None)
    return layers_out_dir, (np.stack(layer_pixels) if layer_pixels else np.zeros((0, 0, 0, 3), np.uint8))


def run_inpainting_on_sketch_dir_template(inpaint_func):

    def wrapper(sketch_dir):
        masks_dir = f"{sketch_dir}/masks_final"
        if not os.path.exists(masks_dir):
            print(f"Directory {masks_dir} does not exist. Please run the segmentation step first.")
            exit(1)
        sketch = np.asarray(Image.open(f"{sketch_dir}/input.png").convert("RGB"))
        return write_layers(sketch_dir, sketch, _load_masks(masks_dir), inpaint_func)[0]

    return wrapper
