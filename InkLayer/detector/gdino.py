"""Detector plugin (reference: InkLayer/detector/gdino.py:12-30), MI355X engine underneath.

`run_ft_dino_on_sketch(path) -> {"bboxes": normalised xyxy lists, "scores": [...], "labels": [...]}`
with caption "object", box_threshold 0.2, text_threshold 0 exactly as the reference.  The model is a
module-level singleton like the reference's `model`, but created on first use and kept resident in
HBM (the reference re-`.to(device)`s it every call, GD/util/inference.py:64)."""
import os
import re

import numpy as np
from PIL import Image

from InkLayer.utils.paths import get_model_path
from InkLayer.utils.processing import cxcywh_to_xyxy

gdino_config_path = get_model_path("GroundingDINO_SwinT_OGC.py")
weights_path = get_model_path("inklayer_gdino.pth")
model = None


def backbone_of_config(config_path):
    """The `backbone = "..."` name of a GroundingDINO config file (GroundingDINO_SwinT_OGC.py / GroundingDINO_SwinB_cfg.py),
    read as TEXT - the file is never executed.  None when there is no such file or no such line."""
    if not config_path or not os.path.isfile(config_path):
        return None
    with open(config_path, "r", encoding="utf-8", errors="replace") as f:
        m = re.search(r"""^\s*backbone\s*=\s*["']([A-Za-z0-9_]+)["']""", f.read(), flags=re.M)
    return m.group(1) if m else None


def random_weights_model():
    """The registry name INKLAYER_GDINO_MODEL picks for INKLAYER_RANDOM_WEIGHTS=1 (default swin_t); ValueError for a
    name the registry does not have, before anything is built."""
    from inklayer_amd import gdino
    name = os.environ.get("INKLAYER_GDINO_MODEL", "swin_t")
    gdino.config_for(name)
    return name


def load_model(config_path=None, checkpoint_path=None, device="cuda"):
    """groundingdino.util.inference.load_model (GD/util/inference.py:29-36) for the HIP engine.  The defaults are the
    module attributes `gdino_config_path` / `weights_path`, read at CALL time.  The model (Swin-T or Swin-B, window 7 or
    12, layer counts) is read off the checkpoint's tensor shapes; a config file, where one exists, is only cross-checked:
    its backbone name must be the checkpoint's (ValueError otherwise)."""
    import torch
    checkpoint_path = weights_path if checkpoint_path is None else checkpoint_path
    config_path = gdino_config_path if config_path is None else config_path
    from inklayer_amd import gdino, text_branch, weights_init
    if os.environ.get("INKLAYER_RANDOM_WEIGHTS") == "1":      # no checkpoints exist offline
        cfg = gdino.config_for(random_weights_model())
        sd = weights_init.random_gdino_state_dict(cfg, device)
        text = weights_init.random_text_features(cfg, device)
    else:
        if not os.path.exists(checkpoint_path):
            raise FileNotFoundError(f"Checkpoint not found at {checkpoint_path}")
        ckpt = torch.load(checkpoint_path, map_location="cpu", weights_only=True)
        sd = gdino.clean_state_dict(ckpt["model"] if "model" in ckpt else ckpt)   # GD/util/inference.py:33-34
        cfg = gdino.config_from_state_dict(sd)
        named, held = backbone_of_config(config_path), gdino.model_name(cfg)
        if named is not None and named != held:
            raise ValueError(f"{config_path} names backbone {named!r}, but {checkpoint_path} holds "
                             f"{held or 'a Swin backbone outside the registry'} (embed dim {cfg.embed_dim}, depths "
                             f"{cfg.depths}, heads {cfg.num_heads}, window {cfg.window_size}): use the config that "
                             f"belongs to the checkpoint")
        text = text_branch.encode_caption_from_checkpoint(sd, gdino.DEFAULT_TOKEN_IDS)
    return gdino.GDinoEngine(sd, cfg, device, encoded_text=text)


def get_model():
    global model
    if model is None:
        model = load_model()
    return model


def run_ft_dino_on_sketch(sketch_path):
    import torch
    from inklayer_amd import gdino
    eng = get_model()
    image_source = np.asarray(Image.open(sketch_path).convert("RGB"))
    from inklayer_amd import ops
    raw = torch.from_numpy(np.ascontiguousarray(image_source)).to(eng.dev)
    oh, ow = gdino.resize_shape(image_source.shape[1], image_source.shape[0])   # load_image's RandomResize([800], 1333)
    boxes, scores = eng.detect([ops.resize_bilinear_u8(raw, oh, ow)])[0]
    normalized = cxcywh_to_xyxy(boxes.tolist()).tolist()        # cxcywh -> xyxy in float64
    return {"bboxes": normalized, "scores": scores.tolist(), "labels": ["object"] * len(normalized)}
