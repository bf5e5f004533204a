"""Segmentor plugin (reference: InkLayer/segmentor/sam.py:16-43), MI355X engine underneath.

`run_SAM(image_pil, boxes_filt, sam_checkpoint=default_ckpt) -> list of HxW bool arrays`."""
import os

import torch

from InkLayer.utils.paths import get_model_path

device = torch.device("cuda" if torch.cuda.is_available() else "cpu")
default_ckpt = get_model_path("sam_vit_h_4b8939.pth")
_engine = None
_engine_model = None    # the model name the cached random-weight engine was built for


def _get_engine(sam_checkpoint):
    global _engine, _engine_model
    from inklayer_amd import sam, weights_init
    if os.environ.get("INKLAYER_RANDOM_WEIGHTS") == "1":
        # INKLAYER_SAM_MODEL picks the random model: vit_h (default), vit_l or vit_b; another name rebuilds the engine
        # (to force a rebuild reset `_engine` to None).  A checkpoint needs no such switch: build_sam reads the model
        # off its tensors.
        name = os.environ.get("INKLAYER_SAM_MODEL", "vit_h")
        if _engine is None or _engine_model != name:
            cfg = sam.config_for(name)                   # ValueError for an unknown name, before anything is built
            _engine = None                               # drop the other model's engine before allocating this one
            _engine = sam.SamEngine(weights_init.random_sam_state_dict(cfg, "cuda"), cfg, "cuda")
            _engine_model = name
        return _engine
    if not os.path.exists(sam_checkpoint):
        raise FileNotFoundError(f"Checkpoint not found at {sam_checkpoint}")   # reference: print + breakpoint()
    return sam.build_sam(sam_checkpoint)


def run_SAM(image_pil, boxes_filt, sam_checkpoint=default_ckpt):
    from inklayer_amd import sam
    if len(boxes_filt) == 0:
        return []                                               # reference returns a 2-tuple of empty arrays
    return sam.run_SAM(image_pil, boxes_filt, engine=_get_engine(sam_checkpoint))
