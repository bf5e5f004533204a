"""Generate tests/golden/depth_models_small.npz by running the REFERENCE's own Depth-Anything-V2 modules for ViT-S and
ViT-L on CPU (build container only), with the same in-memory stubs for `cv2` and `torchvision.transforms` as
tests/golden/make_depth_golden.py (whose ViT-B fixture stays as it is).

Weights: oracle.depth_ref.seeded_state_dict for the model's config, loaded STRICTLY into DepthAnythingV2(encoder, ...)
built from the reference's own depth_model_configs entry - that pins parameter names and shapes; none are stored.
Stored per model: the depth maps of one [2, 3, 126, 154] input (9 x 11 patches: the position-embedding interpolation
path, two different images) and thin slices of the four taps.  The input is stored once, as the f16 numbers it is made of.
"""
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(Path(__file__).resolve().parent))

# name -> (seed, depth_model_configs entry of the reference's depth_sort.py:20-27, DINOv2 dims DA/dinov2.py:339-379,
# intermediate_layer_idx DA/dpt.py:164-169)
MODELS = {
    "vits": (41, dict(features=64, out_channels=[48, 96, 192, 384]), dict(embed_dim=384, depth=12, num_heads=6),
             (2, 5, 8, 11)),
    "vitl": (43, dict(features=256, out_channels=[256, 512, 1024, 1024]), dict(embed_dim=1024, depth=24, num_heads=16),
             (4, 11, 17, 23)),
}


def oracle_config(name):
    from oracle import depth_ref
    _, head, vit, idx = MODELS[name]
    return depth_ref.DepthConfig(features=head["features"], out_channels=tuple(head["out_channels"]), layer_idx=idx, **vit)


def main():
    from make_depth_golden import load_reference
    from oracle import depth_ref
    DepthAnythingV2 = load_reference()
    rs = np.random.RandomState(11)
    x16 = rs.standard_normal((2, 3, 126, 154)).astype(np.float16)
    x = torch.from_numpy(x16.astype(np.float32))
    out = {"x": x16}
    for name, (seed, head, _, idx) in MODELS.items():
        cfg = oracle_config(name)
        sd = depth_ref.seeded_state_dict(cfg, seed)
        torch.manual_seed(0)
        model = DepthAnythingV2(encoder=name, **head).eval()
        print(name, "strict load:", model.load_state_dict(sd, strict=True))
        assert tuple(model.intermediate_layer_idx[name]) == idx
        with torch.no_grad():
            feats = model.pretrained.get_intermediate_layers(x, model.intermediate_layer_idx[name], return_class_token=True)
            depth = model(x)
            mine = depth_ref.forward(sd, cfg, x)
        print(name, "depth", tuple(depth.shape), "oracle-vs-reference max abs diff", (mine - depth).abs().max().item(),
              "depth max", depth.max().item())
        out[f"{name}_seed"] = np.int64(seed)
        out[f"{name}_depth"] = depth.numpy()
        for i, (pt, cls) in enumerate(feats):
            out[f"{name}_feat{i}"] = pt[:, ::7, ::16].numpy()
            out[f"{name}_cls{i}"] = cls.numpy()
    np.savez_compressed(Path(__file__).resolve().parent / "depth_models_small.npz", **out)
    print("wrote depth_models_small.npz")


if __name__ == "__main__":
    main()
