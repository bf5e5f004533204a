"""Generate tests/golden/gdino_swinb_small.npz by running the REFERENCE's own Swin-B/384 backbone
(build_swin_transformer("swin_B_384_22k", 384, ...): embed 128, depths (2, 2, 18, 2), heads (4, 8, 16, 32), window 12)
on the CPU at its true depths, on one seeded 100 x 148 image (stage grids of 3x4, 2x2, 1x1, 1x1 windows: stages 2 and 3
are a single, mostly padded window).  Build container only; the stubs and the loader are make_gdino_golden.py's.

Stored: the seeds, the image size and subsampled feature maps - no weights (they come back from
oracle.sam_ref.seeded_state_dict over oracle.gdino_ref.gdino_param_shapes, backbone keys only).
"""
from pathlib import Path

import numpy as np
import torch

import make_gdino_golden as base       # installs the stubs, imports the reference's modules
from oracle import gdino_ref, sam_ref

SWINB = gdino_ref.GDinoConfig(embed_dim=128, depths=(2, 2, 18, 2), num_heads=(4, 8, 16, 32), window_size=12)
SEED, IMAGE_SEED, HW = 8642, 11, (100, 148)


def backbone_weights(seed):
    shapes = {k: s for k, s in gdino_ref.gdino_param_shapes(SWINB).items() if k.startswith("backbone.0.")}
    return sam_ref.seeded_state_dict(shapes, seed)


def image(seed, hw):
    rs = np.random.RandomState(seed)
    return torch.from_numpy(rs.standard_normal((1, 3, hw[0], hw[1])).astype(np.float32))


@torch.no_grad()
def main():
    sd = backbone_weights(SEED)
    swin = base.build_swin_transformer("swin_B_384_22k", 384, out_indices=(1, 2, 3), dilation=False, use_checkpoint=False)
    swin.eval()
    base.load_prefixed(swin, sd, "backbone.0.")
    img = image(IMAGE_SEED, HW)
    feats = swin(base.NestedTensor(img, torch.zeros((1,) + HW, dtype=torch.bool)))
    f = [feats[i].tensors[0] for i in range(3)]
    out = dict(seed=np.int64(SEED), image_seed=np.int64(IMAGE_SEED), hw=np.array(HW),
               feat1=f[0][::8].numpy(), feat2=f[1][::8].numpy(), feat3=f[2][::16].numpy())
    path = Path(__file__).with_name("gdino_swinb_small.npz")
    np.savez_compressed(path, **out)
    print(path, path.stat().st_size, {k: v.shape for k, v in out.items()})


if __name__ == "__main__":
    main()
