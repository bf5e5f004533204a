"""Float64 restatement of SAM's point / box / mask prompt encoding and of the four-mask decoder (test helper).

Built on oracle.sam_ref's shared pieces (_pe_encoding, _ln2d, two_way_transformer, _mlp3); pinned to the reference's
own modules by tests/golden/sam_prompts_small.npz (tests/test_sam_prompts_cpu.py)."""
from __future__ import annotations

from typing import Dict, Optional, Tuple

import numpy as np
import torch
import torch.nn.functional as F

from oracle import sam_ref

SD = Dict[str, torch.Tensor]


def to64(sd: SD) -> SD:
    return {k: v.detach().double() for k, v in sd.items()}


def embed_sparse(sd: SD, cfg, points: Optional[torch.Tensor], labels: Optional[torch.Tensor],
                 boxes: Optional[torch.Tensor]) -> torch.Tensor:
    """PromptEncoder._embed_points / _embed_boxes + their concatenation (prompt_encoder.py:73-100, 128-166): points
    [P, N, 2], labels [P, N], boxes [P, 4] in the input frame -> [P, n_sparse, E]."""
    P = (points if points is not None else boxes).shape[0]
    E = cfg.prompt_embed_dim
    parts = [torch.zeros((P, 0, E), dtype=torch.float64)]
    if points is not None:
        pts, lab = points.double() + 0.5, labels.long()
        if boxes is None:                       # pad point (0, 0), label -1, appended after the shift
            pts = torch.cat([pts, torch.zeros((P, 1, 2), dtype=torch.float64)], 1)
            lab = torch.cat([lab, -torch.ones((P, 1), dtype=torch.long)], 1)
        e = sam_ref._pe_encoding(sd, pts / cfg.img_size)
        e[lab == -1] = 0.0
        e[lab == -1] += sd["prompt_encoder.not_a_point_embed.weight"]
        e[lab == 0] += sd["prompt_encoder.point_embeddings.0.weight"]
        e[lab == 1] += sd["prompt_encoder.point_embeddings.1.weight"]
        parts.append(e)
    if boxes is not None:
        c = (boxes.double() + 0.5).reshape(-1, 2, 2) / cfg.img_size
        e = sam_ref._pe_encoding(sd, c)
        e[:, 0] += sd["prompt_encoder.point_embeddings.2.weight"]
        e[:, 1] += sd["prompt_encoder.point_embeddings.3.weight"]
        parts.append(e)
    return torch.cat(parts, 1)


def mask_downscaling(sd: SD, mask: torch.Tensor) -> torch.Tensor:
    """PromptEncoder.mask_downscaling (prompt_encoder.py:50-59): [P, 1, 4g, 4g] -> [P, E, g, g]."""
    p = "prompt_encoder.mask_downscaling."
    x = F.conv2d(mask.double(), sd[p + "0.weight"], sd[p + "0.bias"], stride=2)
    x = F.gelu(sam_ref._ln2d(x, sd[p + "1.weight"], sd[p + "1.bias"]))
    x = F.conv2d(x, sd[p + "3.weight"], sd[p + "3.bias"], stride=2)
    x = F.gelu(sam_ref._ln2d(x, sd[p + "4.weight"], sd[p + "4.bias"]))
    return F.conv2d(x, sd[p + "6.weight"], sd[p + "6.bias"])


def dense_pe(sd: SD, cfg) -> torch.Tensor:
    """get_dense_pe (prompt_encoder.py:62-71, 195-206) in float64: [1, E, g, g]."""
    g = cfg.grid
    ar = (torch.arange(g, dtype=torch.float64) + 0.5) / g
    xy = torch.stack([ar[None, :].expand(g, g), ar[:, None].expand(g, g)], -1)
    return sam_ref._pe_encoding(sd, xy).permute(2, 0, 1).unsqueeze(0)


def decode_all(sd: SD, cfg, emb: torch.Tensor, sparse: torch.Tensor,
               mask: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """MaskDecoder.predict_masks (mask_decoder.py:112-149) with all four mask tokens: emb [P, E, g, g] (the image
    embedding of each prompt), sparse [P, n, E], mask [P, 1, 4g, 4g] or None -> (masks [P, 4, 4g, 4g], iou [P, 4])."""
    P = sparse.shape[0]
    out_tok = torch.cat([sd["mask_decoder.iou_token.weight"], sd["mask_decoder.mask_tokens.weight"]], 0)
    tokens = torch.cat([out_tok.unsqueeze(0).expand(P, -1, -1), sparse], 1)
    dense = (mask_downscaling(sd, mask) if mask is not None
             else sd["prompt_encoder.no_mask_embed.weight"].reshape(1, -1, 1, 1))
    src = emb.double() + dense
    pos = dense_pe(sd, cfg).expand(P, -1, -1, -1)
    b, c, h, w = src.shape
    hs, src2 = sam_ref.two_way_transformer(sd, cfg, src, pos, tokens)
    src2 = src2.transpose(1, 2).reshape(b, c, h, w)
    u = "mask_decoder.output_upscaling."
    x = F.conv_transpose2d(src2, sd[u + "0.weight"], sd[u + "0.bias"], stride=2)
    x = F.gelu(sam_ref._ln2d(x, sd[u + "1.weight"], sd[u + "1.bias"]))
    x = F.gelu(F.conv_transpose2d(x, sd[u + "3.weight"], sd[u + "3.bias"], stride=2))
    hyper = torch.stack([sam_ref._mlp3(sd, f"mask_decoder.output_hypernetworks_mlps.{i}.layers.", hs[:, 1 + i])
                         for i in range(cfg.num_mask_tokens)], 1)
    bb, cc, hh, ww = x.shape
    masks = (hyper @ x.view(bb, cc, hh * ww)).view(bb, -1, hh, ww)
    iou = sam_ref._mlp3(sd, "mask_decoder.iou_prediction_head.layers.", hs[:, 0])
    return masks, iou


def apply_coords(coords: np.ndarray, orig_hw, L: int) -> np.ndarray:
    """ResizeLongestSide.apply_coords (utils/transforms.py:33-45)."""
    nh, nw = sam_ref.preprocess_shape(orig_hw[0], orig_hw[1], L)
    c = np.array(coords, dtype=np.float64)
    c[..., 0] *= nw / orig_hw[1]
    c[..., 1] *= nh / orig_hw[0]
    return c
