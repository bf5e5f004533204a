"""SAM ViT-H segmentor on MI355X: host-side composition of the HIP kernels.

Mirrors the reference surfaces for this path
  * segment_anything.build_sam / SamPredictor  (SA/build_sam.py:55-107, SA/predictor.py:17-243)
  * InkLayer.segmentor.sam.run_SAM              (InkLayer/segmentor/sam.py:16-43)
with the same state_dict key names, so `sam_vit_h_4b8939.pth` drops in unchanged; so do `sam_vit_l_0b3195.pth` and
`sam_vit_b_01ec64.pth` (SAM_CONFIGS / sam_model_registry: the encoder's shape is read off the checkpoint; head width 64
runs the templated attention of csrc/attention.hip with f32 rel-pos tables, ViT-H its dedicated kernels).

Design (MI355X-first, not a translation of the nn.Module tree):
  * tokens live as ONE f32 residual stream [B*4096, 1280]; every GEMM input is produced in
    f16 by the kernel that precedes it (LayerNorm, GELU epilogue, attention), every GEMM
    accumulates in f32 and applies bias / GELU / residual / window-unpartition in its epilogue;
  * window partition + zero padding is a row-gather fused into LayerNorm; un-partition + crop
    is a row-scatter fused into the proj GEMM epilogue (same int32 map for both);
  * attention never materialises scores; the decomposed rel-pos bias rides inside the MFMA
    accumulator (attention.hip);
  * ConvTranspose2d k2s2 = a [C -> 4*C'] projection whose pixel shuffle is deferred to the
    final mask-logit kernel; the two bilinear resizes + threshold are one kernel;
  * precision: the 32 ViT-H blocks run on plain f16 operands; the patch embedding, the neck, the
    prompt / mask decoder, the upscaler and the hyper-network - 1 % of the FLOPs, but the layers whose f16 rounding
    dominated the mask error - run on SPLIT-f16 operands (hi + lo, three MFMA products per term, fp32-grade) with f32
    activations and f32-I/O attention, because the reference thresholds fp32 logits at exactly 0.
No torch compute ops are used on the hot path — torch supplies memory, streams, copies.
"""
from __future__ import annotations

import math
from dataclasses import dataclass, replace
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import ops
from ._lru import LRU

F16, F32 = torch.float16, torch.float32


@dataclass
class SamConfig:
    """SA/build_sam.py:14-21,55-101 (defaults = ViT-H, the model InkLayer ships)."""
    embed_dim: int = 1280
    depth: int = 32
    num_heads: int = 16
    global_attn_indexes: Tuple[int, ...] = (7, 15, 23, 31)
    window_size: int = 14
    img_size: int = 1024
    patch_size: int = 16
    mlp_ratio: float = 4.0
    prompt_embed_dim: int = 256
    dec_depth: int = 2
    dec_heads: int = 8
    dec_mlp_dim: int = 2048
    num_mask_tokens: int = 4
    pixel_mean: Tuple[float, ...] = (123.675, 116.28, 103.53)
    pixel_std: Tuple[float, ...] = (58.395, 57.12, 57.375)
    mask_threshold: float = 0.0

    @property
    def grid(self) -> int:
        return self.img_size // self.patch_size

    @property
    def head_dim(self) -> int:
        return self.embed_dim // self.num_heads


# The three encoders of sam_model_registry (SA/build_sam.py:14-52); prompt encoder and mask decoder are the same for all.
SAM_CONFIGS: Dict[str, SamConfig] = {
    "vit_h": SamConfig(embed_dim=1280, depth=32, num_heads=16, global_attn_indexes=(7, 15, 23, 31)),
    "vit_l": SamConfig(embed_dim=1024, depth=24, num_heads=16, global_attn_indexes=(5, 11, 17, 23)),
    "vit_b": SamConfig(embed_dim=768, depth=12, num_heads=12, global_attn_indexes=(2, 5, 8, 11)),
}
HEAD_DIMS = (64, 80)     # head widths the rel-pos attention kernels serve (csrc/attention*.hip)


def config_for(name: str) -> SamConfig:
    """The registry entry of `name` (a copy); "default" is ViT-H as in the reference.  ValueError for an unknown name."""
    key = "vit_h" if name == "default" else name
    if key not in SAM_CONFIGS:
        raise ValueError(f"unknown SAM model {name!r}: one of {sorted(SAM_CONFIGS)}")
    return replace(SAM_CONFIGS[key])


def model_name(cfg: SamConfig) -> Optional[str]:
    """The registry name of a configuration, None when it is none of the three."""
    return next((n for n, c in SAM_CONFIGS.items() if c == cfg), None)


def config_from_state_dict(sd) -> SamConfig:
    """The encoder a SAM state dict holds, from its tensor shapes alone (values: tensors on any device, "meta"
    included, or shape tuples): embed dim and grid from image_encoder.pos_embed, depth from the block count, head dim
    from blocks.0.attn.rel_pos_h, the global blocks are those whose rel_pos_h has 2 * grid - 1 rows, window size from a
    windowed block's table, patch size from patch_embed.proj.weight, mlp_ratio from blocks.0.mlp.lin1.weight.
    ValueError, naming what was found, when that is not a model the kernels serve: head dim in {64, 80}, a 64 x 64 grid,
    14 x 14 windows."""
    def shape(k):
        if k not in sd:
            raise ValueError(f"not a SAM state dict: {k} is missing")
        v = sd[k]
        return tuple(int(d) for d in (v.shape if hasattr(v, "shape") else v))

    pre = "image_encoder.blocks."
    pos = shape("image_encoder.pos_embed")
    if len(pos) != 4 or pos[0] != 1 or pos[1] != pos[2]:
        raise ValueError(f"not a SAM state dict: image_encoder.pos_embed has shape {pos}")
    g, D = pos[1], pos[3]
    blocks = {int(k[len(pre):].split(".", 1)[0]) for k in sd if k.startswith(pre)}
    depth = len(blocks)
    if depth == 0 or blocks != set(range(depth)):
        raise ValueError(f"not a SAM state dict: image encoder blocks {sorted(blocks)}")
    rows = [shape(f"{pre}{i}.attn.rel_pos_h") for i in range(depth)]
    hd = rows[0][1]
    glob = tuple(i for i, r in enumerate(rows) if r[0] == 2 * g - 1)
    wins = sorted({(r[0] + 1) // 2 for i, r in enumerate(rows) if i not in glob})
    patch = shape("image_encoder.patch_embed.proj.weight")[-1]
    hidden = shape(f"{pre}0.mlp.lin1.weight")[0]
    found = (f"embed dim {D}, {depth} blocks, head dim {hd}, a {g} x {g} grid, global blocks {glob}, "
             f"window sizes {wins}, patch size {patch}")
    if any(r[1] != hd for r in rows) or hd <= 0 or D % hd or len(wins) > 1:
        raise ValueError(f"inconsistent SAM image encoder: {found}")
    if hd not in HEAD_DIMS or g != 64 or (wins and wins[0] != 14):
        raise ValueError(f"no kernels for this SAM image encoder ({found}): the attention kernels serve head dim "
                         f"{' or '.join(map(str, HEAD_DIMS))}, a 64 x 64 grid and 14 x 14 windows")
    return SamConfig(embed_dim=D, depth=depth, num_heads=D // hd, global_attn_indexes=glob,
                     window_size=wins[0] if wins else 14, img_size=g * patch, patch_size=patch, mlp_ratio=hidden / D)


def preprocess_shape(h: int, w: int, L: int) -> Tuple[int, int]:
    """ResizeLongestSide.get_preprocess_shape (SA/utils/transforms.py:93-102)."""
    sc = L * 1.0 / max(h, w)
    return int(h * sc + 0.5), int(w * sc + 0.5)


def resize_longest_side(img: np.ndarray, L: int) -> np.ndarray:
    """ResizeLongestSide.apply_image (SA/utils/transforms.py:26-31) with PIL on the host.  Not on the product
    path any more (ops.resize_bilinear_u8 is bit-identical on the GPU); kept as the reference the tests compare to."""
    from PIL import Image
    nh, nw = preprocess_shape(img.shape[0], img.shape[1], L)
    if (nh, nw) == img.shape[:2]:
        return np.ascontiguousarray(img)
    return np.asarray(Image.fromarray(img).resize((nw, nh), Image.BILINEAR))


MAX_TOKENS = 16      # decoder tokens per prompt: 5 output tokens + points (+ pad) + box corners (ink_attn_fewq / _fewkeys)


def _hyp(m: int) -> str:
    """Weight-key prefix of mask token m's hyper-network MLP ('hyp' for token 0, as before multimask output)."""
    return "hyp" if m == 0 else f"m{m}hyp"


def check_prompts(point_coords=None, point_labels=None, boxes=None, mask_input=None,
                  mask_side: int = 256) -> Tuple[int, int]:
    """Validate the batched prompts of SamPredictor.predict_torch (SA/predictor.py:160-243) before anything is launched:
    point_coords [P, N, 2] float with point_labels [P, N] (integer values), boxes [P, 4] float, mask_input
    [P, 1, mask_side, mask_side] float; every given prompt has the same P.  Points without a box get one padding point
    (prompt_encoder.py:150-151).  Returns (P, NT), NT = 5 output tokens + sparse tokens; raises ValueError for a bad
    shape or dtype and for NT > MAX_TOKENS (10 points alone, or a box plus 9 points).  Pure host code."""
    def shape(t):
        return tuple(t.shape) if hasattr(t, "shape") else None

    def is_float(t):
        return (t.dtype.is_floating_point if isinstance(t.dtype, torch.dtype)
                else np.issubdtype(np.dtype(t.dtype), np.floating))

    def is_int_valued(t):
        if isinstance(t.dtype, torch.dtype):
            return not t.dtype.is_complex and t.dtype != torch.bool and (
                not t.dtype.is_floating_point or bool(torch.all(t == torch.round(t))))
        d = np.dtype(t.dtype)
        return np.issubdtype(d, np.integer) or (np.issubdtype(d, np.floating) and bool(np.all(t == np.round(t))))

    Ps = []
    n_sparse = 0
    if (point_coords is None) != (point_labels is None):
        raise ValueError("point_coords and point_labels must be given together")
    if point_coords is not None:
        sc, sl = shape(point_coords), shape(point_labels)
        if sc is None or len(sc) != 3 or sc[2] != 2 or not is_float(point_coords):
            raise ValueError(f"point_coords must be a float tensor [P, N, 2], got {sc}")
        if sl != sc[:2] or not is_int_valued(point_labels):
            raise ValueError(f"point_labels must be integer labels [P, N] = {list(sc[:2])}, got {sl}")
        Ps.append(sc[0])
        n_sparse += sc[1] + (1 if boxes is None else 0)
    if boxes is not None:
        sb = shape(boxes)
        if sb is None or len(sb) != 2 or sb[1] != 4 or not is_float(boxes):
            raise ValueError(f"boxes must be a float tensor [P, 4], got {sb}")
        Ps.append(sb[0])
        n_sparse += 2
    if mask_input is not None:
        sm = shape(mask_input)
        if sm is None or len(sm) != 4 or sm[1:] != (1, mask_side, mask_side) or not is_float(mask_input):
            raise ValueError(f"mask_input must be float low-res logits [P, 1, {mask_side}, {mask_side}], got {sm}")
        Ps.append(sm[0])
    P = Ps[0] if Ps else 1
    if any(p != P for p in Ps):
        raise ValueError(f"the prompts disagree on the batch size: {Ps}")
    if P < 1:
        raise ValueError("at least one prompt is needed")
    NT = 5 + n_sparse
    if NT > MAX_TOKENS:
        raise ValueError(f"{NT} decoder tokens per prompt (5 + {n_sparse} sparse) exceed the limit of {MAX_TOKENS}: "
                         f"at most 10 points without a box, or a box plus 9 points")
    return P, NT


class ResizeLongestSide:
    """Coordinate half of SA/utils/transforms.py:16-102 (the image half is ops.resize_bilinear_u8)."""

    def __init__(self, target_length: int):
        self.target_length = target_length

    def apply_coords(self, coords: np.ndarray, original_size: Tuple[int, int]) -> np.ndarray:
        (oh, ow), (nh, nw) = original_size, preprocess_shape(original_size[0], original_size[1], self.target_length)
        c = np.array(coords, dtype=float)          # copy, float64 as the reference's astype(float)
        c[..., 0] = c[..., 0] * (nw / ow)
        c[..., 1] = c[..., 1] * (nh / oh)
        return c

    def apply_boxes(self, boxes: np.ndarray, original_size: Tuple[int, int]) -> np.ndarray:
        return self.apply_coords(np.asarray(boxes).reshape(-1, 2, 2), original_size).reshape(-1, 4)

    def apply_coords_torch(self, coords: torch.Tensor, original_size: Tuple[int, int]) -> torch.Tensor:
        (oh, ow), (nh, nw) = original_size, preprocess_shape(original_size[0], original_size[1], self.target_length)
        c = coords.detach().clone().to(torch.float)
        c[..., 0] = c[..., 0] * (nw / ow)
        c[..., 1] = c[..., 1] * (nh / oh)
        return c

    def apply_boxes_torch(self, boxes: torch.Tensor, original_size: Tuple[int, int]) -> torch.Tensor:
        return self.apply_coords_torch(boxes.reshape(-1, 2, 2), original_size).reshape(-1, 4)


def window_rows(B: int, g: int, ws: int) -> torch.Tensor:
    """The window gather/scatter map (window_partition / window_unpartition, image_encoder.py:243-289) of B images of
    g x g tokens: int32 [B * n * n * ws * ws] (n = ceil(g / ws)), token i of window w of image b at entry
    (b * n * n + w) * ws * ws + i holds its token row b * g * g + y * g + x, or -1 for window padding."""
    nwin = -(-g // ws)
    Mw = nwin * nwin * ws * ws
    r = torch.arange(B * Mw)
    b, rr = r // Mw, r % Mw
    win, pos = rr // (ws * ws), rr % (ws * ws)
    y = (win // nwin) * ws + pos // ws
    x = (win % nwin) * ws + pos % ws
    m = torch.where((y < g) & (x < g), b * g * g + y * g + x, torch.full_like(r, -1))
    return m.to(torch.int32)


def _to_dev_async(t: torch.Tensor, dev) -> torch.Tensor:
    """Small host tensor -> device through pinned memory, non-blocking.  A pageable `.to(dev)` makes the host wait
    until the stream has drained (here: the whole image encoder) before it can queue the decoder's launches."""
    return t.contiguous().pin_memory().to(dev, non_blocking=True)


class SamEngine:
    """Weights packed for the HIP kernels + preallocated activations for up to `max_batch` images."""

    def __init__(self, state_dict: Dict[str, torch.Tensor], cfg: Optional[SamConfig] = None,
                 device: str | torch.device = "cuda", max_batch: int = 1, bias_correction: bool = True):
        """bias_correction=True (the product setting): the biases of the 4 x 32 block projections absorb the EXPECTED error
        of rounding their weights to f16 (see _calibrate_bias_correction)."""
        cfg = cfg or SamConfig()
        self.cfg, self.dev = cfg, torch.device(device)
        assert self.dev.type == "cuda", "the InkLayer segmentor runs on MI355X only"
        D, g = cfg.embed_dim, cfg.grid
        assert D % cfg.num_heads == 0 and cfg.head_dim in HEAD_DIMS and g == 64 and cfg.window_size == 14, \
            "HIP attention kernels are specialised for SAM's head_dim 80 or 64 / 64x64 grid / 14x14 windows"
        E = cfg.prompt_embed_dim
        assert E // cfg.dec_heads == 32 and (E // 2) // cfg.dec_heads == 16
        self.T = g * g
        assert E == 256 and (self.T * 4) % 32 == 0, \
            "the fused decoder kernels (csrc/proj_ln.hip, csrc/upscale_tail.hip) are built for SAM's widths"
        self.scale = cfg.head_dim ** -0.5
        sd = state_dict
        dev = self.dev

        def h(name):  # matrix -> f16 [N, K]: the 32 blocks
            return sd[name].detach().to(torch.float32).to(dev, F16).contiguous()

        def f(name):  # vector / table -> f32
            return ops.own_f32(sd[name], dev)

        def ws(name, shape=None):  # matrix -> split-f16 [N, 3K] (ops.split_weight): patch embedding, neck, decoder
            t = sd[name].detach().to(dev, torch.float32)
            return ops.split_weight(t if shape is None else shape(t))

        self.w: Dict[str, torch.Tensor] = {}
        w = self.w
        P = cfg.patch_size
        w["pe.ws"] = ws("image_encoder.patch_embed.proj.weight", lambda t: t.reshape(D, 3 * P * P))
        w["pe.b"] = f("image_encoder.patch_embed.proj.bias")
        w["pos"] = f("image_encoder.pos_embed").reshape(self.T, D).contiguous()
        for i in range(cfg.depth):
            p = f"image_encoder.blocks.{i}."
            for n in ("norm1.weight", "norm1.bias", "norm2.weight", "norm2.bias", "attn.qkv.bias",
                      "attn.proj.bias", "mlp.lin1.bias", "mlp.lin2.bias", "attn.rel_pos_h",
                      "attn.rel_pos_w"):
                w[f"b{i}.{n}"] = f(p + n)
            for n in ("attn.qkv.weight", "attn.proj.weight", "mlp.lin1.weight", "mlp.lin2.weight"):
                w[f"b{i}.{n}"] = h(p + n)
            if i not in cfg.global_attn_indexes:
                # window padding (image_encoder.py:256-259 pads AFTER norm1 with zeros): the k / v rows of a
                # padded token are qkv(0) = the bias, rounded to f16 exactly like a projected row would be
                qb = w[f"b{i}.attn.qkv.bias"]
                w[f"b{i}.pad_k"] = qb[D:2 * D].to(F16).contiguous()
                w[f"b{i}.pad_v"] = qb[2 * D:].to(F16).contiguous()
        w["neck0.ws"] = ws("image_encoder.neck.0.weight", lambda t: t.reshape(E, D))
        w["neck1.w"], w["neck1.b"] = f("image_encoder.neck.1.weight"), f("image_encoder.neck.1.bias")
        # 3x3 conv as [co][(ky,kx)][ci]: the NHWC im2col of a split activation row is (ky,kx) x [hi | lo | hi/64]
        w["neck2.ws"] = ws("image_encoder.neck.2.weight", lambda t: t.permute(0, 2, 3, 1).reshape(E, 9, E)) \
            .reshape(E, 27 * E).contiguous()
        w["neck3.w"], w["neck3.b"] = f("image_encoder.neck.3.weight"), f("image_encoder.neck.3.bias")

        # ---- prompt encoder constants
        w["gauss"] = f("prompt_encoder.pe_layer.positional_encoding_gaussian_matrix")
        w["no_mask"] = f("prompt_encoder.no_mask_embed.weight").reshape(-1).contiguous()
        # point and mask prompts (SamEngine.decode_prompts).  A state dict made for the box path alone may lack these
        # weights: they are then absent here and decode_prompts names what is missing.
        # point_embeddings 0..3 (negative, positive, box corners) and not_a_point_embed
        w["pt_emb"] = torch.cat([f(f"prompt_encoder.point_embeddings.{i}.weight") for i in range(4)], 0).contiguous()
        if "prompt_encoder.not_a_point_embed.weight" in sd:
            w["not_a_point"] = f("prompt_encoder.not_a_point_embed.weight").reshape(-1).contiguous()
        # mask_downscaling's ten tensors flattened into one f32 block (layout: ink_sam_mask_embed)
        md = "prompt_encoder.mask_downscaling."
        md_names = ("0.weight", "0.bias", "1.weight", "1.bias", "3.weight", "3.bias", "4.weight", "4.bias", "6.weight",
                    "6.bias")
        if all(md + n in sd for n in md_names):
            w["mask_ds"] = torch.cat([sd[md + n].detach().to(torch.float32).reshape(-1) for n in md_names]) \
                .to(dev).contiguous()
        # dense positional encoding of the 64x64 grid (prompt_encoder.py:195-206): constant
        ar = (torch.arange(g, dtype=torch.float32) + 0.5) / g
        grid_xy = torch.stack([ar[None, :].expand(g, g), ar[:, None].expand(g, g)], -1).reshape(-1, 2)
        self.dense_pe = ops.sam_pe_encode(grid_xy.contiguous().to(dev), w["gauss"])  # [T, E]

        # ---- mask decoder
        t = "mask_decoder.transformer."
        def attn(dst, src):
            for n in ("q_proj", "k_proj", "v_proj", "out_proj"):
                w[f"{dst}.{n}.ws"] = ws(f"{src}.{n}.weight")
                w[f"{dst}.{n}.b"] = f(f"{src}.{n}.bias")

        def cat(dst, names):
            for sfx in (".ws", ".b"):
                w[dst + sfx] = torch.cat([w[n + sfx] for n in names]).contiguous()

        # (keys + pe) W = keys W + pe W: ONE split pass of the image keys feeds the token->image k and v projections and
        # the image->token q projection (one GEMM, N = 384); pe W is a per-position constant [T, 128] that the attention
        # kernels add (k_add / q_add).  The constants come from the same split-f16 GEMM (fp32-grade).
        pe_split = ops.add_split_f16(self.dense_pe)
        for i in range(cfg.dec_depth):
            p, d = f"{t}layers.{i}.", f"d{i}"
            attn(d + ".self", p + "self_attn")
            attn(d + ".t2i", p + "cross_attn_token_to_image")
            attn(d + ".i2t", p + "cross_attn_image_to_token")
            if i == 0:
                cat(d + ".self.qkv", [f"{d}.self.{n}" for n in ("q_proj", "k_proj", "v_proj")])
            else:
                cat(d + ".self.qk", [f"{d}.self.{n}" for n in ("q_proj", "k_proj")])
            for n in ("norm1", "norm2", "norm3", "norm4"):
                w[f"{d}.{n}.w"], w[f"{d}.{n}.b"] = f(p + n + ".weight"), f(p + n + ".bias")
            w[d + ".lin1.ws"], w[d + ".lin1.b"] = ws(p + "mlp.lin1.weight"), f(p + "mlp.lin1.bias")
            w[d + ".lin2.ws"], w[d + ".lin2.b"] = ws(p + "mlp.lin2.weight"), f(p + "mlp.lin2.bias")
            cat(d + ".kvq", [d + ".t2i.k_proj", d + ".t2i.v_proj", d + ".i2t.q_proj"])
            w[d + ".t2i.k_pe"] = ops.gemm(pe_split, w[d + ".t2i.k_proj.ws"]).contiguous()
            w[d + ".i2t.q_pe"] = ops.gemm(pe_split, w[d + ".i2t.q_proj.ws"]).contiguous()
            # image-side out_proj + residual + norm4 (+ the split operand) run as one kernel (csrc/proj_ln.hip)
            w[d + ".i2t.out_proj.blob"] = ops.proj256_ln_pack(w[d + ".i2t.out_proj.ws"].contiguous())
        attn("dfin", t + "final_attn_token_to_image")
        w["dfin.norm.w"], w["dfin.norm.b"] = f(t + "norm_final_attn.weight"), f(t + "norm_final_attn.bias")
        w["dfin.k_pe"] = ops.gemm(pe_split, w["dfin.k_proj.ws"]).contiguous()
        w["out_tok"] = torch.cat([f("mask_decoder.iou_token.weight"),
                                  f("mask_decoder.mask_tokens.weight")], 0).contiguous()  # [5, E]
        # ConvTranspose2d(k2,s2) as a projection to (dy,dx,co): W'[(dy*2+dx)*Co + co][ci]
        u = "mask_decoder.output_upscaling."
        w["up0.ws"] = ws(u + "0.weight", lambda t: t.permute(2, 3, 1, 0).reshape(4 * (E // 4), E))
        w["up0.b"] = f(u + "0.bias").repeat(4).contiguous()
        w["up1.w"], w["up1.b"] = f(u + "1.weight"), f(u + "1.bias")
        up3 = ws(u + "3.weight", lambda t: t.permute(2, 3, 1, 0).reshape(4 * (E // 8), E // 4))
        assert tuple(up3.shape) == (128, 192)
        # LayerNorm2d + GELU + ConvT + GELU + hyper product run as one kernel (csrc/upscale_tail.hip)
        w["up3.blob"] = ops.sam_upscale_pack(up3.contiguous())
        w["up3.b"] = f(u + "3.bias").repeat(4).contiguous()
        # the final token->image k / v projections and the first transposed convolution read the same split operand of
        # the final keys: ONE GEMM [k | v | up0] (N = 128 + 128 + 256)
        cat("dfin.kvu", ["dfin.k_proj", "dfin.v_proj", "up0"])
        for j in range(3):  # hyper-networks of the mask tokens (token 0: multimask_output=False) and the iou head
            w[f"iou{j}.ws"] = ws(f"mask_decoder.iou_prediction_head.layers.{j}.weight")
            w[f"iou{j}.b"] = f(f"mask_decoder.iou_prediction_head.layers.{j}.bias")
            for m in range(cfg.num_mask_tokens):   # a state dict made for the box path alone may lack tokens 1..3
                hk = f"mask_decoder.output_hypernetworks_mlps.{m}.layers.{j}."
                if m == 0 or hk + "bias" in sd:
                    w[f"{_hyp(m)}{j}.b"] = f(hk + "bias")
                if m == 0 or hk + "weight" in sd:
                    w[f"{_hyp(m)}{j}.ws"] = ws(hk + "weight")
        # the last hyper layer has N = 32 outputs, the iou head N = 4: both fine for the GEMM (N % 4)

        self._alloc(max_batch)
        if bias_correction:
            self._calibrate_bias_correction(sd)

    # ------------------------------------------------------------------ load-time bias correction
    @torch.no_grad()
    def _calibrate_bias_correction(self, sd) -> None:
        """More than half of the energy of the ViT-H residual stream - and of the attention / GELU outputs - is a
        per-channel constant (the same for every token, nearly the same for every sketch).  Rounding a weight matrix to
        f16 therefore produces, besides noise, a SYSTEMATIC output error  sum_k (W - f16(W))[n, k] * mean_k  that is the
        same for every token: a bias error.  It is measured once, at load time, on a calibration page (one encoder
        forward of this engine on a blank sketch page; torch reductions, never on the hot path) and folded into the bias:
        b_n += sum_k (W - f16(W))[n, k] * mean_k.  Zero run-time cost; measured
        with tests/precision_study.py it halves the logit error of the 32 blocks (the known "bias correction" of
        post-training quantisation, applied to f16)."""
        cfg, w, D = self.cfg, self.w, self.cfg.embed_dim
        page = torch.full((cfg.img_size, cfg.img_size, 3), 255, dtype=torch.uint8, device=self.dev)
        means: Dict[str, torch.Tensor] = {}
        self._calib = means
        try:
            self.encode([page])
        finally:
            self._calib = None
        for i in range(cfg.depth):
            p = f"image_encoder.blocks.{i}."
            for lin in ("attn.qkv", "mlp.lin1", "attn.proj", "mlp.lin2"):
                W32 = sd[p + lin + ".weight"].detach().to(self.dev, torch.float32)
                w16, bkey = w[f"b{i}.{lin}.weight"], f"b{i}.{lin}.bias"
                # a NEW tensor: w[bkey] may share storage with the caller's state dict, which must stay untouched
                w[bkey] = (w[bkey].double() + (W32 - w16.float()).double() @ means[f"b{i}.{lin}"].double()).float().contiguous()

    # ------------------------------------------------------------------ buffers
    def _alloc(self, B: int) -> None:
        cfg, dev, T, D = self.cfg, self.dev, self.T, self.cfg.embed_dim
        g, ws = cfg.grid, cfg.window_size
        self.max_batch = B
        nwin = -(-g // ws)                       # 5 windows per side (64 -> 70 padded)
        self.nwin = nwin
        Mw = nwin * nwin * ws * ws               # 4900 rows per image after padding
        self.Mw = Mw
        self._enc_graphs = LRU(self.graph_cache_size)
        self._enc_seen: Dict[int, int] = {}
        self.win_map = window_rows(B, g, ws).to(dev)
        P = cfg.patch_size
        e = lambda *s, dt=F16: torch.empty(s, device=dev, dtype=dt)
        self.buf_patches = e(B * T, 3 * P * P * 3)
        self.x = e(B * T, D, dt=F32)
        self.pos_rep = self.w["pos"].repeat(B, 1).contiguous()      # position embedding tiled over the batch (residual of the patch projection)
        self.y = e(B * T, D)
        self.qkv = e(B * T, 3 * D)
        self.att = e(B * T, D)
        self.hid = e(B * T, int(D * cfg.mlp_ratio))
        H = cfg.num_heads
        self.rel_aug = e(B * nwin * nwin * H * ws * ws, 32)
        # decomposed rel-pos terms of the global blocks as f16 tables (the one-wave-per-SIMD kernel converts them on the
        # way into LDS / the exponent: half the bytes written by relpos_bias and read back).  That kernel is head_dim 80
        # only: at head_dim 64 (ViT-B / ViT-L) the templated kernel of attention.hip reads f32 tables
        self.rel_f16 = cfg.head_dim == 80
        self.rel_h = e(B * H * T, 64, dt=F16 if self.rel_f16 else F32)
        self.rel_w = e(B * H * T, 64, dt=F16 if self.rel_f16 else F32)

    # ------------------------------------------------------------------ encoder
    def encode(self, images_u8: Sequence[torch.Tensor], chan_reverse: bool = False,
               upto: Optional[int] = None) -> torch.Tensor:
        """images_u8: resized HWC uint8 CUDA tensors (long side = img_size).
        Returns the image embeddings as tokens [B, 4096, 256] f32 (NHWC; the reference's NCHW
        `features` is `.permute(0, 2, 1).view(B, 256, 64, 64)`)."""
        cfg, w, T, D = self.cfg, self.w, self.T, self.cfg.embed_dim
        B = len(images_u8)
        assert 1 <= B <= self.max_batch
        H, Mw = cfg.num_heads, self.Mw
        x = self.x[:B * T]
        for b, img in enumerate(images_u8):
            # the patch embedding runs on split-f16 operands too: its rounding error would sit in the residual stream
            # of all 32 blocks (measured: the largest single contribution to the mask error)
            ops.sam_patchify(img, cfg.img_size, cfg.patch_size, cfg.pixel_mean, cfg.pixel_std,
                             chan_reverse, self.buf_patches[b * T:(b + 1) * T], split=True)
        # ONE projection for the batch (at 8 images N = 1280 and 512 tiles make it a ping-pong-kernel launch: ~1000 TFLOP/s
        # instead of eight 128-tile launches at ~500), the position embedding as a residual tiled per image
        ops.gemm(self.buf_patches[:B * T], w["pe.ws"], w["pe.b"], residual=self.pos_rep[:B * T], out=x)
        if upto is None and self.graph_blocks and ops.tracing_off():
            return self._blocks_graphed(B)
        return self._blocks(B, upto)

    # ------------------------------------------------------------------ HIP graph of the 32 blocks + neck
    # The blocks and the neck only touch engine-owned buffers of fixed shape per batch size: ~370 launches that can be
    # replayed as one graph.  Measured at batch 8 (tools/host_time.py, tools/bench_ab.py): the host needs 2.4 ms to
    # issue them eagerly (6.4 us per launch through ctypes) and 0.2 ms to replay the graph, against 53 ms of GPU work -
    # the step is not host-bound, and same-box A/B runs of the whole pipeline agree within the pool's noise (76.8-77.7 ms
    # either way).  So the graph is OFF by default and kept for hosts with slow cores (one attribute to flip).  A batch
    # size is captured the second time it is seen (a capture costs three forwards and pins a private pool for the
    # neck's intermediates); the result is cloned out of that pool.
    graph_blocks = False
    graph_cache_size = 2

    def _blocks_graphed(self, B: int) -> torch.Tensor:
        g = self._enc_graphs.get(B)
        if g is None:
            self._enc_seen[B] = self._enc_seen.get(B, 0) + 1
            if self._enc_seen[B] < 2:
                return self._blocks(B, None)
            x0 = self.x[:B * self.T].clone()              # the capture's warm-ups run the blocks in place
            cur = torch.cuda.current_stream(self.dev)
            side = torch.cuda.Stream(device=self.dev)
            side.wait_stream(cur)
            with torch.cuda.stream(side):                 # warm-up off the capture: lazy attribute calls, plans
                self._blocks(B, None)
                self.x[:B * self.T].copy_(x0)
            cur.wait_stream(side)
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                out = self._blocks(B, None)
            self.x[:B * self.T].copy_(x0)
            g = (graph, out)
            self._enc_graphs.put(B, g)
        g[0].replay()
        return g[1].clone()                               # the static output is overwritten by the next replay

    def _blocks(self, B: int, upto: Optional[int]) -> torch.Tensor:
        cfg, w, T, D = self.cfg, self.w, self.T, self.cfg.embed_dim
        H, Mw = cfg.num_heads, self.Mw
        x = self.x[:B * T]
        nblk = cfg.depth if upto is None else upto
        calib = getattr(self, "_calib", None)    # calibration pass only: per-channel means of the f16 GEMM operands
        for i in range(nblk):
            k = f"b{i}."
            y = ops.layernorm_rows(x, w[k + "norm1.weight"], w[k + "norm1.bias"], 1e-6, out=self.y[:B * T])
            if calib is not None:
                calib[k + "attn.qkv"] = y.float().mean(0)
            qkv = ops.gemm(y, w[k + "attn.qkv.weight"], w[k + "attn.qkv.bias"], out=self.qkv[:B * T])
            q, kk, v = qkv[:, :D], qkv[:, D:2 * D], qkv[:, 2 * D:]
            if i in cfg.global_attn_indexes:
                rh, rw = ops.relpos_bias(q, w[k + "attn.rel_pos_h"], w[k + "attn.rel_pos_w"], S=cfg.grid,
                                         n_batch=B, n_heads=H, head_dim=cfg.head_dim, scale=self.scale,
                                         out=(self.rel_h, self.rel_w), f16_tables=self.rel_f16)
                o = ops.flash_attn(q, kk, v, n_batch=B, n_heads=H, head_dim=cfg.head_dim, scale=self.scale,
                                   rel_h=rh, rel_w=rw, grid_w=cfg.grid, out=self.att[:B * T])
            else:
                # windowed block: everything stays in token order; window_partition / window_unpartition
                # (image_encoder.py:243-289) is the token-row map the attention gathers and scatters through,
                # so the 19.6 % padding rows (70x70 vs 64x64) are never normalised, projected or written
                wm = self.win_map[:B * Mw]
                nb = B * self.nwin * self.nwin
                aug = ops.relpos_bias(q, w[k + "attn.rel_pos_h"], w[k + "attn.rel_pos_w"],
                                      S=cfg.window_size, n_batch=nb, n_heads=H, head_dim=cfg.head_dim,
                                      scale=self.scale, out=self.rel_aug, tok_rows=wm)
                o = ops.flash_attn(q, kk, v, n_batch=nb, n_heads=H, head_dim=cfg.head_dim, scale=self.scale,
                                   n_q=cfg.window_size ** 2, n_k=cfg.window_size ** 2,
                                   rel_aug=aug, grid_w=cfg.window_size, tok_rows=wm,
                                   pad_k=w[k + "pad_k"], pad_v=w[k + "pad_v"], out=self.att[:B * T])
            if calib is not None:
                calib[k + "attn.proj"] = o.float().mean(0)
            ops.gemm(o, w[k + "attn.proj.weight"], w[k + "attn.proj.bias"], residual=x, out=x)
            y = ops.layernorm_rows(x, w[k + "norm2.weight"], w[k + "norm2.bias"], 1e-6, out=self.y[:B * T])
            hd = ops.gemm(y, w[k + "mlp.lin1.weight"], w[k + "mlp.lin1.bias"], act="gelu", out=self.hid[:B * T])
            if calib is not None:
                calib[k + "mlp.lin1"], calib[k + "mlp.lin2"] = y.float().mean(0), hd.float().mean(0)
            ops.gemm(hd, w[k + "mlp.lin2.weight"], w[k + "mlp.lin2.bias"], residual=x, out=x)
        if upto is not None:
            return x.view(B, T, D)
        # neck (image_encoder.py:88-104): 1x1 conv -> LN2d -> 3x3 conv -> LN2d, all on NHWC tokens
        n0 = ops.gemm(ops.add_split_f16(x), w["neck0.ws"])
        n1 = ops.layernorm_rows(n0, w["neck1.w"], w["neck1.b"], 1e-6, split=True)       # [B*T, 3E]
        n2 = ops.gemm(ops.im2col3x3(n1, B, cfg.grid, cfg.grid), w["neck2.ws"])
        emb = ops.layernorm_rows(n2, w["neck3.w"], w["neck3.b"], 1e-6, out_dtype=F32)
        return emb.view(B, T, cfg.prompt_embed_dim)

    # ------------------------------------------------------------------ decoder
    def decode(self, emb: torch.Tensor, boxes_input_frame: np.ndarray | torch.Tensor,
               input_hw: Tuple[int, int], orig_hw: Tuple[int, int], want_logits: bool = False):
        """One image: emb [4096, 256] f32 tokens, boxes [n, 4] xyxy in the resized-input frame
        (host memory).  PromptEncoder + MaskDecoder(multimask_output=False) + postprocess.
        Returns uint8 masks [n, H, W] on the GPU (+ low-res logits, iou, full logits if asked)."""
        boxes = torch.as_tensor(np.asarray(boxes_input_frame), dtype=torch.float32).reshape(-1, 4)
        low, iou = self.decode_low_res(emb.reshape(1, self.T, -1), boxes, [0] * boxes.shape[0])
        res = ops.sam_postprocess(low, self.cfg.img_size, input_hw, orig_hw, self.cfg.mask_threshold, want_logits)
        if want_logits:
            return res[0], low, iou, res[1]
        return res

    def decode_low_res(self, emb: torch.Tensor, boxes: torch.Tensor, img_of_box: Sequence[int]):
        """Prompt encoder + mask decoder for N boxes spread over B images in ONE pass (the reference decodes
        one image at a time; batching only changes which rows share a launch).  emb [B, 4096, 256] f32,
        boxes [N, 4] xyxy in the resized-input frame (host), img_of_box[i] = image of box i.
        -> (low-res logits [N, 256, 256] f32, iou [N, 1] f32).  decode_prompts with boxes alone and mask token 0."""
        low, iou = self.decode_prompts(emb, img_of_box, boxes=boxes)
        return low.view(low.shape[0], *low.shape[-2:]), iou

    def decode_prompts(self, emb: torch.Tensor, img_of_prompt: Sequence[int], points: Optional[torch.Tensor] = None,
                       labels: Optional[torch.Tensor] = None, boxes: Optional[torch.Tensor] = None,
                       mask_input: Optional[torch.Tensor] = None, multimask_output: bool = False,
                       masks: Optional[Tuple[int, int]] = None):
        """Prompt encoder + mask decoder for P prompts of any form (SA/modeling/prompt_encoder.py:128-166,
        mask_decoder.py:71-149), spread over the B images of emb [B, 4096, 256] f32 (img_of_prompt[p] = image of prompt p).
        points f32 [P, N, 2] + labels int [P, N], boxes f32 [P, 4] (both in the resized-input frame), mask_input f32
        [P, 1, 256, 256] low-res logits; any of them may be None (check_prompts states the rules).  The token block
        comes from one kernel (ops.sam_prompt_tokens); a mask input makes the keys per prompt from layer 0 on
        (ops.sam_mask_embed).  multimask_output selects mask tokens 1..3, else token 0; masks = (first, count) overrides
        it (count in {1, 3, 4}).  -> (low-res logits [P, M, 256, 256] f32, iou [P, M] f32)."""
        cfg, w, dev, L = self.cfg, self.w, self.dev, self.cfg.img_size
        P, _ = check_prompts(points, labels, boxes, mask_input, mask_side=4 * cfg.grid)
        if len(img_of_prompt) != P or not all(0 <= int(i) < emb.shape[0] for i in img_of_prompt):
            raise ValueError(f"img_of_prompt must name an image of emb for each of the {P} prompts")
        lo, M = masks if masks is not None else ((1, 3) if multimask_output else (0, 1))
        if M not in (1, 3, 4) or not 0 <= lo <= cfg.num_mask_tokens - M:
            raise ValueError(f"masks=(first, count) must select 1, 3 or 4 of the {cfg.num_mask_tokens} mask tokens")
        need = [("not_a_point", points is not None, "prompt_encoder.not_a_point_embed"),
                ("mask_ds", mask_input is not None, "prompt_encoder.mask_downscaling")]
        need += [(f"{_hyp(m)}0.ws", m > 0, f"mask_decoder.output_hypernetworks_mlps.{m}") for m in range(lo, lo + M)]
        missing = [name for key, used, name in need if used and key not in w]
        if missing:
            raise ValueError(f"these prompts need weights the engine's state dict did not have: {missing}")

        def dev32(t, dt=F32):
            t = torch.as_tensor(t)
            return t.to(dev, dt).contiguous() if t.is_cuda else _to_dev_async(t.to(dt), dev)

        pts = lab = bx = None
        if points is not None:
            pts, lab = dev32(points), dev32(labels, torch.int32)
        if boxes is not None:
            bx = dev32(torch.as_tensor(boxes).reshape(-1, 4))
        # not_a_point is read for points alone (checked above): a state dict made for the box path may lack it
        tokens = ops.sam_prompt_tokens(w["gauss"], w["pt_emb"], w.get("not_a_point", w["no_mask"]), w["out_tok"],
                                       float(L), P, points=pts, labels=lab, boxes=bx,
                                       pad=points is not None and boxes is None)
        mi = dev32(mask_input) if mask_input is not None else None
        return self._decode_tokens_split(emb, tokens, img_of_prompt, mask_input=mi, mask_lo=lo, n_masks=M)

    def _decode_tokens_split(self, emb: torch.Tensor, tokens: torch.Tensor, img_of_box: Sequence[int],
                             mask_input: Optional[torch.Tensor] = None, mask_lo: int = 0, n_masks: int = 1):
        """The mask decoder on split-f16 operands: every activation stays f32, every projection multiplies a
        [hi | lo*64 | hi/64] operand (ops.add_split_f16 / layernorm_rows(split=True)) with a '.ws' weight, the three
        attentions read and write f32 rows.  Same structure as the reference (mask_decoder.py:112-149,
        transformer.py:62-106,151-182).  tokens f32 [n, NT, E] (NT <= 16); mask_input f32 [n, 1, 4g, 4g] or None;
        mask tokens mask_lo .. mask_lo + n_masks - 1.  -> (low [n, n_masks, 4g, 4g], iou [n, n_masks])."""
        cfg, w, T, dev = self.cfg, self.w, self.T, self.dev
        E, g = cfg.prompt_embed_dim, cfg.grid
        B = emb.shape[0]
        n, NT = tokens.shape[0], tokens.shape[1]
        assert n > 0 and len(img_of_box) == n and NT <= MAX_TOKENS
        Hh = cfg.dec_heads
        SP = ops.add_split_f16

        def lin(x_split, name, bias=True, **kw):
            return ops.gemm(x_split, w[name + ".ws"], w[name + ".b"] if bias else None, **kw)

        qpe = tokens.view(n * NT, E)
        iob = torch.as_tensor(list(img_of_box), dtype=torch.int64)
        img_rows = _to_dev_async((iob * T).to(torch.int32), dev)
        if mask_input is None:
            keys = ops.add_f32(emb.reshape(B * T, E).contiguous(), w["no_mask"])      # [B*T, E], shared per image
            shared = True                                   # keys still one copy per IMAGE (layer 0)
            ks = None                                       # split-f16 operand of the per-box keys (layers >= 1)
        else:
            # src = emb + mask_downscaling(mask) (mask_decoder.py:123-126): per-prompt keys and their split operand
            keys, ks = ops.sam_mask_embed(mask_input, emb.reshape(B * T, E).contiguous(), img_rows, w["mask_ds"], 1e-6,
                                          split=True)
            shared = False
        queries = qpe
        sc32, sc16 = 1.0 / math.sqrt(32), 1.0 / math.sqrt(16)

        Eh = E // 2                                           # internal width of the cross attentions (128)

        def t2i_attend(name, queries, k, v, k_pe, residual):
            q = lin(SP(queries, qpe), name + ".q_proj")
            a = ops.attn_fewq(q, k, v, n_batch=n, n_heads=Hh, head_dim=16, scale=sc16, n_q=NT, n_k=T,
                              kv_batch_rows=img_rows if shared else None, k_add=k_pe)
            return lin(SP(a), name + ".out_proj", residual=residual)

        for i in range(cfg.dec_depth):
            d = f"d{i}"
            # (1) token self-attention (layer 0: no positional add, output replaces the queries)
            if i == 0:
                qkv = ops.gemm(SP(queries), w[d + ".self.qkv.ws"], w[d + ".self.qkv.b"])
                a = ops.attn_fewkeys(qkv[:, :E], qkv[:, E:2 * E], qkv[:, 2 * E:], B=n, n_heads=Hh, head_dim=32,
                                     scale=sc32)
                queries = lin(SP(a), d + ".self.out_proj")
            else:
                qk = ops.gemm(SP(queries, qpe), w[d + ".self.qk.ws"], w[d + ".self.qk.b"])
                v = lin(SP(queries), d + ".self.v_proj")
                a = ops.attn_fewkeys(qk[:, :E], qk[:, E:], v, B=n, n_heads=Hh, head_dim=32, scale=sc32)
                queries = lin(SP(a), d + ".self.out_proj", residual=queries)
            queries = ops.layernorm_rows(queries, w[d + ".norm1.w"], w[d + ".norm1.b"], 1e-5, out_dtype=F32)
            # image-side projections of this layer from ONE split pass of the keys: [k_t2i | v_t2i | q_i2t]
            # (from layer 1 on the split operand was written by the LayerNorm that produced the keys)
            kvq = ops.gemm(SP(keys) if ks is None else ks, w[d + ".kvq.ws"], w[d + ".kvq.b"])   # [B*T or n*T, 384] f32
            # (2) tokens -> image  (k = (keys + pe) Wk = kvq[:, :128] + pe Wk, added inside the attention)
            queries = ops.layernorm_rows(t2i_attend(d + ".t2i", queries, kvq[:, :Eh], kvq[:, Eh:2 * Eh],
                                                    w[d + ".t2i.k_pe"], queries),
                                         w[d + ".norm2.w"], w[d + ".norm2.b"], 1e-5, out_dtype=F32)
            # (3) token MLP.  The residual is added by the LayerNorm, not preloaded into lin2's accumulator: K' = 3 * 2048
            # products are one chain of 192 MFMA steps, and on top of a residual of 4 - 5 every step rounds at that ulp
            # (measured: up to 1.1e-5 off the exact product against 8 x the float32 evaluation's 1.2e-6)
            hmid = lin(SP(queries), d + ".lin1", act="relu")
            queries = ops.layernorm_rows(lin(SP(hmid), d + ".lin2"), w[d + ".norm3.w"], w[d + ".norm3.b"], 1e-5,
                                         out_dtype=F32, add=queries)
            # (4) image -> tokens: q = (keys + pe) Wq = kvq[:, 256:] + pe Wq, k = queries + qpe, v = queries
            ik = lin(SP(queries, qpe), d + ".i2t.k_proj")
            iv = lin(SP(queries), d + ".i2t.v_proj")
            a = ops.attn_fewkeys(kvq[:, 2 * Eh:], ik, iv, B=n, n_heads=Hh, head_dim=16, scale=sc16, n_q=T,
                                 q_batch_rows=img_rows if shared else None, q_add=w[d + ".i2t.q_pe"])   # [n*T, 128]
            # out_proj + residual + norm4 in one kernel (csrc/proj_ln.hip).  norm4 writes the next consumer's split operand
            # in the same pass (the keys feed only projections from here on); the f32 copy is kept only while a later
            # layer still adds to it.  While the keys are still one copy per IMAGE the residual is gathered per box, so
            # no per-box copy of the image keys (repeat_interleave of mask_decoder.py:124) is made
            last = i + 1 == cfg.dec_depth
            keys, ks = ops.proj256_ln(a, w[d + ".i2t.out_proj.blob"], w[d + ".i2t.out_proj.b"], keys, w[d + ".norm4.w"],
                                      w[d + ".norm4.b"], 1e-5, res_batch_rows=img_rows if shared else None,
                                      rows_per_batch=T if shared else 0, want_f32=not last, want_split=True)
            shared = False
        kvu = ops.gemm(ks, w["dfin.kvu.ws"], w["dfin.kvu.b"])                     # [n*T, k 128 | v 128 | up0 4*64]
        kv = kvu[:, :2 * Eh]
        queries = ops.layernorm_rows(t2i_attend("dfin", queries, kv[:, :Eh], kv[:, Eh:], w["dfin.k_pe"], queries),
                                     w["dfin.norm.w"], w["dfin.norm.b"], 1e-5, out_dtype=F32)
        hs = queries.view(n, NT, E)

        def mlp3(prefix: str, x: torch.Tensor) -> torch.Tensor:
            a = lin(SP(x), prefix + "0", act="relu")
            a = lin(SP(a), prefix + "1", act="relu")
            return lin(SP(a), prefix + "2")

        M = n_masks
        if M == 1:                                          # a view: one mask token costs no launch here
            hyper = mlp3(_hyp(mask_lo), hs[:, 1 + mask_lo].contiguous()).view(n, 1, 32)
        else:                                               # tokens mask_lo .. mask_lo + M - 1 -> [n, M, 32]
            hyper = torch.stack([mlp3(_hyp(m), hs[:, 1 + m].contiguous()) for m in range(mask_lo, mask_lo + M)], 1)
        iou = mlp3("iou", hs[:, 0].contiguous())[:, mask_lo:mask_lo + M]     # iou token -> [n, 4] -> the M masks
        u0 = kvu[:, 2 * Eh:]                                                     # [n*T, 4*64], row stride 512
        # LayerNorm2d + GELU + the second transposed convolution + GELU + the hyper-network product in one kernel
        # (csrc/upscale_tail.hip): u0 is read once, 4 floats per row and mask are written
        low = ops.sam_upscale_tail(u0, n, g, w["up1.w"], w["up1.b"], 1e-6, w["up3.blob"], w["up3.b"], hyper)
        return low, iou


# ----------------------------------------------------------------------------------------
# reference-shaped API
# ----------------------------------------------------------------------------------------
class SamPredictor:
    """Same call surface as SA/predictor.py:17-243: point, box and mask prompts, single or multimask output.
    One divergence: predict_torch defaults to multimask_output=False (InkLayer's box call); predict keeps the
    reference's True."""

    def __init__(self, engine: SamEngine):
        self.engine = engine
        self.cfg = engine.cfg
        self.transform = ResizeLongestSide(engine.cfg.img_size)
        self.reset_image()

    def reset_image(self) -> None:
        self.is_image_set = False
        self.features = None
        self.original_size = None
        self.input_size = None

    def set_image(self, image: np.ndarray, image_format: str = "RGB") -> None:
        assert image_format in ("RGB", "BGR")
        if image_format != "RGB":
            image = image[..., ::-1]
        # ResizeLongestSide.apply_image on the GPU (Pillow-exact, ops.resize_bilinear_u8)
        raw = torch.from_numpy(np.ascontiguousarray(image)).to(self.engine.dev)
        nh, nw = preprocess_shape(image.shape[0], image.shape[1], self.cfg.img_size)
        dev_img = ops.resize_bilinear_u8(raw, nh, nw)
        self.original_size = tuple(image.shape[:2])
        self.input_size = (nh, nw)
        self.features = self.engine.encode([dev_img])[0]
        self.is_image_set = True

    def apply_boxes(self, boxes: torch.Tensor) -> torch.Tensor:
        """ResizeLongestSide.apply_boxes_torch (SA/utils/transforms.py:67-91), host side."""
        return self.transform.apply_boxes_torch(boxes.detach().cpu(), self.original_size)

    def apply_coords(self, coords: np.ndarray, original_size: Optional[Tuple[int, int]] = None) -> np.ndarray:
        """ResizeLongestSide.apply_coords (SA/utils/transforms.py:33-45): original-image pixels -> input frame."""
        return self.transform.apply_coords(coords, original_size or self.original_size)

    def apply_coords_torch(self, coords: torch.Tensor, original_size: Optional[Tuple[int, int]] = None) -> torch.Tensor:
        """ResizeLongestSide.apply_coords_torch (SA/utils/transforms.py:67-81)."""
        return self.transform.apply_coords_torch(coords, original_size or self.original_size)

    def predict(self, point_coords: Optional[np.ndarray] = None, point_labels: Optional[np.ndarray] = None,
                box: Optional[np.ndarray] = None, mask_input: Optional[np.ndarray] = None,
                multimask_output: bool = True, return_logits: bool = False):
        """SA/predictor.py:92-158: one prompt in original-image pixels (point_coords [N, 2], point_labels [N], box [4],
        mask_input [1, 256, 256] low-res logits) -> numpy (masks [C, H, W], iou [C], low-res logits [C, 256, 256])."""
        if not self.is_image_set:
            raise RuntimeError("An image must be set with .set_image(...) before mask prediction.")
        if point_coords is not None and point_labels is None:
            raise ValueError("point_labels must be supplied if point_coords is supplied.")
        coords = labels = boxes = mask = None
        if point_coords is not None:
            coords = torch.as_tensor(self.apply_coords(point_coords), dtype=torch.float)[None]
            labels = torch.as_tensor(np.asarray(point_labels), dtype=torch.int)[None]
        if box is not None:
            boxes = torch.as_tensor(self.transform.apply_boxes(box, self.original_size), dtype=torch.float)[:1]
        if mask_input is not None:
            mask = torch.as_tensor(mask_input, dtype=torch.float)[None]
        masks, iou, low = self.predict_torch(coords, labels, boxes, mask, multimask_output, return_logits=return_logits)
        return masks[0].cpu().numpy(), iou[0].cpu().numpy(), low[0].cpu().numpy()

    def predict_torch(self, point_coords=None, point_labels=None, boxes: torch.Tensor = None,
                      mask_input=None, multimask_output: bool = False, return_logits: bool = False):
        """SA/predictor.py:160-243 with batched prompts already in the input frame: point_coords [B, N, 2],
        point_labels [B, N], boxes [B, 4], mask_input [B, 1, 256, 256].  -> (masks [B, C, H, W] bool (f32 logits with
        return_logits), iou [B, C], low-res logits [B, C, 256, 256]); C = 3 with multimask_output, else 1."""
        if not self.is_image_set:
            raise RuntimeError("An image must be set with .set_image(...) before mask prediction.")
        eng = self.engine
        P, _ = check_prompts(point_coords, point_labels, boxes, mask_input, mask_side=4 * self.cfg.grid)
        low, iou = eng.decode_prompts(self.features.reshape(1, eng.T, -1), [0] * P, point_coords, point_labels, boxes,
                                      mask_input, multimask_output)
        C, S = low.shape[1], low.shape[-1]
        res = ops.sam_postprocess(low.view(P * C, S, S), self.cfg.img_size, self.input_size, self.original_size,
                                  self.cfg.mask_threshold, return_logits)
        out = res[1] if return_logits else res.bool()
        return out.view(P, C, *self.original_size), iou, low


_ENGINES: Dict[str, SamEngine] = {}


def _check_model_type(cfg: SamConfig, model_type: Optional[str], source: str) -> None:
    if model_type is not None and config_for(model_type) != cfg:
        held = model_name(cfg) or f"{cfg.embed_dim}-wide, {cfg.depth}-block"
        raise ValueError(f"{source} holds a SAM {held} model, not the {model_type!r} asked for")


def build_sam(checkpoint: Optional[str] = None, state_dict=None, device="cuda",
              max_batch: int = 1, model_type: Optional[str] = None) -> SamEngine:
    """SA/build_sam.py:55-107 for ViT-H, ViT-L and ViT-B: the encoder's shape is read off the state dict
    (config_from_state_dict), so any of the three checkpoints loads unchanged; model_type, if given, must name what the
    state dict holds (ValueError otherwise).  Unlike the reference (which rebuilds the model and reloads
    the 2.4 GB checkpoint on EVERY run_SAM call, InkLayer/segmentor/sam.py:23) the engine is cached
    per checkpoint path and stays resident in HBM."""
    source = str(checkpoint) if state_dict is None else "the state dict"
    if state_dict is None:
        if checkpoint in _ENGINES:
            _check_model_type(_ENGINES[checkpoint].cfg, model_type, source)
            return _ENGINES[checkpoint]
        state_dict = torch.load(checkpoint, map_location="cpu", weights_only=True)
    cfg = config_from_state_dict(state_dict)
    _check_model_type(cfg, model_type, source)
    eng = SamEngine(state_dict, cfg, device, max_batch)
    if checkpoint is not None:
        _ENGINES[checkpoint] = eng
    return eng


def _registry_builder(model_type: str):
    def builder(checkpoint: Optional[str] = None, device="cuda", max_batch: int = 1) -> SamEngine:
        """sam_model_registry[...](checkpoint=...) of SA/build_sam.py:14-52, returning an engine.  Without a checkpoint the
        reference returns the untrained model; here that is an engine on seeded random weights."""
        if checkpoint is None:
            from . import weights_init
            cfg = config_for(model_type)
            return SamEngine(weights_init.random_sam_state_dict(cfg, device), cfg, device, max_batch)
        return build_sam(checkpoint, device=device, max_batch=max_batch, model_type=model_type)
    builder.__name__ = builder.__qualname__ = f"build_sam_{model_type}"
    return builder


build_sam_vit_h = _registry_builder("vit_h")
build_sam_vit_l = _registry_builder("vit_l")
build_sam_vit_b = _registry_builder("vit_b")
sam_model_registry = {"default": build_sam_vit_h, "vit_h": build_sam_vit_h, "vit_l": build_sam_vit_l,
                      "vit_b": build_sam_vit_b}


def run_SAM(image_pil, boxes_filt: torch.Tensor, sam_checkpoint: Optional[str] = None,
            engine: Optional[SamEngine] = None) -> List[np.ndarray]:
    """InkLayer/segmentor/sam.py:16-43.  Returns a list of HxW bool arrays, one per box.
    Reference quirks kept: the RGB array goes through a channel reversal before being declared
    "RGB" (:24-26).  Deviation (documented reference bug): zero boxes return []."""
    if len(boxes_filt) == 0:
        return []
    eng = engine if engine is not None else build_sam(sam_checkpoint)
    pred = SamPredictor(eng)
    image = np.array(image_pil)[..., ::-1]                 # cv2.COLOR_BGR2RGB on an RGB array
    pred.set_image(np.ascontiguousarray(image))
    tb = pred.apply_boxes(boxes_filt)
    masks, _, _ = pred.predict_torch(None, None, boxes=tb, multimask_output=False)
    m = masks[:, 0].cpu().numpy()                          # ONE device->host copy for all boxes
    return [m[i] for i in range(m.shape[0])]


def __getattr__(name):
    # SamAutomaticMaskGenerator lives in inklayer_amd/amg.py (which imports this module) and is offered here too, next
    # to SamPredictor, where the reference's package offers it
    if name == "SamAutomaticMaskGenerator":
        from .amg import SamAutomaticMaskGenerator
        return SamAutomaticMaskGenerator
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
