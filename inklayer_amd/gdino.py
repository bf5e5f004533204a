"""GroundingDINO (Swin-T / Swin-B) box proposer on MI355X: host-side composition of the HIP kernels.

Mirrors groundingdino.util.inference.{load_image, predict} and GroundingDINO.forward
(GD/util/inference.py:39-97, GD/models/GroundingDINO/groundingdino.py:227-365) with the reference's
state_dict key names, so `inklayer_gdino.pth` drops in unchanged.

MI355X-first structure (not a translation of the nn.Module tree):
  * one f32 residual stream per token set; every GEMM operand is written in f16 by the kernel before
    it, every GEMM fuses bias / activation / layer-scale / residual / window-reverse in its epilogue;
  * pad + cyclic shift + window partition is ONE int32 row map, applied as a gather inside the
    LayerNorm kernel and as a scatter inside the proj-GEMM epilogue; patch merging is a 4-row gather
    fused into its LayerNorm;
  * Swin attention: relative-position bias (+ SW-MSA mask) enters through the MFMA accumulator init;
  * deformable attention: softmax, sampling-location arithmetic and bilinear gather in one kernel on an
    f16 value map; the two small Linear layers feeding it are one [256 -> 384] GEMM;
  * image<->text fusion never builds the 13294 x T score matrix per head beyond a [S,4,T] f32 strip (T <= 4; a
    caption of 5..256 tokens runs the three products on MFMA with no score matrix at all, csrc/biattn_wide.hip);
  * everything that does not depend on the pixels (sine position embeddings, reference points,
    anchors, masks, maps, the BERT text features of the caption - "object." by default) is folded at load, or once
    per caption (set_caption; predict returns a phrase per box); a batch may carry one caption per image
    (set_captions: per-image token counts and text padding masks, csrc/biattn_wide.hip / attn_few.hip varlen forms).
Equal-sized images per batch (NestedTensor masks all False) — what InkLayer feeds.
"""
from __future__ import annotations

import math
from dataclasses import dataclass, replace
from typing import Dict, List, NamedTuple, Optional, Sequence, Tuple

import numpy as np
import torch

from . import ops
from ._lru import LRU

F16, F32, I32 = torch.float16, torch.float32, torch.int32


@dataclass
class GDinoConfig:
    """models/GroundingDINO_SwinT_OGC.py:1-43 + swin_T_224_1k (the default); the Swin-B backbones: GDINO_CONFIGS."""
    embed_dim: int = 96
    depths: Tuple[int, ...] = (2, 2, 6, 2)
    num_heads: Tuple[int, ...] = (3, 6, 12, 24)
    window_size: int = 7
    out_indices: Tuple[int, ...] = (1, 2, 3)
    hidden_dim: int = 256
    nheads: int = 8
    enc_layers: int = 6
    dec_layers: int = 6
    dim_feedforward: int = 2048
    num_queries: int = 900
    num_feature_levels: int = 4
    n_points: int = 4
    max_text_len: int = 256
    pe_temperature: float = 20.0
    box_threshold: float = 0.2
    pixel_mean: Tuple[float, ...] = (0.485, 0.456, 0.406)
    pixel_std: Tuple[float, ...] = (0.229, 0.224, 0.225)


# The backbones of build_swin_transformer (GD/models/GroundingDINO/backbone/swin_transformer.py:757-795) that the two
# public GroundingDINO configs name (GroundingDINO_SwinT_OGC.py, GroundingDINO_SwinB_cfg.py), keyed as there; the
# transformer on top is the same for all of them.
GDINO_CONFIGS: Dict[str, GDinoConfig] = {
    "swin_T_224_1k": GDinoConfig(),
    "swin_B_224_22k": GDinoConfig(embed_dim=128, depths=(2, 2, 18, 2), num_heads=(4, 8, 16, 32), window_size=7),
    "swin_B_384_22k": GDinoConfig(embed_dim=128, depths=(2, 2, 18, 2), num_heads=(4, 8, 16, 32), window_size=12),
}
GDINO_ALIASES = {"swin_t": "swin_T_224_1k", "swin_b": "swin_B_384_22k"}
WINDOW_SIZES = (7, 12)   # 7: ink_flash_attn bias_mode 3 (dense tables); 12: ink_swin_attn (csrc/attention_swin.hip)
HEAD_DIM = 32            # the head width both Swin attention kernels are built for


def config_for(name: str) -> GDinoConfig:
    """The registry entry of `name` (a copy): a backbone name of the reference or one of the aliases swin_t / swin_b.
    ValueError for an unknown name."""
    key = GDINO_ALIASES.get(name, name)
    if key not in GDINO_CONFIGS:
        raise ValueError(f"unknown GroundingDINO model {name!r}: one of {sorted(GDINO_CONFIGS) + sorted(GDINO_ALIASES)}")
    return replace(GDINO_CONFIGS[key])


def model_name(cfg: GDinoConfig) -> Optional[str]:
    """The reference's backbone name of a configuration's Swin shapes, None when it is none of the registry's."""
    key = (cfg.embed_dim, tuple(cfg.depths), tuple(cfg.num_heads), cfg.window_size)
    return next((n for n, c in GDINO_CONFIGS.items()
                 if (c.embed_dim, tuple(c.depths), tuple(c.num_heads), c.window_size) == key), None)


def check_config(cfg: GDinoConfig) -> None:
    """ValueError, naming what was found, unless the kernels serve `cfg`: Swin heads of width 32, a window size with an
    attention kernel, and the transformer shapes the fused detector kernels are built for.  No device is touched."""
    widths = [cfg.embed_dim * 2 ** i / nh for i, nh in enumerate(cfg.num_heads)]
    if len(cfg.depths) != len(cfg.num_heads) or any(wd != HEAD_DIM for wd in widths):
        raise ValueError(f"no kernels for this Swin backbone: head widths {widths} (embed dim {cfg.embed_dim}, heads "
                         f"{tuple(cfg.num_heads)}, depths {tuple(cfg.depths)}); the window attention kernels serve head "
                         f"width {HEAD_DIM}")
    if cfg.window_size not in WINDOW_SIZES:
        raise ValueError(f"no kernels for this Swin backbone: window size {cfg.window_size}; the window attention "
                         f"kernels serve {' and '.join(map(str, WINDOW_SIZES))}")
    if cfg.embed_dim * 2 ** (len(cfg.depths) - 1) > 2048:
        raise ValueError(f"no kernels for this Swin backbone: {cfg.embed_dim * 2 ** (len(cfg.depths) - 1)} channels in "
                         f"the last stage; the row LayerNorm serves at most 2048 (and the patch merging half of that)")
    if (cfg.hidden_dim, cfg.nheads, cfg.num_feature_levels, cfg.n_points) != (256, 8, 4, 4):
        raise ValueError(f"no kernels for this detector transformer: hidden_dim {cfg.hidden_dim}, nheads {cfg.nheads}, "
                         f"num_feature_levels {cfg.num_feature_levels}, n_points {cfg.n_points}; the kernels serve "
                         f"hidden_dim 256, 8 heads, 4 levels, 4 points")


def config_from_state_dict(sd) -> GDinoConfig:
    """The model a GroundingDINO state dict holds, from its tensor shapes alone (values: tensors on any device, "meta"
    included, or shape tuples; a DataParallel "module." prefix is stripped): embed_dim from patch_embed.proj.weight,
    depths by counting each stage's blocks, heads and window size from each stage's relative_position_bias_table
    ((2 ws - 1)^2, nh), out_indices from the backbone.0.norm{i} present, hidden_dim and levels from level_embed, layers
    by counting, queries from tgt_embed, dim_feedforward from linear1.  ValueError, naming what was found, when that is
    not a model the kernels serve (check_config) - before anything is allocated."""
    sd = clean_state_dict(sd)

    def shape(k):
        if k not in sd:
            raise ValueError(f"not a GroundingDINO state dict: {k} is missing")
        v = sd[k]
        return tuple(int(d) for d in (v.shape if hasattr(v, "shape") else v))

    def count(prefix):
        ids = {int(k[len(prefix):].split(".", 1)[0]) for k in sd if k.startswith(prefix)}
        if ids != set(range(len(ids))):
            raise ValueError(f"not a GroundingDINO state dict: {prefix}* holds indices {sorted(ids)}")
        return len(ids)

    bb, t = "backbone.0.", "transformer."
    C0 = shape(bb + "patch_embed.proj.weight")[0]
    depths = tuple(count(f"{bb}layers.{i}.blocks.") for i in range(count(bb + "layers.")))
    if not depths or 0 in depths:
        raise ValueError(f"not a GroundingDINO state dict: Swin stage depths {depths}")
    tabs = [[shape(f"{bb}layers.{i}.blocks.{b}.attn.relative_position_bias_table") for b in range(d)]
            for i, d in enumerate(depths)]
    flat = [tb for st in tabs for tb in st]
    sides = sorted({math.isqrt(tb[0]) for tb in flat})
    heads = tuple(st[0][1] for st in tabs)
    if (any(len(tb) != 2 for tb in flat) or any(tb[1] != st[0][1] for st in tabs for tb in st) or len(sides) != 1
            or sides[0] ** 2 != flat[0][0] or sides[0] % 2 == 0):
        raise ValueError(f"inconsistent Swin backbone: relative_position_bias_table shapes {sorted(set(flat))}")
    ws = (sides[0] + 1) // 2
    out_indices = tuple(i for i in range(len(depths)) if f"{bb}norm{i}.weight" in sd)
    lv = shape(t + "level_embed")
    so = shape(t + "encoder.layers.0.self_attn.sampling_offsets.weight")
    cfg = GDinoConfig(embed_dim=C0, depths=depths, num_heads=heads, window_size=ws, out_indices=out_indices,
                      hidden_dim=lv[1], num_feature_levels=lv[0], enc_layers=count(t + "encoder.layers."),
                      dec_layers=count(t + "decoder.layers."), num_queries=shape(t + "tgt_embed.weight")[0],
                      dim_feedforward=shape(t + "encoder.layers.0.linear1.weight")[0])
    check_config(cfg)
    if so != (cfg.nheads * lv[0] * cfg.n_points * 2, lv[1]):
        raise ValueError(f"no kernels for this detector transformer: sampling_offsets.weight has shape {so}, not "
                         f"{(cfg.nheads * lv[0] * cfg.n_points * 2, lv[1])} (8 heads x 4 levels x 4 points x 2)")
    return cfg


# caption "object." -> [CLS] object . [SEP]; ids of bert-base-uncased ("object" = 4874 cannot be
# confirmed offline: treated as data)
DEFAULT_TOKEN_IDS = (101, 4874, 1012, 102)
SPECIAL_TOKENS = (101, 102, 1012, 1029)


def resize_shape(w: int, h: int, size: int = 800, max_size: int = 1333) -> Tuple[int, int]:
    """get_size_with_aspect_ratio (GD/datasets/transforms.py:90-108) -> (oh, ow)."""
    mn, mx = float(min(w, h)), float(max(w, h))
    if mx / mn * size > max_size:
        size = int(round(max_size * mn / mx))
    if (w <= h and w == size) or (h <= w and h == size):
        return h, w
    if w < h:
        return int(size * h / w), size
    return size, int(size * w / h)


def resize_for_detector(image_rgb: np.ndarray) -> np.ndarray:
    """RandomResize([800], max_size=1333) of load_image (GD/util/inference.py:40-49) with PIL on the host.  Not on
    the product path any more (ops.resize_bilinear_u8 is bit-identical on the GPU); kept as the test reference."""
    from PIL import Image
    im = Image.fromarray(image_rgb)
    oh, ow = resize_shape(im.size[0], im.size[1])
    if (ow, oh) != im.size:
        im = im.resize((ow, oh), Image.BILINEAR)
    return np.ascontiguousarray(np.asarray(im))


def text_masks_and_position_ids(input_ids: Sequence[int], special: Sequence[int] = SPECIAL_TOKENS):
    """generate_masks_with_special_tokens_and_transfer_map (GD/.../bertwarper.py:224-273), one sentence."""
    n = len(input_ids)
    attn = torch.eye(n, dtype=torch.bool)
    pos = torch.zeros(n, dtype=torch.long)
    prev = 0
    for col, tok in enumerate(input_ids):
        if tok not in special:
            continue
        if col == 0 or col == n - 1:
            attn[col, col] = True
            pos[col] = 0
        else:
            attn[prev + 1: col + 1, prev + 1: col + 1] = True
            pos[prev + 1: col + 1] = torch.arange(0, col - prev)
        prev = col
    return attn, pos


SEPARATOR_TOKENS = (101, 102, 1012)      # [CLS], [SEP], "." : the phrase boundaries of predict(remove_combined=True)


def phrase_token_ids(posmap: Sequence[bool], token_ids: Sequence[int], left_idx: int = 0, right_idx: int = 255) -> List[int]:
    """get_phrases_from_posmap (GD/util/utils.py:599-610) up to the tokenizer's decode: the ids of the tokens whose
    posmap entry is set, positions 0..left_idx and right_idx.. excluded."""
    return [int(token_ids[i]) for i, on in enumerate(posmap) if on and left_idx < i < right_idx]


def phrases_from_probs(probs: torch.Tensor, token_ids: Sequence[int], text_threshold: float,
                       remove_combined: bool = False, tokenizer=None) -> list:
    """The phrase of every kept box, as predict (GD/util/inference.py:80-95) forms it from the sigmoided logits
    probs [n, T] of the caption token_ids: the tokens above text_threshold, and with remove_combined only those between
    the two separators ([CLS] / [SEP] / ".") around the box's strongest token (the sep_idx bisect; a strongest token at
    or before the first separator wraps to the last one, as the reference's index -1 does; one past the last separator -
    a caption cut at 256 tokens - ends at T, where the reference raises IndexError).  With a tokenizer (anything with
    decode(ids) -> str) a phrase is the decoded string without "."; without one it is the tuple of ids without the
    id of "." (1012)."""
    import bisect
    T = len(token_ids)
    sep_idx = [i for i, t in enumerate(token_ids) if t in SEPARATOR_TOKENS]
    out = []
    for row in probs:
        posmap = (row > text_threshold).tolist()
        left, right = 0, 255
        if remove_combined:
            at = bisect.bisect_left(sep_idx, int(row.argmax()))
            right = sep_idx[at] if at < len(sep_idx) else T
            left = sep_idx[at - 1]
        ids = phrase_token_ids(posmap, token_ids, left, right)
        out.append(tokenizer.decode(ids).replace(".", "") if tokenizer is not None
                   else tuple(t for t in ids if t != 1012))
    return out


def _interleaved_sincos(v: torch.Tensor) -> torch.Tensor:
    return torch.stack((v[..., 0::2].sin(), v[..., 1::2].cos()), dim=-1).flatten(-2)


class _Plan:
    """Pixel-independent constants for one (h, w, B): maps, masks, position embeddings, anchors."""

    def __init__(self, eng: "GDinoEngine", h: int, w: int, B: int):
        cfg, dev = eng.cfg, eng.dev
        ws, sh = cfg.window_size, cfg.window_size // 2
        self.B = B
        H, W = -(-h // 4), -(-w // 4)
        self.stage_hw: List[Tuple[int, int]] = []
        self.win_map: List[List[torch.Tensor]] = []      # [stage][shifted] int32 [B*nW*49]
        self.nW: List[int] = []
        self.shift_mask: List[torch.Tensor] = []         # [stage] f32 [nW, 49, 64], pre-divided by scale (ws == 7)
        self.region: List[torch.Tensor] = []             # [stage] uint8 [nW, ws*ws] nine-slice ids (ws != 7)
        self.merge_map: List[Optional[torch.Tensor]] = []
        scale = HEAD_DIM ** -0.5
        for i in range(len(cfg.depths)):
            self.stage_hw.append((H, W))
            Hp, Wp = -(-H // ws) * ws, -(-W // ws) * ws
            nW = (Hp // ws) * (Wp // ws)
            self.nW.append(nW)
            wy, wx, iy, ix = torch.meshgrid(torch.arange(Hp // ws), torch.arange(Wp // ws), torch.arange(ws),
                                            torch.arange(ws), indexing="ij")
            maps = []
            for shift in (0, sh):
                y = (wy * ws + iy + shift) % Hp
                x = (wx * ws + ix + shift) % Wp
                tok = torch.where((y < H) & (x < W), y * W + x, torch.full_like(y, -1)).reshape(-1)
                full = torch.cat([torch.where(tok >= 0, tok + b * H * W, tok) for b in range(B)])
                maps.append(full.to(I32).to(dev))
            self.win_map.append(maps)
            # SW-MSA mask of BasicLayer.forward (swin_transformer.py:417-441)
            mw = swin_regions(Hp, Wp, ws)
            if ws == 7:
                diff = mw[:, None, :] - mw[:, :, None]
                m = torch.zeros((nW, ws * ws, 64))
                m[:, :, :ws * ws] = torch.where(diff != 0, torch.tensor(-100.0), torch.tensor(0.0)) / scale
                self.shift_mask.append(m.to(dev).contiguous())
            else:                                # ops.swin_attn compares the ids itself: no [nW, ws^2, ws^2] table
                self.region.append(mw.to(torch.uint8).to(dev).contiguous())
            if i < len(cfg.depths) - 1:
                H2, W2 = (H + 1) // 2, (W + 1) // 2
                y2, x2 = torch.meshgrid(torch.arange(H2), torch.arange(W2), indexing="ij")
                cols = []
                for dy, dx in ((0, 0), (1, 0), (0, 1), (1, 1)):       # x0, x1, x2, x3 (swin_transformer.py:331-334)
                    yy, xx = 2 * y2 + dy, 2 * x2 + dx
                    cols.append(torch.where((yy < H) & (xx < W), yy * W + xx, torch.full_like(yy, -1)).reshape(-1))
                g4 = torch.stack(cols, -1)
                full = torch.cat([torch.where(g4 >= 0, g4 + b * H * W, g4) for b in range(B)])
                self.merge_map.append(full.to(I32).contiguous().to(dev))
                H, W = H2, W2
            else:
                self.merge_map.append(None)
        # ---- multi-scale levels
        shapes = [self.stage_hw[i] for i in cfg.out_indices]
        H3, W3 = shapes[-1]
        for _ in range(cfg.num_feature_levels - len(shapes)):
            shapes.append(((shapes[-1][0] - 1) // 2 + 1, (shapes[-1][1] - 1) // 2 + 1))
        self.shapes = shapes
        self.S = sum(a * b for a, b in shapes)
        starts = np.cumsum([0] + [a * b for a, b in shapes])[:-1]
        self.level_start = [int(s) for s in starts]
        # 3x3 / s2 / p1 im2col map of the extra level (input_proj[3], groundingdino.py:139-147)
        H4, W4 = shapes[len(cfg.out_indices)]
        y4, x4, ky, kx = torch.meshgrid(torch.arange(H4), torch.arange(W4), torch.arange(3), torch.arange(3),
                                        indexing="ij")
        yy, xx = 2 * y4 + ky - 1, 2 * x4 + kx - 1
        self.lvl4_map = torch.where((yy >= 0) & (yy < H3) & (xx >= 0) & (xx < W3), yy * W3 + xx,
                                    torch.full_like(yy, -1)).reshape(-1).to(I32).to(dev)
        # ---- PositionEmbeddingSineHW with an all-False mask (position_encoding.py:98-131) + level_embed
        npf = cfg.hidden_dim // 2
        dim_t = torch.arange(npf, dtype=torch.float32)
        dim_t = cfg.pe_temperature ** (2 * torch.div(dim_t, 2, rounding_mode="floor") / npf)
        pos = []
        for l, (hh, ww) in enumerate(shapes):
            ye = torch.arange(1, hh + 1, dtype=torch.float32)[:, None].expand(hh, ww) / (float(hh) + 1e-6) * (2 * math.pi)
            xe = torch.arange(1, ww + 1, dtype=torch.float32)[None, :].expand(hh, ww) / (float(ww) + 1e-6) * (2 * math.pi)
            px, py = _interleaved_sincos(xe[:, :, None] / dim_t), _interleaved_sincos(ye[:, :, None] / dim_t)
            pos.append(torch.cat((py, px), dim=2).reshape(hh * ww, 2 * npf) + eng.level_embed_cpu[l])
        self.pos = torch.cat(pos, 0).to(dev).contiguous()                       # [S, 256]
        # ---- encoder reference points (transformer.py:465-480) and two-stage anchors (utils.py:56-116)
        refs, props = [], []
        for lvl, (hh, ww) in enumerate(shapes):
            ry, rx = torch.meshgrid(torch.linspace(0.5, hh - 0.5, hh), torch.linspace(0.5, ww - 0.5, ww), indexing="ij")
            refs.append(torch.stack((rx.reshape(-1) / ww, ry.reshape(-1) / hh), -1))
            gy, gx = torch.meshgrid(torch.linspace(0, hh - 1, hh), torch.linspace(0, ww - 1, ww), indexing="ij")
            grid = (torch.stack((gx, gy), -1) + 0.5) / torch.tensor([float(ww), float(hh)])
            props.append(torch.cat((grid, torch.ones_like(grid) * 0.05 * (2.0 ** lvl)), -1).view(-1, 4))
        self.enc_ref = torch.cat(refs, 0).to(dev).contiguous()                  # [S, 2]
        pr = torch.cat(props, 0)
        valid = ((pr > 0.01) & (pr < 0.99)).all(-1)
        pr = torch.log(pr / (1 - pr)).masked_fill(~valid[:, None], float("inf"))
        self.props_unsig = pr.to(dev).contiguous()                              # [S, 4]
        self.valid_map = torch.where(valid, torch.arange(self.S), torch.full((self.S,), -1)).to(I32).to(dev)


def swin_regions(Hp: int, Wp: int, ws: int) -> torch.Tensor:
    """The nine-slice labelling of the padded, shifted image of BasicLayer.forward (swin_transformer.py:417-432) in
    window order: f32 [nW, ws*ws] ids 0..8.  Two tokens of a window attend to each other iff their ids are equal."""
    sh = ws // 2
    img = torch.zeros((Hp, Wp))
    cnt = 0
    for hs in (slice(0, -ws), slice(-ws, -sh), slice(-sh, None)):
        for wsl in (slice(0, -ws), slice(-ws, -sh), slice(-sh, None)):
            img[hs, wsl] = cnt
            cnt += 1
    return img.view(Hp // ws, ws, Wp // ws, ws).permute(0, 2, 1, 3).reshape(-1, ws * ws)


def swin_dense_bias(table: torch.Tensor, ws: int, nh: int, scale: float) -> torch.Tensor:
    """The relative-position bias of one Swin block (swin_transformer.py:111-121, 159-163) as flash_attn's dense_bias:
    f32 [nh, ws*ws, 64], query rows x key columns, pre-divided by the softmax scale, columns ws*ws.. zero."""
    co = torch.stack(torch.meshgrid(torch.arange(ws), torch.arange(ws), indexing="ij")).flatten(1)
    rel = (co[:, :, None] - co[:, None, :]).permute(1, 2, 0).contiguous()
    rel[:, :, 0] += ws - 1
    rel[:, :, 1] += ws - 1
    rel[:, :, 0] *= 2 * ws - 1
    rel_index = rel.sum(-1).view(-1)
    bias = torch.zeros((nh, ws * ws, 64))
    bias[:, :, :ws * ws] = table[rel_index].view(ws * ws, ws * ws, nh).permute(2, 0, 1) / scale
    return bias


def swin_bias_table(table: torch.Tensor, ws: int, nh: int) -> torch.Tensor:
    """The relative-position bias table of one Swin block as ops.swin_attn takes it: f32 [nh, (2 ws - 1)^2], logit
    units, contiguous; the kernel indexes it with (qy - ky + ws - 1) (2 ws - 1) + (qx - kx + ws - 1), which is
    relative_position_index (swin_transformer.py:111-121)."""
    assert tuple(table.shape) == ((2 * ws - 1) ** 2, nh)
    return table.to(torch.float32).t().contiguous()


def clean_state_dict(sd: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
    """clean_state_dict (GD/util/misc.py:711-717): strip the DataParallel "module." prefix the shipped
    GroundingDINO checkpoints carry (GD/util/inference.py:33-34 always applies it)."""
    if any(k.startswith("module.") for k in sd):
        return {(k[7:] if k.startswith("module.") else k): v for k, v in sd.items()}
    return sd


class _TextBatch(NamedTuple):
    """The text side of one per-image-caption forward (GDinoEngine.set_captions), rows of the images in that launch."""
    text0: torch.Tensor      # f32 [B*Tmax, 256], pad rows zero
    t_len: torch.Tensor      # int32 [B] on the device
    blocked: torch.Tensor    # u8 [B, Tmax, Tmax]
    pos_text: torch.Tensor   # f32 [B*Tmax, 256]
    bias: torch.Tensor       # f32 [B, Tc]: -inf at t >= T_b
    Tmax: int
    Tc: int                  # 4 ceil(Tmax / 4): the columns of ContrastiveEmbed's GEMM


class GDinoEngine:
    fuse_ffn = True          # encoder FFN + norm2 as one kernel (csrc/ffn_fused.hip); False: two GEMMs + LayerNorm
    fuse_ffn_pre = True      # ... starting at the deformable attention's output projection (out_proj + norm1 inside)
    fold_fusion = True       # a caption of <= 4 tokens folded through the fusion layers (csrc/fusion_fold.hip); False: the general kernel, csrc/biattn_wide.hip

    def __init__(self, state_dict: Dict[str, torch.Tensor], cfg: Optional[GDinoConfig] = None,
                 device: str | torch.device = "cuda", encoded_text: Optional[torch.Tensor] = None,
                 token_ids: Sequence[int] = DEFAULT_TOKEN_IDS):
        cfg = cfg or GDinoConfig()
        self.cfg, self.dev = cfg, torch.device(device)
        assert self.dev.type == "cuda", "the InkLayer detector runs on MI355X only"
        check_config(cfg)
        sd, dev = clean_state_dict(state_dict), self.dev
        self.w: Dict[str, torch.Tensor] = {}
        w = self.w

        def h(name, shape=None):
            t = sd[name].detach().to(torch.float32)
            return (t.reshape(shape) if shape is not None else t).to(dev, F16).contiguous()

        def f(name):
            return ops.own_f32(sd[name], dev)

        def lin(dst, src):
            w[dst + ".w"], w[dst + ".b"] = h(src + ".weight"), f(src + ".bias")

        def ln(dst, src):
            w[dst + ".w"], w[dst + ".b"] = f(src + ".weight"), f(src + ".bias")

        def cat_lin(dst, srcs):
            w[dst + ".w"] = torch.cat([h(s + ".weight") for s in srcs]).contiguous()
            w[dst + ".b"] = torch.cat([f(s + ".bias") for s in srcs]).contiguous()

        # ---- Swin-T
        bb = "backbone.0."
        pw = sd[bb + "patch_embed.proj.weight"].detach().to(torch.float32).cpu().reshape(cfg.embed_dim, 48)
        w["pe.w"] = torch.cat([pw, torch.zeros(cfg.embed_dim, 16)], 1).to(dev, F16).contiguous()
        w["pe.b"] = f(bb + "patch_embed.proj.bias")
        ln("pe.norm", bb + "patch_embed.norm")
        ws = cfg.window_size
        scale = HEAD_DIM ** -0.5
        for i, (dep, nh) in enumerate(zip(cfg.depths, cfg.num_heads)):
            for b in range(dep):
                p, d = f"{bb}layers.{i}.blocks.{b}.", f"s{i}b{b}"
                ln(d + ".norm1", p + "norm1")
                ln(d + ".norm2", p + "norm2")
                lin(d + ".qkv", p + "attn.qkv")
                lin(d + ".proj", p + "attn.proj")
                lin(d + ".fc1", p + "mlp.fc1")
                lin(d + ".fc2", p + "mlp.fc2")
                tab = sd[p + "attn.relative_position_bias_table"].detach().to(torch.float32).cpu()
                if ws == 7:
                    w[d + ".bias"] = swin_dense_bias(tab, ws, nh, scale).to(dev).contiguous()
                else:
                    w[d + ".table"] = swin_bias_table(tab, ws, nh).to(dev).contiguous()
            if i < len(cfg.depths) - 1:
                ln(f"s{i}.merge.norm", f"{bb}layers.{i}.downsample.norm")
                w[f"s{i}.merge.w"] = h(f"{bb}layers.{i}.downsample.reduction.weight")
            if i in cfg.out_indices:
                ln(f"s{i}.outnorm", f"{bb}norm{i}")
        # ---- input_proj (1x1 conv + GN x3, 3x3 s2 conv + GN)
        for l in range(cfg.num_feature_levels):
            cw = sd[f"input_proj.{l}.0.weight"].detach().to(torch.float32)
            if cw.shape[-1] == 1:
                w[f"ip{l}.w"] = cw.reshape(cw.shape[0], cw.shape[1]).to(dev, F16).contiguous()
            else:
                w[f"ip{l}.w"] = cw.permute(0, 2, 3, 1).reshape(cw.shape[0], -1).to(dev, F16).contiguous()
            w[f"ip{l}.b"] = f(f"input_proj.{l}.0.bias")
            ln(f"ip{l}.gn", f"input_proj.{l}.1")
        t = "transformer."
        self.level_embed_cpu = sd[t + "level_embed"].detach().to(torch.float32).cpu()

        def msda(dst, src):
            cat_lin(dst + ".proj", [src + "sampling_offsets", src + "attention_weights"])   # [384, 256]
            lin(dst + ".value", src + "value_proj")
            lin(dst + ".out", src + "output_proj")

        def mha(dst, src):
            W, b = sd[src + "in_proj_weight"].detach().to(torch.float32), sd[src + "in_proj_bias"].detach().to(torch.float32)
            D = W.shape[1]
            w[dst + ".qk.w"], w[dst + ".qk.b"] = W[:2 * D].to(dev, F16).contiguous(), b[:2 * D].to(dev).contiguous()
            w[dst + ".q.w"], w[dst + ".q.b"] = W[:D].to(dev, F16).contiguous(), b[:D].to(dev).contiguous()
            w[dst + ".kv.w"], w[dst + ".kv.b"] = W[D:].to(dev, F16).contiguous(), b[D:].to(dev).contiguous()
            w[dst + ".v.w"], w[dst + ".v.b"] = W[2 * D:].to(dev, F16).contiguous(), b[2 * D:].to(dev).contiguous()
            lin(dst + ".out", src + "out_proj")

        for i in range(cfg.enc_layers):
            p, d = f"{t}encoder.layers.{i}.", f"e{i}"
            msda(d + ".msda", p + "self_attn.")
            ln(d + ".norm1", p + "norm1"); lin(d + ".lin1", p + "linear1"); lin(d + ".lin2", p + "linear2"); ln(d + ".norm2", p + "norm2")
            if w[d + ".lin1.w"].shape[1] == 256 and w[d + ".lin1.w"].shape[0] % 64 == 0 and w[d + ".lin1.w"].shape[0] <= 2048:
                w[d + ".ffn.blob"] = ops.ffn256_pack(w[d + ".lin1.w"], w[d + ".lin1.b"], w[d + ".lin2.w"])     # csrc/ffn_fused.hip
                # ... and the form that starts at the deformable attention's output projection (out_proj + norm1 inside)
                w[d + ".ffn.blob_pre"] = ops.ffn256_pack(w[d + ".lin1.w"], w[d + ".lin1.b"], w[d + ".lin2.w"],
                                                         w[d + ".msda.out.w"])
            p = f"{t}encoder.text_layers.{i}."
            mha(d + ".txt", p + "self_attn.")
            lin(d + ".txt.lin1", p + "linear1"); lin(d + ".txt.lin2", p + "linear2")
            ln(d + ".txt.norm1", p + "norm1"); ln(d + ".txt.norm2", p + "norm2")
            p = f"{t}encoder.fusion_layers.{i}."
            ln(d + ".fu.lnv", p + "layer_norm_v"); ln(d + ".fu.lnl", p + "layer_norm_l")
            cat_lin(d + ".fu.qv", [p + "attn.v_proj", p + "attn.values_v_proj"])          # [2048, 256]
            cat_lin(d + ".fu.kl", [p + "attn.l_proj", p + "attn.values_l_proj"])
            lin(d + ".fu.outv", p + "attn.out_v_proj"); lin(d + ".fu.outl", p + "attn.out_l_proj")
            w[d + ".fu.gv"], w[d + ".fu.gl"] = f(p + "gamma_v"), f(p + "gamma_l")
        for i in range(cfg.dec_layers):
            p, d = f"{t}decoder.layers.{i}.", f"d{i}"
            msda(d + ".msda", p + "cross_attn.")
            ln(d + ".norm1", p + "norm1")
            mha(d + ".ca", p + "ca_text."); ln(d + ".canorm", p + "catext_norm")
            mha(d + ".sa", p + "self_attn."); ln(d + ".norm2", p + "norm2")
            lin(d + ".lin1", p + "linear1"); lin(d + ".lin2", p + "linear2"); ln(d + ".norm3", p + "norm3")
        ln("dec.norm", t + "decoder.norm")
        lin("rph0", t + "decoder.ref_point_head.layers.0")
        lin("rph1", t + "decoder.ref_point_head.layers.1")
        w["tgt"] = f(t + "tgt_embed.weight")
        lin("enc_output", t + "enc_output"); ln("enc_output_norm", t + "enc_output_norm")
        for j in range(3):
            lin(f"encbox{j}", f"{t}enc_out_bbox_embed.layers.{j}")
            lin(f"box{j}", f"bbox_embed.0.layers.{j}")       # shared by all decoder layers
        dt = torch.arange(128, dtype=torch.float32)
        w["dim_t"] = (10000 ** (2 * torch.div(dt, 2, rounding_mode="floor") / 128)).to(dev)
        # ---- text constants (image independent: caption is hard-coded "object.", InkLayer/detector/gdino.py:18)
        self._graphs = LRU(self.graph_cache_size)
        self._plans = LRU(self.plan_cache_size)
        self._seen: Dict[Tuple[int, int, int], int] = {}
        self._captions = LRU(self.caption_cache_size)          # tuple(ids) -> encoded_text on the host (set_caption)
        self.text_weights: Optional[Dict[str, torch.Tensor]] = None   # the checkpoint's bert.* / feat_map.* (host)
        self.set_text(encoded_text, token_ids)

    @classmethod
    def text_state_only(cls, cfg: Optional[GDinoConfig] = None, device: str | torch.device = "cpu") -> "GDinoEngine":
        """An engine with no weights: everything set_text / set_caption read and write, on `device` (the CPU by default).
        For the host-side checks of caption handling; it cannot run a forward."""
        eng = cls.__new__(cls)
        eng.cfg, eng.dev, eng.w = cfg or GDinoConfig(), torch.device(device), {}
        eng._graphs, eng._plans, eng._seen = LRU(cls.graph_cache_size), LRU(cls.plan_cache_size), {}
        eng._captions, eng.text_weights = LRU(cls.caption_cache_size), None
        return eng

    def set_text(self, encoded_text: Optional[torch.Tensor], token_ids: Sequence[int]) -> None:
        """encoded_text = feat_map(BERT(caption)) [T, 256] (groundingdino.py:277-279), a constant of the caption.
        T <= cfg.max_text_len (256); a longer id list is truncated to that first, as groundingdino.py:259-266 does (a
        phrase the cut runs through is left without its closing separator, so its tokens see only themselves).  This
        is the SHARED-caption form: one caption for every image of a batch, the folded T <= 4 path and graphs
        included.  A batch with one caption per image is set_captions' per-image form; set_text / set_caption leave
        it and clear its state.  Plans stay (they do not depend on the text); captured graphs are dropped."""
        if encoded_text is None:
            raise ValueError("encoded_text [T,256] is required: fold BERT + feat_map once at load "
                             "(inklayer_amd.text_branch) or pass precomputed features")
        assert encoded_text.shape[0] == len(token_ids), "one feature row per token id"
        token_ids = list(token_ids)[:self.cfg.max_text_len]      # groundingdino.py:259-266
        encoded_text = encoded_text[:self.cfg.max_text_len]
        T = len(token_ids)
        assert T >= 1
        self._graphs.clear()                           # captured forwards hold the old text tensors
        self._seen.clear()
        self.captions = self.t_lens = self.t_len = self.Tmax = self.text_position_ids = None   # per-image form off
        self.T = T
        self.token_ids = tuple(int(t) for t in token_ids)
        # dispatch on T alone: _enc_layer folds <= 4 tokens through the fusion layer and runs the general kernel
        # (csrc/biattn_wide.hip) otherwise; the text attentions keep their scores in registers up to 16 keys
        # (csrc/attn_few.hip)
        self._text_attn = ops.attn_fewkeys if T <= 16 else ops.attn_midkeys
        self.text0 = encoded_text.detach().to(self.dev, F32).contiguous()
        self._captions.put(self.token_ids, encoded_text.detach().to("cpu", F32))    # set_caption finds it again
        # ContrastiveEmbed's GEMM writes N % 4 == 0 columns: T is padded with zero text rows whose bias is -inf
        self.Tc, self.logit_bias = -(-T // 4) * 4, None
        if self.Tc != T:
            self.logit_bias = torch.zeros(self.Tc, dtype=F32)
            self.logit_bias[T:] = float("-inf")
            self.logit_bias = self.logit_bias.to(self.dev)
        sm, pid = text_masks_and_position_ids(token_ids)
        self.text_blocked = (~sm).to(torch.uint8).to(self.dev).contiguous()
        dim_t = torch.arange(256, dtype=torch.float32)
        dim_t = 10000.0 ** (2 * torch.div(dim_t, 2, rounding_mode="floor") / 256)
        self.pos_text = _interleaved_sincos(pid.float()[:, None] * (2 * math.pi) / dim_t).to(self.dev).contiguous()

    caption_cache_size = 8
    tokenizer = None         # anything with decode(ids) -> str (inklayer_amd.wordpiece.WordPiece): predict's phrases as text

    text_encoder = "auto"    # where BERT + feat_map of a caption run: "gpu" (inklayer_amd/text_encoder.py: every missing
    #                          caption of a call in ONE pass on the library's kernels), "host" (text_branch.py: f32 torch
    #                          on the CPU, one caption at a time) or "auto": the GPU encoder where the engine is on a GPU,
    #                          text_weights holds a 768-wide BERT and the library is built, the host fold otherwise
    _text_enc = None         # the BertTextEncoder of text_weights: built on the first miss, dropped with them

    def set_caption(self, token_ids: Sequence[int], sd: Optional[Dict[str, torch.Tensor]] = None,
                    encoded_text: Optional[torch.Tensor] = None) -> None:
        """Switch the engine to the caption with these token ids ([CLS] ... [SEP], at most cfg.max_text_len are kept).
        Its text features are encoded_text [T, 256] where given, else feat_map(BERT(ids)) from the checkpoint's bert.* /
        feat_map.* tensors (sd is remembered from the first call that passes one), on the GPU encoder or folded on the
        host as `text_encoder` says - once per caption: the last `caption_cache_size` captions are kept, as host
        copies.  The shared-caption form, see set_text; set_captions takes one caption per image."""
        ids = tuple(int(t) for t in token_ids)[:self.cfg.max_text_len]
        self._take_text_weights(sd)
        self.set_text(self._captions_features([ids], [encoded_text])[0], ids)

    def _take_text_weights(self, sd: Optional[Dict[str, torch.Tensor]]) -> None:
        if sd is not None:
            sd = clean_state_dict(sd)
            self.text_weights = {k: v for k, v in sd.items() if k.startswith(("bert.", "feat_map."))}
            self._captions.clear()                          # features folded from another checkpoint
            self.release_text_encoder()                     # ... and an encoder built from it

    def release_text_encoder(self) -> None:
        """Drop the GPU text encoder (about 0.6 GB for BERT-base); the next caption that misses the cache builds it
        again from text_weights."""
        self._text_enc = None

    def _gpu_text(self) -> bool:
        """Does a cache miss go to the GPU encoder?  (text_encoder, see there.)"""
        mode = self.text_encoder
        if mode not in ("auto", "gpu", "host"):
            raise ValueError(f'text_encoder is "auto", "gpu" or "host", not {mode!r}')
        if mode == "gpu" and self.dev.type != "cuda":
            raise ValueError('text_encoder = "gpu" needs an engine on a GPU; this one is on ' + str(self.dev))
        if mode == "host" or self.dev.type != "cuda":
            return False
        from . import _lib
        from .text_encoder import HIDDEN, bert_hidden_size
        able = bool(self.text_weights) and bert_hidden_size(self.text_weights) == HIDDEN and _lib.lib_path().exists()
        if mode == "gpu" and not able:
            raise ValueError('text_encoder = "gpu" needs the built library and a state dict with a 768-wide bert.*')
        return able

    def _captions_features(self, caps: Sequence[Tuple[int, ...]],
                           encoded_texts: Sequence[Optional[torch.Tensor]]) -> List[torch.Tensor]:
        """[len(ids), 256] text features of every (already truncated) caption: the given ones, the cache's, or BERT's.
        The captions found in neither are encoded together, each distinct one once."""
        gpu = self._gpu_text()
        feats = [f if f is not None else self._captions.get(ids) for ids, f in zip(caps, encoded_texts)]
        missing = list(dict.fromkeys(ids for ids, f in zip(caps, feats) if f is None))
        if missing:
            if not self.text_weights:
                raise ValueError("set_caption needs encoded_text [T, 256] or a state dict with the checkpoint's bert.* "
                                 "and feat_map.* tensors")
            if gpu:
                if self._text_enc is None:
                    from .text_encoder import BertTextEncoder
                    self._text_enc = BertTextEncoder(self.text_weights, self.dev)
                new = [f.to("cpu", F32) for f in self._text_enc.encode(missing)]
            else:
                from .text_branch import encode_caption_from_checkpoint
                new = [encode_caption_from_checkpoint(self.text_weights, ids) for ids in missing]
            new = dict(zip(missing, new))
            feats = [f if f is not None else new[ids] for ids, f in zip(caps, feats)]
        return [f[:len(ids)] for ids, f in zip(caps, feats)]

    def set_captions(self, token_id_lists: Sequence[Sequence[int]], sd: Optional[Dict[str, torch.Tensor]] = None,
                     encoded_texts: Optional[Sequence[Optional[torch.Tensor]]] = None) -> None:
        """One caption PER IMAGE of the next batch (GroundingDINO.forward with a list of captions,
        groundingdino.py:243-279): token_id_lists[i] belongs to image i of the next forward / predict, each truncated
        to cfg.max_text_len; features from encoded_texts[i], the caption cache or BERT, as set_caption finds them (the
        captions that miss both are encoded in one pass, equal ones once).  Equal captions are the shared form: set_caption and its paths, bit for bit.
        Otherwise the engine enters the per-image form, the reference's padding="longest" batch with Tmax = max T_b:
          text0 [B*Tmax, 256] (pad rows zero), t_len int32 [B] on the device, text_blocked u8 [B, Tmax, Tmax] (each
          caption's block-diagonal mask in the corner; pad rows and columns blocked except the diagonal, which is what
          bertwarper.py's generate_masks_with_special_tokens_and_transfer_map gives for pad ids - the key count removes
          the pad keys anyway), pos_text [B*Tmax, 256] (position id 0 at pads; the ids are text_position_ids),
          logit_bias [B, Tc] (-inf at t >= T_b; Tc = 4 ceil(Tmax / 4)).
        A forward in this form runs eager on ops.biattn_wide_varlen / ops.attn_midkeys_varlen: every image pays for
        its own token count, and its results are those of its caption alone (text_token_mask of the reference:
        fuse_modules.py:214-218, transformer.py:903-909, utils.py:259-262)."""
        caps = [tuple(int(t) for t in ids)[:self.cfg.max_text_len] for ids in token_id_lists]
        if not caps or any(len(c) < 1 for c in caps):
            raise ValueError("set_captions needs at least one caption, each of at least one token id")
        if encoded_texts is not None and len(encoded_texts) != len(caps):
            raise ValueError("one encoded_text (or None) per caption")
        feats_in = list(encoded_texts) if encoded_texts is not None else [None] * len(caps)
        if len(set(caps)) == 1:
            return self.set_caption(caps[0], sd=sd, encoded_text=feats_in[0])
        self._take_text_weights(sd)
        feats = [f.detach().to("cpu", F32) for f in self._captions_features(caps, feats_in)]
        for ids, f in zip(caps, feats):
            assert f.shape[0] == len(ids), "one feature row per token id"
            self._captions.put(ids, f)
        B, Tmax = len(caps), max(len(c) for c in caps)
        self._graphs.clear()                           # captured forwards hold the old text tensors
        self._seen.clear()
        self.T = self.token_ids = self._text_attn = None     # the shared form's state: a use of it is an error
        self.captions, self.t_lens, self.Tmax, self.Tc = tuple(caps), tuple(len(c) for c in caps), Tmax, -(-Tmax // 4) * 4
        text0 = torch.zeros(B, Tmax, 256, dtype=F32)
        blocked = ~torch.eye(Tmax, dtype=torch.bool).repeat(B, 1, 1)
        pid = torch.zeros(B, Tmax, dtype=torch.long)
        bias = torch.zeros(B, self.Tc, dtype=F32)
        for b, (ids, f) in enumerate(zip(caps, feats)):
            n = len(ids)
            sm, p = text_masks_and_position_ids(ids)
            text0[b, :n], blocked[b, :n, :n], pid[b, :n] = f, ~sm, p
            bias[b, n:] = float("-inf")
        self.text_position_ids = pid
        self.text0 = text0.view(B * Tmax, 256).to(self.dev).contiguous()
        self.t_len = torch.tensor(self.t_lens, dtype=I32).to(self.dev)
        self.text_blocked = blocked.to(torch.uint8).to(self.dev).contiguous()
        dim_t = torch.arange(256, dtype=torch.float32)
        dim_t = 10000.0 ** (2 * torch.div(dim_t, 2, rounding_mode="floor") / 256)
        self.pos_text = _interleaved_sincos(pid.view(-1).float()[:, None] * (2 * math.pi) / dim_t).to(self.dev).contiguous()
        self.logit_bias = bias.to(self.dev)

    def predict(self, images_u8: Sequence[torch.Tensor], box_threshold: float, text_threshold: float,
                remove_combined: bool = False):
        """predict (GD/util/inference.py:70-97) per image for the engine's caption: [(boxes [n, 4] cxcywh, scores [n],
        phrases)] with the boxes whose best token probability exceeds box_threshold; phrases as phrases_from_probs
        forms them (strings with self.tokenizer set, id tuples without)."""
        logits, boxes = self.forward(images_u8)
        both = torch.cat([logits, boxes], dim=-1).cpu()       # single D2H copy
        TL, res = logits.shape[-1], []                        # T, or Tmax in the per-image form
        for b in range(both.shape[0]):
            # the per-image form slices image b's own T_b columns and forms the phrases from its own ids
            T, ids = (self.T, self.token_ids) if self.captions is None else (self.t_lens[b], self.captions[b])
            prob = both[b, :, :T].contiguous().sigmoid()      # dense [nq, T], as the reference's `.cpu().sigmoid()[0]`
            keep = prob.max(dim=1)[0] > box_threshold
            kept = prob[keep]
            phrases = phrases_from_probs(kept, ids, text_threshold, remove_combined, self.tokenizer)
            res.append((both[b, keep, TL:], kept.max(dim=1)[0] if len(kept) else kept.new_zeros(0), phrases))
        return res

    # ------------------------------------------------------------------ closed-set scoring (csrc/closed_set.hip)
    def _positive_maps(self, positive_maps, B: int):
        """positive_maps for a forward of B images -> (map f32 on the device, [C, T] shared or [B, Cmax, T] per image;
        n_cls int32 [B] on the device or None; class counts).  ONE map [C, >= T] (a tensor) scores every image against
        the same classes and needs the shared-caption form; a LIST of B maps [C_b, >= T_b] gives image b its own.  Maps
        as wide as max_text_len (closed_set.positive_map_from_spans) are cut to the caption's T columns; a map that is
        non-zero beyond its caption's tokens belongs to another caption: ValueError."""
        T = self.T if self.captions is None else self.Tmax
        t_of = [self.T] * B if self.captions is None else list(self.t_lens)

        def cut(pm, Tb):
            pm = torch.as_tensor(pm, dtype=F32).detach().cpu()
            if pm.dim() != 2 or pm.shape[0] < 1 or pm.shape[1] < Tb:
                raise ValueError(f"a positive map is [C >= 1, >= {Tb} token columns], not {tuple(pm.shape)}")
            if bool((pm[:, Tb:] != 0).any()):
                raise ValueError(f"a positive map marks tokens beyond its caption's {Tb}: it was built for another caption")
            return pm[:, :Tb]

        if not isinstance(positive_maps, (list, tuple)):
            if self.captions is not None:
                raise ValueError("one positive map for all images needs one caption for all images (set_caption); after "
                                 "set_captions pass one map per image")
            pm = cut(positive_maps, self.T)
            return pm.contiguous().to(self.dev), None, [pm.shape[0]] * B
        if len(positive_maps) != B:
            raise ValueError(f"{len(positive_maps)} positive maps for {B} images")
        maps = [cut(pm, t_of[b]) for b, pm in enumerate(positive_maps)]
        counts = [m.shape[0] for m in maps]
        full = torch.zeros((B, max(counts), T), dtype=F32)
        for b, m in enumerate(maps):
            full[b, :m.shape[0], :m.shape[1]] = m
        return full.to(self.dev), torch.tensor(counts, dtype=I32).to(self.dev), counts

    def predict_classes(self, images_u8: Sequence[torch.Tensor], positive_maps, num_select: int = 300,
                        sizes: Optional[Sequence[Tuple[int, int]]] = None):
        """PostProcessCocoGrounding.forward (GD/demo/test_ap_on_coco.py:99-137) on the GPU: the score of (query, class) is
        sum_t sigmoid(logit[q, t]) * positive_map[c, t]; per image the num_select best pairs, best first (ties: the
        lower query, then the lower class).  -> [(boxes xyxy f32 [k, 4], scores f32 [k], labels int64 [k])] with
        k = min(num_select, nq * C_b); boxes in the pixels of sizes[b] = (h, w), normalised without sizes.
        positive_maps: see _positive_maps.  Scores, selection and box conversion stay on the device; ONE copy of
        [B, K, 6] (score, label, box) comes back."""
        B, nq = len(images_u8), self.cfg.num_queries
        pm, n_cls, counts = self._positive_maps(positive_maps, B)
        if num_select < 1:
            raise ValueError("num_select >= 1")
        if sizes is not None and len(sizes) != B:
            raise ValueError(f"{len(sizes)} sizes for {B} images")
        Cmax = pm.shape[-2]
        K = min(int(num_select), nq * Cmax)
        nchunk = -(-(nq * Cmax) // 16384)               # ops.topk_rowmax's chunked form: every chunk holds K, the merge nchunk * K
        if nchunk > 1 and (nchunk * K > 16384 or (nq * Cmax) // nchunk < K):
            raise ValueError(f"num_select = {num_select} of {nq * Cmax} (query, class) pairs is more than the selection "
                             f"kernel merges ({16384 // nchunk} here)")
        scale = torch.ones((B, 2), dtype=F32) if sizes is None else \
            torch.tensor([[float(w_), float(h)] for h, w_ in sizes], dtype=F32)
        logits, boxes = self.forward(images_u8)
        prob = ops.class_scores(logits, pm, n_cls)
        idx, val = ops.topk_rowmax(prob.view(B, nq * Cmax, 1), K, want_values=True)
        xyxy, labels, _ = ops.select_boxes(idx, boxes.contiguous(), scale.to(self.dev), Cmax)
        out = torch.cat([val[..., None], labels.to(F32)[..., None], xyxy], dim=-1).cpu()       # single D2H copy
        res = []
        for b in range(B):
            k = min(K, nq * counts[b])                  # classes c >= C_b score -1 and sort behind every real pair
            res.append((out[b, :k, 2:].contiguous(), out[b, :k, 0].contiguous(), out[b, :k, 1].to(torch.int64)))
        return res

    def predict_spans(self, images_u8: Sequence[torch.Tensor], positive_maps, box_threshold: float):
        """The given-phrase mode of GD/demo/inference_on_a_image.py:117-142: per image, for every phrase (a row of its
        positive map) the queries whose phrase score sum_t sigmoid(logit[q, t]) * positive_map[p, t] exceeds
        box_threshold, in phrase order, then query order, as the reference concatenates them.
        -> [(boxes cxcywh f32 [n, 4] normalised, scores f32 [n], phrase index int64 [n])]."""
        B = len(images_u8)
        pm, n_cls, counts = self._positive_maps(positive_maps, B)
        logits, boxes = self.forward(images_u8)
        prob = ops.class_scores(logits, pm, n_cls)
        both = torch.cat([prob, boxes], dim=-1).cpu()         # single D2H copy
        P, res = prob.shape[-1], []
        for b in range(B):
            bx, sc, ph = [], [], []
            for p in range(counts[b]):
                keep = both[b, :, p] > box_threshold
                bx.append(both[b, keep, P:])
                sc.append(both[b, keep, p])
                ph.append(torch.full((int(keep.sum()),), p, dtype=torch.int64))
            res.append((torch.cat(bx), torch.cat(sc), torch.cat(ph)))
        return res

    # ------------------------------------------------------------------ HIP graphs (latency mode)
    # At batch 1 the forward is ~600 small launches whose dependency chain is launch-latency-bound: 11.4 ms eager
    # vs 6.4 ms as a graph replay on MI355X (tools/latency_b1.py); at batch 8 the GPU work dominates and a graph
    # changes nothing.  So forwards of at most `graph_max_batch` equal-size images are captured once per
    # (h, w, B) into a torch.cuda.CUDAGraph with static input/output buffers and replayed afterwards.
    # A replay does not overlap with eager work on another stream (measured: the two-stream pipeline got slower,
    # 16.6 -> 18.5 ms at batch 1), so InkLayerPipeline's overlapped mode passes allow_graph=False; the graph serves
    # the sequential use of the detector (run_ft_dino_on_sketch / detect), which is how the reference runs it.
    # A capture costs two eager warm-ups + the capture (~3 forwards) and pins a private memory pool, so a size is
    # captured only when it is seen the SECOND time, and at most `graph_cache_size` graphs (LRU) are kept: a directory
    # of sketches with many aspect ratios runs eager and HBM stays bounded (tests/test_gdino_gpu.py).
    graph_max_batch = 1
    graph_cache_size = 4
    plan_cache_size = 8

    def _forward_graphed(self, images_u8: Sequence[torch.Tensor], h: int, w_: int):
        B = len(images_u8)
        key = (h, w_, B)
        g = self._graphs.get(key)
        if g is None:
            self._seen[key] = self._seen.get(key, 0) + 1
            if len(self._seen) > 4096:
                self._seen.clear()
            if self._seen[key] < 2:
                return self._forward_eager(images_u8)
            static_in = [torch.empty_like(im) for im in images_u8]
            for dst, src in zip(static_in, images_u8):
                dst.copy_(src)
            side = torch.cuda.Stream(device=self.dev)
            side.wait_stream(torch.cuda.current_stream(self.dev))
            with torch.cuda.stream(side):                 # warm-up off the capture: lazy attribute calls, pools, plans
                for _ in range(2):
                    self._forward_eager(static_in)
            torch.cuda.current_stream(self.dev).wait_stream(side)
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                out = self._forward_eager(static_in)
            g = (graph, static_in, out, self.plan(h, w_, B))   # the graph's kernels read its plan's buffers
            self._graphs.put(key, g)
        graph, static_in, out = g[:3]
        for dst, src in zip(static_in, images_u8):
            dst.copy_(src)
        graph.replay()
        return out[0].clone(), out[1].clone()            # the static outputs are overwritten by the next replay

    def plan(self, h: int, w: int, B: int) -> _Plan:
        return self._plans.get_or_make((h, w, B), lambda: _Plan(self, h, w, B))

    # ------------------------------------------------------------------ pieces
    def _mlp3(self, prefix: str, x16: torch.Tensor) -> torch.Tensor:
        w = self.w
        a = ops.gemm(x16, w[prefix + "0.w"], w[prefix + "0.b"], act="relu", out_dtype=F16)
        a = ops.gemm(a, w[prefix + "1.w"], w[prefix + "1.b"], act="relu", out_dtype=F16)
        return ops.gemm(a, w[prefix + "2.w"], w[prefix + "2.b"])

    def _swin_block(self, x: torch.Tensor, i: int, b: int, pl: _Plan) -> None:
        """Block b of Swin stage i (SwinTransformerBlock.forward, swin_transformer.py:238-298) on the f32 tokens
        x [B*H*W, C] of that stage, in place."""
        cfg, w = self.cfg, self.w
        C, nh, nW = cfg.embed_dim * 2 ** i, cfg.num_heads[i], pl.nW[i]
        d = f"s{i}b{b}"
        shifted = b % 2 == 1
        wm = pl.win_map[i][1 if shifted else 0]
        y = ops.layernorm_rows(x, w[d + ".norm1.w"], w[d + ".norm1.b"], 1e-5, gather=wm)
        qkv = ops.gemm(y, w[d + ".qkv.w"], w[d + ".qkv.b"], out_dtype=F16)
        ws, scale = cfg.window_size, HEAD_DIM ** -0.5
        if ws == 7:
            o = ops.flash_attn(qkv[:, :C], qkv[:, C:2 * C], qkv[:, 2 * C:], n_batch=pl.B * nW, n_heads=nh,
                               head_dim=HEAD_DIM, scale=scale, n_q=ws * ws, n_k=ws * ws, dense_bias=w[d + ".bias"],
                               dense_mask=pl.shift_mask[i] if shifted else None)
        else:
            o = ops.swin_attn(qkv[:, :C], qkv[:, C:2 * C], qkv[:, 2 * C:], n_windows=pl.B * nW, n_heads=nh, ws=ws,
                              scale=scale, bias_table=w[d + ".table"], region=pl.region[i] if shifted else None, nW=nW)
        ops.gemm(o, w[d + ".proj.w"], w[d + ".proj.b"], residual=x, row_map=wm, out=x)
        y = ops.layernorm_rows(x, w[d + ".norm2.w"], w[d + ".norm2.b"], 1e-5)
        hmid = ops.gemm(y, w[d + ".fc1.w"], w[d + ".fc1.b"], act="gelu", out_dtype=F16)
        ops.gemm(hmid, w[d + ".fc2.w"], w[d + ".fc2.b"], residual=x, out=x)

    def backbone(self, images_u8: Sequence[torch.Tensor], pl: _Plan) -> Dict[int, Tuple[torch.Tensor, torch.Tensor]]:
        """Swin-T (swin_transformer.py:712-754): {stage: (f32 tokens, f16 tokens)} after norm{i}."""
        cfg, w, dev = self.cfg, self.w, self.dev
        B = len(images_u8)
        H0, W0 = pl.stage_hw[0]
        T0 = H0 * W0
        patches = torch.empty((B * T0, 64), device=dev, dtype=F16)
        for b, img in enumerate(images_u8):
            ops.swin_patchify(img, cfg.pixel_mean, cfg.pixel_std, patches[b * T0:(b + 1) * T0])
        x = ops.gemm(patches, w["pe.w"], w["pe.b"])
        x = ops.layernorm_rows(x, w["pe.norm.w"], w["pe.norm.b"], 1e-5, out_dtype=F32)
        outs = {}
        for i, dep in enumerate(cfg.depths):
            for b in range(dep):
                self._swin_block(x, i, b, pl)
            if i in cfg.out_indices:
                o32 = torch.empty_like(x)
                o16 = torch.empty(x.shape, device=dev, dtype=F16)
                ops.layernorm_rows(x, w[f"s{i}.outnorm.w"], w[f"s{i}.outnorm.b"], 1e-5, out=o32, out2=o16)
                outs[i] = (o32, o16)
            if i < len(cfg.depths) - 1:
                m = ops.layernorm_merge4(x, w[f"s{i}.merge.norm.w"], w[f"s{i}.merge.norm.b"], 1e-5, pl.merge_map[i])
                x = ops.gemm(m, w[f"s{i}.merge.w"])
        return outs

    def neck(self, feats, pl: _Plan, B: int) -> torch.Tensor:
        """input_proj (groundingdino.py:305-324) -> flattened multi-scale source [B*S, 256] f32."""
        cfg, w, dev = self.cfg, self.w, self.dev
        S = pl.S
        src = torch.empty((B * S, 256), device=dev, dtype=F32)
        nfeat = len(cfg.out_indices)
        for l in range(cfg.num_feature_levels):
            hh, ww = pl.shapes[l]
            Tl = hh * ww
            if l < nfeat:
                a16 = feats[cfg.out_indices[l]][1]
            else:
                f32_last = feats[cfg.out_indices[-1]][0]
                T3 = pl.shapes[nfeat - 1][0] * pl.shapes[nfeat - 1][1]
                col = ops.gather_rows(f32_last, pl.lvl4_map, B, Tl * 9, x_batch_rows=T3, idx_batch_stride=0)
                a16 = col.view(B * Tl, -1)
            y = ops.gemm(a16, w[f"ip{l}.w"], w[f"ip{l}.b"])
            ops.groupnorm_nhwc(y, B, Tl, 32, w[f"ip{l}.gn.w"], w[f"ip{l}.gn.b"], 1e-5,
                               src[pl.level_start[l]:], S * 256)
        return src

    def encoder(self, src: torch.Tensor, pl: _Plan, B: int):
        """TransformerEncoder.forward (transformer.py:481-595): fusion -> text layer -> deformable layer, x6."""
        S = pl.S
        tb = self._tb
        text = self.text0.repeat(B, 1) if tb is None else tb.text0.clone()    # [B*T, 256] (plumbing copy)
        s16 = torch.empty((B * S, 256), device=self.dev, dtype=F16)
        s16p = torch.empty((B * S, 256), device=self.dev, dtype=F16)
        for i in range(self.cfg.enc_layers):
            src, text = self._enc_layer(i, src, text, pl, B, s16, s16p)
        return src, text

    def _enc_layer(self, i: int, src: torch.Tensor, text: torch.Tensor, pl: _Plan, B: int, s16: torch.Tensor,
                   s16p: torch.Tensor):
        """Encoder layer i: fusion, text enhancer, deformable layer on src [B*S, 256] f32 (updated in place on the
        product path) and text [B*T, 256] f32; s16 / s16p are the [B*S, 256] f16 operand buffers every layer re-uses.
        Returns (src, text)."""
        w, dev, T, S, tb = self.w, self.dev, self.T, pl.S, self._tb
        d = f"e{i}"
        have16 = False
        # --- BiAttentionBlock (fuse_modules.py:286-295): residual from the NORMALISED v / l
        ln32 = torch.empty_like(text)
        l16 = torch.empty(text.shape, device=dev, dtype=F16)
        ops.layernorm_rows(text, w[d + ".fu.lnl.w"], w[d + ".fu.lnl.b"], 1e-5, out=ln32, out2=l16)
        if tb is None and self.fold_fusion and T <= 4:
            # the caption's <= 4 tokens folded through the fusion layer (csrc/fusion_fold.hip): no per-token
            # 256 -> 2048 projection, no 1024 -> 256 image output projection, f32 throughout
            kl = ops.gemm(l16, w[d + ".fu.kl.w"], w[d + ".fu.kl.b"])
            # ... and the f16 operands of this layer's deformable attention (x + pos, x) leave in the same pass
            ol = ops.fusion_fold(src, B, S, w[d + ".fu.lnv.w"], w[d + ".fu.lnv.b"], 1e-5, kl, T, w[d + ".fu.qv.w"],
                                 w[d + ".fu.qv.b"], w[d + ".fu.outv.w"], w[d + ".fu.outv.b"], w[d + ".fu.gv"],
                                 256 ** -0.5, pos=pl.pos, out16_pos=s16p, out16=s16)
            have16 = True
        else:
            vn = torch.empty_like(src)
            ops.layernorm_rows(src, w[d + ".fu.lnv.w"], w[d + ".fu.lnv.b"], 1e-5, out=vn, out2=s16)
            qv = ops.gemm(s16, w[d + ".fu.qv.w"], w[d + ".fu.qv.b"], out_dtype=F16)
            kl = ops.gemm(l16, w[d + ".fu.kl.w"], w[d + ".fu.kl.b"], out_dtype=F16)
            if tb is None:
                ov, ol = ops.biattn_wide(qv, kl, B, S, T, 256 ** -0.5)
            else:   # per-image token counts: pad rows of kl are never read, pad rows of ol come back as zeros
                ov, ol = ops.biattn_wide_varlen(qv, kl, B, S, tb.Tmax, tb.t_len, 256 ** -0.5)
            src = ops.gemm(ov, w[d + ".fu.outv.w"], w[d + ".fu.outv.b"], col_scale=w[d + ".fu.gv"], residual=vn, out=vn)
        text = ops.gemm(ol, w[d + ".fu.outl.w"], w[d + ".fu.outl.b"], col_scale=w[d + ".fu.gl"], residual=ln32)
        # --- text enhancer (transformer_vanilla.py:101-123), 4 heads x 64, block-diagonal mask
        qk = ops.gemm(ops.add_cvt_f16(text, self.pos_text if tb is None else tb.pos_text), w[d + ".txt.qk.w"],
                      w[d + ".txt.qk.b"], out_dtype=F16)
        vv = ops.gemm(ops.add_cvt_f16(text), w[d + ".txt.v.w"], w[d + ".txt.v.b"], out_dtype=F16)
        if tb is None:
            a = self._text_attn(qk[:, :256], qk[:, 256:], vv, B=B, n_heads=4, head_dim=64, scale=64 ** -0.5,
                                blocked=self.text_blocked)
        else:       # each image's own mask and key count; a pad row has no key and gives zeros
            a = ops.attn_midkeys_varlen(qk[:, :256], qk[:, 256:], vv, B=B, n_heads=4, head_dim=64, scale=64 ** -0.5,
                                        blocked=tb.blocked, k_len=tb.t_len)
        text = ops.layernorm_rows(ops.gemm(a, w[d + ".txt.out.w"], w[d + ".txt.out.b"], residual=text),
                                  w[d + ".txt.norm1.w"], w[d + ".txt.norm1.b"], 1e-5, out_dtype=F32)
        ff = ops.gemm(ops.add_cvt_f16(text), w[d + ".txt.lin1.w"], w[d + ".txt.lin1.b"], act="relu", out_dtype=F16)
        text = ops.layernorm_rows(ops.gemm(ff, w[d + ".txt.lin2.w"], w[d + ".txt.lin2.b"], residual=text),
                                  w[d + ".txt.norm2.w"], w[d + ".txt.norm2.b"], 1e-5, out_dtype=F32)
        # --- DeformableTransformerEncoderLayer (transformer.py:780-799)
        if have16:
            proj = ops.gemm(s16p, w[d + ".msda.proj.w"], w[d + ".msda.proj.b"])
            val = ops.gemm(s16, w[d + ".msda.value.w"], w[d + ".msda.value.b"], out_dtype=F16)
        else:
            proj = ops.gemm(ops.add_cvt_f16(src, pl.pos, out=s16), w[d + ".msda.proj.w"], w[d + ".msda.proj.b"])
            val = ops.gemm(ops.add_cvt_f16(src, out=s16), w[d + ".msda.value.w"], w[d + ".msda.value.b"], out_dtype=F16)
        o = ops.msda_fused(val, proj, pl.enc_ref, pl.shapes, B, S, ref_batched=False)
        if self.fuse_ffn and self.fuse_ffn_pre and (d + ".ffn.blob_pre") in w:
            # out_proj + residual + norm1 + linear1 + relu + linear2 + residual + norm2: one kernel, `src` read and
            # written once
            ops.ffn256_fused(o, src, w[d + ".ffn.blob_pre"], int(w[d + ".lin1.b"].numel()), w[d + ".lin2.b"],
                             w[d + ".norm2.w"], w[d + ".norm2.b"], 1e-5, out=src,
                             pre=(w[d + ".msda.out.b"], w[d + ".norm1.w"], w[d + ".norm1.b"]))
            return src, text
        y = ops.gemm(o, w[d + ".msda.out.w"], w[d + ".msda.out.b"], residual=src, out=src)
        ops.layernorm_rows(y, w[d + ".norm1.w"], w[d + ".norm1.b"], 1e-5, out=src, out2=s16)
        if self.fuse_ffn and (d + ".ffn.blob") in w:
            # linear1 + relu + linear2 + residual + norm2 in one kernel: the [B*S, 2048] hidden tensor stays in registers
            ops.ffn256_fused(s16, src, w[d + ".ffn.blob"], int(w[d + ".lin1.b"].numel()), w[d + ".lin2.b"],
                             w[d + ".norm2.w"], w[d + ".norm2.b"], 1e-5, out=src)
        else:
            ff = ops.gemm(s16, w[d + ".lin1.w"], w[d + ".lin1.b"], act="relu", out_dtype=F16)
            y = ops.gemm(ff, w[d + ".lin2.w"], w[d + ".lin2.b"], residual=src, out=src)
            ops.layernorm_rows(y, w[d + ".norm2.w"], w[d + ".norm2.b"], 1e-5, out=src)
        return src, text

    def decoder(self, memory: torch.Tensor, text: torch.Tensor, pl: _Plan, B: int, stages: Optional[dict] = None):
        """Two-stage selection + TransformerDecoder + heads (transformer.py:284-327, 665-735;
        groundingdino.py:331-349).  Returns (logits [B,nq,T], boxes [B,nq,4]) f32 on the GPU."""
        cfg, w, dev, S, nq, tb = self.cfg, self.w, self.dev, pl.S, self.cfg.num_queries, self._tb
        T = self.T if tb is None else tb.Tmax                # per-image form: Tmax columns, bias row b = -inf at t >= T_b
        om16 = ops.gather_rows(memory, pl.valid_map, B, S, x_batch_rows=S, idx_batch_stride=0)
        om = ops.gemm(om16, w["enc_output.w"], w["enc_output.b"])
        omn16 = torch.empty((B * S, 256), device=dev, dtype=F16)
        omn = ops.layernorm_rows(om, w["enc_output_norm.w"], w["enc_output_norm.b"], 1e-5, out=om, out2=omn16)
        text16 = ops.add_cvt_f16(text)
        Tc, tw16 = (self.Tc if tb is None else tb.Tc), text16
        tbias = [self.logit_bias] * B if tb is None else list(tb.bias.unbind(0))
        if Tc != T:          # zero text rows with bias -inf (set_text): a pad column is never a row's maximum
            tw16 = torch.zeros((B, Tc, 256), device=dev, dtype=F16)
            tw16[:, :T] = text16.view(B, T, 256)
            tw16 = tw16.view(B * Tc, 256)
        logits = torch.empty((B, S, Tc), device=dev, dtype=F32)
        for b in range(B):   # ContrastiveEmbed: per-image "weights" = that image's text features
            ops.gemm(omn16[b * S:(b + 1) * S], tw16[b * Tc:(b + 1) * Tc], tbias[b], out=logits[b])
        idx = ops.topk_rowmax(logits, nq)
        if stages is not None:
            stages["topk_logits"] = logits if Tc == T else logits[:, :, :T]
            if "force_topk" in stages:                       # test hook: isolate the decoder from tie order
                idx = stages["force_topk"].to(I32).to(dev).contiguous()
        sel16 = ops.gather_rows(omn, idx, B, nq, x_batch_rows=S, idx_batch_stride=nq)
        delta = self._mlp3("encbox", sel16)
        prop = ops.gather_rows(pl.props_unsig, idx, B, nq, x_batch_rows=0, idx_batch_stride=nq, out_dtype=F32)
        ref = ops.box_refine(delta, prop, ref_is_logit=True)                     # sigmoid(delta + proposal)
        if stages is not None:
            stages["topk"], stages["ref0"] = idx, ref
        output = w["tgt"].repeat(B, 1)                       # embed_init_tgt (transformer.py:318-321)
        mem16 = ops.add_cvt_f16(memory)
        hs16 = None
        if stages is not None:
            stages["hs"], stages["refs"] = [], [ref.clone()]
        for i in range(cfg.dec_layers):
            output = self._dec_layer(i, output, ref, mem16, text16, pl, B)
            if stages is not None:                           # BEFORE dec.norm (the oracle's stages["hs"] are after it)
                stages["hs"].append(output.clone())
            if i < cfg.dec_layers - 1:
                ref = ops.box_refine(self._mlp3("box", ops.add_cvt_f16(output)), ref)
                if stages is not None:
                    stages["refs"].append(ref.clone())
            else:
                if stages is not None:                       # the oracle's refs[-1]: refined, never used
                    stages["refs"].append(ops.box_refine(self._mlp3("box", ops.add_cvt_f16(output)), ref))
                hs16 = ops.layernorm_rows(output, w["dec.norm.w"], w["dec.norm.b"], 1e-5)
        boxes = ops.box_refine(self._mlp3("box", hs16), ref).view(B, nq, 4)
        out_logits = torch.empty((B, nq, Tc), device=dev, dtype=F32)
        for b in range(B):
            ops.gemm(hs16[b * nq:(b + 1) * nq], tw16[b * Tc:(b + 1) * Tc], tbias[b], out=out_logits[b])
        return (out_logits if Tc == T else out_logits[:, :, :T]), boxes

    def _dec_layer(self, i: int, output: torch.Tensor, ref: torch.Tensor, mem16: torch.Tensor, text16: torch.Tensor,
                   pl: _Plan, B: int) -> torch.Tensor:
        """Decoder layer i (transformer.py:868-927) on the f32 queries output [B*nq, 256] with the sigmoided reference
        boxes ref [B*nq, 4], the f16 encoder memory [B*S, 256] and the f16 text rows [B*T, 256].  Returns the new
        f32 output (before decoder.norm and the box refinement)."""
        w = self.w
        nq = output.shape[0] // B
        d = f"d{i}"
        qse = ops.sine_embed4(ref, w["dim_t"])
        qpos = ops.gemm(ops.gemm(qse, w["rph0.w"], w["rph0.b"], act="relu", out_dtype=F16), w["rph1.w"], w["rph1.b"])
        # self-attention over the 900 queries
        qk = ops.gemm(ops.add_cvt_f16(output, qpos), w[d + ".sa.qk.w"], w[d + ".sa.qk.b"], out_dtype=F16)
        vv = ops.gemm(ops.add_cvt_f16(output), w[d + ".sa.v.w"], w[d + ".sa.v.b"], out_dtype=F16)
        a = ops.flash_attn(qk[:, :256], qk[:, 256:], vv, n_batch=B, n_heads=8, head_dim=32, scale=32 ** -0.5,
                           n_q=nq, n_k=nq)
        output = ops.layernorm_rows(ops.gemm(a, w[d + ".sa.out.w"], w[d + ".sa.out.b"], residual=output),
                                    w[d + ".norm2.w"], w[d + ".norm2.b"], 1e-5, out_dtype=F32)
        # text cross-attention (keys/values = the T text tokens)
        q = ops.gemm(ops.add_cvt_f16(output, qpos), w[d + ".ca.q.w"], w[d + ".ca.q.b"], out_dtype=F16)
        kv = ops.gemm(text16, w[d + ".ca.kv.w"], w[d + ".ca.kv.b"], out_dtype=F16)
        if self._tb is None:
            a = self._text_attn(q, kv[:, :256], kv[:, 256:], B=B, n_heads=8, head_dim=32, scale=32 ** -0.5)
        else:       # key_padding_mask (transformer.py:903-909): image b's keys end at its own token count
            a = ops.attn_midkeys_varlen(q, kv[:, :256], kv[:, 256:], B=B, n_heads=8, head_dim=32, scale=32 ** -0.5,
                                        k_len=self._tb.t_len)
        output = ops.layernorm_rows(ops.gemm(a, w[d + ".ca.out.w"], w[d + ".ca.out.b"], residual=output),
                                    w[d + ".canorm.w"], w[d + ".canorm.b"], 1e-5, out_dtype=F32)
        # deformable cross-attention into the encoder memory (4-d reference boxes)
        proj = ops.gemm(ops.add_cvt_f16(output, qpos), w[d + ".msda.proj.w"], w[d + ".msda.proj.b"])
        val = ops.gemm(mem16, w[d + ".msda.value.w"], w[d + ".msda.value.b"], out_dtype=F16)
        o = ops.msda_fused(val, proj, ref, pl.shapes, B, nq, ref_batched=True)
        output = ops.layernorm_rows(ops.gemm(o, w[d + ".msda.out.w"], w[d + ".msda.out.b"], residual=output),
                                    w[d + ".norm1.w"], w[d + ".norm1.b"], 1e-5, out_dtype=F32)
        ff = ops.gemm(ops.add_cvt_f16(output), w[d + ".lin1.w"], w[d + ".lin1.b"], act="relu", out_dtype=F16)
        output = ops.layernorm_rows(ops.gemm(ff, w[d + ".lin2.w"], w[d + ".lin2.b"], residual=output),
                                    w[d + ".norm3.w"], w[d + ".norm3.b"], 1e-5, out_dtype=F32)
        return output

    # ------------------------------------------------------------------ whole model
    def forward(self, images_u8: Sequence[torch.Tensor], stages: Optional[dict] = None, allow_graph: bool = True):
        """images_u8: resized HWC uint8 CUDA tensors.  -> (logits [B,nq,T], boxes [B,nq,4]) on the GPU.
        Images of different sizes are run as separate equal-size groups (the reference pads a NestedTensor
        instead; it only ever sees one image per call, GD/util/inference.py:67)."""
        B = len(images_u8)
        if self.captions is not None:
            return self._forward_captions(images_u8, stages)
        sizes = [tuple(im.shape[:2]) for im in images_u8]
        if len(set(sizes)) > 1:
            assert stages is None
            logits = torch.empty((B, self.cfg.num_queries, self.T), device=self.dev, dtype=F32)
            boxes = torch.empty((B, self.cfg.num_queries, 4), device=self.dev, dtype=F32)
            for sz in dict.fromkeys(sizes):
                idx = [i for i, s_ in enumerate(sizes) if s_ == sz]
                lg, bx = self.forward([images_u8[i] for i in idx], allow_graph=allow_graph)
                ii = torch.tensor(idx, device=self.dev)
                logits[ii] = lg
                boxes[ii] = bx
            return logits, boxes
        h, w_ = sizes[0]
        if allow_graph and stages is None and 0 < B <= self.graph_max_batch:
            return self._forward_graphed(images_u8, h, w_)
        return self._forward_eager(images_u8, stages)

    _tb: Optional["_TextBatch"] = None     # the per-image text state of the forward in flight (None: shared caption)

    def _forward_captions(self, images_u8: Sequence[torch.Tensor], stages: Optional[dict] = None):
        """forward in the per-image form (set_captions): caption i belongs to image i.  Eager, no graph.  Images of
        different sizes run as size groups, each with its own images' captions.  -> (logits [B, nq, Tmax] with -inf in
        each image's pad columns, as the reference returns -inf up to max_text_len; boxes [B, nq, 4])."""
        B = len(images_u8)
        if B != len(self.captions):
            raise ValueError(f"{B} images for {len(self.captions)} captions: set_captions takes one caption per image")
        sizes = [tuple(im.shape[:2]) for im in images_u8]
        groups = [[i for i, s_ in enumerate(sizes) if s_ == sz] for sz in dict.fromkeys(sizes)]
        Tmax = self.Tmax
        if len(groups) == 1:
            self._tb = _TextBatch(self.text0, self.t_len, self.text_blocked, self.pos_text, self.logit_bias, Tmax, self.Tc)
            try:
                return self._forward_eager(images_u8, stages)
            finally:
                self._tb = None
        assert stages is None
        logits = torch.full((B, self.cfg.num_queries, Tmax), float("-inf"), device=self.dev, dtype=F32)
        boxes = torch.empty((B, self.cfg.num_queries, 4), device=self.dev, dtype=F32)
        for idx in groups:
            # the group's own longest caption: exactly the launches set_captions + forward of these images alone make
            ii = torch.tensor(idx, device=self.dev)
            Tg = max(self.t_lens[i] for i in idx)
            Tcg = -(-Tg // 4) * 4
            self._tb = _TextBatch(self.text0.view(B, Tmax, 256)[ii, :Tg].reshape(-1, 256), self.t_len[ii].contiguous(),
                                  self.text_blocked[ii, :Tg, :Tg].contiguous(),
                                  self.pos_text.view(B, Tmax, 256)[ii, :Tg].reshape(-1, 256),
                                  self.logit_bias[ii, :Tcg].contiguous(), Tg, Tcg)
            try:
                lg, bx = self._forward_eager([images_u8[i] for i in idx])
            finally:
                self._tb = None
            logits[ii, :, :Tg] = lg
            boxes[ii] = bx
        return logits, boxes

    def _forward_eager(self, images_u8: Sequence[torch.Tensor], stages: Optional[dict] = None):
        B = len(images_u8)
        h, w_ = tuple(images_u8[0].shape[:2])
        pl = self.plan(h, w_, B)
        feats = self.backbone(images_u8, pl)
        src = self.neck(feats, pl, B)
        if stages is not None:
            stages["src"], stages["feats"] = src.clone(), feats
        memory, text = self.encoder(src, pl, B)
        if stages is not None:
            stages["memory"], stages["memory_text"] = memory.clone(), text.clone()
        return self.decoder(memory, text, pl, B, stages)

    def detect(self, images_u8: Sequence[torch.Tensor], top_n: Optional[int] = None):
        """predict() post-processing (GD/util/inference.py:70-75) per image: sigmoid, max over tokens,
        threshold (or fixed top_n for work-invariant benchmarking).  Host side, like the reference
        (`.cpu().sigmoid()`): 900 x (T+4) floats per image cross PCIe in ONE copy."""
        logits, boxes = self.forward(images_u8)
        both = torch.cat([logits, boxes], dim=-1).cpu()       # single D2H copy
        return self.postprocess(both, top_n)

    def postprocess(self, both: torch.Tensor, top_n: Optional[int] = None):
        """Host half of predict(): `both` = cat(logits, boxes) [B, nq, T+4] on the CPU (per-image form: T = Tmax, whose
        pad columns are -inf and never a row's maximum)."""
        T = self.T if self.captions is None else self.Tmax
        res = []
        for b in range(both.shape[0]):
            prob = both[b, :, :T].sigmoid()
            score = prob.max(dim=1)[0]
            if top_n is None:
                keep = score > self.cfg.box_threshold
                res.append((both[b, keep, T:], score[keep]))
            else:
                order = torch.sort(score, descending=True, stable=True)[1][:top_n]
                res.append((both[b, order, T:], score[order]))
        return res
