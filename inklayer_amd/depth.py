"""Depth-Anything-V2 (ViT-S / ViT-B / ViT-L) on MI355X: the depth model InkLayer's refinement uses to
order masks.

Mirrors InkLayer/refinement/depth_sort.py:20-45 (`depth_model_configs`, `depth_model`, `get_depth_map`) and DA/dpt.py
DepthAnythingV2 (`forward`, `infer_image`) with the reference's state_dict key names, so depth_anything_v2_vits.pth,
..._vitb.pth and ..._vitl.pth drop in; the model is read off the checkpoint's tensor shapes (config_from_state_dict).

Same design as the SAM / GroundingDINO engines: tokens and feature maps are [rows, channels] row-major (NHWC), one f32
residual stream, f16 GEMM operands produced by the kernel that precedes the GEMM, everything dense on
`ink_gemm_f16` (LayerScale = its per-column scale, residual in the epilogue), global attention (1370 tokens, heads of
64) on `ink_flash_attn`; the 3x3 convolutions of the DPT head run on `ink_conv3x3_f16` (implicit GEMM on NHWC maps, no
im2col matrix); ConvTranspose2d (k = stride) is a projection to (dy, dx, co) followed by a pixel-shuffle copy.  The
patch embedding runs on split-f16 operands (its rounding error stays in the residual stream of every block).  Images
of equal size run as ONE batch through the encoder and the head (infer_images).  No torch compute ops: torch supplies
memory, streams, copies.
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
class DepthConfig:
    """One Depth-Anything-V2 model; the defaults are ViT-B: depth_model_configs["vitb"] (depth_sort.py:21-22) +
    DINOv2("vitb") (DA/dinov2.py:397-415).  DEPTH_CONFIGS holds the three supported models."""
    embed_dim: int = 768
    depth: int = 12
    num_heads: int = 12
    patch_size: int = 14
    img_size: int = 518
    mlp_ratio: int = 4
    features: int = 128
    out_channels: Tuple[int, ...] = (96, 192, 384, 768)
    layer_idx: Tuple[int, ...] = (2, 5, 8, 11)
    interpolate_offset: float = 0.1
    input_size: int = 518
    pixel_mean: Tuple[float, ...] = (0.485, 0.456, 0.406)
    pixel_std: Tuple[float, ...] = (0.229, 0.224, 0.225)
    encoder: str = "vitb"


# depth_model_configs (depth_sort.py:20-33: features, out_channels) + vit_small / vit_base / vit_large
# (DA/dinov2.py:339-379: embed_dim, depth, num_heads) + DepthAnythingV2.intermediate_layer_idx (DA/dpt.py:164-169)
DEPTH_CONFIGS: Dict[str, DepthConfig] = {
    "vits": DepthConfig(embed_dim=384, depth=12, num_heads=6, features=64, out_channels=(48, 96, 192, 384),
                        layer_idx=(2, 5, 8, 11), encoder="vits"),
    "vitb": DepthConfig(),
    "vitl": DepthConfig(embed_dim=1024, depth=24, num_heads=16, features=256, out_channels=(256, 512, 1024, 1024),
                        layer_idx=(4, 11, 17, 23), encoder="vitl"),
}


def config_for(encoder: str) -> DepthConfig:
    """The registry entry of `encoder` (a copy).  ValueError for an unknown name; NotImplementedError for "vitg"."""
    if encoder == "vitg":
        raise NotImplementedError(
            "Depth-Anything-V2 ViT-g is not supported: its blocks use a SwiGLU FFN (DA/dinov2.py:410, no kernel here), "
            "its 24 heads are not the head count the engines were laid out for, and no public checkpoint exists")
    if encoder not in DEPTH_CONFIGS:
        raise ValueError(f"unknown depth encoder {encoder!r}: one of {sorted(DEPTH_CONFIGS)}")
    return replace(DEPTH_CONFIGS[encoder])


def config_from_state_dict(sd) -> DepthConfig:
    """The registry entry a state dict belongs to, from its tensor shapes alone (values: tensors, or shape tuples):
    embed dim from pretrained.cls_token, block count from the keys, features from depth_head.scratch.layer1_rn.weight,
    out_channels from depth_head.projects.{i}.weight.  ValueError when no entry matches all of them."""
    def shape(k):
        if k not in sd:
            raise ValueError(f"not a Depth-Anything-V2 state dict: {k} is missing")
        v = sd[k]
        return tuple(v.shape) if hasattr(v, "shape") else tuple(v)

    D = shape("pretrained.cls_token")[-1]
    blocks = {int(k.split(".")[2]) for k in sd if k.startswith("pretrained.blocks.")}
    depth = max(blocks) + 1 if blocks else 0
    features = shape("depth_head.scratch.layer1_rn.weight")[0]
    oc = tuple(shape(f"depth_head.projects.{i}.weight")[0] for i in range(4))
    ins = tuple(shape(f"depth_head.projects.{i}.weight")[1] for i in range(4))
    for cfg in DEPTH_CONFIGS.values():
        if (cfg.embed_dim, cfg.depth, cfg.features, cfg.out_channels) == (D, depth, features, oc) and ins == (D,) * 4 \
                and len(blocks) == depth and shape("depth_head.scratch.layer1_rn.weight")[1] == oc[0]:
            return replace(cfg)
    raise ValueError(f"state dict matches no Depth-Anything-V2 model of {sorted(DEPTH_CONFIGS)}: embed dim {D}, "
                     f"{depth} blocks, features {features}, out_channels {oc}")


def pad_channels(c: int) -> int:
    """Channel count of a head level as the kernels hold it: the GEMM needs K % 32 == 0 and the direct convolution
    C % 32 == 0, so ViT-S's 48 becomes 64 (zero channels); every other count of the three models is unchanged."""
    return -(-c // 32) * 32


def pack_head_level(proj_w: torch.Tensor, proj_b: torch.Tensor, up_w: Optional[torch.Tensor],
                    up_b: Optional[torch.Tensor], rn_w: torch.Tensor) -> Dict[str, torch.Tensor]:
    """Host-side packing of one reassemble level of the DPT head (DA/dpt.py:57-77, 92-110), channels zero-padded to
    cp = pad_channels(c).  Takes and returns f32 tensors on the inputs' device (CPU in the tests):
      proj.w [cp, D], proj.b [cp]              projects.{i} (1x1 conv), padded ROWS and bias entries zero;
      up.w [(dy, dx, co) = s*s*cp, cp], up.b   resize_layers.{i} (ConvTranspose2d, kernel = stride = s) as a projection
                                               followed by a pixel shuffle; both channel axes padded (None for no up_w);
      rn.w [features, (ky, kx, ci) = 9*cp]     scratch.layer{i+1}_rn (3x3 conv, no bias), padded INPUT channels zero.
    Exact zeros in, exact zeros out: a padded channel is 0 after projects, stays 0 through the transposed conv (zero
    weights, zero bias) and meets zero weights in layer_rn, so every real output is a sum of the same terms."""
    c, D = proj_w.shape[0], proj_w.shape[1]
    cp = pad_channels(c)
    out = {"proj.w": proj_w.new_zeros(cp, D), "proj.b": proj_b.new_zeros(cp)}
    out["proj.w"][:c] = proj_w.reshape(c, D)
    out["proj.b"][:c] = proj_b
    if up_w is not None:
        s_ = up_w.shape[2]
        t = up_w.new_zeros(s_, s_, cp, cp)                       # ConvTranspose2d [ci, co, dy, dx] -> [dy, dx, co, ci]
        t[:, :, :c, :c] = up_w.permute(2, 3, 1, 0)
        b = up_b.new_zeros(cp)
        b[:c] = up_b
        out["up.w"], out["up.b"] = t.reshape(s_ * s_ * cp, cp), b.repeat(s_ * s_)
    r = rn_w.new_zeros(rn_w.shape[0], 3, 3, cp)                  # [co, ci, 3, 3] -> [co, (ky, kx, ci)]
    r[..., :c] = rn_w.permute(0, 2, 3, 1)
    out["rn.w"] = r.reshape(rn_w.shape[0], 9 * cp)
    return out


def resize_shape(h: int, w: int, target: int = 518, multiple: int = 14) -> Tuple[int, int]:
    """Resize.get_size, keep_aspect_ratio + lower_bound + ensure_multiple_of=14 (DA/util/transform.py:61-108)."""
    sh, sw = target / h, target / w
    if sw > sh:
        sh = sw
    else:
        sw = sh

    def constrain(x):
        y = int(np.round(x / multiple) * multiple)
        if y < target:
            y = int(np.ceil(x / multiple) * multiple)
        return y

    return constrain(sh * h), constrain(sw * w)


class DepthEngine:
    def __init__(self, state_dict: Dict[str, torch.Tensor], cfg: Optional[DepthConfig] = None,
                 device: str | torch.device = "cuda"):
        cfg = cfg or DepthConfig()
        self.cfg, self.dev = cfg, torch.device(device)
        assert self.dev.type == "cuda", "the InkLayer depth model runs on MI355X only"
        D, P = cfg.embed_dim, cfg.patch_size
        assert D // cfg.num_heads == 64, "flash attention instance: head_dim 64"
        sd, dev = state_dict, self.dev
        self.w: Dict[str, torch.Tensor] = {}
        w = self.w

        def m32(name):
            return sd[name].detach().to(dev, torch.float32)

        def h(name, shape=None):
            t = m32(name)
            return (t.reshape(shape) if shape is not None else t).to(F16).contiguous()

        def f(name):
            return ops.own_f32(sd[name], dev)

        # ---- ViT
        self.KP = -(-3 * P * P // 32) * 32                       # 588 -> 608 columns per split segment
        pe = torch.zeros((D, self.KP), device=dev)
        pe[:, :3 * P * P] = m32("pretrained.patch_embed.proj.weight").reshape(D, 3 * P * P)
        w["pe.ws"] = ops.split_weight(pe)
        w["pe.b"] = f("pretrained.patch_embed.proj.bias")
        self.cls = m32("pretrained.cls_token").reshape(1, D)
        self.pos_embed = sd["pretrained.pos_embed"].detach().to(torch.float32).cpu()
        for i in range(cfg.depth):
            p, d = f"pretrained.blocks.{i}.", f"b{i}."
            for n in ("norm1.weight", "norm1.bias", "norm2.weight", "norm2.bias", "attn.qkv.bias", "attn.proj.bias",
                      "mlp.fc1.bias", "mlp.fc2.bias", "ls1.gamma", "ls2.gamma"):
                w[d + n] = f(p + n)
            for n in ("attn.qkv.weight", "attn.proj.weight", "mlp.fc1.weight", "mlp.fc2.weight"):
                w[d + n] = h(p + n)
        w["norm.w"], w["norm.b"] = f("pretrained.norm.weight"), f("pretrained.norm.bias")
        # ---- DPT head
        hd = "depth_head."
        oc, Fe = cfg.out_channels, cfg.features

        def conv3(name):                                         # [co, ci, 3, 3] -> [co, (ky, kx, ci)]
            t = m32(name)
            return t.permute(0, 2, 3, 1).reshape(t.shape[0], -1).to(F16).contiguous()

        self.ocp = tuple(pad_channels(c) for c in oc)            # channels as the kernels hold them (ViT-S: 48 -> 64)
        assert self.ocp[3] == oc[3] and Fe % 64 == 0, "resize_layers.3 / features need no channel padding"
        for i, c in enumerate(oc):
            up = (m32(f"{hd}resize_layers.{i}.weight"), m32(f"{hd}resize_layers.{i}.bias")) if i < 2 else (None, None)
            pk = pack_head_level(m32(f"{hd}projects.{i}.weight"), m32(f"{hd}projects.{i}.bias"), *up,
                                 m32(f"{hd}scratch.layer{i + 1}_rn.weight"))
            w[f"proj{i}.w"], w[f"proj{i}.b"] = pk["proj.w"].to(F16).contiguous(), pk["proj.b"].contiguous()
            w[f"rn{i}.w"] = pk["rn.w"].to(F16).contiguous()
            if i < 2:
                w[f"up{i}.w"], w[f"up{i}.b"] = pk["up.w"].to(F16).contiguous(), pk["up.b"].contiguous()
        w["down3.w"], w["down3.b"] = conv3(hd + "resize_layers.3.weight"), f(hd + "resize_layers.3.bias")
        for r in (1, 2, 3, 4):
            p = f"{hd}scratch.refinenet{r}."
            w[f"ref{r}.out.w"], w[f"ref{r}.out.b"] = h(p + "out_conv.weight", (Fe, Fe)), f(p + "out_conv.bias")
            for u in (1, 2):
                for c in (1, 2):
                    w[f"ref{r}.u{u}.c{c}.w"] = conv3(f"{p}resConfUnit{u}.conv{c}.weight")
                    w[f"ref{r}.u{u}.c{c}.b"] = f(f"{p}resConfUnit{u}.conv{c}.bias")
        w["oc1.w"], w["oc1.b"] = conv3(hd + "scratch.output_conv1.weight"), f(hd + "scratch.output_conv1.bias")
        w["oc2.w"], w["oc2.b"] = conv3(hd + "scratch.output_conv2.0.weight"), f(hd + "scratch.output_conv2.0.bias")
        last = torch.zeros((4, 32), device=dev)                  # 1x1 conv to ONE channel, N padded to 4 for the GEMM
        last[0] = m32(hd + "scratch.output_conv2.2.weight").reshape(32)
        w["oc3.w"] = last.to(F16).contiguous()
        b3 = torch.zeros(4, device=dev)
        b3[0] = m32(hd + "scratch.output_conv2.2.bias").reshape(())
        w["oc3.b"] = b3
        self._pos = LRU(8)                                       # position embeddings per (patch rows, patch cols)

    # ------------------------------------------------------------------ constants per input size
    def _pos_tokens(self, ph: int, pw: int) -> Tuple[torch.Tensor, torch.Tensor]:
        """interpolate_pos_encoding (DA/dinov2.py:179-209) folded per input size: (cls + pos[0] [1, D], pos[1:] [T, D]).
        The reference names the image HEIGHT `w` and the WIDTH `h`; the bicubic interpolation runs once per size on the
        host (a load-time constant, like the sine embeddings of the detector)."""
        def make():
            cfg = self.cfg
            pos = self.pos_embed
            N = pos.shape[1] - 1
            if ph * pw == N and ph == pw:
                patch = pos[0, 1:]
            else:
                sq = math.sqrt(N)
                w0, h0 = ph + cfg.interpolate_offset, pw + cfg.interpolate_offset
                pp = torch.nn.functional.interpolate(
                    pos[:, 1:].reshape(1, int(sq), int(sq), -1).permute(0, 3, 1, 2),
                    scale_factor=(float(w0) / sq, float(h0) / sq), mode="bicubic", antialias=False)
                assert (pp.shape[-2], pp.shape[-1]) == (ph, pw)
                patch = pp.permute(0, 2, 3, 1).reshape(ph * pw, -1)
            cls = (self.cls + pos[0, :1].to(self.dev)).contiguous()
            return cls, patch.to(self.dev).contiguous()
        return self._pos.get_or_make((ph, pw), make)

    # ------------------------------------------------------------------ ViT encoder
    def encode(self, patches: Sequence[torch.Tensor], ph: int, pw: int) -> List[torch.Tensor]:
        """patches: per image the split-f16 im2col rows [T, 3*KP].  -> the 4 normalised patch-token maps
        [B*T, D] f16 (get_intermediate_layers(norm=True), DA/dinov2.py:293-321; the class tokens are unused since
        use_clstoken=False, DA/dpt.py:122-128)."""
        cfg, w = self.cfg, self.w
        B, T, D, H = len(patches), ph * pw, cfg.embed_dim, cfg.num_heads
        N = T + 1
        cls, pos = self._pos_tokens(ph, pw)
        x = torch.empty((B * N, D), device=self.dev, dtype=F32)
        for b, pt in enumerate(patches):
            x[b * N:b * N + 1] = cls                                           # plumbing copy (1 row)
            ops.gemm(pt, w["pe.ws"], w["pe.b"], residual=pos, out=x[b * N + 1:(b + 1) * N])
        outs = []
        scale = 64 ** -0.5
        for i in range(cfg.depth):
            k = f"b{i}."
            y = ops.layernorm_rows(x, w[k + "norm1.weight"], w[k + "norm1.bias"], 1e-6)
            qkv = ops.gemm(y, w[k + "attn.qkv.weight"], w[k + "attn.qkv.bias"], out_dtype=F16)
            o = ops.flash_attn(qkv[:, :D], qkv[:, D:2 * D], qkv[:, 2 * D:], n_batch=B, n_heads=H, head_dim=64,
                               scale=scale, n_q=N, n_k=N)
            # x = x + ls1 * proj(o): LayerScale is the GEMM's per-column scale (needs the late residual form)
            ops.gemm(o, w[k + "attn.proj.weight"], w[k + "attn.proj.bias"], col_scale=w[k + "ls1.gamma"], residual=x, out=x)
            y = ops.layernorm_rows(x, w[k + "norm2.weight"], w[k + "norm2.bias"], 1e-6)
            hmid = ops.gemm(y, w[k + "mlp.fc1.weight"], w[k + "mlp.fc1.bias"], act="gelu", out_dtype=F16)
            ops.gemm(hmid, w[k + "mlp.fc2.weight"], w[k + "mlp.fc2.bias"], col_scale=w[k + "ls2.gamma"], residual=x, out=x)
            if i in cfg.layer_idx:
                n16 = ops.layernorm_rows(x, w["norm.w"], w["norm.b"], 1e-6)   # [B*N, D] f16
                outs.append(n16.view(B, N, D)[:, 1:].reshape(B * T, D) if B > 1 else n16[1:])
        return outs

    # ------------------------------------------------------------------ DPT head (a batch of equal-size images)
    def _conv3(self, x16: torch.Tensor, B: int, hh: int, ww: int, wname: str, bias: Optional[str] = None, *,
               relu_in=False, stride=1, **kw) -> torch.Tensor:
        """A 3x3 / pad 1 convolution of the NHWC map x16 [B*hh*ww, C]: the direct kernel, or the im2col + GEMM pair for
        the forms of CONV_ON_PAIR up to the row count at which the pair was measured faster.  Both give the same bits."""
        wt = self.w[wname]
        C = x16.shape[1]
        M = B * ((hh - 1) // stride + 1) * ((ww - 1) // stride + 1)
        if M <= CONV_ON_PAIR.get((C, wt.shape[0], stride, bool(relu_in)), 0):
            col = ops.im2col3x3(x16, B, hh, ww, stride=stride, relu=relu_in)
            return ops.gemm(col, wt, self.w[bias] if bias else None, **kw)
        return ops.conv3x3(x16, B, hh, ww, wt, self.w[bias] if bias else None, stride=stride, relu_in=relu_in, **kw)

    def _rcu(self, x: torch.Tensor, B: int, hh: int, ww: int, p: str) -> torch.Tensor:
        """ResidualConvUnit (DA/util/blocks.py:59-84): conv2(relu(conv1(relu(x)))) + x, f32 in / f32 out."""
        a = self._conv3(ops.add_cvt_f16(x), B, hh, ww, p + ".c1.w", p + ".c1.b", relu_in=True, act="relu", out_dtype=F16)
        return self._conv3(a, B, hh, ww, p + ".c2.w", p + ".c2.b", residual=x)

    def _fusion(self, r: int, x0: torch.Tensor, x1: Optional[torch.Tensor], B: int, hw: Tuple[int, int],
                size: Optional[Tuple[int, int]]) -> Tuple[torch.Tensor, Tuple[int, int]]:
        """FeatureFusionBlock (DA/util/blocks.py:123-148), align_corners=True."""
        hh, ww = hw
        out = x0
        if x1 is not None:
            out = ops.add_f32(out, self._rcu(x1, B, hh, ww, f"ref{r}.u1"))
        out = self._rcu(out, B, hh, ww, f"ref{r}.u2")
        H2, W2 = size if size is not None else (2 * hh, 2 * ww)
        up16 = ops.resize_bilinear_ac(out, B, hh, ww, H2, W2, out_dtype=F16)
        return ops.gemm(up16, self.w[f"ref{r}.out.w"], self.w[f"ref{r}.out.b"]), (H2, W2)

    def head_batch(self, feats16: Sequence[torch.Tensor], B: int, ph: int, pw: int,
                   stages: Optional[dict] = None) -> torch.Tensor:
        """DPTHead.forward (DA/dpt.py:118-150) for B images of ph x pw patches: 4 x [B*T, D] f16 -> depth
        [B, 14*ph, 14*pw] f32.  Every map is NHWC with the batch outermost, [B*h*w, C]; the 1x1 convolutions are
        row-wise GEMMs, the 3x3 convolutions and the resizes take B.  stages (optional) receives rn (the four layer_rn
        maps, f32 [B*h*w, features]) and path (path_1 .. path_4)."""
        w = self.w
        ocp = self.ocp

        def shuffle(t: torch.Tensor, s: int, c: int) -> torch.Tensor:     # [(b, ph, pw), (dy, dx, c)] -> NHWC upscaled
            return t.view(B, ph, pw, s, s, c).permute(0, 1, 3, 2, 4, 5).reshape(B * ph * s * pw * s, c).contiguous()

        l0 = shuffle(ops.gemm(ops.gemm(feats16[0], w["proj0.w"], w["proj0.b"], out_dtype=F16), w["up0.w"], w["up0.b"],
                              out_dtype=F16), 4, ocp[0])
        l1 = shuffle(ops.gemm(ops.gemm(feats16[1], w["proj1.w"], w["proj1.b"], out_dtype=F16), w["up1.w"], w["up1.b"],
                              out_dtype=F16), 2, ocp[1])
        l2 = ops.gemm(feats16[2], w["proj2.w"], w["proj2.b"], out_dtype=F16)
        l3 = self._conv3(ops.gemm(feats16[3], w["proj3.w"], w["proj3.b"], out_dtype=F16), B, ph, pw, "down3.w", "down3.b",
                         stride=2, out_dtype=F16)
        s0, s1, s2 = (4 * ph, 4 * pw), (2 * ph, 2 * pw), (ph, pw)
        s3 = ((ph - 1) // 2 + 1, (pw - 1) // 2 + 1)
        rn = [self._conv3(l, B, hw[0], hw[1], f"rn{i}.w") for i, (l, hw) in enumerate(((l0, s0), (l1, s1), (l2, s2), (l3, s3)))]
        p4, hw4 = self._fusion(4, rn[3], None, B, s3, s2)
        p3, hw3 = self._fusion(3, p4, rn[2], B, hw4, s1)
        p2, hw2 = self._fusion(2, p3, rn[1], B, hw3, s0)
        p1, hw1 = self._fusion(1, p2, rn[0], B, hw2, None)
        if stages is not None:
            stages.update(rn=rn, path=[p1, p2, p3, p4])
        o = self._conv3(ops.add_cvt_f16(p1), B, hw1[0], hw1[1], "oc1.w", "oc1.b")              # [B*8ph*8pw, features/2] f32
        H, W = 14 * ph, 14 * pw
        o16 = ops.resize_bilinear_ac(o, B, hw1[0], hw1[1], H, W, out_dtype=F16)
        o = self._conv3(o16, B, H, W, "oc2.w", "oc2.b", act="relu", out_dtype=F16)             # [B*H*W, 32]
        d = ops.gemm(o, w["oc3.w"], w["oc3.b"], act="relu")                                    # [B*H*W, 4], column 0
        return d[:, 0].reshape(B, H, W)

    def head(self, feats16: Sequence[torch.Tensor], ph: int, pw: int, stages: Optional[dict] = None) -> torch.Tensor:
        """head_batch for ONE image: 4 x [T, D] f16 -> depth [14*ph, 14*pw] f32."""
        return self.head_batch(feats16, 1, ph, pw, stages)[0]

    # ------------------------------------------------------------------ reference-shaped API
    def _infer_group(self, imgs: Sequence[torch.Tensor], stages: Optional[dict] = None) -> torch.Tensor:
        """Equal-size HWC uint8 BGR device images as one batch -> depth [B, h, w] f32."""
        cfg = self.cfg
        B = len(imgs)
        h, w_ = int(imgs[0].shape[0]), int(imgs[0].shape[1])
        nh, nw = resize_shape(h, w_, cfg.input_size, cfg.patch_size)
        ph, pw = nh // cfg.patch_size, nw // cfg.patch_size
        patches = [ops.depth_patchify(im, nh, nw, cfg.patch_size, self.KP, cfg.pixel_mean, cfg.pixel_std, chan_reverse=True)
                   for im in imgs]
        feats = self.encode(patches, ph, pw)
        if stages is not None:
            stages["feats"] = feats
        d = self.head_batch(feats, B, ph, pw, stages)
        if stages is not None:
            stages["depth_net"] = d[0] if B == 1 else d
        return ops.resize_bilinear_ac(d.reshape(B * nh * nw, 1).contiguous(), B, nh, nw, h, w_).reshape(B, h, w_)

    def _device_image(self, raw_bgr: np.ndarray | torch.Tensor) -> torch.Tensor:
        return raw_bgr if isinstance(raw_bgr, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(raw_bgr)).to(self.dev)

    @torch.no_grad()
    def infer_image(self, raw_bgr: np.ndarray | torch.Tensor, stages: Optional[dict] = None) -> torch.Tensor:
        """DepthAnythingV2.infer_image (DA/dpt.py:189-197) for a BGR uint8 image as cv2.imread returns it
        (host array or HWC uint8 CUDA tensor).  -> depth [h, w] f32 on the GPU."""
        return self._infer_group([self._device_image(raw_bgr)], stages)[0]

    @torch.no_grad()
    def infer_images(self, images: Sequence[np.ndarray | torch.Tensor],
                     stages: Optional[List[dict]] = None) -> List[torch.Tensor]:
        """infer_image for several images: images of equal size run through the encoder and the head as ONE batch,
        several sizes as one batch per size (in order of first appearance); the depth maps [h, w] f32 come back in
        input order.  stages (optional): a list that receives one dict per size group (sizes, indices, and the stages
        of infer_image with the batch outermost in every map)."""
        imgs = [self._device_image(im) for im in images]
        groups: Dict[Tuple[int, int], List[int]] = {}
        for i, im in enumerate(imgs):
            groups.setdefault((int(im.shape[0]), int(im.shape[1])), []).append(i)
        out: List[Optional[torch.Tensor]] = [None] * len(imgs)
        for size, idx in groups.items():
            st = None
            if stages is not None:
                st = {"size": size, "indices": idx}
                stages.append(st)
            d = self._infer_group([imgs[i] for i in idx], st)
            for j, i in enumerate(idx):
                out[i] = d[j]
        return out


# The head's 3x3 convolutions that stay on ops.im2col3x3 + ops.gemm: (C, N, stride, relu_in) -> the largest row count
# M = B*OH*OW at which tools/depth_time.py measured the direct kernel slower than the pair beyond the run-to-run spread
# (profiles/depth_conv_times.txt, 518 x 518 input, by 2 .. 8 %).  All are launches of three M-tiles with a long K loop
# on the 19 x 19 map (361 rows): resize_layers.3 and layer4_rn of the three models and ViT-L's ResidualConvUnit conv1
# (the same conv on the 37 x 37 map is a tie, 1.01, inside the spread).  More rows (a larger input, a batch) run on the
# direct kernel.
CONV_ON_PAIR: Dict[Tuple[int, int, int, bool], int] = {
    (384, 384, 2, False): 361, (384, 64, 1, False): 361,            # ViT-S
    (768, 768, 2, False): 361, (768, 128, 1, False): 361,           # ViT-B
    (1024, 1024, 2, False): 361, (1024, 256, 1, False): 361,        # ViT-L
    (256, 256, 1, True): 361,                                       # ViT-L refinenet4 conv1
}

_ENGINES: Dict[str, DepthEngine] = {}


def build_depth(checkpoint: str, encoder: Optional[str] = None, device="cuda") -> DepthEngine:
    """depth_sort.py:35-40: the model is a module-level singleton there; cached per checkpoint path here.  The model is
    read off the checkpoint's tensor shapes (config_from_state_dict); a given `encoder` name has to agree with it."""
    want = config_for(encoder) if encoder is not None else None
    if checkpoint not in _ENGINES:
        sd = torch.load(checkpoint, map_location="cpu", weights_only=True)
        cfg = config_from_state_dict(sd)
        if want is not None and want.encoder != cfg.encoder:
            raise ValueError(f"{checkpoint} holds a Depth-Anything-V2 {cfg.encoder} model, not the {encoder!r} asked for")
        _ENGINES[checkpoint] = DepthEngine(sd, cfg, device)
    eng = _ENGINES[checkpoint]
    if want is not None and want.encoder != eng.cfg.encoder:
        raise ValueError(f"{checkpoint} holds a Depth-Anything-V2 {eng.cfg.encoder} model, not the {encoder!r} asked for")
    return eng
