"""Fixtures, float64 restatements, yardsticks and named mistakes for the code between the encoders' layers: SAM's patch
embedding and neck (SamEngine.encode / the tail of _blocks) and the detector's Swin stem, stage seams and input_proj
(GDinoEngine.backbone / neck).  Shared by tests/test_encoder_ends_gpu.py, tests/test_detector_seams_gpu.py and
tests/test_encoder_ends_ref_cpu.py; the latter pins every restatement to oracle/sam_ref.py / oracle/gdino_ref.py and
shows on the CPU that each yardstick tells the named mistakes apart.

Every function takes its dtype from the tensors it is given (float64: the reference; float32: SAM's yardstick) and calls
linear / conv2d through the oracle module's `F`, so that sam_ref.f16_operands() / gdino_ref.f16_operands() reach it.

Yardsticks (no absolute tolerance is invented; each bound is a quantile of a reference evaluation's own error):
  * SAM, split-f16 operands: at every quantile HIP <= SAM_MARGIN x the error of the same restatement in float32,
    SAM_MARGIN = 8 = 2^-21 / 2^-24, the accuracy include/inklayer_hip.h states for a split product over f32's.  Cap: the
    bound stays <= 1/16 of the error of the float64 restatement under sam_ref.f16_operands().
  * detector, f16 operands: HIP <= 2 x the float64 restatement under gdino_ref.f16_operands() (+ 2^-11 max|ref| for an
    f16 output: its own rounding, which the emulation does not do)."""
import functools

import numpy as np
import torch

from oracle import gdino_ref as G
from oracle import sam_ref as S

F32, F64 = torch.float32, torch.float64
QUANTILES = (0.5, 0.9, 0.99, 0.999, 1.0)
SAM_MARGIN = 8.0                 # 2^-21 / 2^-24
SAM_CAP = 16.0                   # the SAM bound stays this far below the f16-operand error
DET_FACTOR = 2.0                 # the project's f16-operand yardstick
F16_OUT_ABS = 2.0 ** -11         # one f16 rounding of an output, relative to max|ref|
MIN_FACTOR = 10.0                # a named mistake lands at least this far outside the bound


# ---------------------------------------------------------------------------------------------------------------
# yardstick helpers
# ---------------------------------------------------------------------------------------------------------------
def quantiles(err: torch.Tensor) -> np.ndarray:
    return np.quantile(err.detach().reshape(-1).double().cpu().numpy(), QUANTILES)


def f32_bound(ref: torch.Tensor, f32: torch.Tensor) -> np.ndarray:
    """SAM_MARGIN x the error of the float32 evaluation, per quantile."""
    return SAM_MARGIN * quantiles((f32.double() - ref).abs())


sam_bound = f32_bound


def det_bound(ref: torch.Tensor, emul: torch.Tensor, f16_out: bool = False) -> np.ndarray:
    a = F16_OUT_ABS * float(ref.abs().max()) if f16_out else 0.0
    return DET_FACTOR * quantiles((emul - ref).abs()) + a


def assert_within(got: torch.Tensor, ref: torch.Tensor, bound: np.ndarray, what: str) -> np.ndarray:
    """Prints HIP error / bound per quantile, asserts all finite and every quantile within its bound; -> the ratios."""
    got = got.detach().double().cpu()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert torch.isfinite(got).all(), f"{what}: non-finite output"
    hq = quantiles((got - ref).abs())
    r = hq / bound
    print(f"  {what}: HIP / bound at q{QUANTILES} = " + " ".join(f"{x:.3f}" for x in r)
          + "   (HIP " + " ".join(f"{x:.2e}" for x in hq) + ")")
    assert (hq <= bound).all(), (what, dict(zip(QUANTILES, zip(hq.tolist(), bound.tolist()))))
    return r


def shows_at(share: float) -> np.ndarray:
    """The quantiles at which a mistake that reaches `share` of the elements has to show: those q with
    1 - q < 0.51 share, so that the quantile sits in the upper half of the reached elements, and always the maximum.  The
    share comes from the geometry of the case (which tokens a pad, a border or a tap reaches), never from an evaluation."""
    assert 0 < share <= 1
    return np.array([q == 1.0 or 1 - q < 0.51 * share for q in QUANTILES])


def assert_discriminates(wrong: torch.Tensor, ref: torch.Tensor, bound: np.ndarray, what: str, share: float = 1.0) -> float:
    """The mistaken float64 evaluation exceeds the bound MIN_FACTOR-fold at every quantile of shows_at(share); prints the
    factors (as _discriminates of tests/test_detector_ops_gpu.py does) and returns the smallest."""
    f = quantiles((wrong - ref).abs()) / bound
    m = shows_at(share)
    print(f"  mistake '{what}' (reaches {share:.3f}): "
          + " ".join(f"q{q} {x:.0f}x" + ("" if s else " (n/a)") for q, x, s in zip(QUANTILES, f, m)))
    assert (f[m] >= MIN_FACTOR).all(), f"the bound cannot tell the mistake '{what}' apart: {f.tolist()} at {QUANTILES}"
    return float(f[m].min())


def cast(sd, dtype, prefix=""):
    return {k: v.to(dtype) for k, v in sd.items() if k.startswith(prefix)}


# ---------------------------------------------------------------------------------------------------------------
# SAM: fixture
# ---------------------------------------------------------------------------------------------------------------
SAM_SEED = 11
SAM_SIZES = ((1024, 768), (683, 1024), (1024, 1024), (517, 1024), (1024, 1001), (1024, 650), (777, 1024), (1008, 1024))
NECK_SMALL = 2.0 ** -7           # input (b) = input (a) x this: the first LayerNorm2d's variance comes within reach of eps


def sam_config():
    return S.SamConfig(depth=0, global_attn_indexes=())


@functools.lru_cache(maxsize=None)
def sam_sd(dtype=F32):
    """Depth-0 SAM weights, seed 11 (f32 as seeded; other dtypes are casts of it)."""
    sd = S.seeded_state_dict(S.sam_param_shapes(sam_config()), SAM_SEED)
    return sd if dtype == F32 else cast(sd, dtype, "image_encoder.")


@functools.lru_cache(maxsize=None)
def sam_image(i: int) -> np.ndarray:
    """Image i of the stem cases (a batch of B is images 0 .. B-1): random u8, (h, w) = SAM_SIZES[i].  Image 0 is
    1024 x 768 (zero pad on the right), image 1 683 x 1024 (at the bottom, ending inside a patch row)."""
    h, w = SAM_SIZES[i]
    return np.random.RandomState(500 + i).randint(0, 256, size=(h, w, 3)).astype(np.uint8)


def sam_pixels(img: np.ndarray, cfg, dtype, pad_normalised: bool = False, bgr: bool = False) -> torch.Tensor:
    """sam_ref.preprocess in `dtype`: HWC u8 -> [3, L, L], normalised, zero-padded at the bottom / right.
    pad_normalised: the pad is (0 - mean) / std; bgr: the channels are read in reverse order."""
    x = torch.from_numpy(np.ascontiguousarray(img)).permute(2, 0, 1).to(dtype)
    if bgr:
        x = x.flip(0)
    mean = torch.tensor(cfg.pixel_mean, dtype=dtype).view(3, 1, 1)
    std = torch.tensor(cfg.pixel_std, dtype=dtype).view(3, 1, 1)
    pad = (0, cfg.img_size - x.shape[-1], 0, cfg.img_size - x.shape[-2])
    if pad_normalised:
        return (torch.nn.functional.pad(x, pad) - mean) / std
    return torch.nn.functional.pad((x - mean) / std, pad)


def sam_stem(sd, cfg, x: torch.Tensor, pos_first_only: bool = False) -> torch.Tensor:
    """image_encoder(..., upto=0): [B, 3, L, L] -> NHWC tokens [B, g, g, D].  pos_first_only: pos_embed is added to
    image 0 alone."""
    y = S.F.conv2d(x, sd["image_encoder.patch_embed.proj.weight"], sd["image_encoder.patch_embed.proj.bias"],
                   stride=cfg.patch_size).permute(0, 2, 3, 1)
    pos = sd["image_encoder.pos_embed"]
    if pos_first_only:
        return torch.cat([y[:1] + pos, y[1:]], 0)
    return y + pos


def sam_pad_share(i: int) -> float:
    """The share of image i's tokens whose patch holds at least one pad pixel."""
    h, w = SAM_SIZES[i]
    g, P = sam_config().grid, sam_config().patch_size
    return 1.0 - (h // P) * (w // P) / (g * g)


def sam_pixel_share(i: int) -> float:
    """The share of image i's tokens whose patch holds at least one image pixel."""
    h, w = SAM_SIZES[i]
    g, P = sam_config().grid, sam_config().patch_size
    return -(-h // P) * -(-w // P) / (g * g)


NECK_BORDER_SHARE = (4 * 64 - 4) / 64 ** 2      # tokens with a 3x3 tap outside the 64 x 64 grid


NECK_MISTAKES = ("neck.2 ky/kx transposed", "neck.2 border clamped", "eps 1e-5")


def sam_neck(sd, x: torch.Tensor, mistake=None) -> torch.Tensor:
    """The neck of image_encoder on NHWC tokens [B, g, g, D] -> NHWC [B, g, g, E]."""
    assert mistake is None or mistake in NECK_MISTAKES
    eps = 1e-5 if mistake == "eps 1e-5" else 1e-6
    p = "image_encoder.neck."
    x = S.F.conv2d(x.permute(0, 3, 1, 2), sd[p + "0.weight"])
    x = S._ln2d(x, sd[p + "1.weight"], sd[p + "1.bias"], eps)
    w2 = sd[p + "2.weight"]
    if mistake == "neck.2 ky/kx transposed":
        w2 = w2.transpose(2, 3)
    if mistake == "neck.2 border clamped":
        x = S.F.conv2d(torch.nn.functional.pad(x, (1, 1, 1, 1), mode="replicate"), w2)
    else:
        x = S.F.conv2d(x, w2, padding=1)
    return S._ln2d(x, sd[p + "3.weight"], sd[p + "3.bias"], eps).permute(0, 2, 3, 1)


@functools.lru_cache(maxsize=None)
def neck_tokens(i: int, small: bool) -> torch.Tensor:
    """f32 input of the neck for image i, [g*g, D]: (a) shaped like the residual stream, randn + 3 randn(D) with the same
    per-channel constant for every image; (b) = (a) x NECK_SMALL."""
    cfg = sam_config()
    off = 3 * torch.randn(cfg.embed_dim, generator=torch.Generator().manual_seed(99))
    x = torch.randn(cfg.grid * cfg.grid, cfg.embed_dim, generator=torch.Generator().manual_seed(100 + i)) + off
    return x * NECK_SMALL if small else x


def sam_stem_one(i: int, dtype, **mistake) -> torch.Tensor:
    """The stem of image i on its own: [g*g, D]."""
    cfg = sam_config()
    pix = {k: v for k, v in mistake.items() if k in ("pad_normalised", "bgr")}
    rest = {k: v for k, v in mistake.items() if k not in pix}
    x = sam_pixels(sam_image(i), cfg, dtype, **pix)[None]
    if rest.pop("no_pos", False):                  # what image b >= 1 gets when pos_embed is added to image 0 alone
        x = torch.cat([torch.zeros_like(x), x])
        return sam_stem(sam_sd(dtype), cfg, x, pos_first_only=True)[1].reshape(cfg.grid ** 2, -1)
    assert not rest
    return sam_stem(sam_sd(dtype), cfg, x)[0].reshape(cfg.grid ** 2, -1)


def sam_neck_one(x: torch.Tensor, dtype, mistake=None) -> torch.Tensor:
    """The neck on the f32 tokens [g*g, D] of one image: [g*g, E]."""
    g = sam_config().grid
    return sam_neck(sam_sd(dtype), x.to(dtype).view(1, g, g, -1), mistake).reshape(g * g, -1)


@functools.lru_cache(maxsize=None)
def sam_stem_refs(i: int):
    """(float64 reference, float32 evaluation) of image i's stem: what the GPU test needs, computed once."""
    return sam_stem_one(i, F64), sam_stem_one(i, F32)


@functools.lru_cache(maxsize=None)
def sam_neck_refs(i: int, small: bool):
    x = neck_tokens(i, small)
    return sam_neck_one(x, F64), sam_neck_one(x, F32)


@functools.lru_cache(maxsize=None)
def sam_full_refs(i: int):
    """image_encoder(..., upto=None) of image i in float64 and float32: [g*g, E]."""
    cfg = sam_config()
    out = []
    for dt in (F64, F32):
        e = S.image_encoder(sam_sd(dt), cfg, sam_pixels(sam_image(i), cfg, dt)[None])
        out.append(e[0].permute(1, 2, 0).reshape(cfg.grid ** 2, -1))
    return tuple(out)


# ---------------------------------------------------------------------------------------------------------------
# detector: fixture
# ---------------------------------------------------------------------------------------------------------------
DET_SEED = 21
DET_SIZES = ((300, 412), (160, 224), (150, 203))
DET_B = 2
DET_IDS = (101, 4874, 1012, 102)
PIXEL_MEAN, PIXEL_STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


def det_config():
    return G.GDinoConfig(depths=(0, 0, 0, 0), enc_layers=1, dec_layers=1, num_queries=100)


@functools.lru_cache(maxsize=None)
def det_sd(dtype=F32):
    sd = S.seeded_state_dict(G.gdino_param_shapes(det_config()), DET_SEED)
    return sd if dtype == F32 else cast(sd, dtype)


@functools.lru_cache(maxsize=None)
def det_text():
    return 0.5 * torch.randn(len(DET_IDS), 256, generator=torch.Generator().manual_seed(5))


@functools.lru_cache(maxsize=None)
def det_images(hw) -> np.ndarray:
    """Two different random u8 images [2, h, w, 3]: image 0 over the whole range, image 1 at a quarter of the contrast
    (96 .. 159), so that the two images' statistics differ the way a sketch's and a photo's do."""
    x = np.random.RandomState(700 + hw[0]).randint(0, 256, size=(DET_B, hw[0], hw[1], 3))
    x[1] = 96 + x[1] // 4
    return x.astype(np.uint8)


def det_pixels(imgs: np.ndarray, dtype) -> torch.Tensor:
    """ToTensor + Normalize of gdino_ref.load_image in `dtype`: [B, h, w, 3] u8 -> [B, 3, h, w]."""
    x = torch.from_numpy(imgs).permute(0, 3, 1, 2).to(dtype) / 255.0
    mean = torch.tensor(PIXEL_MEAN, dtype=dtype).view(1, 3, 1, 1)
    std = torch.tensor(PIXEL_STD, dtype=dtype).view(1, 3, 1, 1)
    return (x - mean) / std


def stage_grids(hw):
    H, W = -(-hw[0] // 4), -(-hw[1] // 4)
    out = []
    for _ in range(4):
        out.append((H, W))
        H, W = (H + 1) // 2, (W + 1) // 2
    return out


def level_shapes(hw):
    g = stage_grids(hw)[1:]
    return g + [((g[-1][0] - 1) // 2 + 1, (g[-1][1] - 1) // 2 + 1)]


SEAM_MISTAKES = ("merge x1/x2 swapped", "odd merge pad clamped", "ragged patch pad normalised")


def swin_seams(sd, cfg, img: torch.Tensor, mistake=None):
    """gdino_ref.swin_forward for depths (0, 0, 0, 0): stem, then per stage the output norm and the patch merging.
    -> (NCHW maps of out_indices, the token tensors [B, H*W, C] those norms read)."""
    assert mistake is None or mistake in SEAM_MISTAKES
    assert not any(cfg.depths)
    pfx = "backbone.0."
    _, _, H0, W0 = img.shape
    pad = (0, (-W0) % 4, 0, (-H0) % 4)
    if mistake == "ragged patch pad normalised":          # (0 - mean) / std instead of 0
        fill = (-torch.tensor(PIXEL_MEAN, dtype=img.dtype) / torch.tensor(PIXEL_STD, dtype=img.dtype)).view(1, 3, 1, 1)
        full = fill.expand(img.shape[0], 3, H0 + pad[3], W0 + pad[1]).clone()
        full[:, :, :H0, :W0] = img
        img = full
    else:
        img = torch.nn.functional.pad(img, pad)
    x = G.F.conv2d(img, sd[pfx + "patch_embed.proj.weight"], sd[pfx + "patch_embed.proj.bias"], stride=4)
    B, C, H, W = x.shape
    x = G._ln(x.flatten(2).transpose(1, 2), sd, pfx + "patch_embed.norm")
    outs, pre = [], []
    for i in range(len(cfg.depths)):
        if i in cfg.out_indices:
            pre.append(x)
            outs.append(G._ln(x, sd, f"{pfx}norm{i}").view(B, H, W, -1).permute(0, 3, 1, 2).contiguous())
        if i < len(cfg.depths) - 1:
            p = f"{pfx}layers.{i}.downsample."
            y = x.view(B, H, W, -1)
            if mistake == "odd merge pad clamped":
                if W % 2:
                    y = torch.cat([y, y[:, :, -1:]], 2)
                if H % 2:
                    y = torch.cat([y, y[:, -1:]], 1)
            elif H % 2 or W % 2:
                y = torch.nn.functional.pad(y, (0, 0, 0, W % 2, 0, H % 2))
            parts = [y[:, 0::2, 0::2], y[:, 1::2, 0::2], y[:, 0::2, 1::2], y[:, 1::2, 1::2]]
            if mistake == "merge x1/x2 swapped":
                parts = [parts[0], parts[2], parts[1], parts[3]]
            y = torch.cat(parts, -1)
            x = G.F.linear(G._ln(y.view(B, -1, y.shape[-1]), sd, p + "norm"), sd[p + "reduction.weight"])
            H, W = (H + 1) // 2, (W + 1) // 2
    return outs, pre


def reach(hw, mistake):
    """Which tokens a mistake reaches, from the geometry alone: bool masks [H, W] of the four Swin stages and of the
    extra level (3x3 / stride 2 / pad 1 on stage 3)."""
    pool = torch.nn.functional.max_pool2d
    grids = stage_grids(hw)
    H, W = grids[0]
    m = torch.zeros(H, W)
    if mistake == "ragged patch pad normalised":
        m[-1, :] = float(hw[0] % 4 != 0)
        m[:, -1] = float(hw[1] % 4 != 0)
    masks = [m]
    for H, W in grids[:3]:
        m = pool(torch.nn.functional.pad(m, (0, W % 2, 0, H % 2))[None, None], 2)[0, 0]
        if mistake == "merge x1/x2 swapped":
            m = torch.ones_like(m)
        if mistake == "odd merge pad clamped":
            if H % 2:
                m[-1, :] = 1
            if W % 2:
                m[:, -1] = 1
        masks.append(m)
    masks.append(pool(masks[3][None, None], 3, 2, 1)[0, 0])
    return [x.bool() for x in masks]


def clamped_tap_share(hw) -> float:
    """The share of the extra level's tokens with a tap outside stage 3's map."""
    (H3, W3), (H4, W4) = level_shapes(hw)[2:]
    y, x = torch.meshgrid(torch.arange(H4), torch.arange(W4), indexing="ij")
    out = (y == 0) | (x == 0) | (2 * y + 1 >= H3) | (2 * x + 1 >= W3)
    return float(out.double().mean())


PROJ_MISTAKES = ("level 3 fed from level 2's projection", "level-3 taps clamped", "level-3 ky/kx transposed",
                 "GroupNorm pooled over the batch")


def _group_norm_pooled(s, w, b, groups=32, eps=1e-5):
    """GroupNorm whose statistics run over the whole batch."""
    B, C, H, W = s.shape
    y = s.view(B, groups, C // groups, H * W)
    mu = y.mean((0, 2, 3), keepdim=True)
    var = (y - mu).pow(2).mean((0, 2, 3), keepdim=True)
    return ((y - mu) / torch.sqrt(var + eps)).view(B, C, H, W) * w.view(1, -1, 1, 1) + b.view(1, -1, 1, 1)


def input_proj(sd, cfg, feats, mistake=None) -> torch.Tensor:
    """The conv2d + group_norm lines of gdino_ref.detector_forward: NCHW maps of the three stages -> the flattened
    multi-scale source [B, S, 256] (four levels)."""
    assert mistake is None or mistake in PROJ_MISTAKES
    assert cfg.num_feature_levels == len(feats) + 1

    def gn(s, l):
        w, b = sd[f"input_proj.{l}.1.weight"], sd[f"input_proj.{l}.1.bias"]
        if mistake == "GroupNorm pooled over the batch":
            return _group_norm_pooled(s, w, b)
        return G.F.group_norm(s, 32, w, b)

    srcs = [gn(G.F.conv2d(f, sd[f"input_proj.{l}.0.weight"], sd[f"input_proj.{l}.0.bias"]), l)
            for l, f in enumerate(feats)]
    l = len(feats)
    w, b = sd[f"input_proj.{l}.0.weight"], sd[f"input_proj.{l}.0.bias"]
    inp = feats[-1]
    if mistake == "level 3 fed from level 2's projection":    # 256 channels: against the weight's first 256 inputs
        inp, w = srcs[-1], w[:, :srcs[-1].shape[1]]
    if mistake == "level-3 ky/kx transposed":
        w = w.transpose(2, 3)
    if mistake == "level-3 taps clamped":
        s = G.F.conv2d(torch.nn.functional.pad(inp, (1, 1, 1, 1), mode="replicate"), w, b, stride=2)
    else:
        s = G.F.conv2d(inp, w, b, stride=2, padding=1)
    srcs.append(gn(s, l))
    return torch.cat([s.flatten(2).transpose(1, 2) for s in srcs], 1)


@functools.lru_cache(maxsize=None)
def proj_tokens(hw, seed: int = 0):
    """Hand-made f32 feature tokens {stage: [B, H*W, C]} for input_proj alone: (1 + b) randn + a per-channel offset
    2 randn(C) of image b's own; every image has its own noise, offsets and scale."""
    g = torch.Generator().manual_seed(900 + hw[0] + 7919 * seed)
    out = {}
    for i, (H, W) in zip((1, 2, 3), stage_grids(hw)[1:]):
        C = 96 * 2 ** i
        scale = 1.0 + torch.arange(DET_B).view(DET_B, 1, 1)
        out[i] = scale * torch.randn(DET_B, H * W, C, generator=g) + 2 * torch.randn(DET_B, 1, C, generator=g)
    return out


def tokens_to_maps(tok, hw, dtype):
    """{stage: [B, H*W, C]} -> the NCHW maps input_proj takes."""
    return [tok[i].to(dtype).view(DET_B, H, W, -1).permute(0, 3, 1, 2) for i, (H, W) in zip((1, 2, 3), stage_grids(hw)[1:])]


def level_slices(hw):
    """[(name, rows of dim 1 of src)] of the four levels."""
    out, s = [], 0
    for l, (H, W) in enumerate(level_shapes(hw)):
        out.append((f"level {l} {H}x{W}", slice(s, s + H * W)))
        s += H * W
    return out


def map_tokens(m: torch.Tensor) -> torch.Tensor:
    """NCHW map -> tokens [B, H*W, C]."""
    return m.flatten(2).transpose(1, 2)


def emulated(oracle, fn, *a, **kw):
    with oracle.f16_operands():
        return fn(*a, **kw)


@functools.lru_cache(maxsize=None)
def seam_refs(hw):
    """Backbone seams of det_images(hw): the float64 maps, the float64 tokens the output norms read, and the maps under
    f16_operands."""
    cfg, sd = det_config(), det_sd(F64)
    x = det_pixels(det_images(hw), F64)
    outs, pre = swin_seams(sd, cfg, x)
    emul = emulated(G, swin_seams, sd, cfg, x)[0]
    return outs, pre, emul


def outnorm_refs(hw, j: int):
    """The output norm of stage out_indices[j] on its own, on the float64 pre-norm tokens rounded to f32 (what the GPU test
    uploads): (f32 tokens [B*H*W, C], float64 LayerNorm of them, float32 LayerNorm of them)."""
    cfg = det_config()
    x32 = seam_refs(hw)[1][j].float().reshape(-1, seam_refs(hw)[1][j].shape[-1])
    name = f"backbone.0.norm{cfg.out_indices[j]}"
    return x32, G._ln(x32.double(), det_sd(F64), name), G._ln(x32, det_sd(F32), name)


@functools.lru_cache(maxsize=None)
def proj_refs(hw):
    """input_proj alone on proj_tokens(hw): (float64 src, the same under f16_operands)."""
    cfg, sd = det_config(), det_sd(F64)
    maps = tokens_to_maps(proj_tokens(hw), hw, F64)
    return input_proj(sd, cfg, maps), emulated(G, input_proj, sd, cfg, maps)


@functools.lru_cache(maxsize=None)
def detector_src_refs(hw):
    """stages["src"] of gdino_ref.detector_forward on det_images(hw) in float64 and under f16_operands."""
    cfg, sd = det_config(), det_sd(F64)
    x = det_pixels(det_images(hw), F64)
    sm, pid = G.text_masks_and_position_ids(list(DET_IDS))
    out = []
    for emul in (False, True):
        st = {}
        if emul:
            emulated(G, G.detector_forward, sd, cfg, x, det_text().double(), sm, pid, stages=st)
        else:
            G.detector_forward(sd, cfg, x, det_text().double(), sm, pid, stages=st)
        out.append(st["src"])
    return tuple(out)
