"""numpy restatement of the reference's pre- and post-processing around the diffusion pipe
(InkLayer/inpainting/inpaint_ControlNet.py:49-184, inpaint_single_layer.py:34-78, inpaint_SDXL.py:13-33): the stages
(a)-(h) of csrc/inpaint_ops.hip with the same float types and the same operation order, and the three compositions.
It builds its own tables with math.exp / math.sin and imports nothing of the package.  The Pillow stages are pinned to
Pillow itself in tests/test_inpaint_ref_cpu.py; the OpenCV stages (b), (c), (f), (g) restate OpenCV's published
algorithm and are not pinned to cv2."""
import math

import numpy as np

F32 = np.float32
PRECISION_BITS = 32 - 8 - 2

PROMPT = ("high quality black and white line drawing, clean precise lines, detailed sketch, professional illustration, "
          "sharp edges")
NEGATIVE = "blurry, smudged, messy lines, low quality, artifacts, noise, distorted, pixelated"
SDXL_PROMPT = "black and white sketch, complete lines"


# ---- generated input -------------------------------------------------------------------------------------------------
def make_sketch(shape, seed=0):
    """White page, dark strokes, 30 % of the pixels coloured noise -> (rgb uint8 [H, W, 3], mask uint8 [H, W] 0 / 255)."""
    H, W = shape
    rng = np.random.default_rng(seed)
    img = np.full((H, W, 3), 255, np.uint8)
    yy, xx = np.mgrid[0:H, 0:W]
    for k in range(5):
        cy, cx, r = H * (0.2 + 0.15 * k), W * (0.25 + 0.12 * k), min(H, W) * (0.15 + 0.05 * k)
        ring = np.abs(np.hypot(yy - cy, xx - cx) - r) < 1.5
        img[ring] = 10 + 12 * k
    img[(yy + 2 * xx) % 37 < 2] = 40
    noisy = rng.random((H, W)) < 0.30
    img[noisy] = rng.integers(0, 256, (int(noisy.sum()), 3), dtype=np.uint8)
    mask = np.zeros((H, W), np.uint8)
    mask[H // 4:H // 4 + H // 3, W // 3:W // 3 + W // 2] = 255
    mask[np.hypot(yy - H * 0.7, xx - W * 0.3) < min(H, W) * 0.12] = 255
    return img, mask


# ---- (a) contrast, luma ----------------------------------------------------------------------------------------------
def luma(rgb):
    a = rgb.astype(np.int64)
    return ((19595 * a[..., 0] + 38470 * a[..., 1] + 7471 * a[..., 2] + 0x8000) >> 16).astype(np.uint8)


def gray_rgb(rgb):
    return np.repeat(luma(rgb)[..., None], 3, axis=2)


def contrast_mean(rgb):
    L = luma(rgb)
    n = L.size
    return (2 * int(L.astype(np.int64).sum()) + n) // (2 * n)


def contrast(rgb, factor=1.2):
    mean = contrast_mean(rgb)
    t = F32(mean) + F32(factor) * (rgb.astype(np.int32) - mean).astype(F32)
    out = np.trunc(np.clip(t, F32(0), F32(255))).astype(np.uint8)
    out[t <= 0] = 0
    out[t >= 255] = 255
    return out


# ---- borders ---------------------------------------------------------------------------------------------------------
def _idx(n, r, mode):
    i = np.arange(-r, n + r)
    if mode == "reflect101":
        i = np.where(i < 0, -i, i)
        return np.where(i >= n, 2 * n - 2 - i, i)
    return np.clip(i, 0, n - 1)                         # replicate


def _pad(a, r, mode):
    return a[_idx(a.shape[0], r, mode)][:, _idx(a.shape[1], r, mode)]


# ---- (b) bilateral ---------------------------------------------------------------------------------------------------
BILATERAL_TAPS = [(i, j) for i in range(-2, 3) for j in range(-2, 3) if i * i + j * j <= 4]


def bilateral_tables(sigma_color=50.0, sigma_space=50.0):
    sw = np.array([math.exp(-(i * i + j * j) / (2.0 * sigma_space * sigma_space)) for i, j in BILATERAL_TAPS], F32)
    cw = np.array([math.exp(-(d * d) / (2.0 * sigma_color * sigma_color)) for d in range(768)], F32)
    return sw, cw


def bilateral(rgb):
    H, W = rgb.shape[:2]
    sw, cw = bilateral_tables()
    p = _pad(rgb, 2, "reflect101").astype(np.int32)
    c0 = rgb.astype(np.int32)
    wsum = np.zeros((H, W), F32)
    acc = np.zeros((H, W, 3), F32)
    for k, (i, j) in enumerate(BILATERAL_TAPS):
        q = p[2 + i:2 + i + H, 2 + j:2 + j + W]
        d = np.abs(q - c0).sum(axis=2)
        w = sw[k] * cw[d]
        wsum = wsum + w
        acc = acc + q.astype(F32) * w[..., None]
    return np.rint(acc * (F32(1.0) / wsum)[..., None]).astype(np.uint8)


# ---- (c) mask preparation --------------------------------------------------------------------------------------------
def dilate3(m):
    H, W = m.shape
    p = np.zeros((H + 2, W + 2), np.uint8)
    p[1:-1, 1:-1] = m
    out = m.copy()
    for i in range(3):
        for j in range(3):
            out = np.maximum(out, p[i:i + H, j:j + W])
    return out


def blur3_u8(m):
    H, W = m.shape
    p = _pad(m, 1, "reflect101").astype(np.int32)
    k = (1, 2, 1)
    s = np.zeros((H, W), np.int32)
    for i in range(3):
        for j in range(3):
            s += k[i] * k[j] * p[i:i + H, j:j + W]
    return ((s + 8) >> 4).astype(np.uint8)


def mask_prepare(m, dilate_iterations=1, blur=True):
    for _ in range(dilate_iterations):
        m = dilate3(m)
    return blur3_u8(m) if blur else m


# ---- (d) Pillow's 8-bit resampler ------------------------------------------------------------------------------------
def _sinc(x):
    if x == 0.0:
        return 1.0
    x = x * math.pi
    return math.sin(x) / x


def _lanczos(x):
    return _sinc(x) * _sinc(x / 3) if -3.0 <= x < 3.0 else 0.0


def _bicubic(x):
    a = -0.5
    if x < 0.0:
        x = -x
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


def _bilinear(x):
    if x < 0.0:
        x = -x
    return 1.0 - x if x < 1.0 else 0.0


FILTERS = {"bilinear": (_bilinear, 1.0), "bicubic": (_bicubic, 2.0), "lanczos": (_lanczos, 3.0)}


def resize_coeffs(in_size, out_size, filt):
    fn, fsupport = FILTERS[filt]
    scale = in_size / out_size
    filterscale = max(scale, 1.0)
    support = fsupport * filterscale
    ksize = int(math.ceil(support)) * 2 + 1
    ss = 1.0 / filterscale
    one = float(1 << PRECISION_BITS)
    K = np.zeros((out_size, in_size), np.int64)
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), in_size) - xmin
        assert xmax <= ksize
        ws = [fn((x + xmin - center + 0.5) * ss) for x in range(xmax)]
        ww = 0.0
        for w in ws:
            ww += w
        for x, w in enumerate(ws):
            k = w / ww if ww != 0.0 else w
            K[xx, xmin + x] = int(-0.5 + k * one) if k < 0 else int(0.5 + k * one)
    return K


def _resize_axis(a, out_size, filt, axis):
    K = resize_coeffs(a.shape[axis], out_size, filt)
    s = np.tensordot(K.astype(np.float64), a.astype(np.float64), axes=(1, axis))      # exact: every sum < 2^53
    v = (s.astype(np.int64) + (1 << 21)) >> 22
    return np.moveaxis(np.clip(v, 0, 255).astype(np.uint8), 0, axis)


def resize(a, oh, ow, filt):
    """Image.resize((ow, oh), filt) of uint8 [H, W] or [H, W, 3]: horizontal pass first, each pass stored as u8."""
    if a.shape[1] != ow:
        a = _resize_axis(a, ow, filt, 1)
    if a.shape[0] != oh:
        a = _resize_axis(a, oh, filt, 0)
    return a.copy()


# ---- (e) condition ---------------------------------------------------------------------------------------------------
def condition(rgb, mask):
    c = rgb.astype(F32) / F32(255.0)
    c[mask >= 128] = F32(-1.0)
    return np.ascontiguousarray(c.transpose(2, 0, 1)[None])


# ---- (f) adaptive-threshold clean-up ---------------------------------------------------------------------------------
def cv_gray(rgb):
    a = rgb.astype(np.int64)
    return ((9798 * a[..., 0] + 19235 * a[..., 1] + 3735 * a[..., 2] + 16384) >> 15).astype(np.uint8)


def gauss11():
    c = [math.exp(-0.125 * (i - 5) * (i - 5)) for i in range(11)]
    S = 0.0
    for v in c:
        S += v
    return np.array([v * (1.0 / S) for v in c], F32)


def adaptive_thresh(gray):
    H, W = gray.shape
    k = gauss11()
    p = _pad(gray, 5, "replicate").astype(F32)
    rows = k[0] * p[:, 0:W]
    for t in range(1, 11):
        rows = rows + k[t] * p[:, t:t + W]
    s = k[5] * rows[5:5 + H]
    for t in range(1, 6):
        s = s + k[5 + t] * (rows[5 + t:5 + t + H] + rows[5 - t:5 - t + H])
    mean = np.clip(np.rint(s), 0, 255).astype(np.int32)
    return np.where(gray.astype(np.int32) > mean - 2, 255, 0).astype(np.uint8)


def cleanup(result_rgb):
    thresh = adaptive_thresh(cv_gray(result_rgb))
    return np.where(thresh[..., None] == 255, np.uint8(255), result_rgb), thresh


# ---- (g) soft blend --------------------------------------------------------------------------------------------------
def gauss3_f64():
    c = [math.exp(-0.5), 1.0, math.exp(-0.5)]
    inv = 1.0 / (c[0] + c[1] + c[2])
    return c[1] * inv, c[0] * inv                        # centre, side


def soft_mask(mask):
    H, W = mask.shape
    kc, ks = gauss3_f64()
    m = _pad(mask.astype(np.float64) / 255.0, 1, "reflect101")
    rows = m[:, 1:1 + W] * kc + (m[:, 0:W] + m[:, 2:2 + W]) * ks
    s = rows[1:1 + H] * kc + (rows[0:H] + rows[2:2 + H]) * ks
    return np.clip(s, 0.0, 1.0)


def soft_blend(clean, original, mask):
    soft = soft_mask(mask)[..., None]
    return (clean.astype(np.float64) * soft + original.astype(np.float64) * (1 - soft)).astype(np.uint8)


def postprocess(result_rgb, original_rgb, mask):
    return soft_blend(cleanup(result_rgb)[0], original_rgb, mask)


# ---- (h) finish ------------------------------------------------------------------------------------------------------
def box_weights(radius=0.5, passes=3):
    """Pillow's Gaussian-to-box rule (BoxBlur.c _gaussian_blur_radius, float arithmetic) -> (ww, fw) for box radius < 1."""
    sigma2 = F32(F32(radius) * F32(radius) / F32(passes))
    L = F32(math.sqrt(12.0 * float(sigma2) + 1.0))
    l = F32(math.floor((float(L) - 1.0) / 2.0))
    a = F32(F32(2 * l + 1) * F32(F32(l * F32(l + 1)) - F32(F32(3) * sigma2)))
    a = F32(a / F32(F32(6) * F32(sigma2 - F32(F32(l + 1) * F32(l + 1)))))
    r = F32(l + a)
    assert int(r) == 0
    ww = int(F32(1 << 24) / F32(F32(r * F32(2)) + F32(1)))
    return ww, ((1 << 24) - ww) // 2


def _box_pass(a, axis, ww, fw):
    a = np.moveaxis(a, axis, 0).astype(np.int64)
    p = a[_idx(a.shape[0], 1, "replicate")]
    out = (ww * a + fw * (p[:-2] + p[2:]) + (1 << 23)) >> 24
    return np.moveaxis(out.astype(np.uint8), 0, axis)


def box_blur(a, radius=0.5):
    """ImageFilter.GaussianBlur(radius) for radius < ~0.9 (box radius below 1), any channel count."""
    ww, fw = box_weights(radius)
    for axis in (1, 1, 1, 0, 0, 0):
        a = _box_pass(a, axis, ww, fw)
    return a


def unsharp(a, radius=0.5, percent=150, threshold=3):
    d = a.astype(np.int64) - box_blur(a, radius).astype(np.int64)
    q = np.abs(d) * percent // 100 * np.sign(d)          # C division: truncation toward zero
    return np.where(np.abs(d) > threshold, np.clip(a + q, 0, 255), a).astype(np.uint8)


def finish(rgb):
    return unsharp(gray_rgb(rgb))


# ---- compositions ----------------------------------------------------------------------------------------------------
def _call(pipe, image, mask, **kw):
    from PIL import Image
    return np.asarray(pipe(image=Image.fromarray(image), mask_image=Image.fromarray(mask), **kw).images[0].convert("RGB"))


def preprocess_image(rgb):
    return bilateral(contrast(rgb))


def controlnet_inpaint(pipe, rgb, mask, preprocess_input=True, postprocess_output=True, generator=None):
    import torch
    image, m = (preprocess_image(rgb), mask_prepare(mask)) if preprocess_input else (rgb, mask)
    inp = resize(image, 768, 768, "lanczos")
    mr = resize(m, 768, 768, "lanczos")
    out = None
    for _ in range(2):
        if out is not None:
            inp = resize(out, 768, 768, "lanczos")
        out = _call(pipe, inp, mr, prompt=PROMPT, negative_prompt=NEGATIVE, control_image=torch.from_numpy(condition(inp, mr)),
                    guidance_scale=9.0, num_inference_steps=30, controlnet_conditioning_scale=1.2, generator=generator)
    out = resize(out, rgb.shape[0], rgb.shape[1], "lanczos")
    if postprocess_output:
        out = postprocess(out, rgb, mask)
    return finish(out)


def single_layer_inpaint(pipe, rgb, mask, prompt, generator=None):
    """-> (result rgb, rgba layer)"""
    import torch
    image, m = preprocess_image(rgb), mask_prepare(mask)
    inp = resize(image, 768, 768, "lanczos")
    mr = resize(m, 768, 768, "lanczos")
    out = _call(pipe, inp, mr, prompt=prompt, negative_prompt=NEGATIVE, control_image=torch.from_numpy(condition(inp, mr)),
                guidance_scale=7.0, num_inference_steps=30, controlnet_conditioning_scale=0.6, generator=generator)
    out = resize(out, rgb.shape[0], rgb.shape[1], "lanczos")
    rgba = np.zeros(out.shape[:2] + (4,), np.uint8)
    inside = m > 128
    rgba[..., :3][inside] = out[inside]
    rgba[..., 3][inside] = 255
    return out, rgba


def sdxl_inpaint(pipe, rgb, mask, generator=None):
    out = _call(pipe, resize(rgb, 1024, 1024, "bicubic"), resize(mask, 1024, 1024, "bicubic"), prompt=SDXL_PROMPT,
                guidance_scale=8.0, num_inference_steps=20, strength=0.99, generator=generator)
    return gray_rgb(resize(out, rgb.shape[0], rgb.shape[1], "lanczos"))
