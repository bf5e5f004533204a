"""Pillow-exact resize on the GPU (bilinear, bicubic, Lanczos): host side (coefficient tables, plan cache).

The reference resizes with PIL (torchvision `F.resize` on a PIL image -> `Image.resize(BILINEAR)`), once for the
detector (GD/datasets/transforms.py:87-117) and once for SAM (SA/utils/transforms.py:26-31).  Pillow's 8-bit
resampler is integer arithmetic on 22-bit fixed-point weights; the weights and sample bounds are computed here
exactly as `precompute_coeffs` / `normalize_coeffs_8bpc` (Pillow 12.2 src/libImaging/Resample.c) do, in the same
double-precision operation order, and the two passes run in `ink_resize_u8`.  The inpainting stage resizes with the
bicubic and Lanczos filters and single-channel masks as well (inpaint_ControlNet.py:150-151, 176,
inpaint_SDXL.py:23-24, 31): `pil_resize_coeffs` builds the tables for all three filters, and the same entry point
runs them.
"""
from __future__ import annotations

import math
from typing import Dict, Tuple

import numpy as np
import torch

from ._lru import LRU

PRECISION_BITS = 32 - 8 - 2


def _bilinear(x: float) -> float:
    if x < 0.0:
        x = -x
    return 1.0 - x if x < 1.0 else 0.0


def _bicubic(x: float) -> float:
    a = -0.5
    if x < 0.0:
        x = -x
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


def _sinc(x: float) -> float:
    if x == 0.0:
        return 1.0
    x = x * math.pi
    return math.sin(x) / x


def _lanczos(x: float) -> float:
    return _sinc(x) * _sinc(x / 3) if -3.0 <= x < 3.0 else 0.0


# Pillow's filters (Resample.c bilinear_filter / bicubic_filter / lanczos_filter) with their supports
FILTERS = {"bilinear": (_bilinear, 1.0), "bicubic": (_bicubic, 2.0), "lanczos": (_lanczos, 3.0)}


def pil_resize_coeffs(in_size: int, out_size: int, filter: str = "bilinear") -> Tuple[np.ndarray, np.ndarray]:
    """(bounds int32 [out, 2] = (xmin, count), coef int32 [out, ksize]) of one axis for one of Pillow's filters."""
    fn, fsupport = FILTERS[filter]
    scale = in_size / out_size
    filterscale = scale if scale >= 1.0 else 1.0
    support = fsupport * filterscale
    ksize = int(math.ceil(support)) * 2 + 1
    ss = 1.0 / filterscale
    bounds = np.zeros((out_size, 2), dtype=np.int32)
    coef = np.zeros((out_size, ksize), dtype=np.int32)
    one = float(1 << PRECISION_BITS)
    for xx in range(out_size):
        center = 0.0 + (xx + 0.5) * scale
        xmin = int(center - support + 0.5)           # (int): truncation toward zero, as in C
        if xmin < 0:
            xmin = 0
        xmax = int(center + support + 0.5)
        if xmax > in_size:
            xmax = in_size
        xmax -= xmin
        ws = []
        ww = 0.0
        for x in range(xmax):
            w = fn(((x + xmin) - center + 0.5) * ss)
            ws.append(w)
            ww += w
        for x in range(xmax):
            k = ws[x] / ww if ww != 0.0 else ws[x]
            coef[xx, x] = int(-0.5 + k * one) if k < 0 else int(0.5 + k * one)
        bounds[xx, 0], bounds[xx, 1] = xmin, xmax
    return bounds, coef


def pil_bilinear_coeffs(in_size: int, out_size: int) -> Tuple[np.ndarray, np.ndarray]:
    """(bounds int32 [out, 2] = (xmin, count), coef int32 [out, ksize]) of one axis."""
    return pil_resize_coeffs(in_size, out_size, "bilinear")


class ResizePlan:
    """Device-resident tables for one (h, w) -> (oh, ow) resize."""

    def __init__(self, h: int, w: int, oh: int, ow: int, device, filter: str = "bilinear", channels: int = 3):
        self.h, self.w, self.oh, self.ow = h, w, oh, ow
        dev = torch.device(device)
        self.xb = self.xk = self.yb = self.yk = None
        self.kx = self.ky = 0
        if ow != w:
            b, k = pil_resize_coeffs(w, ow, filter)
            self.xb, self.xk, self.kx = torch.from_numpy(b).to(dev), torch.from_numpy(k).to(dev), k.shape[1]
        if oh != h:
            b, k = pil_resize_coeffs(h, oh, filter)
            self.yb, self.yk, self.ky = torch.from_numpy(b).to(dev), torch.from_numpy(k).to(dev), k.shape[1]
        self.tmp = torch.empty((h, ow, channels), device=dev, dtype=torch.uint8) if (ow != w and oh != h) else None


_PLANS = LRU(32)      # (source size, target size) pairs seen recently; a plan is a few hundred KB of tables


def plan_for(h: int, w: int, oh: int, ow: int, device, filter: str = "bilinear", channels: int = 3) -> ResizePlan:
    key = (h, w, oh, ow, str(device), filter, channels)
    return _PLANS.get_or_make(key, lambda: ResizePlan(h, w, oh, ow, device, filter, channels))
