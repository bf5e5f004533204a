"""Thin torch-tensor wrappers over the C ABI (PyTorch = device memory + streams only).

Every function enqueues hand-written HIP kernels on torch's current stream.
Tensors must live on the GPU; there is no CPU path.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional, Sequence, Tuple

import torch

from . import _lib
from ._lib import InkAttn, InkGemm, check

ACT = {None: 0, "none": 0, "gelu": 1, "relu": 2}
F16, F32 = torch.float16, torch.float32


_GEMM_TRACE = None


def set_gemm_trace(lst) -> None:
    """bench.py instrumentation: when `lst` is a list, every gemm() launch is bracketed by two HIP events
    on the launch stream and (flops, start, end) is appended; None switches it off."""
    global _GEMM_TRACE
    _GEMM_TRACE = lst


_ATTN_TRACE = None


def set_attn_trace(lst) -> None:
    """bench.py instrumentation: when `lst` is a list, every flash_attn() launch is bracketed by two HIP events on
    the launch stream and (n_batch, n_heads, n_q, n_k, head_dim, bias_mode, rows_q, start, end) is appended."""
    global _ATTN_TRACE
    _ATTN_TRACE = lst


def tracing_off() -> bool:
    """No per-launch event bracketing requested (a captured graph would bypass it)."""
    return _GEMM_TRACE is None and _ATTN_TRACE is None


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)
_cur_device = getattr(torch._C, "_cuda_getDevice", None)


def _stream() -> int:
    """Raw handle of torch's current HIP stream.  Called once per kernel launch: the public
    `torch.cuda.current_stream()` builds a Stream object (~8 us); the raw accessor is ~0.3 us."""
    if _raw_stream is not None and _cur_device is not None:
        return _raw_stream(_cur_device())
    return torch.cuda.current_stream().cuda_stream


def own_f32(t: torch.Tensor, dev) -> torch.Tensor:
    """An engine-owned contiguous f32 copy of a parameter on `dev`.  A tensor that is only a VIEW into a larger
    storage (e.g. a slice of dist.broadcast_state_dict's 1 GiB flat buckets) is cloned, so that the engines do not
    keep those buckets alive through a few kilobytes of biases and norm weights."""
    t = t.detach().to(dev, F32).contiguous()
    if t.untyped_storage().nbytes() > t.numel() * t.element_size():
        t = t.clone()
    return t


def _p(t: Optional[torch.Tensor]) -> Optional[int]:
    if t is None:
        return None
    assert t.is_cuda, "InkLayer HIP ops need GPU tensors (no CPU fallback)"
    return t.data_ptr()


def gemm(a: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor] = None, *,
         act: Optional[str] = None, residual: Optional[torch.Tensor] = None,
         col_scale: Optional[torch.Tensor] = None, row_map: Optional[torch.Tensor] = None,
         out: Optional[torch.Tensor] = None, out_dtype: torch.dtype = F32,
         out_rows: Optional[int] = None) -> torch.Tensor:
    """out[row_map[m]] = residual[row_map[m]] + col_scale * act(a[m] @ w.T + bias).

    a: f16 [M, K] (row stride arbitrary, multiple of 8), w: f16 [N, K]."""
    assert a.dtype == F16 and w.dtype == F16
    assert a.dim() == 2 and w.dim() == 2 and a.stride(1) == 1 and w.stride(1) == 1
    M, K = a.shape
    N = w.shape[0]
    assert w.shape[1] == K
    p = InkGemm()
    if out is None:
        rows = out_rows if out_rows is not None else M
        out = torch.empty((rows, N), device=a.device, dtype=out_dtype)
    assert out.dim() == 2 and out.stride(1) == 1 and out.shape[1] == N
    p.A, p.W, p.C = a.data_ptr(), w.data_ptr(), out.data_ptr()
    p.bias, p.col_scale = _p(bias), _p(col_scale)
    p.residual, p.row_map = _p(residual), _p(row_map)
    if bias is not None:
        assert bias.dtype == F32 and bias.numel() == N
    if col_scale is not None:
        assert col_scale.dtype == F32 and col_scale.numel() == N
    if residual is not None:
        assert residual.dtype == F32 and residual.stride(1) == 1 and residual.shape[1] == N
        p.ldr = residual.stride(0)
    if row_map is not None:
        assert row_map.dtype == torch.int32 and row_map.numel() == M
    p.M, p.N, p.K = M, N, K
    p.lda, p.ldw, p.ldc = a.stride(0), w.stride(0), out.stride(0)
    p.act = ACT[act]
    p.c_f16 = 1 if out.dtype == F16 else 0
    assert out.dtype in (F16, F32)
    if _GEMM_TRACE is None:
        check(_lib.lib().ink_gemm_f16(C.byref(p), _stream()), "ink_gemm_f16")
    else:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        check(_lib.lib().ink_gemm_f16(C.byref(p), _stream()), "ink_gemm_f16")
        e1.record()
        _GEMM_TRACE.append((2.0 * M * N * K, e0, e1, (M, N, K, act or '-', 'res' if residual is not None else '-',
                                                      'map' if row_map is not None else '-', 'f16' if p.c_f16 else 'f32')))
    return out


def layernorm_rows(x: torch.Tensor, gamma: Optional[torch.Tensor], beta: Optional[torch.Tensor],
                   eps: float, *, gather: Optional[torch.Tensor] = None,
                   out_dtype: torch.dtype = F16, out: Optional[torch.Tensor] = None,
                   out2: Optional[torch.Tensor] = None, act: Optional[str] = None,
                   split: bool = False, add: Optional[torch.Tensor] = None,
                   add_batch_rows: Optional[torch.Tensor] = None, rows_per_batch: int = 0,
                   split_f32: Optional[torch.Tensor] = None) -> torch.Tensor:
    """LayerNorm over the last dim of f32 x [R, C]; optional row gather (-1 -> zero row).
    `out2` (the other of f16/f32, same shape/stride) receives a second copy in the same pass.
    split=True: the f16 output is a split-f16 GEMM operand [R, 3C] (see add_split_f16); split_f32 (contiguous f32
    [R, C]) then receives the f32 result in the same pass."""
    assert x.dtype == F32 and x.dim() == 2 and x.stride(1) == 1
    Cdim = x.shape[1]
    rows = gather.numel() if gather is not None else x.shape[0]
    wcols = 3 * Cdim if split else Cdim
    if split:
        assert out_dtype == F16 and out2 is None
    if out is None:
        out = torch.empty((rows, wcols), device=x.device, dtype=out_dtype)
    assert out.shape == (rows, wcols) and out.stride(1) == 1
    oh = out.data_ptr() if out.dtype == F16 else None
    of = out.data_ptr() if out.dtype == F32 else None
    if out2 is not None:
        assert out2.shape == out.shape and out2.stride(0) == out.stride(0) and out2.dtype != out.dtype
        if out2.dtype == F16:
            oh = out2.data_ptr()
        else:
            of = out2.data_ptr()
    if split_f32 is not None:
        assert split and out.stride(0) == 3 * Cdim and split_f32.dtype == F32 and split_f32.is_contiguous()
        assert tuple(split_f32.shape) == (rows, Cdim)
        of = split_f32.data_ptr()
    if gather is not None:
        assert gather.dtype == torch.int32
    if add is not None:
        # LN(x[r] + add[add_batch_rows[r // rows_per_batch] + r % rows_per_batch]) (add_batch_rows None: add[r])
        assert gather is None and add.dtype == F32 and add.dim() == 2 and add.stride(1) == 1 and add.shape[1] == Cdim
        if add_batch_rows is not None:
            assert add_batch_rows.dtype == torch.int32 and add_batch_rows.is_cuda and rows_per_batch > 0
            assert add_batch_rows.numel() * rows_per_batch == rows
        else:
            rows_per_batch = rows
    check(_lib.lib().ink_layernorm_rows(x.data_ptr(), x.stride(0), _p(gamma), _p(beta), eps,
                                        _p(gather), rows, Cdim, oh, of, out.stride(0), ACT[act], int(split),
                                        _p(add), add.stride(0) if add is not None else 0, _p(add_batch_rows),
                                        rows_per_batch, _stream()), "ink_layernorm_rows")
    return out


def add_cvt_f16(a: torch.Tensor, b: Optional[torch.Tensor] = None,
                out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """f16(a + b) for contiguous f32 tensors; b may be a (leading-dim) broadcast of a."""
    assert a.dtype == F32 and a.is_contiguous()
    nb = 0
    if b is not None:
        assert b.dtype == F32 and b.is_contiguous() and a.numel() % b.numel() == 0
        nb = b.numel()
    if out is None:
        out = torch.empty(a.shape, device=a.device, dtype=F16)
    assert out.dtype == F16 and out.is_contiguous() and out.numel() == a.numel()
    check(_lib.lib().ink_add_cvt_f16(a.data_ptr(), _p(b), nb, out.data_ptr(), a.numel(), _stream()),
          "ink_add_cvt_f16")
    return out


def add_split_f16(a: torch.Tensor, b: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Split-f16 GEMM operand of v = a + b (contiguous f32 [R, C]; b a leading-dim broadcast): f16 [R, 3C] =
    [hi | (v - hi) * 64 | hi / 64].  gemm() against `split_weight(W)` then yields v @ W.T at fp32-grade accuracy."""
    assert a.dtype == F32 and a.is_contiguous() and a.dim() == 2
    nb = 0
    if b is not None:
        assert b.dtype == F32 and b.is_contiguous() and a.numel() % b.numel() == 0
        nb = b.numel()
    R, Cn = a.shape
    out = torch.empty((R, 3 * Cn), device=a.device, dtype=F16)
    check(_lib.lib().ink_add_split_f16(a.data_ptr(), _p(b), nb, out.data_ptr(), a.numel(), Cn, _stream()),
          "ink_add_split_f16")
    return out


def split_weight(w32: torch.Tensor) -> torch.Tensor:
    """f32 [..., K] -> f16 [..., 3K] = [W_hi | W_hi / 64 | (W - W_hi) * 64]: the weight side of a split-f16 GEMM
    (load-time re-layout, like the f16 cast of the other matrices)."""
    w32 = w32.to(torch.float32)
    hi = w32.to(F16)
    lo = ((w32 - hi.to(torch.float32)) * 64.0).to(F16)
    return torch.cat([hi, (hi.to(torch.float32) / 64.0).to(F16), lo], dim=-1).contiguous()


def add_f32(a: torch.Tensor, b: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """a + b (f32), b broadcast along the leading dims of a (periodic in flat index)."""
    assert a.dtype == F32 and b.dtype == F32 and a.is_contiguous() and b.is_contiguous()
    assert a.numel() % b.numel() == 0
    if out is None:
        out = torch.empty(a.shape, device=a.device, dtype=F32)
    assert out.is_contiguous() and out.numel() == a.numel()
    check(_lib.lib().ink_add_f32(a.data_ptr(), b.data_ptr(), b.numel(), out.data_ptr(), a.numel(),
                                 _stream()), "ink_add_f32")
    return out


def flash_attn(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, *, n_batch: int, n_heads: int,
               head_dim: int, scale: float, n_q: Optional[int] = None, n_k: Optional[int] = None,
               rel_h: Optional[torch.Tensor] = None, rel_w: Optional[torch.Tensor] = None,
               rel_aug: Optional[torch.Tensor] = None, grid_w: int = 0,
               dense_bias: Optional[torch.Tensor] = None, dense_mask: Optional[torch.Tensor] = None,
               q_batch_rows: Optional[torch.Tensor] = None,
               kv_batch_rows: Optional[torch.Tensor] = None,
               tok_rows: Optional[torch.Tensor] = None, pad_k: Optional[torch.Tensor] = None,
               pad_v: Optional[torch.Tensor] = None,
               out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """softmax(scale*q@k^T + bias)@v for f16 row views q [.., >=H*hd], k/v [.., >=H*hd].

    q/k/v may be column slices of one packed qkv buffer (only the row stride matters).
    Batch entry b uses rows q_batch_rows[b] + [0, n_q) of q and kv_batch_rows[b] + [0, n_k) of
    k/v (defaults b*n_q, b*n_k); the output is dense [n_batch*n_q, H*hd].
    With tok_rows (int32 [n_batch, n_q], rel_aug mode) token i of window b is row tok_rows[b, i] of
    q, k, v and `out` (which is then required); -1 marks window padding, whose keys are pad_k / pad_v.
    """
    for t in (q, k, v):
        assert t.dtype == F16 and t.dim() == 2 and t.stride(1) == 1 and t.is_cuda
    if n_q is None:
        n_q = q.shape[0] // n_batch
    if n_k is None:
        n_k = k.shape[0] // n_batch
    if tok_rows is not None:
        assert rel_aug is not None and out is not None and n_q == n_k
        assert tok_rows.dtype == torch.int32 and tok_rows.is_cuda and tok_rows.numel() == n_batch * n_q
        for t in (pad_k, pad_v):
            assert t is not None and t.dtype == F16 and t.is_contiguous() and t.numel() == n_heads * head_dim
        assert out.dtype == F16 and out.stride(1) == 1
        # (the window kernel addresses O, and the gathered q / k / v rows, through 32-bit byte offsets)
        assert out.shape[0] * out.stride(0) * 2 < 2 ** 31 and q.shape[0] * q.stride(0) * 2 < 2 ** 32
    else:
        if out is None:
            out = torch.empty((n_batch * n_q, n_heads * head_dim), device=q.device, dtype=F16)
        assert out.dtype == F16 and out.shape[0] == n_batch * n_q and out.stride(1) == 1
    p = InkAttn()
    p.Q, p.K, p.V, p.O = q.data_ptr(), k.data_ptr(), v.data_ptr(), out.data_ptr()
    p.ldq, p.ldk, p.ldv, p.ldo = q.stride(0), k.stride(0), v.stride(0), out.stride(0)
    p.n_batch, p.n_heads, p.n_q, p.n_k, p.head_dim = n_batch, n_heads, n_q, n_k, head_dim
    p.scale = scale
    p.grid_w = grid_w
    for name, t in (("q_batch_rows", q_batch_rows), ("kv_batch_rows", kv_batch_rows)):
        if t is not None:
            assert t.dtype == torch.int32 and t.numel() == n_batch and t.is_cuda
            setattr(p, name, t.data_ptr())
    if dense_bias is not None:
        assert dense_bias.dtype == F32 and dense_bias.is_contiguous() and dense_bias.shape == (n_heads, n_q, 64)
        p.bias_mode, p.dense_bias = 3, dense_bias.data_ptr()
        if dense_mask is not None:
            assert dense_mask.dtype == F32 and dense_mask.is_contiguous() and dense_mask.shape[1:] == (n_q, 64)
            p.dense_mask, p.n_mask = dense_mask.data_ptr(), dense_mask.shape[0]
    elif rel_aug is not None:
        assert rel_aug.dtype == F16 and rel_aug.is_contiguous()
        p.bias_mode, p.rel_aug = 2, rel_aug.data_ptr()
        if tok_rows is not None:
            p.tok_rows, p.pad_k, p.pad_v = tok_rows.data_ptr(), pad_k.data_ptr(), pad_v.data_ptr()
    elif rel_h is not None:
        assert rel_h.dtype == rel_w.dtype and rel_h.dtype in (F32, F16)      # f16 tables: relpos_bias(..., f16_tables=True)
        assert rel_h.is_contiguous() and rel_w.is_contiguous()
        p.bias_mode, p.rel_h, p.rel_w = 1, rel_h.data_ptr(), rel_w.data_ptr()
        p.rel_f16 = int(rel_h.dtype == F16)
    else:
        p.bias_mode = 0
    if _ATTN_TRACE is None:
        check(_lib.lib().ink_flash_attn(C.byref(p), _stream()), "ink_flash_attn")
    else:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        check(_lib.lib().ink_flash_attn(C.byref(p), _stream()), "ink_flash_attn")
        e1.record()
        _ATTN_TRACE.append((n_batch, n_heads, n_q, n_k, head_dim, int(p.bias_mode), int(out.shape[0]), e0, e1))
    return out


SWIN_ATTN_WINDOWS = (7, 12)        # the window sizes csrc/attention_swin.hip serves


def swin_attn(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, *, n_windows: int, n_heads: int, ws: int, scale: float,
              bias_table: torch.Tensor, region: Optional[torch.Tensor] = None, nW: int = 0,
              out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Swin window attention, head_dim 32, bias and SW-MSA mask computed in the kernel (csrc/attention_swin.hip):
    softmax(scale*q@k^T + bias_table[h][rel(q, k)] + (-100 where region[w % nW] differs))@v per (window, head).

    q/k/v: f16 row views [n_windows*ws*ws, >= n_heads*32] (column slices of one packed qkv buffer: only the row stride
    matters), token i of window w in row w*ws*ws + i.  bias_table f32 [n_heads, (2*ws-1)**2] in logit units; region
    uint8 [nW, ws*ws] ids or None (unshifted block).  The output is dense f16 [n_windows*ws*ws, n_heads*32]."""
    assert ws in SWIN_ATTN_WINDOWS, f"swin_attn serves window sizes {SWIN_ATTN_WINDOWS}, not {ws}"
    rows = n_windows * ws * ws
    for t in (q, k, v):
        assert t.dtype == F16 and t.dim() == 2 and t.stride(1) == 1 and t.is_cuda
        assert t.shape[0] >= rows and t.shape[1] >= n_heads * 32 and t.stride(0) % 8 == 0 and t.data_ptr() % 16 == 0
    assert bias_table.dtype == F32 and bias_table.is_contiguous() and bias_table.is_cuda
    assert bias_table.shape == (n_heads, (2 * ws - 1) ** 2)
    if region is not None:
        assert region.dtype == torch.uint8 and region.is_contiguous() and region.is_cuda
        assert nW > 0 and region.shape == (nW, ws * ws) and n_windows % nW == 0
    if out is None:
        out = torch.empty((rows, n_heads * 32), device=q.device, dtype=F16)
    assert out.dtype == F16 and out.is_cuda and out.shape == (rows, n_heads * 32) and out.stride(1) == 1
    assert out.stride(0) % 8 == 0 and out.data_ptr() % 8 == 0
    check(_lib.lib().ink_swin_attn(q.data_ptr(), k.data_ptr(), v.data_ptr(), q.stride(0), k.stride(0), v.stride(0),
                                   out.data_ptr(), out.stride(0), n_windows, n_heads, ws, scale, bias_table.data_ptr(),
                                   _p(region), nW if region is not None else 0, _stream()), "ink_swin_attn")
    return out


def relpos_bias(q: torch.Tensor, rel_pos_h: torch.Tensor, rel_pos_w: torch.Tensor, *, S: int,
                n_batch: int, n_heads: int, head_dim: int, scale: float, out=None,
                tok_rows: Optional[torch.Tensor] = None, f16_tables: bool = False):
    """SAM decomposed rel-pos terms / scale, head_dim 80 (ViT-H) or 64 (ViT-B / ViT-L).  S == 64 -> (rel_h, rel_w) f32
    (f16 with f16_tables: SAM's own attention shape at head_dim 80 only); S == 14 -> rel_aug f16."""
    assert q.dtype == F16 and q.stride(1) == 1
    assert rel_pos_h.dtype == F32 and rel_pos_h.is_contiguous()
    assert rel_pos_w.dtype == F32 and rel_pos_w.is_contiguous()
    assert rel_pos_h.shape == (2 * S - 1, head_dim)
    n = n_batch * n_heads * S * S
    fn = _lib.lib().ink_relpos_bias
    if S == 64 and f16_tables:
        oh, ow = out if out is not None else (torch.empty((n, 64), device=q.device, dtype=F16),
                                              torch.empty((n, 64), device=q.device, dtype=F16))
        assert oh.dtype == F16 and ow.dtype == F16 and oh.numel() >= n * 64 and ow.numel() >= n * 64
        check(_lib.lib().ink_relpos_bias64_f16(q.data_ptr(), q.stride(0), rel_pos_h.data_ptr(), rel_pos_w.data_ptr(), n_batch,
                                               n_heads, head_dim, scale, oh.data_ptr(), ow.data_ptr(), _stream()),
              "ink_relpos_bias64_f16")
        return oh, ow
    if S == 64:
        oh, ow = out if out is not None else (torch.empty((n, 64), device=q.device, dtype=F32),
                                              torch.empty((n, 64), device=q.device, dtype=F32))
        assert oh.numel() >= n * 64 and ow.numel() >= n * 64
        check(fn(q.data_ptr(), q.stride(0), rel_pos_h.data_ptr(), rel_pos_w.data_ptr(), S, n_batch,
                 n_heads, head_dim, scale, None, oh.data_ptr(), ow.data_ptr(), None, _stream()),
              "ink_relpos_bias")
        return oh, ow
    aug = out if out is not None else torch.empty((n, 32), device=q.device, dtype=F16)
    assert aug.numel() >= n * 32
    if tok_rows is not None:
        assert tok_rows.dtype == torch.int32 and tok_rows.is_cuda and tok_rows.numel() == n_batch * S * S
    check(fn(q.data_ptr(), q.stride(0), rel_pos_h.data_ptr(), rel_pos_w.data_ptr(), S, n_batch,
             n_heads, head_dim, scale, tok_rows.data_ptr() if tok_rows is not None else None,
             None, None, aug.data_ptr(), _stream()), "ink_relpos_bias")
    return aug


def _resize_u8(image_u8: torch.Tensor, oh: int, ow: int, filter: str, out: Optional[torch.Tensor]) -> torch.Tensor:
    """Pillow's resampler on a contiguous uint8 [H, W] or [H, W, 3] CUDA tensor: the plan of tables for the sizes and
    the filter, then the one C call."""
    from .resize import plan_for
    assert image_u8.dtype == torch.uint8 and image_u8.is_cuda and image_u8.is_contiguous() and oh > 0 and ow > 0
    assert image_u8.dim() == 2 or (image_u8.dim() == 3 and image_u8.shape[2] == 3), "[H, W] or [H, W, 3] expected"
    h, w, ch = int(image_u8.shape[0]), int(image_u8.shape[1]), 1 if image_u8.dim() == 2 else 3
    shape = (oh, ow) if ch == 1 else (oh, ow, 3)
    if out is None:
        out = torch.empty(shape, device=image_u8.device, dtype=torch.uint8)
    assert out.dtype == torch.uint8 and out.is_contiguous() and tuple(out.shape) == shape
    pl = plan_for(h, w, oh, ow, image_u8.device, filter, ch)
    ptr = lambda t: t.data_ptr() if t is not None else None
    check(_lib.lib().ink_resize_u8(image_u8.data_ptr(), h, w, ch, out.data_ptr(), oh, ow, ptr(pl.xb), ptr(pl.xk), pl.kx,
                                   ptr(pl.yb), ptr(pl.yk), pl.ky, ptr(pl.tmp), _stream()), "ink_resize_u8")
    return out


def resize_bilinear_u8(image_u8: torch.Tensor, oh: int, ow: int, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """PIL `Image.resize((ow, oh), BILINEAR)` of an HWC uint8 RGB CUDA tensor, bit for bit (antialiased).  The same
    size returns the input itself."""
    assert image_u8.dim() == 3 and image_u8.shape[2] == 3
    if (oh, ow) == tuple(image_u8.shape[:2]):
        return image_u8
    return _resize_u8(image_u8, oh, ow, "bilinear", out)


def sam_patchify(image_u8: torch.Tensor, L: int, P: int, mean: Sequence[float],
                 std: Sequence[float], chan_reverse: bool, out: torch.Tensor, split: bool = False) -> torch.Tensor:
    """uint8 HWC (h,w <= L) -> normalised, zero-padded f16 im2col [ (L/P)^2, 3*P*P ] (split: [.., 3*3*P*P])."""
    assert image_u8.dtype == torch.uint8 and image_u8.is_cuda and image_u8.is_contiguous()
    h, w, c = image_u8.shape
    assert c == 3 and out.dtype == F16 and out.is_contiguous()
    assert out.numel() == (L // P) ** 2 * 3 * P * P * (3 if split else 1)
    m = (C.c_float * 3)(*mean)
    s = (C.c_float * 3)(*std)
    check(_lib.lib().ink_sam_patchify(image_u8.data_ptr(), h, w, L, P, m, s, int(chan_reverse), int(split),
                                      out.data_ptr(), _stream()), "ink_sam_patchify")
    return out


def im2col3x3(x: torch.Tensor, B: int, H: int, W: int, stride: int = 1, relu: bool = False,
              out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """f16 NHWC [B*H*W, C] -> [B*OH*OW, 9*C] (pad 1, stride 1 or 2, optional ReLU on the gathered values)."""
    assert x.dtype == F16 and x.is_contiguous() and x.shape[0] == B * H * W
    Cn = x.shape[1]
    OH, OW = (H - 1) // stride + 1, (W - 1) // stride + 1
    if out is None:
        out = torch.empty((B * OH * OW, 9 * Cn), device=x.device, dtype=F16)
    assert out.dtype == F16 and out.is_contiguous() and out.numel() >= B * OH * OW * 9 * Cn
    check(_lib.lib().ink_im2col3x3_f16(x.data_ptr(), B, H, W, Cn, stride, int(relu), out.data_ptr(), _stream()),
          "ink_im2col3x3_f16")
    return out


def sam_pe_encode(coords01: torch.Tensor, gauss: torch.Tensor,
                  add: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """[sin, cos](2*pi*((2c-1) @ G)) (+ add[n % n_add]) -> f32 [N, 2F]."""
    assert coords01.dtype == F32 and coords01.is_contiguous() and coords01.shape[-1] == 2
    assert gauss.dtype == F32 and gauss.is_contiguous() and gauss.shape[0] == 2
    N, Fd = coords01.numel() // 2, gauss.shape[1]
    if out is None:
        out = torch.empty((N, 2 * Fd), device=coords01.device, dtype=F32)
    assert out.dtype == F32 and out.is_contiguous() and tuple(out.shape) == (N, 2 * Fd)
    n_add = 0
    if add is not None:
        assert add.dtype == F32 and add.is_contiguous() and add.shape[-1] == 2 * Fd
        n_add = add.numel() // (2 * Fd)
    check(_lib.lib().ink_sam_pe_encode(coords01.data_ptr(), gauss.data_ptr(), N, Fd, _p(add), n_add,
                                       out.data_ptr(), _stream()), "ink_sam_pe_encode")
    return out


def sam_prompt_tokens(gauss: torch.Tensor, point_emb: torch.Tensor, not_a_point: torch.Tensor, out_tok: torch.Tensor,
                      input_size: float, P: int, points: Optional[torch.Tensor] = None,
                      labels: Optional[torch.Tensor] = None, boxes: Optional[torch.Tensor] = None, pad: bool = False,
                      out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Token block of the SAM mask decoder for P prompts -> f32 [P, NT, 2F]: the 5 output tokens, the point tokens
    (points f32 [P, N, 2], labels int32 [P, N], resized-input frame; pad appends (0, 0) with label -1), then the box
    corners (boxes f32 [P, 4]).  NT = 5 + N + pad + 2 * (boxes given) <= 16.  See ink_sam_prompt_tokens."""
    Fd = gauss.shape[1]
    assert gauss.dtype == F32 and gauss.is_contiguous() and gauss.shape[0] == 2
    for t, n in ((point_emb, 4), (not_a_point, 1), (out_tok, 5)):
        assert t.dtype == F32 and t.is_contiguous() and t.numel() == n * 2 * Fd
    n_pts = 0
    if points is not None:
        assert labels is not None and points.dtype == F32 and labels.dtype == torch.int32
        assert points.is_contiguous() and labels.is_contiguous() and points.dim() == 3 and points.shape[0] == P
        n_pts = points.shape[1]
        assert tuple(points.shape) == (P, n_pts, 2) and tuple(labels.shape) == (P, n_pts)
    if boxes is not None:
        assert boxes.dtype == F32 and boxes.is_contiguous() and tuple(boxes.shape) == (P, 4)
    NT = 5 + n_pts + int(pad) + (2 if boxes is not None else 0)
    if out is None:
        out = torch.empty((P, NT, 2 * Fd), device=gauss.device, dtype=F32)
    assert out.dtype == F32 and out.is_contiguous() and tuple(out.shape) == (P, NT, 2 * Fd)
    check(_lib.lib().ink_sam_prompt_tokens(_p(points), _p(labels), n_pts, int(pad), _p(boxes), _p(gauss), Fd,
                                           _p(point_emb), _p(not_a_point), _p(out_tok),
                                           float(input_size), P, _p(out), _stream()), "ink_sam_prompt_tokens")
    return out


SAM_MASK_EMBED_PARAMS = 4684     # floats of the packed mask_downscaling parameters (see ink_sam_mask_embed)


def sam_mask_embed(mask: torch.Tensor, emb: torch.Tensor, emb_rows: torch.Tensor, params: torch.Tensor, eps: float,
                   split: bool = False):
    """mask_input logits f32 [P, 1, 4g, 4g] -> the per-prompt keys emb[emb_rows[p] + t] + mask_downscaling(mask[p])[t],
    f32 [P*g*g, 256] (and, with split=True, their split-f16 GEMM operand f16 [P*g*g, 768]; see add_split_f16).
    emb f32 [*, 256] token rows; emb_rows int32 [P] (device) first row of each prompt's image."""
    assert mask.dtype == F32 and mask.is_contiguous() and mask.dim() == 4 and mask.shape[1] == 1
    P, S = mask.shape[0], mask.shape[2]
    assert mask.shape[3] == S and S % 4 == 0
    g = S // 4
    assert emb.dtype == F32 and emb.is_contiguous() and emb.dim() == 2 and emb.shape[1] == 256
    assert emb_rows.dtype == torch.int32 and emb_rows.is_cuda and emb_rows.numel() == P
    assert params.dtype == F32 and params.is_contiguous() and params.numel() == SAM_MASK_EMBED_PARAMS
    keys = torch.empty((P * g * g, 256), device=mask.device, dtype=F32)
    ks = torch.empty((P * g * g, 768), device=mask.device, dtype=F16) if split else None
    check(_lib.lib().ink_sam_mask_embed(_p(mask), _p(emb), _p(emb_rows), _p(params),
                                        params.numel(), eps, P, g, _p(keys), _p(ks), _stream()),
          "ink_sam_mask_embed")
    return (keys, ks) if split else keys


def sam_mask_logits(up: torch.Tensor, hyper: torch.Tensor, n: int, g: int) -> torch.Tensor:
    """hyper[n,C] . up[(((b*g*g + tok)*4 + s1)*4 + s2), C] -> pixel-shuffled [n, 4g, 4g] f32."""
    assert up.dtype == F32 and up.is_contiguous() and hyper.dtype == F32 and hyper.is_contiguous()
    Cn = hyper.shape[1]
    assert up.numel() == n * g * g * 16 * Cn
    out = torch.empty((n, 4 * g, 4 * g), device=up.device, dtype=F32)
    check(_lib.lib().ink_sam_mask_logits(up.data_ptr(), hyper.data_ptr(), n, g, Cn, out.data_ptr(),
                                         _stream()), "ink_sam_mask_logits")
    return out


def sam_postprocess(low: torch.Tensor, L: int, input_hw: Tuple[int, int], orig_hw: Tuple[int, int],
                    thr: float = 0.0, want_logits: bool = False):
    """low [n,S,S] f32 -> uint8 masks [n, H, W] (and optionally the f32 logits)."""
    assert low.dtype == F32 and low.is_contiguous() and low.dim() == 3
    n, S, _ = low.shape
    oh, ow = orig_hw
    out = torch.empty((n, oh, ow), device=low.device, dtype=torch.uint8)
    lg = torch.empty((n, oh, ow), device=low.device, dtype=F32) if want_logits else None
    check(_lib.lib().ink_sam_postprocess(low.data_ptr(), n, S, L, input_hw[0], input_hw[1], oh, ow,
                                         thr, out.data_ptr(), _p(lg), _stream()),
          "ink_sam_postprocess")
    return (out, lg) if want_logits else out


# ---------------------------------------------------------------------------------------------
# SamAutomaticMaskGenerator's tail (inklayer_amd/amg.py)
# ---------------------------------------------------------------------------------------------
NMS_MAX_BOXES = 4096


def sam_amg_stats(low: torch.Tensor, L: int, input_hw: Tuple[int, int], crop_hw: Tuple[int, int], thr: float,
                  offset: float, xy0: Tuple[int, int] = (0, 0), orig_hw: Optional[Tuple[int, int]] = None,
                  index: Optional[torch.Tensor] = None, count: Optional[torch.Tensor] = None,
                  want_logits: bool = False):
    """low [n, S, S] f32 -> (table int32 [m, 8], planes int64 [m, W, ceil(H / 64)]) (and the f32 logits [m, ch, cw] with
    want_logits, a test hook): per mask count(v > thr + offset), count(v > thr - offset), count(v > thr), the box
    x_min, y_min, x_max, y_max of v > thr in crop coordinates, 0; and v > thr as a column-major bit plane of the
    orig_hw frame with the crop at xy0.  v = postprocess_masks(low) at crop_hw, the floats of sam_postprocess.
    index int32 [m] (device) selects and orders the masks; count int32 [1] (device) processes only its first `count`
    entries (the other table rows are zero, the other planes unwritten), so a filter made on the device needs no host round trip."""
    assert low.dtype == F32 and low.is_contiguous() and low.dim() == 3
    n, S, _ = low.shape
    ch, cw = crop_hw
    oh, ow = orig_hw if orig_hw is not None else crop_hw
    if index is not None:
        assert index.dtype == torch.int32 and index.is_cuda and index.is_contiguous() and index.dim() == 1
    if count is not None:
        assert count.dtype == torch.int32 and count.is_cuda and count.numel() == 1
    m = n if index is None else index.numel()
    hp = -(-oh // 64)
    table = torch.empty((m, 8), device=low.device, dtype=torch.int32)
    planes = torch.empty((m, ow, hp), device=low.device, dtype=torch.int64)
    lg = torch.empty((m, ch, cw), device=low.device, dtype=F32) if want_logits else None
    if m > 0:
        check(_lib.lib().ink_sam_amg_stats(low.data_ptr(), n, _p(index), m, _p(count), S, L, input_hw[0], input_hw[1],
                                           ch, cw, thr, offset, xy0[0], xy0[1], oh, ow, table.data_ptr(),
                                           planes.data_ptr(), _p(lg), _stream()), "ink_sam_amg_stats")
    return (table, planes, lg) if want_logits else (table, planes)


def mask_rle(planes: torch.Tensor, H: int, W: int, select: Optional[torch.Tensor] = None):
    """Column-major bit planes int64 [m, W, ceil(H / 64)] -> the `counts` lists of mask_to_rle_pytorch
    (SA/utils/amg.py:107-135) for the planes select[0..k) (all of them when None).  Two launches with the size
    read-back between them; nothing is launched for k == 0."""
    assert planes.dtype == torch.int64 and planes.is_cuda and planes.is_contiguous()
    assert planes.dim() == 3 and tuple(planes.shape[1:]) == (W, -(-H // 64))
    if select is not None:
        assert select.dtype == torch.int32 and select.is_cuda and select.is_contiguous() and select.dim() == 1
    k = planes.shape[0] if select is None else select.numel()
    if k == 0:
        return []
    nc = torch.empty((k,), device=planes.device, dtype=torch.int32)
    check(_lib.lib().ink_mask_rle_counts(planes.data_ptr(), _p(select), k, H, W, nc.data_ptr(), _stream()),
          "ink_mask_rle_counts")
    sizes = nc.cpu()
    ends = torch.cumsum(sizes.long(), 0)
    total = int(ends[-1])
    assert total < 2 ** 31
    offs = (ends - sizes).to(torch.int32).to(planes.device)
    counts = torch.empty((total,), device=planes.device, dtype=torch.int32)
    check(_lib.lib().ink_mask_rle_write(planes.data_ptr(), _p(select), k, H, W, offs.data_ptr(), counts.data_ptr(),
                                        _stream()), "ink_mask_rle_write")
    return [c.tolist() for c in torch.split(counts.cpu(), sizes.tolist())]


def box_nms(boxes: torch.Tensor, scores: torch.Tensor, iou_threshold: float) -> torch.Tensor:
    """torchvision.ops.nms for one category: boxes f32 [n, 4] xyxy, scores f32 [n] (no NaN) -> int64 indices of the
    kept boxes in descending score order, ties in score to the lower index.  n <= NMS_MAX_BOXES."""
    assert boxes.dtype == F32 and boxes.is_cuda and boxes.is_contiguous() and boxes.dim() == 2 and boxes.shape[1] == 4
    assert scores.dtype == F32 and scores.is_cuda and scores.is_contiguous() and scores.shape == boxes.shape[:1]
    n = boxes.shape[0]
    if n > NMS_MAX_BOXES:
        raise ValueError(f"box_nms serves at most {NMS_MAX_BOXES} boxes, got {n}")
    if n == 0:
        return torch.empty((0,), device=boxes.device, dtype=torch.int64)
    ws = torch.empty((n * (-(-n // 64) + 3),), device=boxes.device, dtype=torch.int64)
    keep = torch.empty((n + 1,), device=boxes.device, dtype=torch.int32)
    check(_lib.lib().ink_box_nms(boxes.data_ptr(), scores.data_ptr(), n, iou_threshold, ws.data_ptr(), keep.data_ptr(),
                                 keep[n:].data_ptr(), _stream()), "ink_box_nms")
    host = keep.cpu()
    return host[:int(host[n])].long().to(boxes.device)


def pack_col_planes(masks: torch.Tensor) -> torch.Tensor:
    """bool / uint8 masks [k, H, W] on the device -> column-major bit planes int64 [k, W, ceil(H / 64)] (pixel != 0):
    ink_bitplane_pack on the transposed images."""
    assert masks.is_cuda and masks.dim() == 3 and masks.dtype in (torch.bool, torch.uint8)
    k, H, W = masks.shape
    t = masks.to(torch.uint8).transpose(1, 2).contiguous()
    planes = torch.empty((k, W, -(-H // 64)), device=masks.device, dtype=torch.int64)
    if k:
        check(_lib.lib().ink_bitplane_pack(t.data_ptr(), k, W, H, 0, planes.data_ptr(), _stream()), "ink_bitplane_pack")
    return planes


def remove_small_regions(planes: torch.Tensor, H: int, W: int, min_area: int, max_workspace_bytes: int = 1 << 29,
                         modes: Sequence[str] = ("holes", "islands")) -> Tuple[torch.Tensor, torch.Tensor]:
    """remove_small_regions(mode="holes") then (mode="islands") of SA/utils/amg.py:267-291, as postprocess_small_regions
    applies them, on column-major planes int64 [k, W, ceil(H / 64)] -> (cleaned planes, changed bool [k] = either pass
    found a region below min_area); `modes` runs one of the passes alone.  The planes go through in chunks whose
    component workspace stays below max_workspace_bytes (it is sized for the true run bound, 7 ints per possible run)."""
    assert planes.dtype == torch.int64 and planes.is_cuda and planes.is_contiguous()
    assert planes.dim() == 3 and tuple(planes.shape[1:]) == (W, -(-H // 64))
    k = planes.shape[0]
    out = torch.empty_like(planes)
    changed = torch.zeros((k,), device=planes.device, dtype=torch.int32)
    if k == 0:
        return out, changed.bool()
    L = _lib.lib()
    one = C.c_int64(0)
    check(L.ink_mask_small_regions_workspace_ints(1, H, W, C.byref(one)), "ink_mask_small_regions_workspace_ints")
    chunk = max(1, min(k, max_workspace_bytes // (4 * one.value)))
    need = C.c_int64(0)
    check(L.ink_mask_small_regions_workspace_ints(chunk, H, W, C.byref(need)), "ink_mask_small_regions_workspace_ints")
    ws = torch.empty((need.value,), device=planes.device, dtype=torch.int32)
    tmp = torch.empty_like(planes[:chunk])
    flag = torch.empty((chunk,), device=planes.device, dtype=torch.int32)
    for a in range(0, k, chunk):
        n = min(chunk, k - a)
        src, dst = planes[a:a + n], out[a:a + n]
        for j, mode in enumerate(modes):
            assert mode in ("holes", "islands")
            holes = int(mode == "holes")
            check(L.ink_mask_small_regions((dst if j else src).data_ptr(), n, H, W, int(min_area), holes,
                                           tmp.data_ptr(), ws.data_ptr(), dst.data_ptr(), flag.data_ptr(), _stream()),
                  "ink_mask_small_regions")
            changed[a:a + n] |= flag[:n]
    return out, changed.bool()


# ---------------------------------------------------------------------------------------------
# GroundingDINO-side ops
# ---------------------------------------------------------------------------------------------
_MSDA_DTYPE = {F32: 0, torch.float64: 1}


def _msda_check(value: torch.Tensor, spatial_shapes, level_start_index, sampling_loc: torch.Tensor,
                attn_weight: torch.Tensor, im2col_step: int, *grads: torch.Tensor):
    """The reference's checks (ms_deform_attn_cuda.cu:32-53), raised before anything is launched: float tensors of
    one dtype (f32 / f64), contiguous, on the GPU; int64 shape tables; B % min(B, im2col_step) == 0.  Returns the
    two tables as int64 tensors (host or device, as given) and (B, S, M, C, Q, L, P)."""
    ss = spatial_shapes if isinstance(spatial_shapes, torch.Tensor) else torch.as_tensor(spatial_shapes)
    ls = level_start_index if isinstance(level_start_index, torch.Tensor) else torch.as_tensor(level_start_index)
    floats = (value, sampling_loc, attn_weight, *grads)
    if value.dtype not in _MSDA_DTYPE:
        raise ValueError(f"ms_deform_attn: value must be float32 or float64, got {value.dtype}")
    if any(t.dtype != value.dtype for t in floats):
        raise ValueError("ms_deform_attn: value, sampling_loc, attn_weight (and grad_output) must share one dtype, got "
                         + ", ".join(str(t.dtype) for t in floats))
    if ss.dtype != torch.int64 or ls.dtype != torch.int64:
        raise ValueError(f"ms_deform_attn: spatial_shapes / level_start_index must be int64, got {ss.dtype} / {ls.dtype}")
    if not all(t.is_cuda for t in floats):
        raise ValueError("ms_deform_attn: value, sampling_loc, attn_weight must be GPU tensors (no CPU path)")
    if not all(t.is_contiguous() for t in (*floats, ss, ls)):
        raise ValueError("ms_deform_attn: every tensor must be contiguous")
    if value.dim() != 4 or sampling_loc.dim() != 6 or sampling_loc.shape[-1] != 2:
        raise ValueError("ms_deform_attn: value must be [B,S,M,C] and sampling_loc [B,Q,M,L,P,2]")
    B, S, M, Cn = value.shape
    _, Q, _, L, P, _ = sampling_loc.shape
    if (tuple(sampling_loc.shape[:3]) != (B, Q, M) or tuple(attn_weight.shape) != (B, Q, M, L, P)
            or tuple(ss.shape) != (L, 2) or tuple(ls.shape) != (L,)):
        raise ValueError("ms_deform_attn: inconsistent shapes of value / spatial_shapes / level_start_index / "
                         "sampling_loc / attn_weight")
    if any(tuple(g.shape) != (B, Q, M * Cn) for g in grads):
        raise ValueError(f"ms_deform_attn: grad_output must be [B,Q,M*C] = {(B, Q, M * Cn)}")
    step = min(B, im2col_step)
    if im2col_step <= 0 or B % step != 0:
        raise ValueError(f"ms_deform_attn: im2col_step ({im2col_step}) must divide batch ({B})")
    for t, name in ((ss, "spatial_shapes"), (ls, "level_start_index")):
        if t.is_cuda and t.device != value.device:
            raise ValueError(f"ms_deform_attn: {name} is on {t.device}, value on {value.device}")
    return ss, ls, (B, S, M, Cn, Q, L, P)


def _msda_device_tables(ss: torch.Tensor, ls: torch.Tensor, S: int, dev) -> Tuple[torch.Tensor, torch.Tensor]:
    """Device copies of host tables (checked here first: on the host that costs nothing); device tables as given -
    reading them would synchronise, so the kernels bound every row they touch instead (include/inklayer_hip.h)."""
    if ss.is_cuda and ls.is_cuda:
        return ss, ls
    if ss.is_cuda or ls.is_cuda:
        raise ValueError("ms_deform_attn: spatial_shapes and level_start_index must both be host or both be device tensors")
    hw = [int(h) * int(w) for h, w in ss.tolist()]
    starts = [sum(hw[:i]) for i in range(len(hw))]
    if min(int(v) for v in ss.reshape(-1).tolist()) <= 0 or sum(hw) != S or ls.tolist() != starts:
        raise ValueError(f"ms_deform_attn: spatial_shapes {ss.tolist()} / level_start_index {ls.tolist()} do not "
                         f"describe the {S} rows of value")
    return ss.to(dev), ls.to(dev)


def ms_deform_attn_forward(value: torch.Tensor, spatial_shapes, level_start_index,
                           sampling_loc: torch.Tensor, attn_weight: torch.Tensor,
                           im2col_step: int = 64) -> torch.Tensor:
    """Same argument list and semantics as groundingdino._C.ms_deform_attn_forward (GD/.../csrc/vision.cpp:54):
    value [B,S,M,C], spatial_shapes int64 [L,2], level_start_index int64 [L], sampling_loc [B,Q,M,L,P,2],
    attn_weight [B,Q,M,L,P] -> [B,Q,M*C], f32 or f64, any C and L.  Device shape tables are passed to the kernel
    as they are (no host synchronisation); host tables of the f32 / C == 32 / L <= 8 form take the host-table
    entry point (the same kernel: the same bits), other host tables are copied to the device."""
    ss, ls, (B, S, M, Cn, Q, L, P) = _msda_check(value, spatial_shapes, level_start_index, sampling_loc, attn_weight,
                                                 im2col_step)
    out = torch.empty((B, Q, M * Cn), device=value.device, dtype=value.dtype)
    if not ss.is_cuda and not ls.is_cuda and value.dtype == F32 and Cn == 32 and L <= 8:
        sl = [int(v) for v in ss.reshape(-1).tolist()]
        ll = [int(v) for v in ls.tolist()]
        check(_lib.lib().ink_ms_deform_attn_forward(
            value.data_ptr(), (C.c_int64 * len(sl))(*sl), (C.c_int64 * len(ll))(*ll), sampling_loc.data_ptr(),
            attn_weight.data_ptr(), B, S, M, Cn, Q, L, P, im2col_step, out.data_ptr(), _stream()),
            "ink_ms_deform_attn_forward")
        return out
    ss, ls = _msda_device_tables(ss, ls, S, value.device)
    check(_lib.lib().ink_ms_deform_attn_forward_dev(
        value.data_ptr(), ss.data_ptr(), ls.data_ptr(), sampling_loc.data_ptr(), attn_weight.data_ptr(),
        _MSDA_DTYPE[value.dtype], B, S, M, Cn, Q, L, P, im2col_step, out.data_ptr(), _stream()),
        "ink_ms_deform_attn_forward_dev")
    return out


def ms_deform_attn_backward(value: torch.Tensor, spatial_shapes, level_start_index, sampling_loc: torch.Tensor,
                            attn_weight: torch.Tensor, grad_output: torch.Tensor, im2col_step: int = 64):
    """Same argument list and results as groundingdino._C.ms_deform_attn_backward (GD/.../csrc/vision.cpp:55):
    returns (grad_value, grad_sampling_loc, grad_attn_weight), each with its input's shape and dtype.  grad_value
    is summed with float atomics, so its last bits vary from run to run (as the reference's do)."""
    ss, ls, (B, S, M, Cn, Q, L, P) = _msda_check(value, spatial_shapes, level_start_index, sampling_loc, attn_weight,
                                                 im2col_step, grad_output)
    ss, ls = _msda_device_tables(ss, ls, S, value.device)
    grad_value = torch.empty_like(value)                 # zeroed by the entry point on the stream
    grad_loc = torch.empty_like(sampling_loc)
    grad_aw = torch.empty_like(attn_weight)
    check(_lib.lib().ink_ms_deform_attn_backward_dev(
        value.data_ptr(), ss.data_ptr(), ls.data_ptr(), sampling_loc.data_ptr(), attn_weight.data_ptr(),
        grad_output.data_ptr(), _MSDA_DTYPE[value.dtype], B, S, M, Cn, Q, L, P, im2col_step, grad_value.data_ptr(),
        grad_loc.data_ptr(), grad_aw.data_ptr(), _stream()), "ink_ms_deform_attn_backward_dev")
    return grad_value, grad_loc, grad_aw


class _MSDeformAttnFunction(torch.autograd.Function):
    """Differentiable form (MultiScaleDeformableAttnFunction, GD/models/GroundingDINO/ms_deform_attn.py:45-90):
    once-differentiable, gradients for value, sampling_loc and attn_weight."""

    @staticmethod
    def forward(ctx, value, spatial_shapes, level_start_index, sampling_loc, attn_weight, im2col_step):
        ctx.im2col_step = im2col_step
        ctx.save_for_backward(value, spatial_shapes, level_start_index, sampling_loc, attn_weight)
        return ms_deform_attn_forward(value, spatial_shapes, level_start_index, sampling_loc, attn_weight, im2col_step)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_output):
        value, spatial_shapes, level_start_index, sampling_loc, attn_weight = ctx.saved_tensors
        gv, gl, ga = ms_deform_attn_backward(value, spatial_shapes, level_start_index, sampling_loc, attn_weight,
                                             grad_output.contiguous(), ctx.im2col_step)
        return gv, None, None, gl, ga, None


def ms_deform_attn(value: torch.Tensor, spatial_shapes, level_start_index, sampling_loc: torch.Tensor,
                   attn_weight: torch.Tensor, im2col_step: int = 64) -> torch.Tensor:
    """Differentiable multi-scale deformable attention: ms_deform_attn_forward with a backward through
    ms_deform_attn_backward (for value, sampling_loc and attn_weight)."""
    ss = spatial_shapes if isinstance(spatial_shapes, torch.Tensor) else torch.as_tensor(spatial_shapes)
    ls = level_start_index if isinstance(level_start_index, torch.Tensor) else torch.as_tensor(level_start_index)
    return _MSDeformAttnFunction.apply(value, ss, ls, sampling_loc, attn_weight, im2col_step)


def msda_fused(value16: torch.Tensor, proj: torch.Tensor, ref: torch.Tensor, shapes: Sequence[Tuple[int, int]],
               B: int, Q: int, ref_batched: bool, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """value16 f16 [B*S, 256]; proj f32 [B*Q, >=384]; ref f32 [Q, d] (shared) or [B*Q, d], d in {2,4}."""
    assert value16.dtype == F16 and value16.is_contiguous() and proj.dtype == F32 and proj.stride(1) == 1
    assert ref.dtype == F32 and ref.is_contiguous()
    S = value16.shape[0] // B
    d = ref.shape[-1]
    if out is None:
        out = torch.empty((B * Q, 256), device=value16.device, dtype=F16)
    flat = [v for hw in shapes for v in hw]
    check(_lib.lib().ink_msda_fused(value16.data_ptr(), proj.data_ptr(), proj.stride(0), ref.data_ptr(), d, d,
                                    Q * d if ref_batched else 0, (C.c_int32 * 8)(*flat), B, S, Q,
                                    out.data_ptr(), _stream()), "ink_msda_fused")
    return out


def swin_patchify(image_u8: torch.Tensor, mean: Sequence[float], std: Sequence[float], out: torch.Tensor):
    assert image_u8.dtype == torch.uint8 and image_u8.is_cuda and image_u8.is_contiguous()
    h, w, c = image_u8.shape
    assert c == 3 and out.dtype == F16 and out.is_contiguous() and out.numel() == -(-h // 4) * -(-w // 4) * 64
    check(_lib.lib().ink_swin_patchify(image_u8.data_ptr(), h, w, (C.c_float * 3)(*mean), (C.c_float * 3)(*std),
                                       out.data_ptr(), _stream()), "ink_swin_patchify")
    return out


def layernorm_merge4(x: torch.Tensor, gamma, beta, eps: float, gather4: torch.Tensor,
                     out: Optional[torch.Tensor] = None) -> torch.Tensor:
    assert x.dtype == F32 and x.stride(1) == 1 and gather4.dtype == torch.int32 and gather4.is_contiguous()
    rows, Cn = gather4.shape[0], x.shape[1]
    if out is None:
        out = torch.empty((rows, 4 * Cn), device=x.device, dtype=F16)
    assert out.dtype == F16 and out.is_contiguous() and tuple(out.shape) == (rows, 4 * Cn)
    check(_lib.lib().ink_layernorm_merge4(x.data_ptr(), x.stride(0), gamma.data_ptr(), beta.data_ptr(), eps,
                                          gather4.data_ptr(), rows, Cn, out.data_ptr(), _stream()),
          "ink_layernorm_merge4")
    return out


def groupnorm_nhwc(x: torch.Tensor, B: int, T: int, G: int, gamma, beta, eps: float, out: torch.Tensor,
                   out_batch_stride: int) -> None:
    """x f32 [B*T, C] -> out (f32) at out + b*out_batch_stride + t*C (writes into the level's slice of
    the flattened multi-scale source)."""
    assert x.dtype == F32 and x.is_contiguous() and out.dtype == F32
    Cn = x.shape[1]
    ws = torch.empty(B * G * 2, device=x.device, dtype=F32)
    check(_lib.lib().ink_groupnorm_nhwc(x.data_ptr(), B, T, Cn, G, gamma.data_ptr(), beta.data_ptr(), eps,
                                        ws.data_ptr(), out.data_ptr(), out_batch_stride, _stream()),
          "ink_groupnorm_nhwc")


def gather_rows(x: torch.Tensor, idx: torch.Tensor, B: int, rows_per_batch: int, *, x_batch_rows: int,
                idx_batch_stride: int, out_dtype=F16, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out[b*rows_per_batch + r] = x[b*x_batch_rows + idx[b*idx_batch_stride + r]] (-1 -> zero row); `out` (f16 or
    f32, contiguous) overrides out_dtype."""
    assert x.dtype == F32 and x.stride(1) == 1 and idx.dtype == torch.int32 and idx.is_cuda
    Cn = x.shape[1]
    if out is None:
        out = torch.empty((B * rows_per_batch, Cn), device=x.device, dtype=out_dtype)
    out_dtype = out.dtype
    assert out_dtype in (F16, F32) and out.is_contiguous() and tuple(out.shape) == (B * rows_per_batch, Cn)
    oh = out.data_ptr() if out_dtype == F16 else None
    of = out.data_ptr() if out_dtype == F32 else None
    check(_lib.lib().ink_gather_rows(x.data_ptr(), x.stride(0), x_batch_rows, idx.data_ptr(), idx_batch_stride,
                                     rows_per_batch, B, Cn, oh, of, _stream()), "ink_gather_rows")
    return out


def biattn_wide(qv16: torch.Tensor, kl16: torch.Tensor, B: int, S: int, T: int, scale: float):
    """BiMultiHeadAttention's core, both directions, for 1 <= T <= 256 text tokens on f16 MFMA (csrc/biattn_wide.hip):
    qv16 f16 [B*S, 2048] = [v_proj(v) | values_v_proj(v)], kl16 f16 [B*T, 2048] = [l_proj(l) | values_l_proj(l)], 4 heads
    x 256 -> (out_v f16 [B*S, 1024], softmax over the text tokens; out_l f16 [B*T, 1024], softmax over the image
    tokens).  No score matrix in HBM."""
    assert qv16.dtype == F16 and qv16.is_contiguous() and kl16.dtype == F16 and kl16.is_contiguous()
    assert tuple(qv16.shape) == (B * S, 2048) and tuple(kl16.shape) == (B * T, 2048)
    dev = qv16.device
    need = C.c_int64(0)
    check(_lib.lib().ink_biattn_wide_workspace(B, S, T, C.byref(need)), "ink_biattn_wide_workspace")
    ws = torch.empty(need.value, device=dev, dtype=F32)
    out_v = torch.empty((B * S, 1024), device=dev, dtype=F16)
    out_l = torch.empty((B * T, 1024), device=dev, dtype=F16)
    check(_lib.lib().ink_biattn_wide(qv16.data_ptr(), kl16.data_ptr(), B, S, T, 1024, scale, ws.data_ptr(),
                                     out_v.data_ptr(), out_l.data_ptr(), _stream()), "ink_biattn_wide")
    return out_v, out_l


def biattn_wide_varlen(qv16: torch.Tensor, kl16: torch.Tensor, B: int, S: int, Tmax: int, t_len: torch.Tensor,
                       scale: float):
    """biattn_wide for a batch whose captions differ in length: kl16 f16 [B*Tmax, 2048] holds image b's t_len[b] text
    rows at b*Tmax (the pad rows behind them are never read), t_len int32 [B] on the device (clamped into 1..Tmax by
    the kernels).  -> (out_v f16 [B*S, 1024]; out_l f16 [B*Tmax, 1024] with zeros in the pad rows).  Image b's results
    are bitwise those of biattn_wide(B=1, T=t_len[b]) on its rows."""
    assert qv16.dtype == F16 and qv16.is_contiguous() and kl16.dtype == F16 and kl16.is_contiguous()
    assert tuple(qv16.shape) == (B * S, 2048) and tuple(kl16.shape) == (B * Tmax, 2048)
    dev = qv16.device
    assert t_len.dtype == torch.int32 and t_len.is_contiguous() and tuple(t_len.shape) == (B,) and t_len.device == dev
    need = C.c_int64(0)
    check(_lib.lib().ink_biattn_wide_workspace(B, S, Tmax, C.byref(need)), "ink_biattn_wide_workspace")
    ws = torch.empty(need.value, device=dev, dtype=F32)
    out_v = torch.empty((B * S, 1024), device=dev, dtype=F16)
    out_l = torch.empty((B * Tmax, 1024), device=dev, dtype=F16)
    check(_lib.lib().ink_biattn_wide_varlen(qv16.data_ptr(), kl16.data_ptr(), B, S, Tmax, t_len.data_ptr(), 1024, scale,
                                            ws.data_ptr(), out_v.data_ptr(), out_l.data_ptr(), _stream()),
          "ink_biattn_wide_varlen")
    return out_v, out_l


def fusion_fold(v: torch.Tensor, B: int, S: int, lnv_g: torch.Tensor, lnv_b: torch.Tensor, eps: float,
                text_kv: torch.Tensor, T: int, Wqv: torch.Tensor, bqv: torch.Tensor, Wo: torch.Tensor, bo: torch.Tensor,
                gamma_v: torch.Tensor, scale: float, pos: Optional[torch.Tensor] = None,
                out16_pos: Optional[torch.Tensor] = None, out16: Optional[torch.Tensor] = None) -> torch.Tensor:
    """BiAttentionBlock with the <= 4 caption tokens folded through it (csrc/fusion_fold.hip): v f32 [B*S, 256] is
    updated IN PLACE; returns the text-side attention output f16 [B*T, 1024].  text_kv: f32 [B*T, 2048] =
    [l_proj | values_l_proj] of LN_l(l); Wqv f16 [2048, 256] / bqv f32 [2048] = [v_proj ; values_v_proj].  out16 /
    out16_pos (f16 [B*S, 256], optional): f16(v) and f16(v + pos[s]) of the UPDATED v, pos f32 [S, 256]."""
    for t in (out16, out16_pos):
        assert t is None or (t.dtype == F16 and t.is_contiguous() and tuple(t.shape) == (B * S, 256))
    assert out16_pos is None or (pos is not None and pos.dtype == F32 and pos.is_contiguous() and tuple(pos.shape) == (S, 256))
    assert v.dtype == F32 and v.is_contiguous() and tuple(v.shape) == (B * S, 256)
    assert text_kv.dtype == F32 and text_kv.stride(1) == 1 and tuple(text_kv.shape) == (B * T, 2048)
    assert Wqv.dtype == F16 and Wqv.is_contiguous() and tuple(Wqv.shape) == (2048, 256) and bqv.dtype == F32
    assert Wo.dtype == F16 and Wo.is_contiguous() and tuple(Wo.shape) == (256, 1024)
    need = C.c_int64(0)
    check(_lib.lib().ink_fusion_fold_workspace(B, S, C.byref(need)), "ink_fusion_fold_workspace")
    ws = torch.empty(need.value, device=v.device, dtype=F32)
    out_l = torch.empty((B * T, 1024), device=v.device, dtype=F16)
    check(_lib.lib().ink_fusion_fold(v.data_ptr(), B, S, lnv_g.data_ptr(), lnv_b.data_ptr(), eps, text_kv.data_ptr(),
                                     text_kv[:, 1024:].data_ptr(), text_kv.stride(0), T, Wqv.data_ptr(), bqv.data_ptr(),
                                     Wqv[1024:].data_ptr(), bqv[1024:].data_ptr(), Wo.data_ptr(), bo.data_ptr(),
                                     gamma_v.data_ptr(), scale, ws.data_ptr(), out_l.data_ptr(), _p(pos), _p(out16_pos),
                                     _p(out16), _stream()),
          "ink_fusion_fold")
    return out_l


def proj256_ln_pack(ws: torch.Tensor) -> torch.Tensor:
    """A [128 -> 256] projection as the split-f16 matrix [256, 384] -> the LDS image of proj256_ln (load time)."""
    assert ws.dtype == F16 and ws.is_contiguous() and tuple(ws.shape) == (256, 384)
    blob = torch.empty(3 * 64 * 64 * 8, device=ws.device, dtype=F16)
    check(_lib.lib().ink_proj256_ln_pack(ws.data_ptr(), blob.data_ptr(), _stream()), "ink_proj256_ln_pack")
    return blob


def proj256_ln(a: torch.Tensor, blob: torch.Tensor, bias: torch.Tensor, res: torch.Tensor, ln_g: torch.Tensor,
               ln_b: torch.Tensor, eps: float, *, res_batch_rows: Optional[torch.Tensor] = None, rows_per_batch: int = 0,
               want_f32: bool = True, want_split: bool = True):
    """LayerNorm(res + a W^T + bias) in one kernel (transformer.py:175-182: out_proj + residual + norm4 of the image
    tokens; csrc/proj_ln.hip).  a f32 [R, 128]; res f32 [R, 256] or, with res_batch_rows (int32 per box), a tensor shared
    by the boxes of an image.  -> (f32 [R, 256] or None, split-f16 operand [R, 768] or None)."""
    R = int(a.shape[0])
    assert a.dtype == F32 and a.is_contiguous() and tuple(a.shape) == (R, 128)
    assert blob.dtype == F16 and blob.numel() == 3 * 64 * 64 * 8
    assert res.dtype == F32 and res.is_contiguous() and res.shape[1] == 256
    assert all(t.dtype == F32 and t.is_contiguous() and t.numel() == 256 for t in (bias, ln_g, ln_b))
    if res_batch_rows is not None:
        assert res_batch_rows.dtype == torch.int32 and res_batch_rows.is_cuda and rows_per_batch > 0
        assert res_batch_rows.numel() * rows_per_batch == R
    else:
        assert res.shape[0] == R
    of = torch.empty((R, 256), device=a.device, dtype=F32) if want_f32 else None
    osp = torch.empty((R, 768), device=a.device, dtype=F16) if want_split else None
    check(_lib.lib().ink_proj256_ln(a.data_ptr(), blob.data_ptr(), bias.data_ptr(), res.data_ptr(), _p(res_batch_rows),
                                    rows_per_batch, ln_g.data_ptr(), ln_b.data_ptr(), eps, R, _p(of), _p(osp), _stream()),
          "ink_proj256_ln")
    return of, osp


def sam_upscale_pack(ws: torch.Tensor) -> torch.Tensor:
    """output_upscaling.3 as the split-f16 matrix [128, 192] -> the LDS image of sam_upscale_tail (load time)."""
    assert ws.dtype == F16 and ws.is_contiguous() and tuple(ws.shape) == (128, 192)
    blob = torch.empty(4 * 12 * 64 * 8, device=ws.device, dtype=F16)
    check(_lib.lib().ink_sam_upscale_pack(ws.data_ptr(), blob.data_ptr(), _stream()), "ink_sam_upscale_pack")
    return blob


def sam_upscale_tail(u0: torch.Tensor, n: int, g: int, ln_g: torch.Tensor, ln_b: torch.Tensor, eps: float,
                     blob: torch.Tensor, b3: torch.Tensor, hyper: torch.Tensor) -> torch.Tensor:
    """LayerNorm2d + GELU + ConvTranspose2d(k2 s2) + GELU + hyper-network product of the mask decoder in one kernel
    (mask_decoder.py:54-60, 138-145) for M in {1, 3, 4} mask tokens per box at once: u0 f32 [n*g*g, 256] (4 sub-pixels x
    64 channels per token; rows may be a column block of a wider tensor) or [n*g*g*4, 64] contiguous, hyper f32
    [n, M, 32] -> low-res mask logits f32 [n, M, 4g, 4g].  The upscaling is computed once per row and shared by the M masks."""
    if u0.shape[1] == 64:
        assert u0.is_contiguous() and u0.shape[0] == n * g * g * 4
        u0 = u0.view(n * g * g, 256)
    assert u0.dtype == F32 and u0.stride(1) == 1 and tuple(u0.shape) == (n * g * g, 256) and u0.stride(0) % 4 == 0
    assert blob.dtype == F16 and blob.numel() == 4 * 12 * 64 * 8 and b3.dtype == F32 and b3.numel() == 128
    assert hyper.dtype == F32 and hyper.is_contiguous() and hyper.dim() == 3 and hyper.shape[0] == n and hyper.shape[2] == 32
    assert ln_g.dtype == F32 and ln_b.dtype == F32 and ln_g.numel() == 64 and ln_b.numel() == 64
    M = hyper.shape[1]
    low = torch.empty((n, M, 4 * g, 4 * g), device=u0.device, dtype=F32)
    check(_lib.lib().ink_sam_upscale_tail(_p(u0), u0.stride(0), n, g, _p(ln_g), _p(ln_b), eps, _p(blob), _p(b3), _p(hyper), M,
                                          _p(low), _stream()), "ink_sam_upscale_tail")
    return low


def ffn256_pack(w1: torch.Tensor, b1: torch.Tensor, w2: torch.Tensor, w_pre: Optional[torch.Tensor] = None) -> torch.Tensor:
    """linear1.weight f16 [hid, 256] + linear1.bias f32 [hid] + linear2.weight f16 [256, hid] (+ the weight f16 [256, 256] of
    a preceding projection, see ffn256_fused) -> the packed weight blob (done once at load time; csrc/ffn_fused.hip)."""
    hid = int(w1.shape[0])
    assert w1.dtype == F16 and w2.dtype == F16 and w1.is_contiguous() and w2.is_contiguous()
    assert tuple(w1.shape) == (hid, 256) and tuple(w2.shape) == (256, hid)
    assert b1.dtype == F32 and b1.is_contiguous() and b1.numel() == hid
    assert w_pre is None or (w_pre.dtype == F16 and w_pre.is_contiguous() and tuple(w_pre.shape) == (256, 256))
    need = C.c_int64(0)
    check(_lib.lib().ink_ffn256_pack_bytes(hid, int(w_pre is not None), C.byref(need)), "ink_ffn256_pack_bytes")
    blob = torch.empty(need.value // 2, device=w1.device, dtype=F16)
    check(_lib.lib().ink_ffn256_pack(w1.data_ptr(), b1.data_ptr(), w2.data_ptr(), hid, _p(w_pre), blob.data_ptr(), _stream()),
          "ink_ffn256_pack")
    return blob


def ffn256_fused(x16: torch.Tensor, res: torch.Tensor, blob: torch.Tensor, hid: int, b2: torch.Tensor,
                 ln_g: torch.Tensor, ln_b: torch.Tensor, eps: float, out: Optional[torch.Tensor] = None,
                 pre: Optional[Tuple[torch.Tensor, torch.Tensor, torch.Tensor]] = None) -> torch.Tensor:
    """LayerNorm(res + linear2(relu(linear1(x16)))) for d_model 256 in one kernel (transformer.py:780-799).  x16 f16
    [M, 256] (row stride free), res f32 [M, 256]; blob = ffn256_pack(...) of a d_ffn = hid layer; out f32 [M, 256] (may be
    `res`).  pre = (bias, ln_weight, ln_bias) of a preceding projection whose weight is in the blob: then
    s = LayerNorm_pre(res + x16 W_pre^T + bias) is formed first and the block runs on s (x16 = that projection's input)."""
    M = int(x16.shape[0])
    assert x16.dtype == F16 and x16.stride(1) == 1 and x16.shape[1] == 256
    assert res.dtype == F32 and res.is_contiguous() and tuple(res.shape) == (M, 256)
    need = C.c_int64(0)
    check(_lib.lib().ink_ffn256_pack_bytes(hid, int(pre is not None), C.byref(need)), "ink_ffn256_pack_bytes")
    assert blob.dtype == F16 and blob.numel() * 2 == need.value and b2.dtype == F32
    assert b2.numel() == 256 and ln_g.numel() == 256 and ln_b.numel() == 256 and ln_g.dtype == F32 and ln_b.dtype == F32
    if pre is not None:
        assert all(t.dtype == F32 and t.is_contiguous() and t.numel() == 256 for t in pre)
    if out is None:
        out = torch.empty_like(res)
    assert out.dtype == F32 and out.is_contiguous() and tuple(out.shape) == (M, 256)
    pb, pg, pe = pre if pre is not None else (None, None, None)
    check(_lib.lib().ink_ffn256_fused(x16.data_ptr(), x16.stride(0), res.data_ptr(), blob.data_ptr(), b2.data_ptr(),
                                      ln_g.data_ptr(), ln_b.data_ptr(), eps, M, hid, _p(pb), _p(pg), _p(pe), out.data_ptr(),
                                      _stream()), "ink_ffn256_fused")
    return out


def attn_fewkeys(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, *, B: int, n_heads: int, head_dim: int,
                 scale: float, blocked: Optional[torch.Tensor] = None, n_q: Optional[int] = None,
                 q_batch_rows: Optional[torch.Tensor] = None, q_add: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Attention against n_k <= 16 keys per batch entry; q/k/v/out are all f16 (head_dim 32, 64) or all f32 rows
    (head_dim 16, 32); f32 math either way.  q_batch_rows: first q row of each batch entry (then n_q must be given)."""
    io = q.dtype
    for t in (q, k, v):
        assert t.dtype == io and io in (F16, F32) and t.dim() == 2 and t.stride(1) == 1
        assert t.data_ptr() % 16 == 0                      # 16-byte vector loads (the row strides: ld % 8 in the C entry)
    if n_q is None:
        n_q = q.shape[0] // B
    n_k = k.shape[0] // B
    out = torch.empty((B * n_q, n_heads * head_dim), device=q.device, dtype=io)
    if blocked is not None:
        assert blocked.dtype == torch.uint8 and blocked.is_contiguous() and blocked.shape == (n_q, n_k)
    if q_batch_rows is not None:
        assert q_batch_rows.dtype == torch.int32 and q_batch_rows.numel() == B and q_batch_rows.is_cuda
    if q_add is not None:
        assert q_add.dtype == F32 and q_add.is_contiguous() and tuple(q_add.shape) == (n_q, n_heads * head_dim)
    check(_lib.lib().ink_attn_fewkeys(q.data_ptr(), q.stride(0), k.data_ptr(), k.stride(0), v.data_ptr(),
                                      v.stride(0), B, n_q, n_k, n_heads, head_dim, scale, _p(blocked),
                                      _p(q_batch_rows), _p(q_add), int(io == F32), out.data_ptr(), out.stride(0), _stream()),
          "ink_attn_fewkeys")
    return out


def attn_midkeys(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, *, B: int, n_heads: int, head_dim: int,
                 scale: float, blocked: Optional[torch.Tensor] = None) -> torch.Tensor:
    """attn_fewkeys' contract for n_k <= 256 keys per batch entry on f16 rows (head_dim 32, 64; f32 math); a fully
    blocked row gives zeros."""
    for t in (q, k, v):
        assert t.dtype == F16 and t.dim() == 2 and t.stride(1) == 1
        assert t.data_ptr() % 16 == 0                      # 16-byte vector loads (the row strides: ld % 8 in the C entry)
    n_q, n_k = q.shape[0] // B, k.shape[0] // B
    out = torch.empty((B * n_q, n_heads * head_dim), device=q.device, dtype=F16)
    if blocked is not None:
        assert blocked.dtype == torch.uint8 and blocked.is_contiguous() and blocked.shape == (n_q, n_k)
    check(_lib.lib().ink_attn_midkeys(q.data_ptr(), q.stride(0), k.data_ptr(), k.stride(0), v.data_ptr(), v.stride(0),
                                      B, n_q, n_k, n_heads, head_dim, scale, _p(blocked), out.data_ptr(),
                                      out.stride(0), _stream()), "ink_attn_midkeys")
    return out


def attn_midkeys_varlen(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, *, B: int, n_heads: int, head_dim: int,
                        scale: float, blocked: Optional[torch.Tensor] = None,
                        k_len: Optional[torch.Tensor] = None) -> torch.Tensor:
    """attn_midkeys with a mask per batch entry (blocked u8 [n_q, n_k] shared or [B, n_q, n_k]) and a key count per
    batch entry (k_len int32 [B] on the device, clamped into 0..n_k by the kernel): the keys t >= k_len[b] do not exist
    for entry b and their rows are never loaded.  Key rows stay at b*n_k + t.  A row with no allowed key gives zeros."""
    for t in (q, k, v):
        assert t.dtype == F16 and t.dim() == 2 and t.stride(1) == 1
        assert t.data_ptr() % 16 == 0                      # 16-byte vector loads (the row strides: ld % 8 in the C entry)
    n_q, n_k = q.shape[0] // B, k.shape[0] // B
    out = torch.empty((B * n_q, n_heads * head_dim), device=q.device, dtype=F16)
    bstride = 0
    if blocked is not None:
        assert blocked.dtype == torch.uint8 and blocked.is_contiguous() and blocked.device == q.device
        assert tuple(blocked.shape) in ((n_q, n_k), (B, n_q, n_k))
        bstride = n_q * n_k if blocked.dim() == 3 else 0
    if k_len is not None:
        assert k_len.dtype == torch.int32 and k_len.is_contiguous() and tuple(k_len.shape) == (B,) and k_len.device == q.device
    check(_lib.lib().ink_attn_midkeys_varlen(q.data_ptr(), q.stride(0), k.data_ptr(), k.stride(0), v.data_ptr(),
                                             v.stride(0), B, n_q, n_k, n_heads, head_dim, scale, _p(blocked), bstride,
                                             _p(k_len), out.data_ptr(), out.stride(0), _stream()),
          "ink_attn_midkeys_varlen")
    return out


def text_embed_ln(ids, pos_ids, word: torch.Tensor, pos: torch.Tensor, type_row: torch.Tensor, gamma: torch.Tensor,
                  beta: torch.Tensor, eps: float) -> Tuple[torch.Tensor, torch.Tensor]:
    """BERT's embedding block for R packed token rows: LN(word[ids] + pos[pos_ids] + type_row) * gamma + beta ->
    (f32 [R, C], split-f16 operand [R, 3C] as add_split_f16 lays it out).  ids / pos_ids: sequences of ints or host
    tensors (checked against the tables here: ValueError before any launch, then uploaded) or int32 device tensors
    (the kernel clamps those into range)."""
    V, Cn = word.shape
    P = pos.shape[0]
    dev = word.device
    for t, n in ((word, V), (pos, P)):
        assert t.dtype == F32 and t.is_contiguous() and t.shape == (n, Cn)
    for t in (type_row, gamma, beta):
        assert t.dtype == F32 and t.is_contiguous() and t.numel() == Cn and t.device == dev
    dev_ids = []
    for t, n, what in ((ids, V, "token id"), (pos_ids, P, "position id")):
        if not (isinstance(t, torch.Tensor) and t.is_cuda):
            t = torch.as_tensor(t, dtype=torch.int64).reshape(-1)
            if t.numel() and (int(t.min()) < 0 or int(t.max()) >= n):
                raise ValueError(f"{what} outside 0..{n - 1}")
            t = t.to(torch.int32).to(dev)
        assert t.dtype == torch.int32 and t.dim() == 1 and t.is_contiguous() and t.device == dev
        dev_ids.append(t)
    R = dev_ids[0].numel()
    assert R >= 1 and dev_ids[1].numel() == R
    out = torch.empty((R, Cn), device=dev, dtype=F32)
    split = torch.empty((R, 3 * Cn), device=dev, dtype=F16)
    check(_lib.lib().ink_text_embed_ln(dev_ids[0].data_ptr(), dev_ids[1].data_ptr(), R, word.data_ptr(), V,
                                       pos.data_ptr(), P, type_row.data_ptr(), gamma.data_ptr(), beta.data_ptr(), eps,
                                       Cn, out.data_ptr(), split.data_ptr(), _stream()), "ink_text_embed_ln")
    return out, split


def attn_text_f32(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, row_start: torch.Tensor, *, Tmax: int,
                  n_heads: int, scale: float, blocked: Optional[torch.Tensor] = None,
                  want_f32: bool = False) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
    """BERT's self-attention for packed captions on f32 rows [R, n_heads * 64] (views into the fused qkv projection;
    head_dim 64): caption b owns rows row_start[b] .. row_start[b + 1] (int32 [B + 1] on the device, at most Tmax <= 256
    rows each).  blocked: u8 [Tmax, Tmax] shared or [B, Tmax, Tmax].  -> (split-f16 operand [R, 3 * n_heads * 64] of the
    context, its f32 copy [R, n_heads * 64] or None).  A row with no allowed key gives zeros."""
    E = n_heads * 64
    for t in (q, k, v):
        assert t.dtype == F32 and t.dim() == 2 and t.stride(1) == 1 and t.shape[1] == E
        assert t.data_ptr() % 16 == 0                      # 16-byte vector loads (the row strides: ld % 4 in the C entry)
    R = q.shape[0]
    assert k.shape[0] == R and v.shape[0] == R
    assert row_start.dtype == torch.int32 and row_start.dim() == 1 and row_start.is_contiguous() and row_start.device == q.device
    B = row_start.numel() - 1
    bstride = 0
    if blocked is not None:
        assert blocked.dtype == torch.uint8 and blocked.is_contiguous() and blocked.device == q.device
        assert tuple(blocked.shape) in ((Tmax, Tmax), (B, Tmax, Tmax))
        bstride = Tmax * Tmax if blocked.dim() == 3 else 0
    out = torch.empty((R, 3 * E), device=q.device, dtype=F16)
    out32 = torch.empty((R, E), device=q.device, dtype=F32) if want_f32 else None
    check(_lib.lib().ink_attn_text_f32(q.data_ptr(), q.stride(0), k.data_ptr(), k.stride(0), v.data_ptr(), v.stride(0),
                                       row_start.data_ptr(), B, R, Tmax, n_heads, 64, scale, _p(blocked), bstride,
                                       out.data_ptr(), out.stride(0), _p(out32), E if want_f32 else 0, _stream()),
          "ink_attn_text_f32")
    return out, out32


def attn_fewq(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, *, n_batch: int, n_heads: int, head_dim: int,
              scale: float, n_q: int, n_k: int, q_batch_rows: Optional[torch.Tensor] = None,
              kv_batch_rows: Optional[torch.Tensor] = None, k_add: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Few queries (<= 16) against many keys on f32 rows (head_dim 16, n_heads % 4 == 0); same row conventions as
    flash_attn."""
    for t in (q, k, v):
        assert t.dtype == F32 and t.dim() == 2 and t.stride(1) == 1
        assert t.data_ptr() % 16 == 0                      # 16-byte vector loads (the row strides: ld % 8 in the C entry)
    for rows in (q_batch_rows, kv_batch_rows):
        assert rows is None or (rows.dtype == torch.int32 and rows.numel() == n_batch and rows.is_cuda)
    out = torch.empty((n_batch * n_q, n_heads * head_dim), device=q.device, dtype=F32)
    if k_add is not None:
        assert k_add.dtype == F32 and k_add.is_contiguous() and tuple(k_add.shape) == (n_k, n_heads * head_dim)
    check(_lib.lib().ink_attn_fewq(q.data_ptr(), q.stride(0), k.data_ptr(), k.stride(0), v.data_ptr(), v.stride(0),
                                   n_batch, n_q, n_k, n_heads, head_dim, scale, _p(q_batch_rows),
                                   _p(kv_batch_rows), _p(k_add), out.data_ptr(), out.stride(0), _stream()),
          "ink_attn_fewq")
    return out


def topk_rowmax(logits: torch.Tensor, K: int, want_values: bool = False):
    """logits f32 [B,S,T] -> int32 [B,K] indices of the K largest row maxima (descending, stable)."""
    assert logits.dtype == F32 and logits.is_contiguous() and logits.dim() == 3
    B, S, T = logits.shape
    idx = torch.empty((B, K), device=logits.device, dtype=torch.int32)
    val = torch.empty((B, K), device=logits.device, dtype=F32) if want_values else None
    nchunk = -(-S // 16384)
    ws = torch.empty((B * nchunk * K,), device=logits.device, dtype=torch.int64) if nchunk > 1 else None
    check(_lib.lib().ink_topk_rowmax(logits.data_ptr(), B, S, T, K, idx.data_ptr(), _p(val), _p(ws), _stream()),
          "ink_topk_rowmax")
    return (idx, val) if want_values else idx


def class_scores(logits: torch.Tensor, pos_map: torch.Tensor, n_cls: Optional[torch.Tensor] = None,
                 out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """prob[b, q, c] = sum_t sigmoid(logits[b, q, t]) * pos_map[c, t] (csrc/closed_set.hip): logits f32 [B, nq, T] whose
    rows may be a slice of wider ones (stride(1) >= T, as forward returns them for T % 4 != 0), pos_map f32 [C, T] for
    every image or [B, C, T] per image, n_cls int32 [B]: classes c >= n_cls[b] score -1.0.  -> f32 [B, nq, C]."""
    assert logits.dtype == F32 and logits.dim() == 3 and pos_map.dtype == F32 and pos_map.is_contiguous()
    B, nq, T = logits.shape
    assert logits.stride(2) == 1 and (B == 1 or logits.stride(0) == nq * logits.stride(1)), "rows (b, q): one strided matrix"
    assert pos_map.dim() in (2, 3) and pos_map.shape[-1] == T and (pos_map.dim() == 2 or pos_map.shape[0] == B)
    Cn = pos_map.shape[-2]
    if n_cls is not None:
        assert n_cls.dtype == torch.int32 and n_cls.is_contiguous() and tuple(n_cls.shape) == (B,)
    if out is None:
        out = torch.empty((B, nq, Cn), device=logits.device, dtype=F32)
    assert out.dtype == F32 and out.is_contiguous() and tuple(out.shape) == (B, nq, Cn)
    check(_lib.lib().ink_class_scores(_p(logits), logits.stride(1), _p(pos_map), Cn * T if pos_map.dim() == 3 else 0,
                                      _p(n_cls), B, nq, T, Cn, _p(out), _stream()), "ink_class_scores")
    return out


def select_boxes(idx: torch.Tensor, boxes: torch.Tensor, scale_wh: torch.Tensor, Cmax: int):
    """The selected (query, class) pairs idx int32 [B, K] (= query * Cmax + class) of boxes f32 [B, nq, 4] cxcywh ->
    (xyxy boxes f32 [B, K, 4] times scale_wh f32 [B, 2] = (w, h), labels int32 [B, K], queries int32 [B, K])."""
    assert idx.dtype == torch.int32 and idx.is_contiguous() and idx.dim() == 2
    assert boxes.dtype == F32 and boxes.is_contiguous() and boxes.dim() == 3 and boxes.shape[2] == 4
    B, K = idx.shape
    assert boxes.shape[0] == B and scale_wh.dtype == F32 and scale_wh.is_contiguous() and tuple(scale_wh.shape) == (B, 2)
    out = torch.empty((B, K, 4), device=idx.device, dtype=F32)
    labels, query = torch.empty_like(idx), torch.empty_like(idx)
    check(_lib.lib().ink_select_boxes(_p(idx), _p(boxes), _p(scale_wh), B, K, boxes.shape[1], Cmax, _p(out), _p(labels),
                                      _p(query), _stream()), "ink_select_boxes")
    return out, labels, query


def sine_embed4(ref: torch.Tensor, dim_t: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    assert ref.dtype == F32 and ref.is_contiguous() and ref.shape[-1] == 4 and dim_t.numel() == 128
    N = ref.numel() // 4
    if out is None:
        out = torch.empty((N, 512), device=ref.device, dtype=F16)
    assert out.dtype == F16 and out.is_contiguous() and tuple(out.shape) == (N, 512)
    check(_lib.lib().ink_sine_embed4(ref.data_ptr(), dim_t.data_ptr(), N, out.data_ptr(), _stream()),
          "ink_sine_embed4")
    return out


def box_refine(delta: torch.Tensor, ref: torch.Tensor, ref_is_logit: bool = False,
               out: Optional[torch.Tensor] = None) -> torch.Tensor:
    assert delta.dtype == F32 and delta.stride(1) == 1 and ref.dtype == F32 and ref.is_contiguous()
    N = ref.numel() // 4
    if out is None:
        out = torch.empty_like(ref)
    assert out.dtype == F32 and out.is_contiguous() and out.shape == ref.shape
    check(_lib.lib().ink_box_refine(delta.data_ptr(), delta.stride(0), ref.data_ptr(), N, int(ref_is_logit),
                                    out.data_ptr(), _stream()), "ink_box_refine")
    return out


# ---------------------------------------------------------------------------------------------
# refinement hand-off ops
# ---------------------------------------------------------------------------------------------
def mask_cleanup(masks_u8: torch.Tensor, k: int, area_threshold: int = 500, aspect_threshold: float = 1.1,
                 out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """clean_up_mask (InkLayer/refinement/mask_cleaner.py:11-36) for [n, H, W] uint8 masks (> 127 = foreground) on
    the GPU: k x k closing, 8-connected components, area / aspect filter.  -> uint8 0/255 [n, H, W]."""
    assert masks_u8.dtype == torch.uint8 and masks_u8.is_cuda and masks_u8.is_contiguous() and masks_u8.dim() == 3
    n, H, W = masks_u8.shape
    if out is None:
        out = torch.empty_like(masks_u8)
    if n == 0:
        return out
    assert out.dtype == torch.uint8 and out.is_contiguous() and out.shape == masks_u8.shape
    need = C.c_int64(0)
    check(_lib.lib().ink_mask_cleanup_workspace_ints(n, H, W, k, C.byref(need)), "ink_mask_cleanup_workspace_ints")
    ws = torch.empty(need.value, device=masks_u8.device, dtype=torch.int32)
    ta, tb = torch.empty_like(masks_u8), torch.empty_like(masks_u8)
    check(_lib.lib().ink_mask_cleanup(masks_u8.data_ptr(), n, H, W, k, area_threshold, float(aspect_threshold),
                                      ta.data_ptr(), tb.data_ptr(), ws.data_ptr(), out.data_ptr(), _stream()),
          "ink_mask_cleanup")
    out._ink_overflow_flag = ws[:1]        # stays 0 by construction (run bound of a closed image); tests read it
    return out


def mask_sketch_iou_counts(masks_u8: torch.Tensor, sketch_rgb_u8: torch.Tensor) -> torch.Tensor:
    """int32 [n, n, 2] = (|r_i & r_j|, |r_i | r_j|), r = (mask > 0) & (PIL-luma(sketch) < 250)
    (InkLayer/refinement/nms_sketch.py:62-78, 186-234)."""
    assert masks_u8.dtype == torch.uint8 and masks_u8.is_cuda and masks_u8.is_contiguous() and masks_u8.dim() == 3
    n, H, W = masks_u8.shape
    assert sketch_rgb_u8.dtype == torch.uint8 and sketch_rgb_u8.is_cuda and sketch_rgb_u8.is_contiguous()
    assert tuple(sketch_rgb_u8.shape) == (H, W, 3), "masks and sketch have the same size on this path"
    counts = torch.empty((n, n, 2), device=masks_u8.device, dtype=torch.int32)
    if n == 0:
        return counts
    bits = torch.empty((n, (H * W + 63) // 64), device=masks_u8.device, dtype=torch.int64)
    check(_lib.lib().ink_mask_sketch_iou_counts(masks_u8.data_ptr(), sketch_rgb_u8.data_ptr(), n, H, W,
                                                bits.data_ptr(), counts.data_ptr(), _stream()),
          "ink_mask_sketch_iou_counts")
    return counts


# ---------------------------------------------------------------------------------------------
# Depth-Anything-V2 pixel-side ops
# ---------------------------------------------------------------------------------------------
def depth_patchify(image_u8: torch.Tensor, nh: int, nw: int, P: int, KP: int, mean: Sequence[float],
                   std: Sequence[float], chan_reverse: bool) -> torch.Tensor:
    """image2tensor (cv2 cubic resize to (nh, nw), normalise) + 14x14 patch gather -> split-f16 [T, 3*KP]."""
    assert image_u8.dtype == torch.uint8 and image_u8.is_cuda and image_u8.is_contiguous() and image_u8.shape[2] == 3
    H, W = int(image_u8.shape[0]), int(image_u8.shape[1])
    out = torch.empty(((nh // P) * (nw // P), 3 * KP), device=image_u8.device, dtype=F16)
    check(_lib.lib().ink_depth_patchify(image_u8.data_ptr(), H, W, nh, nw, P, KP, (C.c_double * 3)(*mean),
                                        (C.c_double * 3)(*std), int(chan_reverse), out.data_ptr(), _stream()),
          "ink_depth_patchify")
    return out


def resize_bilinear_ac(x: torch.Tensor, B: int, h: int, w: int, H: int, W: int, out_dtype=F32) -> torch.Tensor:
    """F.interpolate(bilinear, align_corners=True) of an NHWC f32 map [B*h*w, C] -> [B*H*W, C] (f32 or f16)."""
    assert x.dtype == F32 and x.is_contiguous() and x.shape[0] == B * h * w
    Cn = x.shape[1]
    out = torch.empty((B * H * W, Cn), device=x.device, dtype=out_dtype)
    check(_lib.lib().ink_resize_bilinear_ac_nhwc(x.data_ptr(), B, h, w, Cn, H, W,
                                                 out.data_ptr() if out_dtype == F32 else None,
                                                 out.data_ptr() if out_dtype == F16 else None, _stream()),
          "ink_resize_bilinear_ac_nhwc")
    return out


def conv3x3(x16: torch.Tensor, B: int, H: int, W: int, w: torch.Tensor, bias: Optional[torch.Tensor] = None, *,
            stride: int = 1, relu_in: bool = False, act: Optional[str] = None, residual: Optional[torch.Tensor] = None,
            out: Optional[torch.Tensor] = None, out_dtype: torch.dtype = F32) -> torch.Tensor:
    """Direct 3x3 / pad 1 convolution (ink_conv3x3_f16): out = residual + act(conv(relu_in?(x16), w) + bias).

    x16: f16 NHWC [B*H*W, C]; w: f16 [N, 9*C] in (ky, kx, c) order; bias f32 [N]; residual f32 [B*OH*OW, N];
    act None / "relu".  -> [B*OH*OW, N] f32 or f16."""
    assert x16.dtype == F16 and w.dtype == F16 and x16.dim() == 2 and w.dim() == 2
    assert x16.is_contiguous() and w.is_contiguous() and x16.shape[0] == B * H * W
    assert stride in (1, 2) and act in (None, "relu")
    Cn, N = x16.shape[1], w.shape[0]
    assert w.shape[1] == 9 * Cn
    M = B * ((H - 1) // stride + 1) * ((W - 1) // stride + 1)
    if out is None:
        out = torch.empty((M, N), device=x16.device, dtype=out_dtype)
    assert out.dtype in (F16, F32) and out.is_contiguous() and tuple(out.shape) == (M, N)
    if bias is not None:
        assert bias.dtype == F32 and bias.numel() == N and bias.is_contiguous()
    if residual is not None:
        assert residual.dtype == F32 and residual.is_contiguous() and tuple(residual.shape) == (M, N)
    check(_lib.lib().ink_conv3x3_f16(_p(x16), B, H, W, Cn, _p(w), N, _p(bias), stride, int(relu_in), ACT[act],
                                     _p(residual), _p(out), int(out.dtype == F16), _stream()), "ink_conv3x3_f16")
    return out


# ---------------------------------------------------------------------------------------------
# Layer assembly: bit planes are int64 [n, H, ceil(W / 64)], images uint8
# ---------------------------------------------------------------------------------------------
def _planes_like(n: int, H: int, W: int, dev) -> torch.Tensor:
    return torch.empty((n, H, (W + 63) // 64), device=dev, dtype=torch.int64)


def _check_planes(p: torch.Tensor, W: int):
    assert p.dtype == torch.int64 and p.is_cuda and p.is_contiguous() and p.dim() == 3 and p.shape[2] == (W + 63) // 64
    return int(p.shape[0]), int(p.shape[1])


def layers_otsu_planes(gray_u8: torch.Tensor, invert: bool = True) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """[n, H, W] uint8 -> (planes of v > Otsu(v), hist int32 [n, 256], thresh int32 [n]); v = 255 - grey if invert."""
    assert gray_u8.dtype == torch.uint8 and gray_u8.is_cuda and gray_u8.is_contiguous() and gray_u8.dim() == 3
    n, H, W = (int(v) for v in gray_u8.shape)
    dev = gray_u8.device
    hist = torch.empty((n, 256), device=dev, dtype=torch.int32)
    thresh = torch.empty(n, device=dev, dtype=torch.int32)
    planes = _planes_like(n, H, W, dev)
    check(_lib.lib().ink_layers_otsu_planes(gray_u8.data_ptr(), n, H, W, int(invert), hist.data_ptr(), thresh.data_ptr(),
                                            planes.data_ptr(), _stream()), "ink_layers_otsu_planes")
    return planes, hist, thresh


def layers_dilate(planes: torch.Tensor, W: int, kernel_size: int, iterations: int) -> torch.Tensor:
    """cv2.dilate with the k x k ellipse (k = 3 or 5), `iterations` times."""
    n, H = _check_planes(planes, W)
    if iterations <= 0:
        return planes.clone()
    tmp, out = torch.empty_like(planes), torch.empty_like(planes)
    check(_lib.lib().ink_layers_dilate(planes.data_ptr(), n, H, W, kernel_size, iterations, tmp.data_ptr(), out.data_ptr(),
                                       _stream()), "ink_layers_dilate")
    return out


def layers_border_band(planes: torch.Tensor, W: int, band: int) -> torch.Tensor:
    """int32 [n]: 1 where the plane has a pixel within `band` of an image edge."""
    n, H = _check_planes(planes, W)
    flags = torch.empty(n, device=planes.device, dtype=torch.int32)
    check(_lib.lib().ink_layers_border_band(planes.data_ptr(), n, H, W, band, flags.data_ptr(), _stream()),
          "ink_layers_border_band")
    return flags


LAYERS_MODES = {"flood": 0, "fill_all": 1, "fill_rule": 2, "largest": 3}


def layers_components(planes: torch.Tensor, W: int, mode: str) -> Tuple[torch.Tensor, torch.Tensor]:
    """One component pass of get_mask (see ink_layers_components) -> (planes, workspace header int32 [514]:
    [0] overflow flag, [1] number of undecided holes of mode 'fill_rule', then their 8-int records).

    Mode 'largest' ranks components by a closed-form contour area that holds for components WITHOUT enclosed background;
    the caller guarantees it (get_mask hands over the complement of the corner flood, which has none).
    Mode 'fill_rule' records at most 64 undecided holes PER CALL, summed over all planes of the batch: [1] keeps
    counting beyond that, the records of the surplus are lost, and layers._resolve_undecided refuses such a header."""
    n, H = _check_planes(planes, W)
    need = C.c_int64(0)
    check(_lib.lib().ink_layers_components_workspace_ints(n, H, W, C.byref(need)), "ink_layers_components_workspace_ints")
    ws = torch.empty(need.value, device=planes.device, dtype=torch.int32)
    tmp = torch.empty((3,) + tuple(planes.shape), device=planes.device, dtype=torch.int64)
    out = torch.empty_like(planes)
    check(_lib.lib().ink_layers_components(planes.data_ptr(), n, H, W, LAYERS_MODES[mode], tmp.data_ptr(), ws.data_ptr(),
                                           out.data_ptr(), _stream()), "ink_layers_components")
    return out, ws[:514]


def layers_chamfer(mask_planes: torch.Tensor, stroke_planes: torch.Tensor, W: int, safety_margin: int = 0,
                   full: bool = False):
    """5x5 chamfer distance int32 16.16 [n, H, W] of the planes + get_mask's shrink step ->
    (dist, min over the stroke pixels int32 [n], shrink_by int32 [n], thresholded planes)."""
    n, H = _check_planes(mask_planes, W)
    assert _check_planes(stroke_planes, W) == (n, H)
    dev = mask_planes.device
    need = C.c_int64(0)
    check(_lib.lib().ink_layers_chamfer_workspace_ints(n, H, W, C.byref(need)), "ink_layers_chamfer_workspace_ints")
    ws = torch.empty(need.value, device=dev, dtype=torch.int32)
    dist = torch.empty((n, H, W), device=dev, dtype=torch.int32)
    mn = torch.empty(n, device=dev, dtype=torch.int32)
    shrink = torch.empty(n, device=dev, dtype=torch.int32)
    out = torch.empty_like(mask_planes)
    check(_lib.lib().ink_layers_chamfer(mask_planes.data_ptr(), stroke_planes.data_ptr(), n, H, W, safety_margin, int(full),
                                        dist.data_ptr(), ws.data_ptr(), mn.data_ptr(), shrink.data_ptr(), out.data_ptr(),
                                        _stream()), "ink_layers_chamfer")
    return dist, mn, shrink, out


def layers_mask_tables(masks_u8: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """[n, H, W] uint8 -> (bbox int32 [n, 4] with inclusive maxima, overlap int32 [n, n])."""
    assert masks_u8.dtype == torch.uint8 and masks_u8.is_cuda and masks_u8.is_contiguous() and masks_u8.dim() == 3
    n, H, W = (int(v) for v in masks_u8.shape)
    bbox = torch.empty((n, 4), device=masks_u8.device, dtype=torch.int32)
    overlap = torch.empty((n, n), device=masks_u8.device, dtype=torch.int32)
    check(_lib.lib().ink_layers_mask_tables(masks_u8.data_ptr(), n, H, W, bbox.data_ptr(), overlap.data_ptr(), _stream()),
          "ink_layers_mask_tables")
    return bbox, overlap


def layers_assemble(sketch_rgb_u8: torch.Tensor, masks_u8: torch.Tensor, bg_planes: torch.Tensor, bbox: torch.Tensor,
                    overlap: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """-> (sketch layers uint8 [n, H, W, 3] in (B, G, R), edit masks uint8 [n, H, W], debug images uint8 [n, H, W, 3])."""
    assert masks_u8.dtype == torch.uint8 and masks_u8.is_cuda and masks_u8.is_contiguous() and masks_u8.dim() == 3
    n, H, W = (int(v) for v in masks_u8.shape)
    assert sketch_rgb_u8.dtype == torch.uint8 and sketch_rgb_u8.is_cuda and sketch_rgb_u8.is_contiguous()
    assert tuple(sketch_rgb_u8.shape) == (H, W, 3) and _check_planes(bg_planes, W) == (n, H)
    assert bbox.dtype == torch.int32 and tuple(bbox.shape) == (n, 4) and bbox.is_contiguous() and bbox.is_cuda
    assert overlap.dtype == torch.int32 and tuple(overlap.shape) == (n, n) and overlap.is_contiguous() and overlap.is_cuda
    dev = masks_u8.device
    sketch = torch.empty((n, H, W, 3), device=dev, dtype=torch.uint8)
    edit = torch.empty((n, H, W), device=dev, dtype=torch.uint8)
    debug = torch.empty((n, H, W, 3), device=dev, dtype=torch.uint8)
    check(_lib.lib().ink_layers_assemble(sketch_rgb_u8.data_ptr(), masks_u8.data_ptr(), bg_planes.data_ptr(), bbox.data_ptr(),
                                         overlap.data_ptr(), n, H, W, sketch.data_ptr(), edit.data_ptr(), debug.data_ptr(),
                                         _stream()), "ink_layers_assemble")
    return sketch, edit, debug


def layers_composite(inpainted_rgb_u8: torch.Tensor, sketch_layer_u8: torch.Tensor) -> torch.Tensor:
    """The inpainted image with the sketch layer's own pixels put back (R, G, B)."""
    for t in (inpainted_rgb_u8, sketch_layer_u8):
        assert t.dtype == torch.uint8 and t.is_cuda and t.is_contiguous() and t.dim() == 3 and t.shape[2] == 3
    assert inpainted_rgb_u8.shape == sketch_layer_u8.shape
    H, W = int(inpainted_rgb_u8.shape[0]), int(inpainted_rgb_u8.shape[1])
    out = torch.empty_like(inpainted_rgb_u8)
    check(_lib.lib().ink_layers_composite(inpainted_rgb_u8.data_ptr(), sketch_layer_u8.data_ptr(), H, W, out.data_ptr(),
                                          _stream()), "ink_layers_composite")
    return out


def layers_gray(rgb_u8: torch.Tensor) -> torch.Tensor:
    """[n, H, W, 3] uint8 (R, G, B) -> the grey image cv2.imread(IMREAD_GRAYSCALE) gives, [n, H, W]."""
    assert rgb_u8.dtype == torch.uint8 and rgb_u8.is_cuda and rgb_u8.is_contiguous() and rgb_u8.dim() == 4 and rgb_u8.shape[3] == 3
    n, H, W = (int(v) for v in rgb_u8.shape[:3])
    gray = torch.empty((n, H, W), device=rgb_u8.device, dtype=torch.uint8)
    check(_lib.lib().ink_layers_gray(rgb_u8.data_ptr(), n, H, W, gray.data_ptr(), _stream()), "ink_layers_gray")
    return gray


def layers_rgba(gray_u8: torch.Tensor, bg_planes: torch.Tensor) -> torch.Tensor:
    """-> uint8 [n, H, W, 4]: the RGBA layers."""
    assert gray_u8.dtype == torch.uint8 and gray_u8.is_cuda and gray_u8.is_contiguous() and gray_u8.dim() == 3
    n, H, W = (int(v) for v in gray_u8.shape)
    assert _check_planes(bg_planes, W) == (n, H)
    rgba = torch.empty((n, H, W, 4), device=gray_u8.device, dtype=torch.uint8)
    check(_lib.lib().ink_layers_rgba(gray_u8.data_ptr(), bg_planes.data_ptr(), n, H, W, rgba.data_ptr(), _stream()),
          "ink_layers_rgba")
    return rgba


# ---------------------------------------------------------------------------------------------
# Visualisation: the coloured sketch (csrc/visualize.hip)
# ---------------------------------------------------------------------------------------------
def _check_sketch(t: torch.Tensor, what: str) -> Tuple[int, int, int]:
    assert t.dtype == torch.uint8 and t.is_cuda and t.is_contiguous(), f"{what}: contiguous uint8 CUDA tensor expected"
    assert t.dim() == 2 or (t.dim() == 3 and t.shape[2] == 3), f"{what}: sketch [H, W, 3] or [H, W] expected"
    return (1 if t.dim() == 2 else 3), int(t.shape[0]), int(t.shape[1])


def vis_gray_min(sketch_u8: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """int32 [1] on the device: the smallest grey over the stroke pixels (grey < 250) of the sketch, 0x7f7f7f7f when it
    has none.  `out`: a buffer to reuse (it is reset on the stream)."""
    ch, H, W = _check_sketch(sketch_u8, "vis_gray_min")
    if out is None:
        out = torch.empty(1, device=sketch_u8.device, dtype=torch.int32)
    assert out.dtype == torch.int32 and out.is_cuda and out.numel() == 1
    check(_lib.lib().ink_vis_gray_min(sketch_u8.data_ptr(), ch, H, W, out.data_ptr(), _stream()), "ink_vis_gray_min")
    return out


def vis_colour(sketch_u8: torch.Tensor, masks_or_label_u8: torch.Tensor, tables_u8: torch.Tensor, gray_min: torch.Tensor,
               by_label: bool = False) -> torch.Tensor:
    """color_sketch_by_masks -> uint8 [H, W, 3].  masks_or_label_u8: the masks [n, H, W] (non-zero = inside, the last one
    holding a pixel wins) or, by_label, the label image [H, W]; tables_u8: [2, n + 1, 256, 3] from
    visualize.colour_tables; gray_min: what vis_gray_min returned for this sketch."""
    ch, H, W = _check_sketch(sketch_u8, "vis_colour")
    m = masks_or_label_u8
    assert m.dtype == torch.uint8 and m.is_cuda and m.is_contiguous(), "vis_colour: contiguous uint8 CUDA masks expected"
    assert tables_u8.dtype == torch.uint8 and tables_u8.is_cuda and tables_u8.is_contiguous() and tables_u8.dim() == 4
    n = int(tables_u8.shape[1]) - 1
    assert tuple(tables_u8.shape) == (2, n + 1, 256, 3)
    assert tuple(m.shape) == ((H, W) if by_label else (n, H, W)), "vis_colour: masks / label image do not fit the tables"
    assert gray_min.dtype == torch.int32 and gray_min.is_cuda and gray_min.numel() == 1
    out = torch.empty((H, W, 3), device=sketch_u8.device, dtype=torch.uint8)
    check(_lib.lib().ink_vis_colour(sketch_u8.data_ptr(), ch, m.data_ptr() if m.numel() else None, n, int(bool(by_label)),
                                    tables_u8.data_ptr(), gray_min.data_ptr(), H, W, out.data_ptr(), _stream()),
          "ink_vis_colour")
    return out


# ---------------------------------------------------------------------------------------------
# Evaluation: counting predictions against a ground-truth label image (csrc/evaluate.hip)
# ---------------------------------------------------------------------------------------------
EVAL_MAX_VALUES = 256       # columns of a contingency table (csrc/evaluate.hip EVAL_MAX_U)
_EVAL_ELEM = {torch.uint8: 1, torch.uint16: 2, torch.int32: 4}


def _check_rank(rank_u16: torch.Tensor, what: str) -> Tuple[int, int]:
    assert rank_u16.dtype == torch.uint16 and rank_u16.is_cuda and rank_u16.is_contiguous() and rank_u16.dim() == 2, \
        f"{what}: contiguous uint16 CUDA rank image [H, W] expected"
    return int(rank_u16.shape[0]), int(rank_u16.shape[1])


def eval_label_ranks(labels: torch.Tensor, values_cap: int = EVAL_MAX_VALUES):
    """-> (rank uint16 [H, W], values int32 [values_cap], info int32 [2]), all on the device: values[:U] = the sorted
    distinct values of the label image (uint8, uint16 or int32, 0 .. 65535), rank = each pixel's index among them,
    info = (U, error flag: some value negative or above 65535).  The caller reads `info` (one synchronisation)."""
    assert labels.dtype in _EVAL_ELEM and labels.is_cuda and labels.is_contiguous() and labels.dim() == 2, \
        "eval_label_ranks: contiguous uint8 / uint16 / int32 CUDA label image [H, W] expected"
    H, W = (int(v) for v in labels.shape)
    dev = labels.device
    work = torch.empty(4096, device=dev, dtype=torch.int32)
    values = torch.zeros(int(values_cap), device=dev, dtype=torch.int32)
    info = torch.empty(2, device=dev, dtype=torch.int32)
    rank = torch.empty((H, W), device=dev, dtype=torch.uint16)
    check(_lib.lib().ink_eval_label_ranks(labels.data_ptr(), _EVAL_ELEM[labels.dtype], H, W, work.data_ptr(),
                                          values.data_ptr(), int(values_cap), info.data_ptr(), rank.data_ptr(), _stream()),
          "ink_eval_label_ranks")
    return rank, values, info


def eval_contingency(pred_u8: torch.Tensor, rank_u16: torch.Tensor, n_values: int, n_labels: Optional[int] = None,
                     sketch_u8: Optional[torch.Tensor] = None) -> torch.Tensor:
    """-> int32 [n + 1, n_values]: [i, u] = pixels inside prediction i with ground-truth rank u, row n = every counted
    pixel.  pred_u8: the masks [n, H, W] (non-zero = inside) or, with n_labels = n given, a label image [H, W] (l = mask
    l - 1).  sketch_u8 given: only its stroke pixels (grey < 250) count."""
    H, W = _check_rank(rank_u16, "eval_contingency")
    by_label = n_labels is not None
    assert pred_u8.dtype == torch.uint8 and pred_u8.is_cuda and pred_u8.is_contiguous(), \
        "eval_contingency: contiguous uint8 CUDA predictions expected"
    n = int(n_labels) if by_label else int(pred_u8.shape[0])
    assert tuple(pred_u8.shape) == ((H, W) if by_label else (n, H, W)), "eval_contingency: predictions do not fit the rank image"
    ch = 1
    if sketch_u8 is not None:
        ch, sh, sw = _check_sketch(sketch_u8, "eval_contingency")
        assert (sh, sw) == (H, W), "eval_contingency: sketch does not fit the rank image"
    table = torch.empty((n + 1, int(n_values)), device=rank_u16.device, dtype=torch.int32)
    check(_lib.lib().ink_eval_contingency(pred_u8.data_ptr() if pred_u8.numel() else None, n, int(by_label), rank_u16.data_ptr(),
                                          int(n_values), None if sketch_u8 is None else sketch_u8.data_ptr(), ch,
                                          int(sketch_u8 is not None), H, W, table.data_ptr(), _stream()),
          "ink_eval_contingency")
    return table


def eval_label_boxes(rank_u16: torch.Tensor, n_values: int) -> torch.Tensor:
    """-> int32 [n_values, 4]: xmin, ymin, xmax, ymax (inclusive) of the pixels of every rank."""
    H, W = _check_rank(rank_u16, "eval_label_boxes")
    boxes = torch.empty((int(n_values), 4), device=rank_u16.device, dtype=torch.int32)
    check(_lib.lib().ink_eval_label_boxes(rank_u16.data_ptr(), int(n_values), H, W, boxes.data_ptr(), _stream()),
          "ink_eval_label_boxes")
    return boxes


def eval_paint_labels(rank_u16: torch.Tensor, colors_u8: torch.Tensor) -> torch.Tensor:
    """-> uint8 [H, W, 3]: colors_u8 [U, 3] looked up by rank."""
    H, W = _check_rank(rank_u16, "eval_paint_labels")
    assert colors_u8.dtype == torch.uint8 and colors_u8.is_cuda and colors_u8.is_contiguous() and colors_u8.dim() == 2 \
        and colors_u8.shape[1] == 3, "eval_paint_labels: contiguous uint8 CUDA colours [U, 3] expected"
    out = torch.empty((H, W, 3), device=rank_u16.device, dtype=torch.uint8)
    check(_lib.lib().ink_eval_paint_labels(rank_u16.data_ptr(), colors_u8.data_ptr(), int(colors_u8.shape[0]), H, W,
                                           out.data_ptr(), _stream()), "ink_eval_paint_labels")
    return out


# ---------------------------------------------------------------------------------------------
# Inpainting pre- and post-processing (csrc/inpaint_ops.hip): uint8 [H, W, 3] (R, G, B) and uint8 [H, W]
# ---------------------------------------------------------------------------------------------
def _check_img(t: torch.Tensor, channels: int, what: str) -> Tuple[int, int]:
    assert t.dtype == torch.uint8 and t.is_cuda and t.is_contiguous(), f"{what}: contiguous uint8 CUDA tensor expected"
    if channels == 1:
        assert t.dim() == 2, f"{what}: [H, W] expected"
    else:
        assert t.dim() == 3 and t.shape[2] == channels, f"{what}: [H, W, {channels}] expected"
    return int(t.shape[0]), int(t.shape[1])


def _stencil_size(H: int, W: int, what: str) -> None:
    if H < 3 or W < 3:
        raise ValueError(f"{what}: images smaller than 3 pixels on a side are not supported (got {W}x{H})")


def inp_contrast(rgb_u8: torch.Tensor, factor: float = 1.2) -> torch.Tensor:
    """ImageEnhance.Contrast(image).enhance(factor), bit for bit."""
    H, W = _check_img(rgb_u8, 3, "inp_contrast")
    _stencil_size(H, W, "inp_contrast")
    ws = torch.empty(1, device=rgb_u8.device, dtype=torch.int64)
    out = torch.empty_like(rgb_u8)
    check(_lib.lib().ink_inp_contrast(rgb_u8.data_ptr(), H, W, float(factor), ws.data_ptr(), out.data_ptr(), _stream()),
          "ink_inp_contrast")
    return out


def inp_bilateral(rgb_u8: torch.Tensor, tables: torch.Tensor) -> torch.Tensor:
    """cv2.bilateralFilter(rgb, 5, sigma, sigma); tables f32 [13 + 768] from inpaint.bilateral_tables."""
    H, W = _check_img(rgb_u8, 3, "inp_bilateral")
    _stencil_size(H, W, "inp_bilateral")
    assert tables.dtype == F32 and tables.is_cuda and tables.is_contiguous() and tables.numel() == 13 + 768
    out = torch.empty_like(rgb_u8)
    check(_lib.lib().ink_inp_bilateral(rgb_u8.data_ptr(), H, W, tables.data_ptr(), out.data_ptr(), _stream()),
          "ink_inp_bilateral")
    return out


def inp_mask_prepare(mask_u8: torch.Tensor, dilate_iterations: int = 1, blur: bool = True) -> torch.Tensor:
    """preprocess_mask: 3x3 dilation `dilate_iterations` times, then cv2.GaussianBlur((3, 3), 0)."""
    H, W = _check_img(mask_u8, 1, "inp_mask_prepare")
    _stencil_size(H, W, "inp_mask_prepare")
    if dilate_iterations <= 0 and not blur:
        return mask_u8.clone()
    tmp = torch.empty((2, H, W), device=mask_u8.device, dtype=torch.uint8)
    out = torch.empty_like(mask_u8)
    check(_lib.lib().ink_inp_mask_prepare(mask_u8.data_ptr(), H, W, max(int(dilate_iterations), 0), int(bool(blur)),
                                          tmp.data_ptr(), out.data_ptr(), _stream()), "ink_inp_mask_prepare")
    return out


def inp_resize_u8(image_u8: torch.Tensor, oh: int, ow: int, filter: str = "lanczos") -> torch.Tensor:
    """PIL `Image.resize((ow, oh), filter)` of a uint8 [H, W] or [H, W, 3] CUDA tensor, bit for bit; filter is
    "bilinear", "bicubic" or "lanczos".  The same size gives a copy."""
    return _resize_u8(image_u8, oh, ow, filter, None)


def inp_condition(rgb_u8: torch.Tensor, mask_u8: torch.Tensor) -> torch.Tensor:
    """make_inpaint_condition -> f32 [1, 3, H, W]."""
    H, W = _check_img(rgb_u8, 3, "inp_condition")
    assert _check_img(mask_u8, 1, "inp_condition") == (H, W), "image and mask must have the same dimensions"
    out = torch.empty((1, 3, H, W), device=rgb_u8.device, dtype=F32)
    check(_lib.lib().ink_inp_condition(rgb_u8.data_ptr(), mask_u8.data_ptr(), H, W, out.data_ptr(), _stream()),
          "ink_inp_condition")
    return out


def inp_cleanup(result_rgb_u8: torch.Tensor, taps11: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """The adaptive-threshold half of _adaptive_threshold_blend -> (clean uint8 [H, W, 3], thresh uint8 [H, W])."""
    H, W = _check_img(result_rgb_u8, 3, "inp_cleanup")
    _stencil_size(H, W, "inp_cleanup")
    assert taps11.dtype == F32 and taps11.is_cuda and taps11.is_contiguous() and taps11.numel() == 11
    dev = result_rgb_u8.device
    tmp = torch.empty((H, W), device=dev, dtype=F32)
    thresh = torch.empty((H, W), device=dev, dtype=torch.uint8)
    clean = torch.empty_like(result_rgb_u8)
    check(_lib.lib().ink_inp_cleanup(result_rgb_u8.data_ptr(), H, W, taps11.data_ptr(), tmp.data_ptr(), thresh.data_ptr(),
                                     clean.data_ptr(), _stream()), "ink_inp_cleanup")
    return clean, thresh


def inp_soft_blend(clean_rgb_u8: torch.Tensor, original_rgb_u8: torch.Tensor, mask_u8: torch.Tensor,
                   taps2: torch.Tensor) -> torch.Tensor:
    """The soft-mask half of _adaptive_threshold_blend (f64)."""
    H, W = _check_img(clean_rgb_u8, 3, "inp_soft_blend")
    _stencil_size(H, W, "inp_soft_blend")
    assert _check_img(original_rgb_u8, 3, "inp_soft_blend") == (H, W) and _check_img(mask_u8, 1, "inp_soft_blend") == (H, W)
    assert taps2.dtype == torch.float64 and taps2.is_cuda and taps2.is_contiguous() and taps2.numel() == 2
    tmp = torch.empty((H, W), device=clean_rgb_u8.device, dtype=torch.float64)
    out = torch.empty_like(clean_rgb_u8)
    check(_lib.lib().ink_inp_soft_blend(clean_rgb_u8.data_ptr(), original_rgb_u8.data_ptr(), mask_u8.data_ptr(), H, W,
                                        taps2.data_ptr(), tmp.data_ptr(), out.data_ptr(), _stream()), "ink_inp_soft_blend")
    return out


def inp_luma(rgb_u8: torch.Tensor, out_channels: int = 3) -> torch.Tensor:
    """image.convert("L") (out_channels 1) or .convert("L").convert("RGB") (3)."""
    H, W = _check_img(rgb_u8, 3, "inp_luma")
    assert out_channels in (1, 3)
    out = torch.empty((H, W) if out_channels == 1 else (H, W, 3), device=rgb_u8.device, dtype=torch.uint8)
    check(_lib.lib().ink_inp_luma(rgb_u8.data_ptr(), H, W, out_channels, out.data_ptr(), _stream()), "ink_inp_luma")
    return out


def inp_unsharp(image_u8: torch.Tensor, ww: int, fw: int, percent: int = 150, threshold: int = 3) -> torch.Tensor:
    """ImageFilter.UnsharpMask for a box radius below 1; (ww, fw) from inpaint.box_weights(radius)."""
    ch = 1 if image_u8.dim() == 2 else 3
    H, W = _check_img(image_u8, ch, "inp_unsharp")
    tmp = torch.empty(2 * H * W * ch, device=image_u8.device, dtype=torch.uint8)
    out = torch.empty_like(image_u8)
    check(_lib.lib().ink_inp_unsharp(image_u8.data_ptr(), H, W, ch, int(ww), int(fw), int(percent), int(threshold),
                                     tmp.data_ptr(), out.data_ptr(), _stream()), "ink_inp_unsharp")
    return out


def inp_rgba_cut(rgb_u8: torch.Tensor, mask_u8: torch.Tensor) -> torch.Tensor:
    """uint8 [H, W, 4]: the image with alpha 255 where mask > 128, zeros elsewhere."""
    H, W = _check_img(rgb_u8, 3, "inp_rgba_cut")
    assert _check_img(mask_u8, 1, "inp_rgba_cut") == (H, W)
    out = torch.empty((H, W, 4), device=rgb_u8.device, dtype=torch.uint8)
    check(_lib.lib().ink_inp_rgba_cut(rgb_u8.data_ptr(), mask_u8.data_ptr(), H, W, out.data_ptr(), _stream()),
          "ink_inp_rgba_cut")
    return out
