"""float64 references and per-element error bounds of the kernels under inklayer_amd/depth.py (Depth-Anything-V2 ViT-B +
DPT head) at the shapes production runs: flash attention at head_dim 64 with ragged key tiles, every GEMM form of the
engine on the two 128x128 tile families, the bilinear resize.  Shared by tests/test_depth_ops_gpu.py (the kernels) and
tests/test_depth_plan_cpu.py (dispatch / token tables, and that the bounds tell named mistakes apart, on the CPU).
Every function runs on whatever device its inputs live on."""
import math
from collections import namedtuple

import torch

from vith_ref import F16, F32, F64, GELU_ERF, H16, SUB16, U, assert_discriminates, assert_within, discrimination  # noqa: F401

DD, DHEADS, DHD = 768, 12, 64
SCALE64 = DHD ** -0.5
KP = 608                      # 3 * 14 * 14 = 588 patch columns padded to a multiple of 32 (DepthEngine.KP)

# token counts N = ph * pw + 1 the GPU attention cases run (ph = 37; pw = 37, 49, 38, 41, 51, 64, 83): the key tail
# n_k % 64 of each and why it is there (tests/test_depth_plan_cpu.py asserts the table)
ATTN_TOKENS = (1370, 1814, 1407, 1518, 1888, 2369, 3072)
ATTN_B2 = (1370, 1814)


def token_tail(N):
    """(keys in the last 64-key tile (64 = full), valid rows of the last 128-query block (128 = full))."""
    return (N - 1) % 64 + 1, (N - 1) % 128 + 1


# ---------------------------------------------------------------------------------------------------------------
# flash_attn, head_dim 64, no bias (flash_attn_kernel<64, 0, 4>)
# ---------------------------------------------------------------------------------------------------------------
PROBE_COL = 3
V_SHIFT = slice(8, 16)


def probe_rows(N):
    return (9, 600, N - 2)


def lastkey_rows(N):
    return (5, N - 1)


def attn64_data(N, B, gen, dev):
    """Packed f16 qkv [B*N, 2304] as the qkv GEMM writes it.  q, k ~ N(0, 1.4^2) (logit std ~2: peaked rows), v ~ N(0, 1);
    every 16th query scaled by 1/40 (near-uniform rows).  Gaussian data alone cannot show an unmasked key tail: a zero
    phantom key has logit 0, the typical logit, and V ~ 0 on average.  So per batch entry and head:
      * column 3 of every key is the constant 4, and queries 9, 600, N-2 are 0.1 N(0, 1) with -24 in that column: every
        real key's logit is shifted by -12 (no change to the softmax), a phantom zero key keeps logit 0 and takes the row;
      * V columns 8..15 of every head get +1, so that such a row's output is far from the phantom's 0;
      * key N-1 is scaled by 1.5 (but column 3) and queries 5 and N-1 are set to it: the last key is their row maximum by
        >= 8 logits, so the running max rises inside the ragged tile and a dropped last key takes the row's weight."""
    qkv = torch.randn(B * N, 3 * DD, generator=gen, device=dev)
    qkv[:, :2 * DD] *= 1.4
    for b in range(B):
        e = qkv[b * N:(b + 1) * N]
        q, k, v = (e[:, i * DD:(i + 1) * DD].unflatten(1, (DHEADS, DHD)) for i in range(3))
        q[::16] /= 40
        k[:, :, PROBE_COL] = 4.0
        v[:, :, V_SHIFT] += 1.0
        for r in probe_rows(N):
            q[r] = 0.1 * torch.randn(DHEADS, DHD, generator=gen, device=dev)
            q[r, :, PROBE_COL] = -24.0
        k[N - 1] *= 1.5
        k[N - 1, :, PROBE_COL] = 4.0
        for r in lastkey_rows(N):
            q[r] = k[N - 1]
    return qkv.half()


def attn64_split(qkv, N, b, heads=slice(None), rows=None):
    """float64 (q [H, nq, 64], k, v [H, N, 64]) of batch entry b of a packed qkv; rows: query rows (default all)."""
    e = qkv[b * N:(b + 1) * N].double()
    q, k, v = (e[:, i * DD:(i + 1) * DD].unflatten(1, (DHEADS, DHD))[:, heads].permute(1, 0, 2) for i in range(3))
    if rows is not None:
        q = q[:, rows]
    return q, k, v


def attn64_ref(q, k, v, *, drop=None, phantom=0, scale=SCALE64):
    """float64 softmax(scale q k^T) v; returns (o, P, s).  Mistakes: drop (key indices / slice left out), phantom (that
    many zero K / V rows after the last key take part: an unmasked tile tail), scale (1.0: scale omitted)."""
    s = scale * (q @ k.transpose(-1, -2))
    if phantom:
        s = torch.cat([s, s.new_zeros(*s.shape[:-1], phantom)], -1)
        v = torch.cat([v, v.new_zeros(*v.shape[:-2], phantom, v.shape[-1])], -2)
    if drop is not None:
        s = s.clone()
        s[..., drop] = -math.inf
    P = torch.softmax(s, -1)
    return P @ v, P, s


def attn64_tol(q, k, v, P, s, o):
    """Bound of flash_attn_kernel<HD = 64, MODE 0, 4 waves> (attention.hip), per output element; logit units.
    Scores: q.k is 4 MFMA 32x32x16 steps of 16 exact f16 products, <= 6 roundings each: 24 u mag_k, mag_k = scale |q|.|k|.
    p_k = exp2(fma(s_k, c, -m)) with m the true running max (rescale by alpha = exp2(m_old - m_new) whenever it rises):
    c = f32(scale) * f32(log2 e) is off by <= 2 u relative (2 u |s_k|), the fma rounds once (u (|s_k| + |m|), |m| <=
    max_j |s_j|), v_exp_f32 is good to 1 ulp (2 u): delta_k <= 24 u mag_k + 4 u (|s_k| + max_j |s_j|) + 4 u relative on p_k.
    An error of m or alpha is common to a row's numerator and denominator.  For HD = 64 there is no ones-column in V
    (DVP == HD): the row sum l is added on the VALU from the UNROUNDED f32 p, the numerator uses f16(p).  So delta_k is
    common to both and moves o by sum_k P_k delta_k |v_k - o|, but the f16 rounding of P is in the numerator alone and
    does not cancel: 2^-11 sum_k P_k |v_k|, and 2^-25 sum_k |v_k| for p in the f16 subnormal range (p <= 1 when it is
    rounded, later rescales only shrink it; l >= 1 at the end since the row max has p = 1).
    Numerator: 4 P.V MFMA steps per 64-key tile, <= 6 roundings each, and at most one rescale per tile: 25 T u sum P |v|
    (T = ceil(n_k / 64) tiles).  l: 32 adds per tile and lane (<= 32 u of the tile's part), one add per tile into l_run,
    one rescale per tile, one cross-half add: (34 + 2 T) u relative, times |o|.  o = O * (1 / l): 3 u |o|; the f16 store
    2^-11 |o| + 2^-25.  |v_k - o| <= |v_k| + |o|, so every term is a matrix product."""
    nk = k.shape[-2]
    T = -(-nk // 64)
    mag = SCALE64 * (q.abs() @ k.abs().transpose(-1, -2))
    smax = s.abs().amax(-1, keepdim=True)
    Pd = P * (24 * U * mag + 4 * U * (s.abs() + smax) + 4 * U)
    va, oa = v.abs(), o.abs()
    A = P @ va
    return (Pd @ va + Pd.sum(-1, keepdim=True) * oa + H16 * A + SUB16 * va.sum(-2, keepdim=True)
            + 25 * T * U * A + ((37 + 2 * T) * U + H16) * oa + SUB16)


def attn64_mistakes(q, k, v, N):
    """(name, wrong o) of the mistakes a ragged-tile kernel can make on one batch entry (q [H, nq, 64], k, v [H, N, 64],
    H >= 2).  'keys 32..63 of the last tile dropped' exists where the tail is longer than 32."""
    tail = token_tail(N)[0]
    t0 = N - tail if tail < 64 else N - 64
    out = [("last key dropped", attn64_ref(q, k, v, drop=slice(N - 1, N))[0])]
    if tail < 64:
        out.append(("tail unmasked", attn64_ref(q, k, v, phantom=64 - tail)[0]))
    if tail > 32:
        out.append(("keys 32..63 of the last tile dropped", attn64_ref(q, k, v, drop=slice(t0 + 32, N))[0]))
    out.append(("V of head h + 1", attn64_ref(q, k, v.roll(-1, 0))[0]))
    out.append(("scale omitted", attn64_ref(q, k, v, scale=1.0)[0]))
    return out


# ---------------------------------------------------------------------------------------------------------------
# the engine's GEMM forms
# ---------------------------------------------------------------------------------------------------------------
# kind: None (plain), "res" (linear residual, preloaded into the accumulators, not in place), "late" (col_scale, then
# the residual added in place: the late-residual epilogue), "pe" (split-f16 operands, residual = pos, out a view one row
# into the token buffer)
Form = namedtuple("Form", "rows N K act f16 bias kind")
_T = lambda ph, pw: ph * pw                                   # noqa: E731
_S3 = lambda ph, pw: ((ph - 1) // 2 + 1) * ((pw - 1) // 2 + 1)  # noqa: E731
DEPTH_GEMMS = {
    "pe": Form(_T, DD, 3 * KP, None, False, True, "pe"),
    "qkv": Form(lambda ph, pw: ph * pw + 1, 3 * DD, DD, None, True, True, None),
    "proj": Form(lambda ph, pw: ph * pw + 1, DD, DD, None, False, True, "late"),
    "fc1": Form(lambda ph, pw: ph * pw + 1, 4 * DD, DD, "gelu", True, True, None),
    "fc2": Form(lambda ph, pw: ph * pw + 1, DD, 4 * DD, None, False, True, "late"),
    "up0": Form(_T, 1536, 96, None, True, True, None),
    "rn0": Form(lambda ph, pw: 16 * ph * pw, 128, 864, None, False, False, None),
    "down3": Form(_S3, 768, 6912, None, True, True, None),
    "rcu1": Form(lambda ph, pw: 16 * ph * pw, 128, 1152, "relu", True, True, None),
    "rcu2": Form(lambda ph, pw: 16 * ph * pw, 128, 1152, None, False, True, "res"),
    "oc1": Form(lambda ph, pw: 64 * ph * pw, 64, 1152, None, False, True, None),
    "oc2": Form(lambda ph, pw: 196 * ph * pw, 32, 576, "relu", True, True, None),
    "oc3": Form(lambda ph, pw: 196 * ph * pw, 4, 32, "relu", False, True, None),
}
DEPTH_SIZES = ((37, 37), (37, 49))
# the forms test_depth_ops_gpu runs at 37 x 49 too (M changes the raggedness of the last tile row)
GEMM_AT_37x49 = ("pe", "qkv", "proj", "oc2", "oc3")
PROBE = 8                     # pe: rows / output columns 0..7 carry coherent f16 rounding errors


def gemm_shape(name, ph, pw):
    f = DEPTH_GEMMS[name]
    return f.rows(ph, pw), f.N, f.K


def gemm_bk(name):
    """K step of the 128x128 tile family the form runs on: 32 when K % 64 != 0 (variant 32), else 64 (variant 0)."""
    return 32 if DEPTH_GEMMS[name].K % 64 else 64


def _pow2_up(x):
    """|x| rounded down to a power of two, times (1 + 0.49 * 2^-10): 0.49 f16 ulp above an f16 number, always upward."""
    _, e = torch.frexp(x.abs().clamp(min=2.0 ** -10))
    return torch.ldexp(torch.full_like(x, 0.5 * (1 + 0.49 * 2.0 ** -10)), e)


def split_act(a32):
    """The activation side of a split-f16 GEMM as ink_add_split_f16 / ink_depth_patchify write it: [hi | (v - hi) * 64 |
    hi / 64] in f16 (the weight side is ops.split_weight: [W_hi | W_hi / 64 | (W - W_hi) * 64])."""
    hi = a32.to(F16)
    lo = ((a32 - hi.float()) * 64.0).to(F16)
    return torch.cat([hi, lo, (hi.float() * 0.015625).to(F16)], -1).contiguous()


def split_weight(w32):
    hi = w32.to(F16)
    lo = ((w32 - hi.float()) * 64.0).to(F16)
    return torch.cat([hi, (hi.float() / 64.0).to(F16), lo], -1).contiguous()


def gemm_data(name, M, gen, dev):
    """Operands of one engine GEMM at M rows, as a dict: a f16 [M, K] ~ N(0, 1), w f16 [N, K] ~ N(0, 1 / K), b ~ 0.1 N
    (None for rn0), r ~ N(0, 1) for the residual forms, cs ~ 0.5 + 0.1 N (LayerScale) for the late-residual forms.
    pe: a32 [M, 608] f32 ~ N(0, 1) and w32 [768, 608] ~ N(0, 1 / 588), columns 588.. zero, split into a / w [., 1824].
    Random rounding errors of a plain-f16 product stay within ~8x the bound (they add up like sqrt K against the bound's
    K), so the first 8 rows of a32 and the first 8 rows of w32 are powers of two times (1 + 0.49 * 2^-10): each is 0.49
    f16 ulp above its f16 rounding, all in one direction, and the low segments of that 8 x 8 block add up coherently."""
    f = DEPTH_GEMMS[name]
    d = {}
    if f.kind == "pe":
        a32 = torch.randn(M, KP, generator=gen, device=dev)
        w32 = torch.randn(f.N, KP, generator=gen, device=dev) / math.sqrt(588)
        a32[:PROBE], w32[:PROBE] = _pow2_up(a32[:PROBE]), _pow2_up(w32[:PROBE])
        a32[:, 588:], w32[:, 588:] = 0, 0
        d.update(a32=a32, w32=w32, a=split_act(a32), w=split_weight(w32))
    else:
        d["a"] = torch.randn(M, f.K, generator=gen, device=dev).half()
        d["w"] = (torch.randn(f.N, f.K, generator=gen, device=dev) / math.sqrt(f.K)).half()
    d["b"] = 0.1 * torch.randn(f.N, generator=gen, device=dev) if f.bias else None
    d["r"] = torch.randn(M, f.N, generator=gen, device=dev) if f.kind else None
    d["cs"] = 0.5 + 0.1 * torch.randn(f.N, generator=gen, device=dev) if f.kind == "late" else None
    return d


def gemm_ref(name, d, *, skip_k=None, drop_bias=False, drop_relu=False, drop_cs=False, cs_on_sum=False, res_times=1,
             plain_f16=False):
    """float64 out = res_times * r + cs * act(a w^T + b), the pre-activation lin, and mag = sum_k |a_k w_k| + |b| (+ |r|
    where the residual is preloaded into the accumulator: kinds 'res' and 'pe').  pe: lin from the f32 operands a32, w32;
    mag from the split operands the kernel multiplies.
    Mistakes: skip_k (the K slice of the kernel's operands [k0, k0 + width) left out), drop_bias, drop_relu, drop_cs
    (col_scale = 1), cs_on_sum (col_scale applied to residual + product), res_times (0 / 2), plain_f16 (pe: only the
    high segments multiplied)."""
    f = DEPTH_GEMMS[name]
    a64, w64 = d["a"].double(), d["w"].double()
    if f.kind == "pe":
        lin = a64[:, :KP] @ w64[:, :KP].t() if plain_f16 else d["a32"].double() @ d["w32"].double().t()
    else:
        lin = a64 @ w64.t()
    if skip_k is not None:
        k0, kw = skip_k
        lin = lin - a64[:, k0:k0 + kw] @ w64[:, k0:k0 + kw].t()
    mag = a64.abs() @ w64.abs().t()
    if f.bias:
        mag = mag + d["b"].double().abs()
        if not drop_bias:
            lin = lin + d["b"].double()
    act = f.act
    out = torch.nn.functional.gelu(lin) if act == "gelu" else lin.clamp(min=0) if act == "relu" and not drop_relu else lin
    if f.kind == "late":
        r, cs = d["r"].double(), d["cs"].double()
        if cs_on_sum:
            out = cs * (res_times * r + out)
        else:
            out = res_times * r + (out if drop_cs else cs * out)
    elif f.kind:
        out = out + res_times * d["r"].double()
        mag = mag + d["r"].double().abs()
    return out, lin, mag


def gemm_tol(name, d, out, lin, mag):
    """gemm_f16_nt<128, 128, 64, 2, 2> and <128, 128, 32, 2, 2> both run BK / 32 MFMA 16x16x32 steps per K tile and
    K / BK tiles: K / 32 steps (K % 32 == 0 is an argument check), as vith_ref.gemm_tol assumes.  The f16 products are
    exact; a step sums its 32 products in <= 5 rounding levels (5 u sum_k |a_k w_k| over all steps) and adds them to
    the f32 accumulator once (K / 32 u mag, mag including a preloaded residual); the bias add 2 u mag: (K / 32 + 7) u mag.
    ReLU is exact and 1-Lipschitz.  GELU as in vith_ref.gemm_tol.  Late residual (col_scale set): v = cs * (a w^T + b)
    rounds once (u |cs lin|) on top of |cs| times the above, r + v rounds once more (u |out|).  f16 outputs add half an
    f16 ulp (2^-11 relative, 2^-25 in the subnormal range).
    pe (split f16): the kernel multiplies [a_hi | 64 a_lo | a_hi / 64] by [w_hi | w_hi / 64 | 64 w_lo]: a w - a_lo w_lo
    with every segment rounded to f16.  Per k: the dropped a_lo w_lo <= 2^-22 |a w|, the f16 rounding of 64 a_lo and of
    64 w_lo <= 2^-22 |a w| each (less than 2^-20 |a w| in all, with the second-order terms); a segment in the f16
    subnormal range (|64 a_lo| or |w_hi / 64| < 2^-14) is off by 2^-25 absolute instead: <= 2^-29 (|a_k| + |w_k|) + 2^-42."""
    f = DEPTH_GEMMS[name]
    t = (f.K / 32 + 7) * U * mag
    if f.kind == "pe":
        a, w = d["a32"].double().abs(), d["w32"].double().abs()
        t = t + 2.0 ** -20 * (a @ w.t()) + 2.0 ** -29 * (a.sum(1, keepdim=True) + w.sum(1)[None]) + KP * 2.0 ** -42
    if f.act == "gelu":
        t = 1.13 * t + (GELU_ERF / 2 + 6 * U) * lin.abs() + U * out.abs()
    if f.kind == "late":
        cs = d["cs"].double()
        t = cs.abs() * t + U * (cs * lin).abs() + U * out.abs()
    if f.f16:
        t = t + H16 * out.abs() + SUB16
    return t


def gemm_mistakes(name, d):
    """(what, wrong output, required factor) of the mistakes that apply to the form.  The K step left out is the last
    one of the kernel's K loop; for pe that step holds 12 columns of a_hi w_lo and 20 of padding - under 2^-11 of 2 %
    of the product, inside any bound that allows an f32 accumulation - so there the last step of the HIGH segment
    (columns 576..607) is left out; the end of the K loop of that kernel instance is pinned by up0, rn0 and oc3."""
    f = DEPTH_GEMMS[name]
    bk = gemm_bk(name)
    k0 = KP - 32 if f.kind == "pe" else f.K - bk
    out = [(f"K step {k0}..{k0 + bk - 1} skipped", gemm_ref(name, d, skip_k=(k0, bk))[0], 100)]
    if f.bias:
        out.append(("bias dropped", gemm_ref(name, d, drop_bias=True)[0], 100))
    if f.act == "relu":
        out.append(("relu dropped", gemm_ref(name, d, drop_relu=True)[0], 100))
    if f.kind == "late":
        out.append(("col_scale dropped", gemm_ref(name, d, drop_cs=True)[0], 100))
        out.append(("col_scale applied to residual + product", gemm_ref(name, d, cs_on_sum=True)[0], 100))
    if f.kind:
        out.append(("residual dropped", gemm_ref(name, d, res_times=0)[0], 100))
        out.append(("residual added twice", gemm_ref(name, d, res_times=2)[0], 100))
        # half an f16 ulp is 2^13 / (K / 32 + 7) times the accumulation term on a residual-dominated element
        out.append(("f32 stream rounded to f16", gemm_ref(name, d)[0].to(F16).double(), 2))
    if f.kind == "pe":
        out.append(("low segments dropped (plain f16 product)", gemm_ref(name, d, plain_f16=True)[0], 100))
    return out


# ---------------------------------------------------------------------------------------------------------------
# resize_bilinear_ac (align_corners = True) on NHWC maps
# ---------------------------------------------------------------------------------------------------------------
def resize_ref(x, h, w, H, W, align_corners=True):
    """float64 F.interpolate(bilinear) of the NHWC map x [h*w, C] -> [H*W, C]."""
    C = x.shape[1]
    y = torch.nn.functional.interpolate(x.double().view(1, h, w, C).permute(0, 3, 1, 2), (H, W), mode="bilinear",
                                        align_corners=align_corners)
    return y.permute(0, 2, 3, 1).reshape(H * W, C)


def resize_tol(x, h, w, H, W, ref, f16_out):
    """resize_bilinear_ac_kernel: the source coordinate is f32 scale * dst with scale = f32((h - 1) / (H - 1)): two
    roundings, |fy - y| <= 2.5 u y; ly = fy - (int)fy is exact.  The interpolant is continuous and piecewise linear, so a
    coordinate error dy moves it by at most dy times the largest vertical difference of neighbouring rows in the cell
    of (y, x) and the eight cells around it (fy, fx may fall into the next cell); the same along x.  Two lerps (1 - l) a + l b, each: 1 - l rounds once, two products, one sum: <= 3 u max(|a|, |b|), so
    6 u max |v| over those cells (an fma contraction only removes roundings).  f16 out: 2^-11 |ref| + 2^-25."""
    C = x.shape[1]
    v = x.double().view(h, w, C)
    dev = x.device
    ys = torch.arange(H, device=dev, dtype=F64) * ((h - 1) / (H - 1) if H > 1 else 0.0)
    xs = torch.arange(W, device=dev, dtype=F64) * ((w - 1) / (W - 1) if W > 1 else 0.0)
    y0 = ys.floor().long().clamp(max=h - 1)
    x0 = xs.floor().long().clamp(max=w - 1)
    y1, x1 = (y0 + 1).clamp(max=h - 1), (x0 + 1).clamp(max=w - 1)

    def pool3(dif, dim):                     # max over an entry and its two neighbours along dim
        p = torch.nn.functional.pad(dif.movedim(dim, -1), (1, 1))
        return torch.maximum(torch.maximum(p[..., :-2], p[..., 1:-1]), p[..., 2:]).movedim(-1, dim)

    dyv = torch.zeros_like(v)
    dyv[:-1] = (v[1:] - v[:-1]).abs()
    dxv = torch.zeros_like(v)
    dxv[:, :-1] = (v[:, 1:] - v[:, :-1]).abs()
    dyv, dxv, av = (pool3(pool3(t, 0), 1) for t in (dyv, dxv, v.abs()))

    def corners(t):
        return torch.maximum(torch.maximum(t[y0][:, x0], t[y0][:, x1]), torch.maximum(t[y1][:, x0], t[y1][:, x1]))

    tol = (2.5 * U * ys)[:, None, None] * corners(dyv) + (2.5 * U * xs)[None, :, None] * corners(dxv) + 6 * U * corners(av)
    tol = tol.reshape(H * W, C)
    if f16_out:
        tol = tol + H16 * ref.abs() + SUB16
    return tol + 2.0 ** -149                # (an exactly-zero neighbourhood: 0 <= 0 must hold with a positive bound)
