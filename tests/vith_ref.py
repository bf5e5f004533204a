"""float64 references and per-element error bounds of the SAM ViT-H encoder kernels (block GEMMs, layernorm_rows,
relpos_bias, the window and global attention kernels, the LayerNorm fold), shared by tests/test_vith_ops_gpu.py (the
kernels at production shapes) and tests/test_vith_plan_cpu.py (that the bounds tell named mistakes apart, on the CPU).
Every function runs on whatever device its inputs live on."""
import math

import torch

F16, F32, F64 = torch.float16, torch.float32, torch.float64
U = 2.0 ** -24            # f32 unit roundoff
H16 = 2.0 ** -11          # half an f16 ulp, relative (normal range)
SUB16 = 2.0 ** -25        # half the f16 subnormal spacing
D, HEADS, HD, T, G, WS = 1280, 16, 80, 4096, 64, 14
SCALE = HD ** -0.5
GELU_ERF = 1.5e-7         # |erf - A&S 7.1.26| (gelu_erf in common.h)


def discrimination(wrong, ref, tol) -> float:
    """max |wrong - ref| / tol: how far outside the bound a mistake lands (a NaN result counts as infinitely far)."""
    return ((wrong - ref).abs() / tol).nan_to_num(nan=math.inf).max().item()


def assert_discriminates(wrong, ref, tol, what, factor=100):
    m = discrimination(wrong, ref, tol)
    assert m >= factor, f"the bound cannot tell the mistake '{what}' apart: max deviation {m:.1f}x the bound"
    return m


def assert_within(got, ref, tol, what) -> float:
    """Per-element check (NaN-safe: a NaN output is out of bound); returns the worst error as a fraction of the bound."""
    err = (got - ref).abs()
    bad = ~(err <= tol)
    if bad.any():
        i = int(bad.flatten().nonzero()[0])
        raise AssertionError(f"{what}: {int(bad.sum())} / {bad.numel()} elements out of bound; first at flat {i}: "
                             f"got {got.flatten()[i].item()!r}, ref {ref.flatten()[i].item()!r}, "
                             f"tol {tol.flatten()[i].item() if torch.is_tensor(tol) else tol!r}")
    return (err / tol).max().item()


# ---------------------------------------------------------------------------------------------------------------
# block GEMMs: qkv (f16 out), proj (f32, residual in place), lin1 (GELU, f16 out), lin2 (K = 5120, in place)
# ---------------------------------------------------------------------------------------------------------------
# name -> (N, K, act, f16 output, in-place residual)
GEMM_FORMS = {"qkv": (3 * D, D, None, True, False), "proj": (D, D, None, False, True),
              "lin1": (4 * D, D, "gelu", True, False), "lin2": (D, 4 * D, None, False, True)}


def gemm_data(form, M, gen, dev):
    """Operands of one block GEMM at M rows: a ~ N(0, 1) (the LayerNorm output / attention output / GELU output
    scale), w ~ N(0, 1 / K) (seeded ViT-H weights), bias ~ N(0, 0.1), residual ~ N(0, 1)."""
    N, K, _, _, res = GEMM_FORMS[form]
    a = torch.randn(M, K, generator=gen, device=dev).half()
    w = (torch.randn(N, K, generator=gen, device=dev) / math.sqrt(K)).half()
    b = 0.1 * torch.randn(N, generator=gen, device=dev)
    r = torch.randn(M, N, generator=gen, device=dev) if res else None
    return a, w, b, r


def gemm_ref(form, a, w, b, r, skip_k=None, drop_bias=False, res_times=1):
    """float64 out = res_times * r + act(a w^T + b) and the linear part's magnitude sum_k |a_k w_k| + |r| + |b|.
    skip_k: the 64-wide K slice starting there left out (a mistake)."""
    act = GEMM_FORMS[form][2]
    a64, w64 = a.double(), w.double()
    lin = a64 @ w64.t()
    if skip_k is not None:
        lin = lin - a64[:, skip_k:skip_k + 64] @ w64[:, skip_k:skip_k + 64].t()
    if not drop_bias:
        lin = lin + b.double()
    mag = a64.abs() @ w64.abs().t() + b.double().abs()
    if r is not None:
        mag = mag + r.double().abs()
    out = torch.nn.functional.gelu(lin) if act == "gelu" else lin
    if r is not None:
        out = out + res_times * r.double()
    return out, lin, mag


def gemm_tol(form, out, lin, mag):
    """The MFMA 16x16x32 f16 products are exact.  Each of the K/32 MFMA steps sums its 32 products in at most 5 levels
    of roundings, each bounded by that step's own sum |a_k w_k|: over all steps 5 u sum_k |a_k w_k|.  Its one add
    to the f32 accumulator rounds against the running sum, <= sum |a_k w_k| + |residual| (the residual is preloaded
    into the accumulator): K/32 u mag.  The epilogue's bias add 2 u mag.  So (K/32 + 7) u mag.
    GELU (gelu_erf): |gelu'| <= 1.13 carries that through, the A&S erf error 1.5e-7
    enters times |x| / 2, its exp2 / rcp / polynomial roundings 6 u |x|.  f16 outputs add half an f16 ulp of the result
    (2^-11 relative, 2^-25 absolute in the subnormal range)."""
    N, K, act, f16, _ = GEMM_FORMS[form]
    t = (K / 32 + 7) * U * mag
    if act == "gelu":
        t = 1.13 * t + (GELU_ERF / 2 + 6 * U) * lin.abs() + U * out.abs()
    if f16:
        t = t + H16 * out.abs() + SUB16
    return t


def f16_stream(ref):
    """The in-place f32 output rounded to f16 on the way out (a mistake: the residual stream losing f32 precision)."""
    return ref.to(F16).double()


def swap_tiles(ref, BM=256, BN=320):
    """ref with output tile (0, 0) and its grouped-order neighbour (1, 0) exchanged (a mistake)."""
    wrong = ref.clone()
    wrong[:BM, :BN], wrong[BM:2 * BM, :BN] = ref[BM:2 * BM, :BN], ref[:BM, :BN]
    return wrong


# ---------------------------------------------------------------------------------------------------------------
# layernorm_rows at C = 1280
# ---------------------------------------------------------------------------------------------------------------
def layernorm_data(R, gen, dev, C=D):
    """R rows of C (default 1280) with the hard cases up front: rows 0-7 a common offset of 30 std (|mean| / std = 30), rows
    8-15 four 'massive' channels 100x the rest, rows 16-19 constant (var = 0: rstd = eps^-1/2; 3.25 sums exactly),
    rows 20-23 N(0, 1) on an offset of +-3000 (where a one-pass E[x^2] - mean^2 variance in f32 is lost), the rest
    N(0.5, 3).  gamma 1 + 0.1 N and beta 0.1 N, but channels 0-63 have gamma 2^-18, beta 0 (f16-subnormal outputs)."""
    x = 3 * torch.randn(R, C, generator=gen, device=dev) + 0.5
    x[0:8] = torch.randn(8, C, generator=gen, device=dev) + 30 * torch.tensor([1, -1, 1, -1, 1, -1, 1, -1.0], device=dev)[:, None]
    x[8:16] = torch.randn(8, C, generator=gen, device=dev)
    x[8:16, [3, 700, 701, C - 1]] *= 100
    x[16:20] = 3.25
    x[20:24] = torch.randn(4, C, generator=gen, device=dev) + 3000 * torch.tensor([1, -1, 1, -1.0], device=dev)[:, None]
    gamma = 1 + 0.1 * torch.randn(C, generator=gen, device=dev)
    gamma[:64] = 2.0 ** -18
    beta = 0.1 * torch.randn(C, generator=gen, device=dev)
    beta[:64] = 0
    return x, gamma, beta


def layernorm_ref(x, gamma, beta, eps=1e-6):
    return torch.nn.functional.layer_norm(x.double(), (x.shape[1],), gamma.double(), beta.double(), eps)


def layernorm_wrong(x, gamma, beta, mistake, eps=1e-6):
    """Mistakes: 'one-pass' (mean and E[x^2] in f32, var = E[x^2] - mean^2), 'no-eps' (eps left out of the sqrt)."""
    if mistake == "one-pass":
        mean = x.mean(1, keepdim=True)
        var = (x * x).mean(1, keepdim=True) - mean * mean
        rstd = torch.rsqrt(var + eps).double()
        mean = mean.double()
    else:
        x64 = x.double()
        mean = x64.mean(1, keepdim=True)
        rstd = 1.0 / torch.sqrt(x64.var(1, unbiased=False, keepdim=True))
    return (x.double() - mean) * rstd * gamma.double() + beta.double()


def layernorm_tol(x, gamma, beta, ref, eps=1e-6):
    """layernorm_rows (two-pass, one wave per row): the sums of x and of (x - mean)^2 are each <= 24 f32 roundings
    deep (5 float4 loads per lane, two-level pair sums, 6 shuffle levels), so |d mean| <= 26 u mean|x| (with the
    division); the variance carries 28 u relative plus d mean^2 / var (the cross term of the shifted sum vanishes),
    eps / sqrt / reciprocal 3 u, so rstd is off by <= 17 u + d mean^2 / (2 (var + eps)) relative; (x - mean) rstd gamma
    + beta adds 4 roundings.  Per element: |gamma| rstd (|x - mean| (22 u + d mean^2 / (var + eps)) + d mean) + u |ref|,
    and the f16 store half an ulp (2^-11 |ref|, 2^-25 subnormal)."""
    x64 = x.double()
    C = x.shape[1]
    mean = x64.mean(1, keepdim=True)
    var = x64.var(1, unbiased=False, keepdim=True)
    rstd = 1.0 / torch.sqrt(var + eps)
    dmu = 26 * U * x64.abs().mean(1, keepdim=True)
    g = gamma.double().abs()
    return (g * rstd * ((x64 - mean).abs() * (22 * U + dmu ** 2 / (var + eps)) + dmu) + U * ref.abs()
            + H16 * ref.abs() + SUB16)


# ---------------------------------------------------------------------------------------------------------------
# relpos_bias: rel_x[b, h, q, j] = (q . R_x[q_x - j + S - 1]) / scale
# ---------------------------------------------------------------------------------------------------------------
def relpos_ref(q, Rh, Rw, S, qrows, *, swap=False, flip=False, head_shift=0, scale_mode="div"):
    """float64 (rel_h, rel_w, mag_h, mag_w) [n, H, S*S, S] and qabs [n, H, S*S, 1] for the f16 query rows q[qrows]
    ([n, S*S] row indices, -1 = padding: zero query); mag = sum_d |q_d R_d| / scale, qabs = sum_d |q_d| / scale.
    Mistakes: swap (rel_h / rel_w tables exchanged), flip
    (k - q instead of q - k), head_shift (the q of head h + shift), scale_mode 'mul' (times scale) / 'none'."""
    n = qrows.shape[0]
    qq = torch.where((qrows >= 0)[..., None], q[qrows.clamp(min=0).long()].double(), torch.zeros((), dtype=F64, device=q.device))
    qq = qq.view(n, S * S, HEADS, HD).permute(0, 2, 1, 3)                   # [n, H, S*S, 80]
    if head_shift:
        qq = qq.roll(-head_shift, 1)
    if swap:
        Rh, Rw = Rw, Rh
    pos = torch.arange(S * S, device=q.device)
    j = torch.arange(S, device=q.device)
    f = {"div": 1 / SCALE, "mul": SCALE, "none": 1.0}[scale_mode]
    outs = []
    for R, coord in ((Rh, pos // S), (Rw, pos % S)):
        R64 = R.double()
        idx = (j[None, :] - coord[:, None] + S - 1) if flip else (coord[:, None] - j[None, :] + S - 1)
        full = qq @ R64.t()                                                   # [n, H, S*S, 2S-1]
        absf = qq.abs() @ R64.abs().t()
        gi = idx[None, None].expand(n, HEADS, S * S, S)
        outs.append((f * full.gather(-1, gi), absf.gather(-1, gi) / SCALE))
    qabs = qq.abs().sum(-1, keepdim=True) / SCALE
    return outs[0][0], outs[1][0], outs[0][1], outs[1][1], qabs


def relpos_tol(ref, mag, qabs, f16_out):
    """relpos_mfma_kernel: the f32 table is rounded to f16 in LDS (2^-11 |R_d| for a normal entry, 2^-25 for a
    subnormal one: 2^-11 mag + 2^-25 qabs); q is f16 already; 5 MFMA steps of 16 exact products, <= 6 roundings each:
    30 u mag; 1/scale rounded and the product 2 u |ref|; the output rounded to f16 (2^-11 |ref| + 2^-25) or f32
    (u |ref|)."""
    t = (H16 + 30 * U) * mag + SUB16 * qabs + 2 * U * ref.abs()
    return t + (H16 * ref.abs() + SUB16 if f16_out else U * ref.abs())


# ---------------------------------------------------------------------------------------------------------------
# attention (window and global kernels share the arithmetic the bound is derived from)
# ---------------------------------------------------------------------------------------------------------------
def attn_ref(q, k, v, bias):
    """float64 softmax(scale q k^T + bias) v for q [.., nq, 80], k, v [.., nk, 80], bias [.., nq, nk] in logit units;
    returns (o, P, s)."""
    s = SCALE * (q @ k.transpose(-1, -2)) + bias
    P = torch.softmax(s, -1)
    return P @ v, P, s


def attn_tol(q, k, v, bias_mag, P, s, o):
    """Bound of the one-wave-per-SIMD attention kernels (attention_win.hip, attention_glob.hip), per output element.
    Scores: the 80 exact f16 products of q.k and the rel-pos terms (in the MFMA as extra k-steps for the window
    kernel, as the accumulator init / exponent addend for the global one) go through <= 7 MFMA steps of <= 6 roundings:
    48 u mag_k (mag_k = scale |q| |k| + |rel terms|, logit units).  p = 2^(s c - m): an error common to a row cancels in
    the normalisation; c = f32(scale log2 e), the fma and v_exp add <= 4 u (|s_k| + |max s| + 9) (the deferred max m
    sits up to 12 log2-units below the row max) + 4 u.  So p_k is off by a relative delta_k, moving o by
    <= sum_k P_k delta_k |v_k - o|.  P is rounded to f16 before the PV MFMA and l = sum P comes from the same
    rounded P (ones-column of V): 2^-11 sum_k P_k |v_k - o|, and 2^-25 sum_k |v_k - o| for p in the f16 subnormal range
    (l >= 1: the row max has p >= 1).  PV and l accumulate n_k keys in f32 MFMA steps of 16 (<= 6 roundings each):
    (0.75 n_k + 16) u sum P |v|; o = O / l 3 u |o|; the f16 store 2^-11 |o| + 2^-25.
    |v_k - o| <= |v_k| + |o| throughout, so every term is a matrix product."""
    nk = k.shape[-2]
    mag = SCALE * (q.abs() @ k.abs().transpose(-1, -2)) + bias_mag
    smax = s.amax(-1, keepdim=True).abs()
    delta = 48 * U * mag + 4 * U * (s.abs() + smax + 9) + 4 * U
    Pd = P * delta + H16 * P
    va, oa = v.abs(), o.abs()
    A = P @ va
    return (Pd @ va + Pd.sum(-1, keepdim=True) * oa + SUB16 * (va.sum(-2, keepdim=True) + nk * oa)
            + (0.75 * nk + 16) * U * A + (3 * U + H16) * oa + SUB16)


def qkv_data(B, gen, dev, sigma=1.4):
    """Packed f16 qkv [B*4096, 3840] as the qkv GEMM writes it: q, k ~ N(0, sigma^2) (logit std sigma^2 ~ 2: peaked
    softmax), v ~ N(0, 1); every 16th token's q scaled by 1/40 (near-uniform rows)."""
    qkv = torch.randn(B * T, 3 * D, generator=gen, device=dev)
    qkv[:, :2 * D] *= sigma
    qkv[::16, :D] /= 40
    return qkv.half()


def rel_tables(S, gen, dev, std=0.1):
    return (std * torch.randn(2 * S - 1, HD, generator=gen, device=dev),
            std * torch.randn(2 * S - 1, HD, generator=gen, device=dev))


def win_item_ref(qkv, rel_aug, win_rows, pad_k, pad_v, windows, *, neighbour_key=False, zero_pad_k=False,
                 stale_kv=False, drop_key=False):
    """float64 window attention of `windows` (window indices into win_rows [nw, 196]) for all 16 heads, with rel_aug
    f16 [nw * 16, 196, 32] as the kernel reads it.  Returns (o, tol-or-None pieces) as [n, H, 196, 80] tensors plus the
    query-row mask [n, 196].  Mistakes: neighbour_key (key 0 of window w taken from window w + 1), zero_pad_k (padded
    keys get k = 0 instead of pad_k), stale_kv (K / V of the previous (window, head) item), drop_key (key 195 left out)."""
    rows = win_rows[windows].long()                                           # [n, 196]
    n = rows.shape[0]
    valid = rows >= 0
    kv_rows = win_rows[(windows + 1) % win_rows.shape[0]].long() if neighbour_key else None

    def gather(col0, pad, zero_pad=False, rr=rows):
        t = qkv[rr.clamp(min=0), col0:col0 + D].double()
        fill = torch.zeros(D, dtype=F64, device=qkv.device) if zero_pad else pad.double()
        t = torch.where((rr >= 0)[..., None], t, fill)
        return t.view(n, 196, HEADS, HD).permute(0, 2, 1, 3)                 # [n, H, 196, 80]

    q = gather(0, torch.zeros(D, device=qkv.device))
    k = gather(D, pad_k, zero_pad_k)
    v = gather(2 * D, pad_v)
    if neighbour_key:
        k2, v2 = gather(D, pad_k, rr=kv_rows), gather(2 * D, pad_v, rr=kv_rows)
        k[:, :, 0], v[:, :, 0] = k2[:, :, 0], v2[:, :, 0]
    if stale_kv:
        k = k.reshape(n * HEADS, 196, HD).roll(1, 0).view(n, HEADS, 196, HD)
        v = v.reshape(n * HEADS, 196, HD).roll(1, 0).view(n, HEADS, 196, HD)
    ra = rel_aug.view(-1, HEADS, 196, 32)[windows].double()                   # [n, H, 196, 32]
    ra = torch.where(valid[:, None, :, None], ra, torch.zeros((), dtype=F64, device=ra.device))   # padding queries: unwritten
    pos = torch.arange(196, device=qkv.device)
    rh = ra[..., :14][..., pos // 14]                                         # [n, H, 196(q), 196(k)]
    rw = ra[..., 14:28][..., pos % 14]
    bias = SCALE * (rh + rw)
    bmag = SCALE * (rh.abs() + rw.abs())
    if drop_key:
        bias[..., 195] = -math.inf
    o, P, s = attn_ref(q, k, v, bias)
    return q, k, v, bmag, P, s, o, valid


def glob_ref(q, k, v, rh, rw, *, drop_tile=None, last_tile_rows=False, swap=False):
    """float64 global attention of one (image, head): q, k, v [4096, 80] (f64), rh, rw [4096, 64] the kernel's rel
    tables (logit / scale units).  Mistakes: drop_tile (keys 64 t .. 64 t + 63 left out), last_tile_rows (queries
    3840-4095 use the rel rows of queries 3584-3839), swap (rel_h / rel_w exchanged)."""
    if last_tile_rows:
        rh, rw = rh.clone(), rw.clone()
        rh[3840:], rw[3840:] = rh[3584:3840], rw[3584:3840]
    if swap:
        rh, rw = rw, rh
    kk = torch.arange(T, device=q.device)
    rhe, rwe = rh[:, kk // G], rw[:, kk % G]
    bias = SCALE * (rhe + rwe)
    bmag = SCALE * (rhe.abs() + rwe.abs())
    if drop_tile is not None:
        bias[:, 64 * drop_tile:64 * drop_tile + 64] = -math.inf
    o, P, s = attn_ref(q, k, v, bias)
    return o, P, s, bmag

