"""float64 restatements, derived per-element bounds, a float32 host mimic and the shared case tables for the kernels that
turn a token row into a normalised row: ink_layernorm_rows, ink_add_cvt_f16, ink_add_split_f16, ink_add_f32
(inklayer_amd/csrc/norm.hip), ink_proj256_ln (proj_ln.hip) and ink_ffn256_fused (ffn_fused.hip).
tests/test_row_kernels_ref_cpu.py holds the reference and the bound to account without a GPU (torch's layer_norm, the
mimic's headroom, six named mistakes); tests/test_row_kernels_gpu.py runs the kernels.  CPU-only: nothing here touches
the library."""
import math

import torch

U = 2.0 ** -24
F64, F32, F16 = torch.float64, torch.float32, torch.float16
I32 = torch.int32


# ---------------------------------------------------------------------------------------------------------------
# split-f16 operand [ hi | lo * 64 | hi / 64 ]  (common.h split_f16)
# ---------------------------------------------------------------------------------------------------------------
def check_split(split, f32, what):
    """split f16 [rows, 3C] against f32 [rows, C] of the same launch."""
    C = f32.shape[1]
    hi, lo, hs = (split[:, i * C:(i + 1) * C] for i in range(3))
    assert torch.equal(hi, f32.to(F16)), what
    assert torch.equal(hs, (hi.float() / 64.0).to(F16)), what
    rec = hi.double() + lo.double() / 64.0
    err = (rec - f32.double()).abs()
    assert (err <= 2.0 ** -21 * f32.double().abs() + 2.0 ** -31).all(), (what, err.max().item())


def bits(t):
    """The tensor's bit patterns as integers (so that -0.0 != 0.0 and NaN == NaN)."""
    return t.contiguous().view({F16: torch.int16, F32: torch.int32}[t.dtype])


def split_ref(v):
    """f32 [R, C] -> the three segments as the kernel forms them: v - hi is exact in f32, so is the product with 64."""
    hi = v.to(F16)
    lo = ((v - hi.float()) * 64.0).to(F16)
    hs = (hi.float() * 0.015625).to(F16)
    return torch.cat([hi, lo, hs], 1)


def check_split_rule(split, f32, what):
    """check_split, and the middle segment bit for bit wherever (v - hi) * 64 is an f16 NORMAL number (below 2^-14 the
    rule leaves the treatment of subnormals open), and the outer two segments bit for bit including the sign of zero."""
    split, f32 = split.cpu(), f32.cpu()
    check_split(split, f32, what)
    C = f32.shape[1]
    want = split_ref(f32)
    assert torch.equal(bits(split[:, :C]), bits(want[:, :C])), what
    assert torch.equal(bits(split[:, 2 * C:]), bits(want[:, 2 * C:])), what
    normal = ((f32 - f32.to(F16).float()) * 64.0).abs() >= 2.0 ** -14
    assert torch.equal(bits(split[:, C:2 * C])[normal], bits(want[:, C:2 * C])[normal]), what


# ---------------------------------------------------------------------------------------------------------------
# ink_add_cvt_f16 / ink_add_split_f16 / ink_add_f32: exact
# ---------------------------------------------------------------------------------------------------------------
def _bcast(a, b):
    """b broadcast over a, periodic in the flat index (b[(r C + c) % numel(b)])."""
    assert a.numel() % b.numel() == 0
    return b.reshape(-1).repeat(a.numel() // b.numel()).view_as(a)


def add_f32_ref(a, b=None):
    """One f32 addition per element: torch's on the CPU is the same IEEE operation."""
    return a.clone() if b is None else a + _bcast(a, b)


def add_cvt_ref(a, b=None):
    return add_f32_ref(a, b).to(F16)


def add_split_ref(a, b=None):
    return split_ref(add_f32_ref(a, b))


# ---------------------------------------------------------------------------------------------------------------
# GELU as common.h gelu_erf computes it
# ---------------------------------------------------------------------------------------------------------------
_AS = (0.254829592, -0.284496736, 1.421413741, -1.453152027, 1.061405429)     # Abramowitz-Stegun 7.1.26
_AS_P = 0.3275911


def gelu_ref(y):
    return 0.5 * y * (1.0 + torch.erf(y / math.sqrt(2.0)))


def gelu_err(y):
    """Bound of |gelu_erf(y) - gelu(y)| for an exact f32 argument y (float64 tensor in, float64 bound out).

    gelu_erf(x) = max(x, 0) - (|x| / 2) e,  e = Q(t) 2^(-w),  Q(t) = a1 t + ... + a5 t^5,  t = 1 / (1 + p |x| / sqrt 2),
    w = x^2 log2(e) / 2.  The error of e is
      1.5e-7            the approximant's own (common.h, A-S 7.1.26)
      |Q'(t)| 6 u t     t: the constant and the product of `u` (2 u), the constant and the fma of 1 + c u (<= 2 u of a
                        sum that 1 dominates), and v_rcp_f32 at the instruction specification's 1 ulp (<= 2 u relative);
      6 u sum|a_k| t^k  Horner by four fma, the product with t and the coefficients' own f32 rounding;
      (2 + 2 + 2) u e   v_exp_f32 at the specification's 1 ulp (<= 2 u relative), its argument's three roundings
                        (w 2^-w ln 2 <= 1 / e of 5 u, under 2 u), and the two products that form e.
    Nobody has MEASURED v_rcp / v_exp on this part: the 1 ulp is the specification's figure.  The result is
    (|x| / 2) de plus one rounding of the final fma."""
    ax = y.abs()
    t = 1.0 / (1.0 + _AS_P * ax / math.sqrt(2.0))
    q = sum(a * t ** (k + 1) for k, a in enumerate(_AS))
    dq = sum((k + 1) * a * t ** k for k, a in enumerate(_AS)).abs()
    qa = sum(abs(a) * t ** (k + 1) for k, a in enumerate(_AS))
    e = q * torch.exp(-0.5 * y * y)
    de = 1.5e-7 + 1.01 * (dq * 6 * U * t + 6 * U * qa) + 6 * U * e.abs()
    return 0.5 * ax * de + U * (gelu_ref(y).abs() + 0.5 * ax * de)


# ---------------------------------------------------------------------------------------------------------------
# ink_layernorm_rows
# ---------------------------------------------------------------------------------------------------------------
N_SUM = 2 + 8 + 6                     # roundings on the way of one term into a row sum: group of four, <= 8 partials, butterfly


def layernorm_ref(x, gamma, beta, eps, add=None, act=None):
    """LayerNorm(x + add) [* gamma] [+ beta] [-> GELU] over the last dim of x [R, C] (add [R, C]: the addend ROW of every
    x row, already looked up) in float64, and a per-element bound of layernorm_rows_kernel's f32 arithmetic.

    The kernel (one wave per row, u = 2^-24):
      z     = fl(x + add): one rounding, e_i <= u |z_i|, only with `add`;
      mean  : the lane sums a group of four as (a + b) + (c + d) and adds it to its partial (<= 8 groups, sequential),
              six butterfly levels join the lanes, one division by C: a term passes <= 2 + 8 + 6 additions, so the
              mean is off by dm <= 17 u mean|z|;
      centred values z_i - mean_hat differ from the true ones by p_i = e_i - mean(e) - dm, |p_i| <= P_i;
      var   : a second pass over (z_i - mean_hat)^2: EXACTLY var + 2 mean((z - m) p) + mean(p^2) before its own
              roundings (19 u: the subtraction twice, the square, 16 additions), the division, eps as an f32 and its addition (3 u); the
              second-order term mean(p^2) is kept because at a row offset of 1000 and a spread of 0.05 it is not small
              against u.  With rho the relative change of var + eps, rstd moves by <= (1 - rho)^-1/2 - 1, plus the
              square root and the division (<= 1 ulp each: 4 u);
      y     = ((z - mean_hat) rstd) gamma + beta: four roundings, counted TWICE (8 u |gamma yhat| + 2 u |beta|).  The sums'
              worst cases are never attained, but a single rounding is: where the output is beta plus something small
              the whole error is the last addition's, up to u |y| itself, and the bound has to keep the factor of two
              of headroom that tests/test_row_kernels_ref_cpu.py asks of the f32 host mimic on every case.
    So |yhat_hat - yhat| <= |yhat| RR + P r (1 + RR), and never more than sqrt(C) + |yhat| (|d_i| / rms(d) <= sqrt C),
    which is what remains for a row whose var + eps is itself rounding noise (a constant row at a tiny eps).
    act = "gelu": the bound passes through |gelu'| <= 1.13 and gelu_err() of the kernel's approximant is added."""
    C = x.shape[1]
    z = x.to(F64) if add is None else x.to(F64) + add.to(F64)
    g = torch.ones(C, dtype=F64) if gamma is None else gamma.to(F64)
    b = torch.zeros(C, dtype=F64) if beta is None else beta.to(F64)
    mu = z.mean(-1, keepdim=True)
    zc = z - mu
    var = (zc ** 2).mean(-1, keepdim=True)
    r = 1.0 / torch.sqrt(var + eps)
    yhat = zc * r
    ref = yhat * g + b

    E = U * z.abs() if add is not None else torch.zeros_like(z)
    DM = (N_SUM + 1) * U * (z.abs() + E).mean(-1, keepdim=True) * (1 + 32 * U)
    P = E + E.mean(-1, keepdim=True) + DM
    DV = 2 * (zc.abs() * P).mean(-1, keepdim=True) + (P ** 2).mean(-1, keepdim=True)
    rho = (DV + (19 + 3) * U * (var + DV + eps)) / (var + eps)
    RR = torch.where(rho < 0.5, (1 - rho.clamp(max=0.5)) ** -0.5 - 1, torch.full_like(rho, float("inf"))) + 4 * U
    RR = RR * (1 + 8 * U)
    DH = yhat.abs() * RR + P * r * (1 + RR)
    DH = torch.where(torch.isfinite(DH), DH, torch.full_like(DH, float("inf")))
    DH = torch.minimum(DH, math.sqrt(C) * (1 + 64 * U) + yhat.abs())
    tol = g.abs() * (DH * (1 + 8 * U) + 8 * U * yhat.abs()) + 2 * U * b.abs() + 1e-30
    if act == "gelu":
        # the kernel's argument lies within tol of ref: the approximant's bound at the worse end of that interval
        tol = 1.13 * tol + torch.maximum(gelu_err(ref), torch.maximum(gelu_err(ref - tol), gelu_err(ref + tol)))
        ref = gelu_ref(ref)
    else:
        assert act is None
    return ref, tol


def _xor_sum(s):
    """wave_sum: v += v[lane ^ o] for o = 32, 16, ... 1 on s [R, 64] f32; every lane ends with the same bits."""
    lane = torch.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        s = s + s[:, lane ^ o]
    return s[:, :1]


MISTAKES = ("one_pass_variance", "last_group_dropped", "padded_width", "add_omitted", "add_row_not_looked_up",
            "eps_outside_sqrt")


def layernorm_mimic(x, gamma, beta, eps, add=None, mistake=None, add_plain=None):
    """layernorm_rows_kernel's arithmetic in float32 on the host, in the kernel's order (torch's CPU f32 operations are
    the same IEEE operations; the build has -ffp-contract=off).  x, add as layernorm_ref.  `mistake` is one of MISTAKES:
    the wrong kernels the bound must tell from the right one; add_plain is the addend a kernel would read that took
    add[r] for row r instead of looking the row up ("add_row_not_looked_up")."""
    assert mistake is None or mistake in MISTAKES
    R, C = x.shape
    nv = C // 4
    NV = -(-nv // 64)
    if mistake == "add_omitted":
        add = None
    if mistake == "add_row_not_looked_up":
        add = add_plain
    z = x.to(F32) if add is None else x.to(F32) + add.to(F32)
    pad = torch.zeros(R, NV * 256, dtype=F32)
    pad[:, :C] = z
    r = pad.view(R, NV, 64, 4)                                   # vector v = lane + 64 j holds columns 4 v .. 4 v + 3
    live = (torch.arange(NV)[:, None] * 64 + torch.arange(64)[None, :]) < nv        # [NV, 64]
    if mistake == "last_group_dropped" and nv % 64:
        live = live & (torch.arange(NV)[:, None] < NV - 1)
        r = r * live[None, :, :, None]
    n = float(NV * 256) if mistake == "padded_width" else float(C)
    s = torch.zeros(R, 64, dtype=F32)
    for j in range(NV):
        s = s + ((r[:, j, :, 0] + r[:, j, :, 1]) + (r[:, j, :, 2] + r[:, j, :, 3]))
    mean = _xor_sum(s) / torch.tensor(n, dtype=F32)              # [R, 1]
    q = torch.zeros(R, 64, dtype=F32)
    if mistake == "one_pass_variance":
        for j in range(NV):
            t = r[:, j]
            q = q + ((t[..., 0] * t[..., 0] + t[..., 1] * t[..., 1]) + (t[..., 2] * t[..., 2] + t[..., 3] * t[..., 3]))
        var = _xor_sum(q) / torch.tensor(n, dtype=F32) - mean * mean
    else:
        for j in range(NV):
            d = (r[:, j] - mean[:, :, None]) * live[j][None, :, None]
            q = q + ((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + (d[..., 2] * d[..., 2] + d[..., 3] * d[..., 3]))
        var = _xor_sum(q) / torch.tensor(n, dtype=F32)
    e = torch.tensor(eps, dtype=F32)
    if mistake == "eps_outside_sqrt":
        rstd = 1.0 / (torch.sqrt(var) + e)
    else:
        rstd = 1.0 / torch.sqrt(var + e)
    y = (pad[:, :C] - mean) * rstd
    if gamma is not None:
        y = y * gamma.to(F32)
    if beta is not None:
        y = y + beta.to(F32)
    return y


# ---------------------------------------------------------------------------------------------------------------
# case tables of ops.layernorm_rows, shared by the CPU and the GPU tests
# ---------------------------------------------------------------------------------------------------------------
WIDTHS = (4, 252, 256, 260, 512, 516, 1024, 1028, 1280, 1284, 1540, 2044, 2048)      # NV = 1 1 1 2 2 3 4 5 5 6(8) 7(8) 8 8
ROW_COUNTS = (1, 3, 4, 5)
MODE_WIDTHS = (260, 1284)
EPS_LIST = (1e-12, 1e-5, 1e-6)
MAGNITUDES = ((0.5, 3.0), (100.0, 1.0), (1000.0, 0.05), (0.0, 1e-3))                   # (offset, std)
HEADROOM_WIDTHS = (4, 252, 260, 1284, 2048)


class LnCase:
    """One ops.layernorm_rows launch: x [Rin, C]; gather (list, -1 = zero row) or None; add [Ra, ld >= C] with its
    column block add[:, add_col:add_col + C], add_rows (list, one per batch entry of rows_per_batch rows) or None."""

    def __init__(self, name, x, gamma, beta, eps, *, act=None, gather=None, add=None, add_col=0, add_rows=None,
                 rows_per_batch=0):
        self.name, self.x, self.gamma, self.beta, self.eps, self.act = name, x, gamma, beta, eps, act
        self.gather, self.add, self.add_col, self.add_rows, self.rows_per_batch = gather, add, add_col, add_rows, rows_per_batch
        self.C = x.shape[1]
        self.rows = len(gather) if gather is not None else x.shape[0]

    def add_block(self):
        return None if self.add is None else self.add[:, self.add_col:self.add_col + self.C]

    def inputs(self):
        """-> (x rows [rows, C], addend rows or None, the addend rows of the add[r] misreading or None, bool [rows]: a
        gathered -1 row)."""
        if self.gather is not None:
            idx = torch.tensor(self.gather)
            return self.x[idx.clamp(min=0)], None, None, idx < 0
        none = torch.zeros(self.rows, dtype=torch.bool)
        if self.add is None:
            return self.x, None, None, none
        blk = self.add_block()
        if self.add_rows is None:
            return self.x, blk[:self.rows], blk[:self.rows], none
        idx = torch.cat([torch.arange(r0, r0 + self.rows_per_batch) for r0 in self.add_rows])
        return self.x, blk[idx], blk[:self.rows], none

    def reference(self):
        """-> (float64 [rows, C], bound); a gathered -1 row is zeros with bound 0."""
        if not hasattr(self, "_ref"):
            x, add, _, dead = self.inputs()
            ref, tol = layernorm_ref(x, self.gamma, self.beta, self.eps, add=add, act=self.act)
            ref[dead], tol[dead] = 0.0, 0.0
            self._ref = (ref, tol)
        return self._ref


def _rows(g, R, C, offset, std):
    return torch.randn(R, C, generator=g) * std + offset


def _affine(g, C):
    return 1 + 0.3 * torch.randn(C, generator=g), 0.5 * torch.randn(C, generator=g)


def numerics_rows(g, C=256):
    """Nine rows: two each at offset 1000 / std 0.05, offset 100 / std 1, scale 1e4, scale 1e-4, and a constant row."""
    x = torch.cat([_rows(g, 2, C, 1000.0, 0.05), _rows(g, 2, C, 100.0, 1.0), _rows(g, 2, C, 0.0, 1e4),
                   _rows(g, 2, C, 0.0, 1e-4), torch.full((1, C), 0.3)])
    return x


CONSTANT_ROW = 8                        # of numerics_rows


def _build_cases():
    cases = []
    for C in WIDTHS:
        g = torch.Generator().manual_seed(1000 + C)
        cases.append(LnCase(f"width-{C}", _rows(g, 9, C, 0.5, 3.0), *_affine(g, C), 1e-6))
    for R in ROW_COUNTS:
        g = torch.Generator().manual_seed(2000 + R)
        cases.append(LnCase(f"rows-{R}", _rows(g, R, 260, 0.5, 3.0), *_affine(g, 260), 1e-6))
    for C in MODE_WIDTHS:
        g = torch.Generator().manual_seed(3000 + C)
        x = _rows(g, 9, C, 0.5, 3.0)
        gamma, beta = _affine(g, C)
        cases.append(LnCase(f"no-gamma-{C}", x, None, beta, 1e-6))
        cases.append(LnCase(f"no-beta-{C}", x, gamma, None, 1e-6))
        cases.append(LnCase(f"no-affine-{C}", x, None, None, 1e-6))
        cases.append(LnCase(f"gelu-{C}", _rows(g, 9, C, 0.1, 1.0), gamma, beta, 1e-6, act="gelu"))
        # six input rows, fourteen output rows: -1 first, last and inside, repeats, every input row used
        cases.append(LnCase(f"gather-{C}", x[:6].clone(), gamma, beta, 1e-6,
                            gather=[-1, 5, 0, 0, 3, -1, 2, 5, 1, 4, 4, -1, 0, -1]))
        cases.append(LnCase(f"gather-gelu-{C}", x[:6].clone(), gamma, beta, 1e-6, act="gelu", gather=[2, -1, 2, 5, 0, -1, 1]))
        cases.append(LnCase(f"add-{C}", x, gamma, beta, 1e-6, add=_rows(g, 9, C, -0.3, 2.0)))
        # three batch entries of three rows; the addend rows of entry b start at add_rows[b] of a tensor of two images
        # of five rows each, read out of order, as the column block [8, 8 + C) of a wider tensor
        wide = _rows(g, 10, C + 24, -0.3, 2.0)
        cases.append(LnCase(f"add-table-{C}", x, gamma, beta, 1e-6, add=wide, add_col=8, add_rows=[7, 0, 2], rows_per_batch=3))
    for eps in EPS_LIST:
        g = torch.Generator().manual_seed(4000)
        cases.append(LnCase(f"numerics-eps{eps:g}", numerics_rows(g), *_affine(g, 256), eps))
        cases.append(LnCase(f"numerics-add-eps{eps:g}", numerics_rows(g) * 0.5, *_affine(g, 256), eps,
                            add=numerics_rows(g) * 0.5))
    return cases


CASES = _build_cases()
CASE = {c.name: c for c in CASES}


def headroom_grid():
    """The grid the bound's headroom was first checked on: five widths x four magnitudes, with and without `add`."""
    for C in HEADROOM_WIDTHS:
        for k, (offset, std) in enumerate(MAGNITUDES):
            for with_add in (False, True):
                g = torch.Generator().manual_seed(5000 + 10 * C + k)
                x = _rows(g, 9, C, offset, std)
                gamma, beta = _affine(g, C)
                add = _rows(g, 9, C, 0.5 * offset, std) if with_add else None
                yield LnCase(f"grid-{C}-{offset:g}-{std:g}-{'add' if with_add else 'plain'}", x, gamma, beta, 1e-6, add=add)


# ---------------------------------------------------------------------------------------------------------------
# ink_proj256_ln and ink_ffn256_fused: the data of the existing op tests at any size, and their float64 references
# ---------------------------------------------------------------------------------------------------------------
def proj_ln_data(R=600, seed=7):
    """a [R, 128], w [256, 128], bias, residual [R, 256], gamma, beta: tests/test_sam_gpu.py's, shared = False."""
    gen = torch.Generator().manual_seed(seed)
    a = torch.randn(R, 128, generator=gen) * 0.8
    w = torch.randn(256, 128, generator=gen) / 11
    b = torch.randn(256, generator=gen) * 0.2
    lg, lb = 1 + 0.1 * torch.randn(256, generator=gen), 0.1 * torch.randn(256, generator=gen)
    res = torch.randn(R, 256, generator=gen)
    return a, w, b, res, lg, lb


def proj_ln_ref(a, w, b, res, lg, lb, eps):
    return torch.nn.functional.layer_norm(res.double() + a.double() @ w.double().t() + b.double(), (256,), lg.double(),
                                          lb.double(), eps)


def ffn_data(M, hid, pre=False):
    """tests/test_ops_gpu.py's generators (test_fused_ffn_equals_the_two_projection_form, ..._with_the_preceding_projection)."""
    if not pre:
        g = torch.Generator().manual_seed(M + hid)
        x32 = torch.randn(M, 256, generator=g) * 1.5 + 0.3
        w1 = (torch.randn(hid, 256, generator=g) / 16).half()
        w2 = (torch.randn(256, hid, generator=g) / 45).half()
        b1, b2 = torch.randn(hid, generator=g) * 0.2, torch.randn(256, generator=g) * 0.2
        lg, lb = 1 + 0.1 * torch.randn(256, generator=g), 0.1 * torch.randn(256, generator=g)
        return dict(x16=x32.half(), res=x32, w1=w1, b1=b1, w2=w2, b2=b2, lg=lg, lb=lb)
    g = torch.Generator().manual_seed(M)
    x16 = (torch.randn(M, 256, generator=g) * 0.8).half()
    res = torch.randn(M, 256, generator=g) * 1.5 + 0.3
    wp = (torch.randn(256, 256, generator=g) / 16).half()
    w1 = (torch.randn(hid, 256, generator=g) / 16).half()
    w2 = (torch.randn(256, hid, generator=g) / 45).half()
    bp, b1, b2 = torch.randn(256, generator=g) * 0.2, torch.randn(hid, generator=g) * 0.2, torch.randn(256, generator=g) * 0.2
    g1, e1 = 1 + 0.1 * torch.randn(256, generator=g), 0.1 * torch.randn(256, generator=g)
    lg, lb = 1 + 0.1 * torch.randn(256, generator=g), 0.1 * torch.randn(256, generator=g)
    return dict(x16=x16, res=res, wp=wp, bp=bp, g1=g1, e1=e1, w1=w1, b1=b1, w2=w2, b2=b2, lg=lg, lb=lb)


def ffn_ref(d, eps=1e-5):
    """float64 with the kernel's rounding points: f16 operand, f16 hidden activations (and, with the preceding
    projection, the f16 rounding of its normalised output as the operand)."""
    ln = torch.nn.functional.layer_norm
    if "wp" in d:
        s = ln(d["res"].double() + d["x16"].double() @ d["wp"].double().T + d["bp"].double(), (256,), d["g1"].double(),
               d["e1"].double(), eps)
        op = s.float().half()
    else:
        s, op = d["res"].double(), d["x16"]
    h = torch.relu(op.double() @ d["w1"].double().T + d["b1"].double()).float().half()
    return ln(s + h.double() @ d["w2"].double().T + d["b2"].double(), (256,), d["lg"].double(), d["lb"].double(), eps)
