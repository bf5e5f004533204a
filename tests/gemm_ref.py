"""float64 statement, per-element bound, case tables, named mistakes and branch predicates of ink_gemm_f16
(csrc/gemm.hip) at the edges of its four tile families and of every epilogue branch.  Shared by
tests/test_gemm_edges_gpu.py (the kernels) and tests/test_gemm_edges_ref_cpu.py (that the statement, the bound, the guards
and the case tables do what they claim, on the CPU).

The statement:  out[row_map[m], n] = residual[row_map[m], n] + col_scale[n] * act(sum_k a[m, k] w[n, k] + bias[n]),
rows with row_map[m] = -1 dropped, every other element of the output buffer left as it was.

Families (how ink_gemm_f16 picks the kernel once ink_gemm_set_variant forces a variant; family_run states the rule):
  F0   gemm_f16_nt<128,128,64,2,2>   row-major tile order          variant 0,  K % 64 == 0
  F32  gemm_f16_nt<128,128,32,2,2>   row-major tile order          K % 64 == 32 (launched before the variant is read)
  F10  gemm_f16_nt<256,256,64,4,4>   groups of 4 M-tiles           variant 10, K % 64 == 0
  F45  gemm_f16_nt_pp 256x320        groups of 4 M-tiles, K ring   variant 45, K % 64 == 0, K >= 128

Two kinds of data.  'exact': a, w integers in [-3, 3], bias integers in [-8, 8], residual integers in [-64, 64],
col_scale in {-2, -1, -0.5, 0.5, 1, 2}, activation none / ReLU: the f16 products are exact, every partial sum is an
integer below 2^24, the bias / residual adds and the col_scale product are exact in f32, so the kernel must reproduce
the float64 statement bit for bit in any summation order (exact_preconditions asserts what that needs).  'bounded': a ~
N(0, 1), w ~ N(0, 1 / K), b ~ 0.1 N, r ~ N(0, 1), cs ~ 0.5 + 0.1 N (the data of depth_ops_ref.gemm_data), compared per
element with gemm_tol.  The operands are drawn on the CPU from a seed that depends on (M, N, K, kind) alone, so the
CPU tests check the very numbers the GPU tests multiply.

Buffers (buffers()): the output is the view [:rows, :N] of a NaN-filled [rows + 64, ldc] buffer; a and w are views into
NaN-filled buffers with 8 more rows and, for the padded forms, lda = K + 8, ldw = K + 24; a separate residual is a
view into a NaN-filled buffer whose rows the row map does not target stay NaN.  An in-place residual is the output
view itself; there the rows a scattering row map does not target hold finite residual values (a read-modify-write of
such a row would go unseen on NaN), and must come back bit-unchanged."""
import math
from collections import namedtuple
from functools import lru_cache
from types import SimpleNamespace

import torch

from vith_ref import F16, F32, F64, GELU_ERF, H16, SUB16, U, assert_discriminates, assert_within, discrimination  # noqa: F401

NAN = float("nan")
GUARD_ROWS = 64
SCATTER_EXTRA = 37

Family = namedtuple("Family", "name variant BM BN BK WNC group_m")
FAMILIES = {
    "F0": Family("F0", 0, 128, 128, 64, 64, 1),
    "F32": Family("F32", 0, 128, 128, 32, 64, 1),      # the variant is ignored: any value runs this kernel
    "F10": Family("F10", 10, 256, 256, 64, 64, 4),
    "F45": Family("F45", 45, 256, 320, 32, 80, 4),
}
FAMS = tuple(FAMILIES)
SAME_BITS_FAMS = ("F0", "F10", "F45")                  # the three a K % 64 == 0 problem can be forced onto
PP_RING = 4                                            # granules in the ping-pong kernel's LDS ring


def family_run(variant, K):
    """The family ink_gemm_f16 launches for a forced variant: K % 64 != 0 goes to the 128x128x32 kernel before the
    variant is looked at; variant 45 needs K / 32 >= PP_RING (launch_gemm_pp returns an argument error otherwise)."""
    assert K > 0 and K % 32 == 0 and variant in (0, 10, 45)
    if K % 64:
        return "F32"
    if variant == 45:
        assert K // 32 >= PP_RING, "launch_gemm_pp rejects K < 128"
        return "F45"
    return {0: "F0", 10: "F10"}[variant]


# ---------------------------------------------------------------------------------------------------------------
# epilogue forms
# ---------------------------------------------------------------------------------------------------------------
# res: None / "sep" (a buffer of its own, ldr = N + ldr_pad) / "inplace" (out is residual); row_map: None / "perm" /
# "drop" (a permutation with ~10 % of the rows -1, the source of row 0 and the last row among them) / "scatter" (into a
# buffer of M + 37 rows); pad: lda = K + 8, ldw = K + 24
Form = namedtuple("Form", "bias act cs res ldr_pad row_map f16 pad", defaults=(True, None, False, None, 0, None, False, False))
FORMS = {
    "a": Form(bias=False),
    "b": Form(f16=True),
    "c": Form(act="relu", f16=True),
    "d": Form(act="relu"),
    "e": Form(res="sep", ldr_pad=8),
    "f": Form(res="inplace"),
    "g": Form(res="sep", f16=True),
    "h": Form(cs=True, res="inplace"),
    "i": Form(act="relu", res="sep", f16=True),
    "j": Form(cs=True, f16=True),
    "k": Form(res="inplace", row_map="perm"),
    "l": Form(res="sep", ldr_pad=8, row_map="drop"),
    "m": Form(cs=True, res="inplace", row_map="scatter"),
    "n": Form(f16=True, pad=True),
    "o": Form(res="sep", ldr_pad=8, row_map="drop", f16=True),
    "bias_f32": Form(),
    "gelu_f16": Form(act="gelu", f16=True),
    "gelu_f32": Form(act="gelu"),
    "gelu_res_f16": Form(act="gelu", res="sep", f16=True),
    "gelu_cs_f32": Form(act="gelu", cs=True),
}
EPILOGUE_FORMS = tuple("abcdefghijklmno")
BOUNDED_FORMS = ("b", "c", "e", "g", "h", "i", "l", "o", "gelu_f16", "gelu_f32", "gelu_res_f16", "gelu_cs_f32")
GELU_FORMS = tuple(f for f in BOUNDED_FORMS if FORMS[f].act == "gelu")


def residual_preloaded(f):
    """residual_preloaded() of gemm.hip: the residual goes into the accumulators before the K loop."""
    return f.res is not None and f.act is None and not f.cs


def res_late(f):
    return f.res is not None and not residual_preloaded(f)


def pp_store_form(f):
    """Which of the five store_wave_tile instantiations of gemm_f16_nt_pp the form takes."""
    plain = not f.cs and not res_late(f)
    if f.f16:
        return "pp_f16_gelu" if plain and f.act == "gelu" else "pp_f16_none" if plain and f.act is None else "pp_f16_runtime"
    return "pp_f32_none" if plain and f.act is None else "pp_f32_runtime"


# ---------------------------------------------------------------------------------------------------------------
# case tables
# ---------------------------------------------------------------------------------------------------------------
Case = namedtuple("Case", "test fam M N K form ldc_pad data")

WALK_TILES = ((1, 1), (2, 1), (3, 1), (1, 3), (4, 2), (5, 1), (5, 2), (9, 1), (7, 3))
K_LOOP = {"F0": (64, 128, 192, 320), "F10": (64, 128, 192, 320), "F32": (32, 96, 160, 288),
          "F45": (128, 192, 256, 320, 448)}
EDGE_K = {"F0": 64, "F10": 64, "F32": 96, "F45": 128}
M_EDGES = (1, 2, 15, 16, 17, 31, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257)
M_EDGE_N = (72, 76)
N_EDGES = (4, 8, 12, 16, 20, 60, 64, 68, 76, 80, 84, 124, 128, 132, 156, 160, 164, 236, 240, 244, 252, 256, 260, 316,
           320, 324)
N_EDGE_LDC = (0, 4, 64)
EPI_M, EPI_N = 300, 332
EPI_K = {"F0": 192, "F10": 192, "F32": 160, "F45": 192}
BOUNDED_K = {"F0": (128, 1024), "F10": (128, 1024), "F32": (160, 1056), "F45": (128, 1024)}


def tile_walk_cases(fam):
    """K = 128; the 128x128x32 family only ever sees K % 64 == 32 and walks its tiles at K = 96."""
    f = FAMILIES[fam]
    return [Case("walk", fam, ntm * f.BM - 5, ntn * f.BN - 12, 128 if fam != "F32" else 96, "a", 0, "exact")
            for ntm, ntn in WALK_TILES]


def k_loop_cases(fam):
    f = FAMILIES[fam]
    return [Case("kloop", fam, 2 * f.BM - 5, 2 * f.BN - 12, K, form, 0, "exact") for K in K_LOOP[fam] for form in ("bias_f32", "e")]


def m_edge_cases(fam):
    return [Case("medge", fam, M, N, EDGE_K[fam], form, 0, "exact") for M in M_EDGES for N in M_EDGE_N for form in ("d", "c")]


def n_edge_cases(fam):
    return [Case("nedge", fam, 40, N, EDGE_K[fam], form, pad, "exact") for N in N_EDGES for pad in N_EDGE_LDC
            for form in ("bias_f32", "b")]


def epilogue_cases(fam, data="exact", K=None):
    return [Case("epilogue", fam, EPI_M, EPI_N, K or EPI_K[fam], form, 0, data) for form in EPILOGUE_FORMS]


def bounded_cases(fam):
    return [Case("bounded", fam, EPI_M, EPI_N, K, form, 0, "bounded") for K in BOUNDED_K[fam] for form in BOUNDED_FORMS]


def same_bits_cases(fam):
    """Test 7: the forms of test 5 and (reported, not asserted) the GELU forms, K = 192, both kinds of data."""
    return ([c._replace(test="samebits") for data in ("exact", "bounded") for c in epilogue_cases(fam, data, 192)]
            + [Case("samebits", fam, EPI_M, EPI_N, 192, form, 0, "bounded") for form in GELU_FORMS])


def gpu_cases():
    """Every case tests/test_gemm_edges_gpu.py launches."""
    out = []
    for fam in FAMS:
        out += tile_walk_cases(fam) + k_loop_cases(fam) + m_edge_cases(fam) + n_edge_cases(fam) + epilogue_cases(fam)
        out += bounded_cases(fam)
        if fam in SAME_BITS_FAMS:
            out += same_bits_cases(fam)
    return out


# ---------------------------------------------------------------------------------------------------------------
# branch predicates (pure Python: what a case reaches, read off gemm.hip)
# ---------------------------------------------------------------------------------------------------------------
def geometry(c):
    f = FAMILIES[c.fam]
    ntm, ntn = -(-c.M // f.BM), -(-c.N // f.BN)
    return SimpleNamespace(ntm=ntm, ntn=ntn, wgs=ntm * ntn, steps=c.K // f.BK)


def branches(c):
    """The set of branch names a case takes."""
    fam, f, g = FAMILIES[c.fam], FORMS[c.form], geometry(c)
    assert family_run(fam.variant, c.K) == c.fam
    b = {"ragged_m" if c.M % fam.BM else "full_m", "ragged_n" if c.N % fam.BN else "full_n",
         f"ntm%4={g.ntm % 4}", f"ntn={min(g.ntn, 3)}{'+' if g.ntn > 3 else ''}",
         "wgs<8" if g.wgs < 8 else "wgs=8" if g.wgs == 8 else "wgs%8=0" if g.wgs % 8 == 0 else "wgs>8,%8!=0",
         "f16" if f.f16 else "f32", f"act={f.act or 'none'}", "bias" if f.bias else "no_bias",
         f"row_map={f.row_map or 'none'}", f"data={c.data}"}
    if c.M < 16:
        b.add("m<16")
    if c.fam == "F45":
        b.add(f"granules={g.steps}")
        b.add(pp_store_form(f))
        b.add("pp_prologue_drain" if residual_preloaded(f) else "pp_prologue_counted")
        if g.steps > PP_RING:
            b.add("ring_wrap")
    else:
        b.add("ksteps=1" if g.steps == 1 else "ksteps=2" if g.steps == 2 else "ksteps>2")
        b.add("ksteps_odd" if g.steps % 2 else "ksteps_even")
    if f.res:
        b.add("residual_preloaded" if residual_preloaded(f) else "res_late")
        b.add(f"res_{f.res}")
        if f.res == "sep" and f.ldr_pad + c.N != c.N + c.ldc_pad:
            b.add("ldr!=ldc")
    if f.cs:
        b.add("scaled")
    if c.ldc_pad:
        b.add("ldc>N")
    if f.pad:
        b.add("lda>K,ldw>K")
    if f.f16:
        b.add("wide16" if (c.N + c.ldc_pad) % 8 == 0 else "narrow8")
        if c.N % 8 == 4:
            b.add("half_chunk")
        if res_late(f):
            b.add("f16_double_rounding")
    # a wave tile column (16 wide) cut by N, and wave tiles wholly outside N
    if c.N % 16:
        b.add("n_cuts_mfma_tile")
    if c.N % fam.BN and c.N % fam.BN <= fam.BN - fam.WNC:
        b.add("idle_wave_columns")
    return b


# ---------------------------------------------------------------------------------------------------------------
# data and buffers
# ---------------------------------------------------------------------------------------------------------------
@lru_cache(maxsize=16)
def operands(M, N, K, data):
    """CPU operands of one problem: a f16 [M, K], w f16 [N, K], b f32 [N], cs f32 [N], r f32 [M + 37, N]."""
    g = torch.Generator().manual_seed(1_000_003 * M + 1009 * N + K + (7 if data == "exact" else 0))
    R = M + SCATTER_EXTRA
    if data == "exact":
        ri = lambda lo, hi, *shape: torch.randint(lo, hi + 1, shape, generator=g)   # noqa: E731
        a, w = ri(-3, 3, M, K).to(F16), ri(-3, 3, N, K).to(F16)
        b, r = ri(-8, 8, N).to(F32), ri(-64, 64, R, N).to(F32)
        cs = torch.tensor([-2, -1, -0.5, 0.5, 1, 2], dtype=F32)[ri(0, 5, N)]
    else:
        rn = lambda *shape: torch.randn(*shape, generator=g)   # noqa: E731
        a, w = rn(M, K).to(F16), (rn(N, K) / math.sqrt(K)).to(F16)
        b, r, cs = 0.1 * rn(N), rn(R, N), 0.5 + 0.1 * rn(N)
    return SimpleNamespace(a=a, w=w, b=b, cs=cs, r=r)


def row_map_of(c):
    """(row map as int64 [M] or None, rows of the output view)."""
    kind, M = FORMS[c.form].row_map, c.M
    if kind is None:
        return None, M
    g = torch.Generator().manual_seed(M + 3)
    if kind == "scatter":
        return torch.randperm(M + SCATTER_EXTRA, generator=g)[:M].clone(), M + SCATTER_EXTRA
    rm = torch.randperm(M, generator=g)
    if kind == "drop":
        drop = torch.rand(M, generator=g) < 0.1
        drop[M - 1] = True
        drop |= rm == 0                    # the source of output row 0: row 0 is not targeted
        rm[drop] = -1
    return rm, M


def _nan_view(t, rows_extra, ld, dev):
    buf = torch.full((t.shape[0] + rows_extra, ld), NAN, dtype=t.dtype, device=dev)
    buf[:t.shape[0], :t.shape[1]] = t.to(dev)
    return buf[:t.shape[0], :t.shape[1]]


def buffers(c, dev="cpu"):
    """Everything one launch needs, on dev, and what the reference needs of it (see the module docstring)."""
    f, o = FORMS[c.form], operands(c.M, c.N, c.K, c.data)
    M, N, K = c.M, c.N, c.K
    rm, rows = row_map_of(c)
    dest = (rm if rm is not None else torch.arange(M)).to(dev)
    B = SimpleNamespace(case=c, rows=rows, dest=dest, row_map=None if rm is None else rm.to(dev, torch.int32))
    B.a = _nan_view(o.a, 8, K + (8 if f.pad else 0), dev)
    B.w = _nan_view(o.w, 8, K + (24 if f.pad else 0), dev)
    B.bias = o.b.to(dev) if f.bias else None
    B.cs = o.cs.to(dev) if f.cs else None
    B.outbuf = torch.full((rows + GUARD_ROWS, N + c.ldc_pad), NAN, dtype=F16 if f.f16 else F32, device=dev)
    B.out = B.outbuf[:rows, :N]
    r = o.r[:rows].to(dev)
    B.residual = None
    if f.res == "inplace":
        assert not f.f16
        B.out.copy_(r)
        B.residual = B.out
    elif f.res == "sep":
        resbuf = torch.full((rows + 8, N + f.ldr_pad), NAN, dtype=F32, device=dev)
        t = dest[dest >= 0]
        resbuf[t, :N] = r[t]
        B.residual = resbuf[:rows, :N]
    B.init = B.outbuf.clone()
    B.res64 = None if f.res is None else B.residual.double().clone()
    a64, w64 = B.a.double(), B.w.double()
    B.prod, B.absprod = a64 @ w64.t(), a64.abs() @ w64.abs().t()
    return B


# ---------------------------------------------------------------------------------------------------------------
# the float64 statement, with the named mistakes
# ---------------------------------------------------------------------------------------------------------------
MISTAKES = ("last K step skipped", "first K step skipped", "tile exchanged with its grouped-order neighbour",
            "bias dropped", "bias shifted by one 4-column chunk", "relu dropped", "col_scale dropped",
            "col_scale applied to residual + product", "residual dropped", "residual added twice",
            "residual row m instead of row_map[m]", "output row not mapped", "dropped rows written to row 0",
            "last 4 columns missing when N % 8 == 4", "f32 stream rounded to f16")
# the mistakes that (also) write outside the targeted region: the guard / unchanged-row check has to see them
GUARD_MISTAKES = {"dropped rows written to row 0": ("drop",), "output row not mapped": ("drop", "scatter")}


def applicable(c):
    """(mistake, factor by which it has to leave the bound) for the case."""
    fam, f, g = FAMILIES[c.fam], FORMS[c.form], geometry(c)
    out = [("last K step skipped", 100), ("first K step skipped", 100)]
    if (g.ntm if fam.group_m > 1 else g.ntn) >= 2:
        out.append(("tile exchanged with its grouped-order neighbour", 100))
    if f.bias:
        out.append(("bias dropped", 100))
        if c.N >= 8:
            out.append(("bias shifted by one 4-column chunk", 100))
    if f.act == "relu":
        out.append(("relu dropped", 100))
    if f.cs:
        out.append(("col_scale dropped", 100))
    if f.cs and f.res:
        out.append(("col_scale applied to residual + product", 100))
    if f.res:
        out += [("residual dropped", 100), ("residual added twice", 100)]
        if f.row_map:
            out.append(("residual row m instead of row_map[m]", 100))
        if not f.f16 and c.data == "bounded":
            # half an f16 ulp is 2^13 / (K / 32 + 7) times the accumulation term on a residual-dominated element; on
            # exact data the small integers are f16 numbers and the mistake changes nothing
            out.append(("f32 stream rounded to f16", 2))
    if f.row_map:
        out.append(("output row not mapped", 100))
    if f.row_map == "drop":
        out.append(("dropped rows written to row 0", 100))
    if f.f16 and c.N % 8 == 4:
        out.append(("last 4 columns missing when N % 8 == 4", 100))
    return out


Ref = namedtuple("Ref", "out dest cols lin y v mag")


def reference(B, mistake=None):
    """float64 values out [M, N] of the statement, the output row dest [M] of each (-1: dropped) and the number of
    columns written; lin, y = act(lin), v = cs * y and mag = sum_k |a_k w_k| + |b| (+ |r| where the residual is
    preloaded) for the bound.  mistake: one of MISTAKES, each a change of one index or one rule."""
    c = B.case
    fam, f = FAMILIES[c.fam], FORMS[c.form]
    M, N, K = c.M, c.N, c.K
    assert mistake is None or mistake in MISTAKES
    a64, w64 = B.a.double(), B.w.double()
    prod = B.prod
    if mistake in ("last K step skipped", "first K step skipped"):
        k0 = K - fam.BK if mistake.startswith("last") else 0
        prod = prod - a64[:, k0:k0 + fam.BK] @ w64[:, k0:k0 + fam.BK].t()
    mag = B.absprod
    lin = prod
    if f.bias:
        b = B.bias.double()
        mag = mag + b.abs()
        if mistake == "bias shifted by one 4-column chunk":
            b = b.roll(4)
        if mistake != "bias dropped":
            lin = lin + b
    if f.act == "gelu":
        y = torch.nn.functional.gelu(lin)
    elif f.act == "relu" and mistake != "relu dropped":
        y = lin.clamp(min=0)
    else:
        y = lin
    dest = B.dest
    valid = dest >= 0
    v = y * B.cs.double() if f.cs and mistake != "col_scale dropped" else y
    out = v
    if f.res:
        ridx = torch.arange(M, device=dest.device) if mistake == "residual row m instead of row_map[m]" else dest
        r = B.res64[ridx.clamp(min=0)]
        if mistake == "dropped rows written to row 0":
            r = torch.where(valid[:, None], r, torch.zeros((), dtype=F64, device=r.device))   # acc = 0 for r = -1
        times = {"residual dropped": 0, "residual added twice": 2}.get(mistake, 1)
        if mistake == "col_scale applied to residual + product":
            out = B.cs.double() * (r + y)
        elif times:
            out = v + times * r
        if residual_preloaded(f):
            mag = mag + r.abs()
    if mistake == "tile exchanged with its grouped-order neighbour":
        out = out.clone()
        if fam.group_m > 1:
            h, wd = min(fam.BM, M - fam.BM), min(fam.BN, N)
            out[:h, :wd], out[fam.BM:fam.BM + h, :wd] = out[fam.BM:fam.BM + h, :wd].clone(), out[:h, :wd].clone()
        else:
            h, wd = min(fam.BM, M), min(fam.BN, N - fam.BN)
            out[:h, :wd], out[:h, fam.BN:fam.BN + wd] = out[:h, fam.BN:fam.BN + wd].clone(), out[:h, :wd].clone()
    if mistake == "f32 stream rounded to f16":
        out = out.to(F16).double()
    if mistake == "output row not mapped":
        dest = torch.where(valid, torch.arange(M, device=dest.device), dest)
    if mistake == "dropped rows written to row 0":
        dest = dest.clamp(min=0)
    cols = N - 4 if mistake == "last 4 columns missing when N % 8 == 4" else N
    return Ref(out, dest, cols, lin, y, v, mag)


def reference_rowloop(B):
    """The same statement as a plain loop over the rows (scatter and residual indexing spelled out)."""
    c = B.case
    f = FORMS[c.form]
    out = torch.full((c.M, c.N), NAN, dtype=F64, device=B.dest.device)
    dest = []
    for m in range(c.M):
        r = int(B.row_map[m]) if B.row_map is not None else m
        dest.append(r)
        if r < 0:
            continue
        row = B.a[m].double() @ B.w.double().t()
        if f.bias:
            row = row + B.bias.double()
        if f.act == "gelu":
            row = 0.5 * row * (1 + torch.erf(row / math.sqrt(2)))
        elif f.act == "relu":
            row = torch.where(row > 0, row, torch.zeros_like(row))
        if f.cs:
            row = row * B.cs.double()
        if f.res:
            row = row + B.residual[r].double()
        out[m] = row
    return out, torch.tensor(dest, device=B.dest.device)


def gemm_tol(B, ref):
    """Per-element bound of ink_gemm_f16, all four families: each runs K / 32 MFMA 16x16x32 steps per accumulator.  The
    f16 products are exact; a step sums its 32 products in <= 5 rounding levels (5 u sum_k |a_k w_k| over all steps) and
    adds them to the f32 accumulator once (K / 32 u mag, mag including a preloaded residual); the bias add 2 u mag:
        t = (K / 32 + 7) u mag.
    ReLU is exact and 1-Lipschitz.  GELU (gelu_erf, |gelu'| <= 1.13; the A&S erf error enters times |lin| / 2, its
    exp2 / rcp / polynomial roundings 6 u |lin|, the final fma u |y|): 1.13 t + (GELU_ERF / 2 + 6 u) |lin| + u |y|.
    col_scale: v = cs * y rounds once: |cs| t + u |v|.  A late residual (activation or col_scale present) is added to
    the f32 value read back from the LDS patch: + u |out| for an f32 output.  An f16 output without a late residual
    rounds once: + 2^-11 |out| + 2^-25.
    An f16 output WITH a late residual rounds twice, as store_wave_tile does it: the patch row is written as f16
    (2^-11 |v| + 2^-25), read back, the f32 residual is added in f32 (u |out|) and the sum is rounded to f16 again
    (2^-11 |out| + 2^-25).  That is a property of the kernel (the patch of an f16 output is f16), not a defect; no
    production call uses the form."""
    c = B.case
    f = FORMS[c.form]
    t = (c.K / 32 + 7) * U * ref.mag
    if f.act == "gelu":
        t = 1.13 * t + (GELU_ERF / 2 + 6 * U) * ref.lin.abs() + U * ref.y.abs()
    if f.cs:
        t = B.cs.double().abs() * t + U * ref.v.abs()
    oa = ref.out.abs()
    if not f.f16:
        return t + U * oa if res_late(f) else t
    if res_late(f):
        return t + H16 * ref.v.abs() + SUB16 + U * oa + H16 * oa + SUB16
    return t + H16 * oa + SUB16


# ---------------------------------------------------------------------------------------------------------------
# buffer checks (the same code judges the kernel's buffer and a simulated one)
# ---------------------------------------------------------------------------------------------------------------
def target_mask(B, ref=None):
    """bool [rows + 64, ldc]: the elements the statement writes."""
    dest = B.dest if ref is None else ref.dest
    mask = torch.zeros(B.outbuf.shape, dtype=torch.bool, device=B.outbuf.device)
    mask[dest[dest >= 0], :B.case.N] = True
    return mask


def place(B, ref):
    """The float64 image of the whole output buffer after a kernel that computes `ref` (possibly a mistake)."""
    buf = B.init.double()
    sel = ref.dest >= 0
    buf[ref.dest[sel], :ref.cols] = ref.out[sel, :ref.cols]
    return buf


def same_values(x, y):
    """Elementwise x == y with NaN equal to NaN."""
    return (x == y) | (x.isnan() & y.isnan())


def untouched_ok(B, buf):
    """Guard rows, guard columns and the rows the row map does not target are as they were before the call."""
    keep = ~target_mask(B)
    return bool(same_values(buf.double()[keep], B.init.double()[keep]).all())


def targeted(B, buf, ref):
    """(values of buf at the targeted elements [n_valid, N] as float64, the reference's, the row selector)."""
    sel = B.dest >= 0
    return buf[B.dest[sel], :B.case.N].double(), ref.out[sel], sel


def exact_preconditions(B, ref):
    """What bit-exactness of the exact data rests on: every operand an integer (col_scale a power of two up to sign),
    sum |a||w| + |b| + |r| < 2^24, and for f16 outputs ref (and the f16 patch value v of a late residual) f16 numbers."""
    c = B.case
    f = FORMS[c.form]
    sel = B.dest >= 0
    assert bool((B.a == B.a.round()).all() and (B.w == B.w.round()).all())
    mag = B.absprod[sel]
    if f.bias:
        assert bool((B.bias == B.bias.round()).all())
        mag = mag + B.bias.double().abs()
    if f.res:
        r = B.res64[B.dest[sel]]
        assert bool((r == r.round()).all())
        mag = mag + r.abs()
    if f.cs:
        assert bool(((B.cs.abs().log2() % 1) == 0).all())
        mag = mag * B.cs.double().abs().clamp(min=1)
    assert mag.max().item() < 2 ** 24
    out = ref.out[sel]
    assert bool((out.float().double() == out).all())
    if f.f16:
        assert bool((out.half().double() == out).all()) and bool((ref.v[sel].half().double() == ref.v[sel]).all())
