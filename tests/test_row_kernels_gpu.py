"""The kernels that turn a token row into a normalised row, each launch on its own, in every mode: ops.layernorm_rows,
ops.add_cvt_f16 / add_split_f16 / add_f32 (csrc/norm.hip), ops.proj256_ln (proj_ln.hip) and ops.ffn256_fused
(ffn_fused.hip).  GPU box only.  References, derived bounds and the case tables are tests/row_kernels_ref.py's
(tests/test_row_kernels_ref_cpu.py holds them to account on the CPU).  Conventions:
  * f32 outputs are compared with the float64 reference under the derived per-element bound (LayerNorm) or under the
    existing op tests' own assertions (the two MFMA kernels);
  * f16 and split outputs are compared bit for bit with the f32 output of the SAME launch (the kernel converts one y);
  * a row's arithmetic depends on that row alone in all three kernels (one wave per row, or one MFMA B-operand column
    per row), so a launch on a prefix or a window of the rows is bit for bit the matching rows of the full launch;
  * a sentinel is a buffer pre-filled with one bit pattern that must be unchanged wherever the kernel may not write."""
import pytest
import torch

import row_kernels_ref as K

pytestmark = pytest.mark.gpu

F16, F32, I32 = torch.float16, torch.float32, torch.int32
SENTINEL32, SENTINEL16 = 0x7FC12345, 0x7E55                 # quiet NaNs with a payload


def _sentinel(shape, dtype, dev):
    if dtype == F32:
        return torch.full(shape, SENTINEL32, dtype=torch.int32, device=dev).view(F32)
    return torch.full(shape, SENTINEL16, dtype=torch.int16, device=dev).view(F16)


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(K.bits(a), K.bits(b))


def _untouched(buf, written):
    """Every element of the sentinel-filled `buf` outside the boolean mask `written` still holds the sentinel."""
    want = SENTINEL32 if buf.dtype == F32 else SENTINEL16
    return bool((K.bits(buf)[~written] == want).all())


# ---------------------------------------------------------------------------------------------------------------
# ops.layernorm_rows
# ---------------------------------------------------------------------------------------------------------------
def _ln_launch(dev, c, *, split=False, x=None, out=None, out2=None, out_dtype=F32, split_f32=None):
    """One ops.layernorm_rows launch of the case (x: a device tensor to use in place of the case's own)."""
    from inklayer_amd import ops
    d = lambda t: None if t is None else t.to(dev)
    xd = d(c.x) if x is None else x
    kw = {}
    if c.gather is not None:
        kw["gather"] = torch.tensor(c.gather, dtype=I32).to(dev)
    if c.add is not None:
        kw["add"] = d(c.add)[:, c.add_col:c.add_col + c.C]
        if c.add_rows is not None:
            kw["add_batch_rows"], kw["rows_per_batch"] = torch.tensor(c.add_rows, dtype=I32).to(dev), c.rows_per_batch
    return ops.layernorm_rows(xd, d(c.gamma), d(c.beta), c.eps, act=c.act, split=split, out=out, out2=out2,
                              out_dtype=F16 if split else out_dtype, split_f32=split_f32, **kw)


def _ln_check(dev, c):
    """Both launch forms of a case: f32 `out` + f16 `out2`, and split + split_f32.  -> (f32, worst error / bound)."""
    o32 = torch.empty(c.rows, c.C, device=dev, dtype=F32)
    o16 = torch.empty(c.rows, c.C, device=dev, dtype=F16)
    assert _ln_launch(dev, c, out=o32, out2=o16) is o32
    ref, tol = c.reference()
    got = o32.cpu()
    assert torch.isfinite(got).all(), c.name
    err = (got.double() - ref).abs()
    ratio = (err / tol.clamp(min=1e-300))[tol > 0].max().item()
    print(f"row_kernels layernorm {c.name}: R={c.rows} C={c.C} max abs err {err.max().item():.3g}, worst error / bound {ratio:.3f}")
    assert (err <= tol).all(), (c.name, ratio)
    assert _same_bits(o16, o32.to(F16)), c.name                 # the f16 copy is the rounding of the same y
    sf = torch.empty(c.rows, c.C, device=dev, dtype=F32)
    sp = _ln_launch(dev, c, split=True, split_f32=sf)
    assert sp.shape == (c.rows, 3 * c.C) and sp.dtype == F16
    assert _same_bits(sf, o32), c.name                          # the same arithmetic whatever the output form
    K.check_split_rule(sp, sf, c.name)
    if c.gather is not None:                                    # -1 rows: exact (positive) zeros in every output
        dead = torch.tensor(c.gather) < 0
        assert dead.any()
        for t in (o32, o16, sf, sp):
            assert (K.bits(t).cpu()[dead] == 0).all(), c.name
    return o32, ratio


@torch.no_grad()
@pytest.mark.parametrize("C", K.WIDTHS)
def test_layernorm_rows_width_sweep(dev, C):
    """Every instantiation (NV = 1..5 and 6, 7, 8 through `default`), each boundary from both sides; R = 9 is two full
    four-row workgroups and one row."""
    _ln_check(dev, K.CASE[f"width-{C}"])


@torch.no_grad()
@pytest.mark.parametrize("R", K.ROW_COUNTS)
def test_layernorm_rows_row_counts(dev, R):
    _ln_check(dev, K.CASE[f"rows-{R}"])


@torch.no_grad()
@pytest.mark.parametrize("C", K.MODE_WIDTHS)
@pytest.mark.parametrize("mode", ["no-gamma", "no-beta", "no-affine", "gelu", "gather", "gather-gelu", "add", "add-table"])
def test_layernorm_rows_modes(dev, mode, C):
    """gamma / beta absent; GELU; gather with -1 rows, repeats and more output rows than input rows; the addend row by
    row and through add_batch_rows (three entries of three rows into a shared tensor, out of order, ld_add > C)."""
    c = K.CASE[f"{mode}-{C}"]
    o32, _ = _ln_check(dev, c)
    if mode == "gelu":
        # the approximant on its own: the launch without `act` gives the kernel's y bit for bit (the same arithmetic up to
        # the activation), so GELU's own error - A-S 7.1.26, v_rcp, v_exp - is measured against gelu_err(y) alone
        y = _ln_launch(dev, K.LnCase("no-act", c.x, c.gamma, c.beta, c.eps)).cpu().double()
        err, bound = (o32.cpu().double() - K.gelu_ref(y)).abs(), K.gelu_err(y)
        print(f"row_kernels gelu_erf {c.name}: |y| <= {y.abs().max().item():.2f}, max abs err {err.max().item():.3g}, "
              f"worst error / bound {(err / bound.clamp(min=1e-300)).max().item():.3f}")
        assert (err <= bound).all()
    if mode == "gather":
        assert c.rows > c.x.shape[0]
        first = {}
        for i, s in enumerate(c.gather):                        # a repeated source row gives the same bits
            if s >= 0 and s in first:
                assert _same_bits(o32[i], o32[first[s]])
            first.setdefault(s, i)
    if mode == "add-table":
        assert c.add.shape[1] > C and sorted(c.add_rows) != list(c.add_rows)
        # bit for bit the launch on the materialised addend rows
        _, add, _, _ = c.inputs()
        plain = K.LnCase("materialised", c.x, c.gamma, c.beta, c.eps, add=add.contiguous())
        assert _same_bits(_ln_launch(dev, plain), o32)


@torch.no_grad()
@pytest.mark.parametrize("eps", K.EPS_LIST)
@pytest.mark.parametrize("with_add", [False, True], ids=["plain", "add"])
def test_layernorm_rows_numerics(dev, eps, with_add):
    """Rows at offset 1000 / spread 0.05, offset 100 / spread 1, scale 1e4, scale 1e-4 and a constant row in one launch;
    the constant row at C = 256 is beta exactly (every sum only doubles)."""
    c = K.CASE[f"numerics-{'add-' if with_add else ''}eps{eps:g}"]
    o32, _ = _ln_check(dev, c)
    assert _same_bits(o32[K.CONSTANT_ROW].cpu(), c.beta)


@torch.no_grad()
@pytest.mark.parametrize("C", K.MODE_WIDTHS)
def test_layernorm_rows_strided_with_sentinels(dev, C):
    """x, out and out2 as column blocks of wider tensors; the split operand as a column block too.  The gap columns and
    the rows past R keep the sentinel."""
    c = K.CASE[f"width-{C}"]
    R = c.rows
    xw = _sentinel((R + 2, C + 12), F32, dev)
    xw[1:R + 1, 8:8 + C] = c.x.to(dev)
    x = xw[1:R + 1, 8:8 + C]
    want = _ln_launch(dev, c, x=c.x.to(dev))
    big32, big16 = _sentinel((R + 3, C + 8), F32, dev), _sentinel((R + 3, C + 8), F16, dev)
    written = torch.zeros(R + 3, C + 8, dtype=torch.bool, device=dev)
    written[:R, 4:4 + C] = True
    _ln_launch(dev, c, x=x, out=big32[:R, 4:4 + C], out2=big16[:R, 4:4 + C])
    assert _same_bits(big32[:R, 4:4 + C], want) and _same_bits(big16[:R, 4:4 + C], want.to(F16))
    assert _untouched(big32, written) and _untouched(big16, written)
    held = torch.zeros(R + 2, C + 12, dtype=torch.bool, device=dev)
    held[1:R + 1, 8:8 + C] = True
    assert _untouched(xw, held) and _same_bits(x, c.x.to(dev))              # (the input is only read)
    bigs = _sentinel((R + 3, 3 * C + 16), F16, dev)
    ws = torch.zeros(R + 3, 3 * C + 16, dtype=torch.bool, device=dev)
    ws[:R, 8:8 + 3 * C] = True
    _ln_launch(dev, c, x=x, split=True, out=bigs[:R, 8:8 + 3 * C])
    K.check_split_rule(bigs[:R, 8:8 + 3 * C], want, ("strided split", C))
    assert _untouched(bigs, ws)


@torch.no_grad()
@pytest.mark.parametrize("C", K.MODE_WIDTHS)
def test_layernorm_rows_in_place(dev, C):
    """out is x (f32) with an f16 out2, as the detector's decoder norms its queries: the row is in registers before the
    first store, so the result is that of the out-of-place launch."""
    c = K.CASE[f"add-{C}"]
    want32 = torch.empty(c.rows, C, device=dev, dtype=F32)
    want16 = torch.empty(c.rows, C, device=dev, dtype=F16)
    _ln_launch(dev, c, out=want32, out2=want16)
    x = c.x.to(dev)
    o16 = torch.empty(c.rows, C, device=dev, dtype=F16)
    got = _ln_launch(dev, c, x=x, out=x, out2=o16)
    assert got.data_ptr() == x.data_ptr() and _same_bits(x, want32) and _same_bits(o16, want16)


@torch.no_grad()
@pytest.mark.parametrize("C", K.MODE_WIDTHS)
def test_layernorm_rows_row_independence(dev, C):
    """Row i of the nine-row launch is bit for bit a one-row launch on that row."""
    c = K.CASE[f"gelu-{C}"]
    full = _ln_launch(dev, c)
    xd = c.x.to(dev)
    for i in range(c.rows):
        one = K.LnCase("one", c.x[i:i + 1], c.gamma, c.beta, c.eps, act=c.act)
        assert _same_bits(_ln_launch(dev, one, x=xd[i:i + 1]), full[i:i + 1]), (C, i)


# ---------------------------------------------------------------------------------------------------------------
# ops.add_cvt_f16 / ops.add_split_f16 / ops.add_f32: exact
# ---------------------------------------------------------------------------------------------------------------
def _add_all(dev, a, b, what):
    """The three kernels on (a, b) against the exact references; b None skips add_f32 (its b is not optional)."""
    from inklayer_amd import ops
    ad, bd = a.to(dev), None if b is None else b.to(dev)
    assert _same_bits(ops.add_cvt_f16(ad, bd).cpu(), K.add_cvt_ref(a, b)), what
    sp = ops.add_split_f16(ad, bd).cpu()
    assert sp.shape == (a.shape[0], 3 * a.shape[1])
    K.check_split_rule(sp, K.add_f32_ref(a, b), what)
    if b is not None:
        assert _same_bits(ops.add_f32(ad, bd).cpu(), K.add_f32_ref(a, b)), what


@torch.no_grad()
@pytest.mark.parametrize("kind", ["none", "row", "block", "full"])
def test_add_kernels_broadcast(dev, kind):
    """No b; b one row of C values (a bias); b = k C values for a k that divides the row count (a per-image block); b of
    full size.  1030 x 12: five blocks of 256 vectors with a ragged tail, and a C that is no power of two."""
    g = torch.Generator().manual_seed(60)
    Rn, C = 1030, 12
    a = torch.randn(Rn, C, generator=g) * 3
    b = {"none": None, "row": torch.randn(C, generator=g), "block": torch.randn(5, C, generator=g),
         "full": torch.randn(Rn, C, generator=g)}[kind]
    _add_all(dev, a, b, kind)


@torch.no_grad()
@pytest.mark.parametrize("op", ["add_cvt_f16", "add_f32", "add_split_f16"])
def test_add_kernels_second_trip_of_the_grid_stride_loop(dev, op):
    """n / 4 just above the block cap x 256 (2048 blocks; 4096 for add_split_f16): the first 150 rows of the second trip
    exist, and they and the last rows of the first trip carry values of their own."""
    from inklayer_amd import ops
    C = 8
    cap = 4096 if op == "add_split_f16" else 2048
    Rn = cap * 256 * 4 // C + 150
    g = torch.Generator().manual_seed(61)
    a = torch.randn(Rn, C, generator=g)
    edge = cap * 256 * 4 // C
    a[edge - 4:edge] = torch.arange(4 * C, dtype=F32).view(4, C) + 1000.25       # the first trip's last rows
    a[edge:edge + 4] = -(torch.arange(4 * C, dtype=F32).view(4, C) + 2000.5)     # the second trip's first rows
    a[-1] = torch.arange(C, dtype=F32) + 3000.75
    b = torch.randn(2, C, generator=g)
    ad, bd = a.to(dev), b.to(dev)
    if op == "add_cvt_f16":
        assert _same_bits(ops.add_cvt_f16(ad, bd).cpu(), K.add_cvt_ref(a, b))
    elif op == "add_f32":
        assert _same_bits(ops.add_f32(ad, bd).cpu(), K.add_f32_ref(a, b))
    else:
        K.check_split_rule(ops.add_split_f16(ad, bd), K.add_f32_ref(a, b), op)


@torch.no_grad()
def test_add_split_f16_edge_values(dev):
    """Values below 2^-9 (the low part is an f16 subnormal), exact f16 ties (round to even), signed zeros, and 60000-odd
    magnitudes inside f16's range."""
    tiny = torch.tensor([2.0 ** -10 * 1.3, -2.0 ** -12 * 1.7, 2.0 ** -15, 2.0 ** -20 * 1.1, 2.0 ** -25, -2.0 ** -26, 1e-8, -3e-10])
    ties = torch.tensor([1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11, -(2 + 2.0 ** -10), 2 + 3 * 2.0 ** -10, 1024.5, -1025.5, 2.0 ** -14 * (1 + 2.0 ** -11), 0.5 + 2.0 ** -12])
    zeros = torch.tensor([0.0, -0.0, 0.0, -0.0, 1.0, -1.0, -0.0, 0.0])
    big = torch.tensor([60000.0, 60001.3, -60015.9, 65503.9, -65519.0, 59999.99, 32767.9, -49152.7])
    a = torch.stack([tiny, ties, zeros, big])
    from inklayer_amd import ops
    sp = ops.add_split_f16(a.to(dev)).cpu()
    K.check_split_rule(sp, a, "no b")
    assert torch.isfinite(sp).all()
    # with b: -0 + +0 = +0, and sums that land on the same edge values
    b = torch.stack([torch.zeros(8), torch.zeros(8), torch.tensor([0.0, 0.0, -0.0, -0.0, 0.0, 0.0, 0.0, -0.0]), torch.zeros(8)])
    _add_all(dev, a, b, "with b")
    half = torch.stack([tiny, ties, zeros, big]) * 0.5          # exact halves: a + a is the edge value again
    _add_all(dev, half, half.clone(), "halves")


@torch.no_grad()
def test_add_outputs_given_and_aliased(dev):
    """out= given to add_cvt_f16; add_f32 with out aliasing a (the SAM decoder's in-place token update)."""
    from inklayer_amd import ops
    g = torch.Generator().manual_seed(62)
    a, b = torch.randn(37, 256, generator=g), torch.randn(256, generator=g)
    ad, bd = a.to(dev), b.to(dev)
    o16 = _sentinel((37, 256), F16, dev)
    assert ops.add_cvt_f16(ad, bd, out=o16) is o16 and _same_bits(o16.cpu(), K.add_cvt_ref(a, b))
    got = ops.add_f32(ad, bd, out=ad)
    assert got.data_ptr() == ad.data_ptr() and _same_bits(ad.cpu(), K.add_f32_ref(a, b))


# ---------------------------------------------------------------------------------------------------------------
# ops.proj256_ln
# ---------------------------------------------------------------------------------------------------------------
_PROJ = {}


def _proj_base(dev):
    """The R = 600 launch on the existing op test's data, once: (device inputs, blob, f32, split)."""
    if not _PROJ:
        from inklayer_amd import ops
        a, w, b, res, lg, lb = K.proj_ln_data()
        d = lambda t: t.to(dev).contiguous()
        blob = ops.proj256_ln_pack(ops.split_weight(d(w)))
        dd = dict(a=d(a), b=d(b), res=d(res), lg=d(lg), lb=d(lb), blob=blob)
        of, osp = ops.proj256_ln(dd["a"], blob, dd["b"], dd["res"], dd["lg"], dd["lb"], 1e-5)
        _PROJ.update(host=(a, w, b, res, lg, lb), dev=dd, of=of, osp=osp)
    return _PROJ


def _proj(dev, rows, **kw):
    from inklayer_amd import ops
    p = _proj_base(dev)["dev"]
    return ops.proj256_ln(p["a"][rows], p["blob"], p["b"], p["res"][rows], p["lg"], p["lb"], 1e-5, **kw)


@torch.no_grad()
def test_proj256_ln_base_launch(dev):
    """R = 600 (four full tiles and a ragged one) under tests/test_sam_gpu.py's own assertions: max-rel < 3e-6 against
    float64, the split reconstruction within 2e-5, the third segment exact; and the full split rule."""
    p = _proj_base(dev)
    want = K.proj_ln_ref(*p["host"], 1e-5)
    of, osp = p["of"], p["osp"]
    err = ((of.double().cpu() - want).abs().max() / want.abs().max()).item()
    rec = ((osp[:, :256].float() + osp[:, 256:512].float() / 64.0).double().cpu() - want).abs().max().item()
    print(f"row_kernels proj256_ln R=600: max-rel {err:.3g} (limit 3e-6: error / limit {err / 3e-6:.3f}), split reconstruction {rec:.3g}")
    assert torch.isfinite(of).all() and err < 3e-6 and rec < 2e-5
    assert torch.equal(osp[:, 512:], (osp[:, :256].float() / 64.0).half())
    K.check_split_rule(osp, of, "proj256_ln")


@torch.no_grad()
@pytest.mark.parametrize("R", [1, 31, 32, 33, 127, 128, 129])
def test_proj256_ln_prefix_is_bitwise(dev, R):
    """One wave's 32 rows and one workgroup's 128 from below, exactly and from above: the clamped lanes of a ragged wave
    (they recompute row R - 1) change nothing in the rows that exist."""
    p = _proj_base(dev)
    of, osp = _proj(dev, slice(0, R))
    assert _same_bits(of, p["of"][:R]) and _same_bits(osp, p["osp"][:R])


@torch.no_grad()
def test_proj256_ln_shifted_rows_and_single_outputs(dev):
    """Rows [5, 134) as a launch of their own: a row's result does not depend on which lane, wave or tile computes it.
    want_split = False / want_f32 = False return the other output with the same bits."""
    p = _proj_base(dev)
    of, osp = _proj(dev, slice(5, 134))
    assert _same_bits(of, p["of"][5:134]) and _same_bits(osp, p["osp"][5:134])
    of2, none = _proj(dev, slice(0, 129), want_split=False)
    assert none is None and _same_bits(of2, p["of"][:129])
    none, osp2 = _proj(dev, slice(0, 129), want_f32=False)
    assert none is None and _same_bits(osp2, p["osp"][:129])


@torch.no_grad()
def test_proj256_ln_residual_row_table(dev):
    """rows_per_batch = 5, R = 35: seven batch entries whose boundaries fall inside a wave's 32 rows, the table out of
    order into a residual of two images of 20 rows each.  Bit for bit the launch on the materialised residual."""
    from inklayer_amd import ops
    p = _proj_base(dev)["dev"]
    table = [20, 0, 35, 5, 25, 15, 10]
    shared = p["res"][100:140].contiguous()
    rows = torch.cat([torch.arange(t, t + 5) for t in table]).to(dev)
    a = p["a"][:35]
    want = ops.proj256_ln(a, p["blob"], p["b"], shared[rows].contiguous(), p["lg"], p["lb"], 1e-5)
    got = ops.proj256_ln(a, p["blob"], p["b"], shared, p["lg"], p["lb"], 1e-5,
                         res_batch_rows=torch.tensor(table, dtype=I32).to(dev), rows_per_batch=5)
    assert _same_bits(got[0], want[0]) and _same_bits(got[1], want[1])
    assert not _same_bits(got[0], _proj(dev, slice(0, 35))[0])          # (the table does matter)


@torch.no_grad()
def test_proj256_ln_writes_no_row_past_R(dev):
    """The C entry point with output buffers one 128-row tile longer than R = 129: rows at and past R keep the sentinel."""
    from inklayer_amd import _lib
    p = _proj_base(dev)
    dd, R = p["dev"], 129
    of, osp = _sentinel((R + 128, 256), F32, dev), _sentinel((R + 128, 768), F16, dev)
    from inklayer_amd import ops
    rc = _lib.lib().ink_proj256_ln(dd["a"].data_ptr(), dd["blob"].data_ptr(), dd["b"].data_ptr(), dd["res"].data_ptr(), None, 0,
                                   dd["lg"].data_ptr(), dd["lb"].data_ptr(), 1e-5, R, of.data_ptr(), osp.data_ptr(),
                                   ops._stream())
    assert rc == 0
    torch.cuda.synchronize()
    assert _same_bits(of[:R], p["of"][:R]) and _same_bits(osp[:R], p["osp"][:R])
    for buf in (of, osp):
        written = torch.zeros(buf.shape, dtype=torch.bool, device=dev)
        written[:R] = True
        assert _untouched(buf, written)


# ---------------------------------------------------------------------------------------------------------------
# ops.ffn256_fused, plain and pre=
# ---------------------------------------------------------------------------------------------------------------
_FFN = {}


def _ffn_setup(dev, M, hid, pre):
    """Device tensors, blob and the full launch of (M, hid, pre), once."""
    key = (M, hid, pre)
    if key not in _FFN:
        from inklayer_amd import ops
        h = K.ffn_data(M, hid, pre)
        d = {k: v.to(dev).contiguous() for k, v in h.items()}
        d["blob"] = ops.ffn256_pack(d["w1"], d["b1"], d["w2"], d["wp"] if pre else None)
        d["pre"] = (d["bp"], d["g1"], d["e1"]) if pre else None
        _FFN[key] = (h, d, hid)
        _FFN[key] += (_ffn(dev, key, slice(0, M)),)
    return _FFN[key]


def _ffn(dev, key, rows, x16=None, res=None, out=None):
    from inklayer_amd import ops
    _, d, hid = _FFN[key][:3]
    return ops.ffn256_fused(d["x16"][rows] if x16 is None else x16, d["res"][rows] if res is None else res, d["blob"], hid,
                            d["b2"], d["lg"], d["lb"], 1e-5, out=out, pre=d["pre"])


@torch.no_grad()
@pytest.mark.parametrize("pre", [False, True], ids=["plain", "pre"])
@pytest.mark.parametrize("hid", [64, 192, 320, 2048])
def test_ffn256_fused_base_launch(dev, hid, pre):
    """One, three, five and 32 chunks of 64 hidden units (odd counts end on the first LDS weight buffer, whose bytes the
    epilogue reuses) at M = 1000, under tests/test_ops_gpu.py's own assertions against float64."""
    h, d, _, got = _ffn_setup(dev, 1000, hid, pre)
    ea = (got.double().cpu() - K.ffn_ref(h)).abs()
    mx, mean = ea.max().item(), ea.mean().item()
    lim_max, lim_mean = (2e-3, 1e-5) if pre else (1e-3, 5e-6)
    print(f"row_kernels ffn256_fused {'pre' if pre else 'plain'} hid={hid} M=1000: max abs {mx:.3g} (error / limit {mx / lim_max:.3f}), "
          f"mean abs {mean:.3g} (error / limit {mean / lim_mean:.3f})")
    assert torch.isfinite(got).all() and mx < lim_max and mean < lim_mean


@torch.no_grad()
@pytest.mark.parametrize("pre", [False, True], ids=["plain", "pre"])
@pytest.mark.parametrize("M", [1, 31, 32, 33, 127, 128, 129, 1153])
def test_ffn256_fused_prefix_is_bitwise(dev, M, pre):
    """hid = 192.  The base launch has M = 1153: ten workgroups, a tile count with remainder 2 mod 8 in xcd_remap, the
    last tile one row.  A launch on the first M rows (another tile count, another remap, clamped lanes in its last
    wave) is bit for bit rows [:M] of it; M = 1153 itself: the launch repeats bit for bit."""
    key = (1153, 192, pre)
    base = _ffn_setup(dev, *key)[3]
    assert torch.isfinite(base).all()
    assert _same_bits(_ffn(dev, key, slice(0, M)), base[:M])


@torch.no_grad()
@pytest.mark.parametrize("pre", [False, True], ids=["plain", "pre"])
def test_ffn256_fused_shifted_strided_in_place_and_sentinel(dev, pre):
    """Rows [5, 134) as a launch of their own; x16 as a column block of a [M, 512] tensor (ldx = 512); out = res in place
    at M = 129; out as the first M rows of a sentinel-filled [M + 128, 256] buffer, whose other rows stay unchanged."""
    key = (1153, 192, pre)
    _, d, _, base = _ffn_setup(dev, *key)
    assert _same_bits(_ffn(dev, key, slice(5, 134)), base[5:134])
    M = 129
    wide = _sentinel((M, 512), F16, dev)
    wide[:, 128:384] = d["x16"][:M]
    assert _same_bits(_ffn(dev, key, slice(0, M), x16=wide[:, 128:384]), base[:M])
    res = d["res"][:M].clone()
    got = _ffn(dev, key, slice(0, M), res=res, out=res)
    assert got.data_ptr() == res.data_ptr() and _same_bits(res, base[:M])
    big = _sentinel((M + 128, 256), F32, dev)
    _ffn(dev, key, slice(0, M), out=big[:M])
    written = torch.zeros(M + 128, 256, dtype=torch.bool, device=dev)
    written[:M] = True
    assert _same_bits(big[:M], base[:M]) and _untouched(big, written)
