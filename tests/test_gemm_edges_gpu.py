"""ink_gemm_f16 against its float64 statement at the edges of every tile family (128x128x64, 128x128x32, 16-wave 256x256,
ping-pong 256x320) and of every epilogue branch, at the smallest shapes that have the branch.  Statement, bound, case
tables and named mistakes are in tests/gemm_ref.py; tests/test_gemm_edges_ref_cpu.py shows on the CPU that each case
runs on the family it names, that the tables reach every branch and that the checks used here tell the named mistakes
apart.  Exact data (small integers) is compared with torch.equal, bounded data per element with gemm_tol (worst <= 1.0,
no margin).  Every output is a view into a NaN-filled buffer with 64 guard rows (and guard columns where ldc > N); the
guards and every row the row map does not target must come back bit-unchanged; a and w are views into NaN-filled
buffers.  GPU box only."""
from contextlib import contextmanager

import pytest
import torch

import gemm_ref as R

pytestmark = pytest.mark.gpu


@contextmanager
def forced(fam):
    """The tile family forced through the process-wide test hook, the heuristic restored whatever happens."""
    from inklayer_amd import _lib
    lib = _lib.lib()
    assert lib.ink_gemm_set_variant(R.FAMILIES[fam].variant) == 0
    try:
        yield
    finally:
        lib.ink_gemm_set_variant(-1)


def _launch(c, dev):
    from inklayer_amd import ops
    f = R.FORMS[c.form]
    assert R.family_run(R.FAMILIES[c.fam].variant, c.K) == c.fam
    B = R.buffers(c, dev)
    with forced(c.fam):
        ops.gemm(B.a, B.w, B.bias, act=f.act, residual=B.residual, col_scale=B.cs, row_map=B.row_map, out=B.out)
    return B


def _bits(t):
    return t.view(torch.int16 if t.dtype == R.F16 else torch.int32)


def _check(c, B, ref=None):
    """Guards and untargeted rows bit-unchanged; the targeted elements equal to the float64 statement (exact data) or
    within gemm_tol (bounded data).  Returns the worst error as a fraction of the bound (0.0 for exact data)."""
    ref = ref or R.reference(B)
    keep = ~R.target_mask(B)
    assert torch.equal(_bits(B.outbuf)[keep], _bits(B.init)[keep]), f"{c}: guard or untargeted elements were written"
    got, want, sel = R.targeted(B, B.outbuf, ref)
    if c.data == "exact":
        if not torch.equal(got, want):
            bad = (got != want) | got.isnan()
            i = bad.nonzero()[0].tolist()
            raise AssertionError(f"{c}: {int(bad.sum())} / {bad.numel()} elements differ; first at (valid row, col) {i}: "
                                 f"got {got[i[0], i[1]].item()!r}, ref {want[i[0], i[1]].item()!r}")
        return 0.0
    return R.assert_within(got, want, R.gemm_tol(B, ref)[sel], str(c))


def _run(c, dev):
    B = _launch(c, dev)
    return _check(c, B)


@torch.no_grad()
@pytest.mark.parametrize("fam", R.FAMS)
def test_tile_walk(dev, fam):
    """1 .. 21 ragged tiles (M = ntm BM - 5, N = ntn BN - 12): workgroup counts 1, 2, 3, 3, 8, 5, 10, 9, 21 for xcd_remap,
    M-tile counts with a last group of 1, 2 and 3 for tile_of.  A tile mapped twice or never leaves NaN or a wrong block."""
    for c in R.tile_walk_cases(fam):
        _run(c, dev)


@torch.no_grad()
@pytest.mark.parametrize("fam", R.FAMS)
def test_k_loop(dev, fam):
    """One ragged 2x2-tile problem, 1 .. 5 K tiles of the generic kernels and 4, 6, 8, 10, 14 granules of the ping-pong
    ring (minimum, wrap, drained tail), with and without a preloaded residual (the prologue waits differently)."""
    for c in R.k_loop_cases(fam):
        _run(c, dev)


@torch.no_grad()
@pytest.mark.parametrize("fam", R.FAMS)
def test_m_edges(dev, fam):
    """M = 1 .. 257 around every slab, wave and tile boundary, bias + ReLU, f32 and f16 out, N = 72 / 76."""
    for c in R.m_edge_cases(fam):
        _run(c, dev)


@torch.no_grad()
@pytest.mark.parametrize("fam", R.FAMS)
def test_n_edges(dev, fam):
    """N at -4, 0, +4 around every wave-column and tile boundary of the four families, ldc = N, N + 4, N + 64 (16-byte or
    8-byte f16 stores, the N % 8 == 4 half chunk), M = 40."""
    for c in R.n_edge_cases(fam):
        _run(c, dev)


@torch.no_grad()
@pytest.mark.parametrize("fam", R.FAMS)
def test_epilogue_forms_exact(dev, fam):
    """The fifteen epilogue forms (a) .. (o) of gemm_ref.FORMS at 300 x 332, exact data."""
    for c in R.epilogue_cases(fam):
        _run(c, dev)


@torch.no_grad()
@pytest.mark.parametrize("fam", R.FAMS)
def test_bounded_forms(dev, fam):
    """The rounding forms and the four GELU forms on random data at a short and a long K, every element within gemm_tol;
    every applicable named mistake re-checked on the full data (>= its factor outside the bound, or a broken guard)."""
    for form in R.BOUNDED_FORMS:
        worst = {}
        for c in (c for c in R.bounded_cases(fam) if c.form == form):
            B = _launch(c, dev)
            ref = R.reference(B)
            worst[c.K] = _check(c, B, ref)
            tol = R.gemm_tol(B, ref)
            for what, factor in R.applicable(c):
                wrong = R.place(B, R.reference(B, what))
                got, want, sel = R.targeted(B, wrong, ref)
                m = R.discrimination(got, want, tol[sel])
                guards = R.untouched_ok(B, wrong)
                assert m >= factor or not guards, f"{c}: '{what}' lands {m:.1f}x the bound, guards intact"
                print(f"    {fam} {form} K={c.K}: {what}: {m:.0f}x the bound{'' if guards else ', guards broken'}")
        print(f"  gemm_edges {fam} {form}: worst error / bound " + ", ".join(f"K={k}: {v:.3f}" for k, v in worst.items())
              + f"  -> {max(worst.values()):.3f}")


@torch.no_grad()
@pytest.mark.parametrize("data", ["exact", "bounded"])
def test_same_bits_across_families(dev, data):
    """K = 192, the forms of test_epilogue_forms_exact under variants 0, 10 and 45: the same bits.  Each accumulator
    starts from the same value (0 or the preloaded residual), every kernel adds the same 32-wide K groups, one MFMA each,
    in increasing k, and the epilogue applies the same f32 operations in the same order.  The GELU forms are reported,
    not asserted: the ping-pong kernel's compile-time GELU epilogue and the run-time one are different instantiations."""
    for form in R.EPILOGUE_FORMS + (R.GELU_FORMS if data == "bounded" else ()):
        bufs = []
        for fam in R.SAME_BITS_FAMS:
            c = R.Case("samebits", fam, R.EPI_M, R.EPI_N, 192, form, 0, data)
            B = _launch(c, dev)
            _check(c, B)
            bufs.append(_bits(B.outbuf))
        same = torch.equal(bufs[0], bufs[1]) and torch.equal(bufs[0], bufs[2])
        if form in R.GELU_FORMS:
            print(f"  gemm_edges same bits under variants 0 / 10 / 45, {form}: {same}")
        else:
            assert same, f"form {form} ({data} data): the outputs under variants 0, 10, 45 differ"


@torch.no_grad()
def test_determinism_pingpong(dev):
    """Form (m) on exact data and the plain GELU f16 form on random data, twice on the ping-pong kernel: the same bits."""
    for c in (R.Case("det", "F45", R.EPI_M, R.EPI_N, 192, "m", 0, "exact"),
              R.Case("det", "F45", R.EPI_M, R.EPI_N, 1024, "gelu_f16", 0, "bounded")):
        first, second = _launch(c, dev), _launch(c, dev)
        _check(c, first)
        assert torch.equal(_bits(first.outbuf), _bits(second.outbuf)), c
