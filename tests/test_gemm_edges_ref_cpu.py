"""CPU side of the GEMM edge suite (tests/gemm_ref.py, tests/test_gemm_edges_gpu.py): the float64 statement agrees with
a second statement of it, the exact data meets the preconditions of bit-exactness, the bound and the guard checks tell
every named mistake apart, every case runs on the family it names, the case tables reach every (family, branch) pair
the kernels have, and ink_gemm_f16 refuses malformed arguments before it launches.  No GPU."""
import ctypes

import pytest
import torch

import gemm_ref as R


def _unique(cases):
    """One case per distinct problem: the family only selects the kernel, except through BK / tile size in the mistakes."""
    seen, out = set(), []
    for c in cases:
        key = c._replace(test="")
        if key not in seen:
            seen.add(key)
            out.append(c)
    return out


ALL = R.gpu_cases()
EXACT = _unique(c for c in ALL if c.data == "exact")
BOUNDED = _unique(c for c in ALL if c.data == "bounded")


def test_case_tables_are_what_the_suite_was_asked_for():
    assert len(R.WALK_TILES) == 9 and max(c.M * c.N for c in ALL if c.test == "walk") == 1787 * 948
    assert [R.geometry(c).wgs for c in R.tile_walk_cases("F10")] == [1, 2, 3, 3, 8, 5, 10, 9, 21]
    assert [c.K // 32 for c in R.k_loop_cases("F45")][::2] == [4, 6, 8, 10, 14]
    assert len(R.M_EDGES) == 16 and len(R.N_EDGES) == 26 and len(R.EPILOGUE_FORMS) == 15
    assert all(c.N % 4 == 0 and c.K % 32 == 0 and (c.N + c.ldc_pad) % 4 == 0 for c in ALL)
    for c in ALL:                                       # exact data: no GELU
        assert c.data == "bounded" or R.FORMS[c.form].act in (None, "relu")


def test_every_case_runs_on_the_family_it_names():
    """From K % 64 and the forcing rule of ink_gemm_f16 (family_run) alone; no case relies on the heuristic."""
    for c in ALL:
        fam = R.FAMILIES[c.fam]
        assert R.family_run(fam.variant, c.K) == c.fam, c
        if c.fam == "F32":                              # whatever is forced
            assert all(R.family_run(v, c.K) == "F32" for v in (0, 10, 45))
        else:
            assert c.K % 64 == 0 and (c.fam != "F45" or c.K >= 128)
    assert {c.fam for c in ALL} == set(R.FAMS)


@torch.no_grad()
@pytest.mark.parametrize("form,fam,M,N,K", [("o", "F32", 45, 36, 96), ("m", "F45", 37, 332, 128),
                                            ("gelu_res_f16", "F0", 33, 20, 64)])
def test_reference_agrees_with_a_row_loop(form, fam, M, N, K):
    """The vectorised statement (scatter by index_put, residual gathered through the row map) against a plain loop over
    the rows, on a dropping map, a scattering in-place map and the GELU form."""
    c = R.Case("ref", fam, M, N, K, form, 0, "bounded")
    B = R.buffers(c)
    ref = R.reference(B)
    out2, dest2 = R.reference_rowloop(B)
    assert torch.equal(ref.dest, dest2)
    sel = dest2 >= 0
    assert sel.sum() >= M - 12 and (form != "o" or (~sel).sum() >= 2)
    assert not ref.out[sel].isnan().any()
    assert (ref.out[sel] - out2[sel]).abs().max().item() <= 1e-13 * ref.mag[sel].max().item()
    # the placed buffer: targeted rows carry the values, everything else is the initial content
    buf = R.place(B, ref)
    assert R.untouched_ok(B, buf) and torch.equal(buf[dest2[sel], :N], ref.out[sel])
    assert buf[B.rows:].isnan().all()


@torch.no_grad()
def test_exact_data_preconditions():
    """Every exact case: integer operands, sum |a||w| + |b| + |r| < 2^24, the float64 result an f32 (and, for f16
    outputs, an f16) number - on the very operands the GPU test multiplies (drawn on the CPU from the shape's seed)."""
    assert len(EXACT) > 300
    for c in EXACT:
        B = R.buffers(c)
        R.exact_preconditions(B, R.reference(B))


def _judge(B, ref, tol, what, factor):
    """How one mistake shows: (x the bound at the targeted elements, guards intact?)."""
    wrong = R.place(B, R.reference(B, what))
    got, want, sel = R.targeted(B, wrong, ref)
    m = R.discrimination(got, want, tol[sel]) if tol is not None else float((~R.same_values(got, want)).any())
    return m, R.untouched_ok(B, wrong)


@torch.no_grad()
def test_bound_discriminates_on_bounded_cases():
    """Every applicable mistake lands >= 100x outside gemm_tol ('f32 stream rounded to f16': 2x, as in depth_ops_ref),
    or - the mistakes that write outside the targeted rows - breaks the guard / unchanged-row check."""
    seen = set()
    for c in BOUNDED:
        B = R.buffers(c)
        ref = R.reference(B)
        tol = R.gemm_tol(B, ref)
        got, want, sel = R.targeted(B, R.place(B, ref), ref)
        assert (tol[sel] > 0).all()
        assert R.discrimination(got, want, tol[sel]) == 0          # the statement itself passes its own check
        for what, factor in R.applicable(c):
            m, guards = _judge(B, ref, tol, what, factor)
            kinds = R.GUARD_MISTAKES.get(what, ())
            if R.FORMS[c.form].row_map in kinds:
                assert not guards, (c, what)
            if what != "dropped rows written to row 0":
                wrong = R.targeted(B, R.place(B, R.reference(B, what)), ref)[0]
                R.assert_discriminates(wrong, want, tol[sel], f"{c}: {what}", factor=factor)
            seen.add(what)
    assert seen == set(R.MISTAKES)


@torch.no_grad()
def test_exact_check_discriminates_on_exact_cases():
    """Every applicable mistake changes at least one targeted element of every exact case, or - 'dropped rows written to
    row 0' - only elements outside the targeted rows, which the guard check sees on a simulated output buffer."""
    seen = set()
    for c in EXACT:
        B = R.buffers(c)
        ref = R.reference(B)
        assert R.untouched_ok(B, R.place(B, ref))
        for what, factor in R.applicable(c):
            changed, guards = _judge(B, ref, None, what, factor)
            if R.FORMS[c.form].row_map in R.GUARD_MISTAKES.get(what, ()):
                assert not guards, (c, what)
            if what != "dropped rows written to row 0":
                assert changed, (c, what)
            seen.add(what)
    assert seen == set(R.MISTAKES) - {"f32 stream rounded to f16"}


# every (family, branch) pair named in the issue; written out
_COMMON = ["ragged_m", "full_m", "ragged_n", "full_n", "m<16", "ntm%4=1", "ntm%4=2", "ntm%4=3", "ntm%4=0",
           "ntn=1", "ntn=2", "ntn=3", "wgs<8", "wgs=8", "wgs>8,%8!=0",
           "f32", "f16", "act=none", "act=relu", "act=gelu", "bias", "no_bias",
           "residual_preloaded", "res_late", "scaled", "res_sep", "res_inplace", "ldr!=ldc", "ldc>N", "lda>K,ldw>K",
           "wide16", "narrow8", "half_chunk", "f16_double_rounding", "n_cuts_mfma_tile", "idle_wave_columns",
           "row_map=none", "row_map=perm", "row_map=drop", "row_map=scatter", "data=exact", "data=bounded"]
_GENERIC_K = ["ksteps=1", "ksteps=2", "ksteps>2", "ksteps_odd", "ksteps_even"]
REQUIRED = ([("F0", b) for b in _COMMON + _GENERIC_K]
            + [("F32", b) for b in _COMMON + ["ksteps=1", "ksteps>2", "ksteps_odd"]]     # K % 64 == 32: always odd
            + [("F10", b) for b in _COMMON + _GENERIC_K]
            + [("F45", b) for b in _COMMON + ["granules=4", "granules=6", "granules=8", "granules=10", "granules=14",
                                              "ring_wrap", "pp_prologue_drain", "pp_prologue_counted",
                                              "pp_f16_gelu", "pp_f16_none", "pp_f16_runtime", "pp_f32_none",
                                              "pp_f32_runtime"]])


def test_coverage_plan():
    """Each required (family, branch) pair is hit by at least one GPU case; the ragged-tile GELU epilogue of the
    ping-pong kernel (store_wave_tile<8, 5, 1, INK_ACT_GELU>) and the combinations the issue names are among them."""
    hit = {}
    for c in ALL:
        for b in R.branches(c):
            hit.setdefault((c.fam, b), c)
    missing = [p for p in REQUIRED if p not in hit]
    assert not missing, f"(family, branch) pairs without a GPU case: {missing}"
    # combinations
    both = lambda fam, *bs: any(c.fam == fam and set(bs) <= R.branches(c) for c in ALL)   # noqa: E731
    for fam in R.FAMS:
        assert both(fam, "half_chunk", "narrow8") and both(fam, "half_chunk", "wide16"), fam
        assert both(fam, "res_late", "scaled", "row_map=scatter") and both(fam, "residual_preloaded", "row_map=drop", "f16")
        assert both(fam, "act=gelu", "ragged_m", "ragged_n", "f16"), fam
    assert both("F45", "pp_f16_gelu", "ragged_m", "ragged_n", "half_chunk")
    for g in (4, 6, 8, 10, 14):
        assert both("F45", f"granules={g}", "pp_prologue_drain") and both("F45", f"granules={g}", "pp_prologue_counted")
    for fam in ("F10", "F45"):                          # tile_of: a last group of 1, 2, 3 M-tiles; of 1 and 3 after a full one
        for r, least in ((1, 5), (2, 2), (3, 7)):
            assert any(c.fam == fam and R.geometry(c).ntm >= least and R.geometry(c).ntm % 4 == r for c in ALL), (fam, r)


def _well_formed():
    from inklayer_amd import _lib
    p = _lib.InkGemm()
    p.A, p.W, p.C = 4096, 8192, 16384                   # fake, 16-byte aligned
    p.M, p.N, p.K = 64, 64, 128
    p.lda = p.ldw = 128
    p.ldc = 64
    return p


def test_gemm_argument_contract():
    """ink_gemm_f16 returns 1 (INK_ERR_ARG) before any HIP call for each single violation of its contract; the
    well-formed struct they start from is never passed as it is (it would launch).  Forced variant 45 with K = 64 is
    refused by launch_gemm_pp (fewer granules than the ring holds) before it launches.
    NOT checked by ink_gemm_f16 today: the 16-byte alignment of bias, col_scale and residual (their float4 loads need
    it; ink_conv3x3_f16 does check bias and residual).  ops.gemm only passes torch allocations and row views of them
    with row strides that are multiples of 4.  Tightening that contract would change behaviour and is not done here."""
    from inklayer_amd import _lib
    lib = _lib.lib()
    bad = [dict(M=0), dict(M=-1), dict(N=0), dict(N=-4), dict(K=0), dict(K=-32),
           dict(K=48, lda=48, ldw=48), dict(K=16, lda=16, ldw=16),
           dict(N=62), dict(N=66, ldc=68),
           dict(lda=132), dict(ldw=132), dict(lda=120), dict(ldw=120),
           dict(ldc=66), dict(ldc=60),
           dict(residual=4096, ldr=66), dict(residual=4096, ldr=60), dict(residual=4096, ldr=0),
           dict(A=4104), dict(W=8196), dict(C=16392), dict(A=None), dict(W=None), dict(C=None),
           dict(act=3), dict(act=-1), dict(c_f16=2), dict(c_f16=-1)]
    for kw in bad:
        p = _well_formed()
        for k, v in kw.items():
            setattr(p, k, v)
        assert lib.ink_gemm_f16(ctypes.byref(p), None) == 1, kw
    assert lib.ink_gemm_f16(None, None) == 1
    p = _well_formed()
    p.K = p.lda = p.ldw = 64
    assert R.PP_RING == 4 and p.K // 32 < R.PP_RING
    try:
        assert lib.ink_gemm_set_variant(45) == 0
        assert lib.ink_gemm_f16(ctypes.byref(p), None) == 1
    finally:
        lib.ink_gemm_set_variant(-1)
