"""CPU half of the ink_flash_attn parity net (tests/test_flash_attn_edges_gpu.py runs the kernels):
  * the coverage plan: every flash_attn_kernel instantiation in inklayer_amd/csrc/attention.hip (parsed out of the source)
    and the dedicated kernels, with the branches each must be driven through, is hit by a row of flash_attn_ref.CASES
    or by an existing strict test named in EXISTING (checked by ast to exist);
  * the yardstick: on one small case per instance the float64 reference is inside its own bound and every applicable
    named mistake lands >= 100x outside it; the planted late maxima do rise where branches() says they do;
  * the argument contract: ink_flash_attn refuses, before any launch, what instance_of() maps to None;
  * the header's sentence on the row tables."""
import ast
import ctypes
import re
from pathlib import Path

import pytest
import torch

import flash_attn_ref as R

ROOT = Path(__file__).resolve().parent.parent
INK_ERR_ARG = 1

# every instantiation in attention.hip, as instance_of() names it
GENERIC = {(80, 1, 8, False), (80, 2, 7, True), (64, 1, 8, False), (64, 2, 7, True), (80, 0, 4, False), (64, 0, 4, False),
           (32, 0, 1, False), (32, 0, 4, False), (32, 3, 2, False), (16, 0, 1, False), (16, 0, 4, False)}
DEDICATED = {"win4", "win4_tok", "glob4"}

# what is already held strictly elsewhere (production shapes): instance -> "file::test"
EXISTING = {
    (64, 0, 4, False): "test_depth_ops_gpu.py::test_flash_attn_hd64_ragged_tiles",
    (32, 3, 2, False): "test_detector_ops_gpu.py::test_flash_attn_swin_windows",
    (64, 2, 7, True): "test_vit_hd64_ops_gpu.py::test_window_attention_hd64",
    (64, 1, 8, False): "test_vit_hd64_ops_gpu.py::test_global_attention_hd64",
    "win4_tok": "test_vith_ops_gpu.py::test_window_attention_persistent_walk",
    "glob4": "test_vith_ops_gpu.py::test_global_attention_b2",
}

_STREAM1 = ["tiles=1", "tiles>=3", "tail=full", "n_q=1", "ragged_q", "idle_waves", "nqb=1", "nqb>1",
            "grid_not_multiple_of_8", "kv_rows_shared", "rescale_late", "ldo>width", "ldo%8=4"]
_ALLKV = ["tiles>=3", "half_tail", "full_tail", "n_q=1", "ragged_q", "idle_waves", "nqb=1", "nqb>1",
          "persistent_multi_block", "window_change_in_walk", "tok_rows", "pad_keys", "all_pad_wave", "packed_qkv",
          "rescale_late", "ldo>width", "ldo%8=4"]
_BRANCHES = {
    (16, 0, 1, False): ["tiles=1", "tail=1", "tail=33..63", "tail=full", "ragged_q", "n_q=1", "n_k=1", "nqb=1", "ldo>width"],
    (16, 0, 4, False): ["tiles=2", "tiles>=3", "tail=1", "tail<=32", "tail=full", "ragged_q", "idle_waves", "nqb=1", "nqb>1",
                        "kv_rows_shared", "rescale_late", "ldo>width"],
    (32, 0, 1, False): ["tiles=1", "tiles=2", "tiles>=3", "tail=1", "n_k=1", "ragged_q", "nqb=1", "rescale_late", "ldo>width"],
    (32, 0, 4, False): ["tiles=1", "tiles>=3", "tail<=32", "tail=33..63", "ragged_q", "idle_waves", "nqb=1", "nqb>1",
                        "q_rows_shared", "rescale_late", "ldo>width"],
    (80, 0, 4, False): ["tiles=1", "tiles>=3", "tail<=32", "tail=33..63", "tail=full", "ragged_q", "idle_waves", "nqb=1",
                        "nqb>1", "packed_qkv", "rescale_late", "ldo>width", "ldo%8=4"],
    (64, 0, 4, False): ["tiles=1", "tiles>=3", "tail<=32", "tail=33..63", "ragged_q", "idle_waves", "nqb>1", "ldo%8=4"],
    (80, 1, 8, False): _STREAM1,
    (64, 1, 8, False): _STREAM1,
    (80, 2, 7, True): _ALLKV,
    (64, 2, 7, True): _ALLKV,
    "win4": ["tail=1", "tail<=32", "n_q=1", "ragged_q", "idle_waves", "q_rows_shared", "kv_rows_shared", "rescale_late",
             "ldo>width", "ldo%8=4"],
    "win4_tok": ["tok_rows", "pad_keys", "all_pad_wave", "persistent_multi_block", "window_change_in_walk", "ldo>width",
                 "ldo%8=4"],
    "glob4": ["tiles>=3", "q_rows_shared", "kv_rows_shared", "grid_not_multiple_of_8", "ldo>width", "ldo%8=4"],
}
REQUIRED = [(inst, br) for inst, brs in _BRANCHES.items() for br in brs]


def _instantiations():
    """Every INK_FA( / INK_FA_X( use in ink_flash_attn (the #define lines left out), as instance tuples."""
    src = (ROOT / "inklayer_amd" / "csrc" / "attention.hip").read_text()
    body = "\n".join(line for line in src.splitlines() if not line.lstrip().startswith("#define"))
    found = [(int(a), int(b), int(c), False) for a, b, c in re.findall(r"INK_FA\((\d+),\s*(\d+),\s*(\d+)\)", body)]
    found += [(int(a), int(b), int(c), d == "true")
              for a, b, c, d in re.findall(r"INK_FA_X\((\d+),\s*(\d+),\s*(\d+),\s*(true|false)\)", body)]
    return found


def covered(cases):
    hit = {}
    for c in cases:
        hit.setdefault(R.case_instance(c), set()).update(R.branches(c))
    return hit


def missing(cases):
    """What of the plan a case table leaves open: instances with neither a case nor an EXISTING entry, REQUIRED pairs no
    case drives."""
    hit = covered(cases)
    gaps = [inst for inst in GENERIC | DEDICATED if inst not in hit and inst not in EXISTING]
    gaps += [(inst, br) for inst, br in REQUIRED if br not in hit.get(inst, ())]
    return gaps


def test_every_instantiation_is_listed():
    """The instantiations parsed out of attention.hip are exactly GENERIC, each once: a new INK_FA( line fails here until
    it has a place in the plan."""
    found = _instantiations()
    assert len(found) == len(set(found)) and set(found) == GENERIC, sorted(set(found) ^ GENERIC)
    assert set(_BRANCHES) | set(EXISTING) == GENERIC | DEDICATED


def test_cases_cover_the_plan():
    """Every REQUIRED (instance, branch) pair is driven by a case; no case is refused; deleting the only case of an
    instance opens a gap (a twelfth instantiation fails test_every_instantiation_is_listed)."""
    assert all(R.case_instance(c) is not None for c in R.CASES)
    assert missing(R.CASES) == []
    for inst in _BRANCHES:
        rest = [c for c in R.CASES if R.case_instance(c) != inst]
        assert missing(rest), inst
    one = [c for c in R.CASES if R.case_instance(c) == (16, 0, 1, False)]
    for c in one:                                        # each of the three <16, 0, 1> rows is the only one for some branch
        assert missing([x for x in R.CASES if x is not c]), c.name


def test_existing_tests_exist():
    for inst, where in EXISTING.items():
        fname, test = where.split("::")
        tree = ast.parse((ROOT / "tests" / fname).read_text())
        assert any(isinstance(n, ast.FunctionDef) and n.name == test for n in tree.body), where


def test_minimum_contents():
    """The shapes the plan names, per instance."""
    shapes = {}
    for c in R.CASES:
        shapes.setdefault(R.case_instance(c), set()).add((c.n_q, c.n_k))
    assert {(7, 40), (32, 64), (1, 1)} <= shapes[(16, 0, 1, False)]
    assert {(33, 65), (100, 77), (129, 192)} <= shapes[(16, 0, 4, False)]
    assert {(32, 65), (5, 1), (20, 129)} <= shapes[(32, 0, 1, False)]
    assert {(33, 33), (900, 900), (130, 31)} <= shapes[(32, 0, 4, False)]
    assert {(70, 33), (129, 192), (196, 196)} <= shapes[(80, 0, 4, False)]
    for hd in (80, 64):
        s1 = shapes[(hd, 1, 8, False)]
        assert {k for _, k in s1} == {64, 192, 1024} and {q for q, _ in s1} == {1, 255, 257, 320}
        s2 = [c for c in R.CASES if R.case_instance(c) == (hd, 2, 7, True)]
        assert {(c.grid_w, c.n_k) for c in s2 if not c.tok} == {(12, 144), (14, 192), (15, 209), (15, 225), (16, 256)}
        assert {c.n_q for c in s2 if not c.tok and c.n_q != c.n_k} == {1, 100}
        assert len([c for c in s2 if c.tok]) >= 2 and any(c.tok and c.n_q == 256 for c in s2)
        assert any(c.B * c.H > R.N_CUS for c in s2)
    w = [c for c in R.CASES if R.case_instance(c) == "win4"]
    assert {c.n_k for c in w} >= {193, 208} and {c.n_q for c in w} == {1, 100, 256} and all(c.n_q != c.n_k for c in w)
    assert {c.grid_w for c in w if c.n_k == 208} == {15}
    assert any(c.q_share for c in w) and any(c.kv_share for c in w)
    assert (256, 256, True, True) in [(c.n_q, c.n_k, c.q_share, c.kv_share) for c in R.CASES if R.case_instance(c) == "glob4"]
    kvs = next(c for c in R.CASES if c.kv_share and c.hd == 16)
    assert kvs.B == 3 and R.IMG_OF == (1, 0, 1)


def test_window_walks():
    """The tok_rows cases make more items than workgroups with 3 heads, so some workgroup's walk crosses a window; the
    bottom windows of the token map have waves of padded queries only."""
    for c in R.CASES:
        if c.tok and c.B > 4:                              # (the one-image case is there for its O stride)
            br = R.branches(c)
            assert {"persistent_multi_block", "window_change_in_walk", "pad_keys", "all_pad_wave"} <= br, c.name
            rows, n = R.tok_table(c)
            assert sorted(rows[rows >= 0].tolist()) == list(range(n))          # every token in exactly one window


# ---------------------------------------------------------------------------------------------------------------
# yardstick (float64, CPU)
# ---------------------------------------------------------------------------------------------------------------
YARD = [c for c in R.CASES if c.yard]


def test_yardstick_reaches_every_family():
    assert {R.case_instance(c) for c in YARD} == set(_BRANCHES)


@torch.no_grad()
@pytest.mark.parametrize("case", YARD, ids=[c.name for c in YARD])
def test_bound_discriminates(case):
    """The reference is within its own bound (error 0, bound > 0 everywhere it writes); every applicable mistake is
    >= 100x outside.  The planted rows do what make_data says: the last key is the row maximum of the lastkey queries,
    key 64 t + 5 the row maximum of tile t's late query, in every entry whose row is a real query."""
    d = R.make_data(case)
    ref, tol = R.expected(d)
    w = ~ref.isnan()
    assert (tol[w] > 0).all() and R.buf_within(ref, ref, tol, case.name) == 0.0
    names = []
    for what, wrong in R.mistakes(d):
        m = R.buf_discrimination(wrong, ref, tol)
        print(f"  {case.name}: {what}: {m:.0f}x the bound")
        assert m >= 100, (what, m)
        names.append(what)
    assert ("scale omitted" in names) == (case.n_k > 1)
    assert ("O written at the shared Q rows instead of densely" in names) == case.q_share
    assert ("kv_batch_rows ignored" in names) == case.kv_share and ("padded query stored" in names) == case.tok
    assert ("rel_h and rel_w swapped" in names) == (case.mode in (1, 2))
    s, valid = R.reference(d)[2], R.operands(d)[3]
    T = -(-case.n_k // 64)
    for b in range(case.B):
        blk = R.IMG_OF[b] if case.q_share else b
        lastkey, _, late = R.roles(case.n_q, T, blk)
        for r in lastkey:
            if valid[b, r] and case.n_k > 1 and (not case.tok or valid[b, case.n_k - 1]):     # (a padded key is pad_k)
                assert (s[b, :, r].argmax(-1) == case.n_k - 1).all(), (b, r)
        for t, r in late.items():
            if valid[b, r] and R.late_key(t, case.n_k) is not None and (not case.tok or valid[b, R.late_key(t, case.n_k)]):
                assert (s[b, :, r].argmax(-1) == R.late_key(t, case.n_k)).all(), (b, t, r)


# ---------------------------------------------------------------------------------------------------------------
# argument contract
# ---------------------------------------------------------------------------------------------------------------
def _call(**kw):
    """ink_flash_attn on a well-formed head_dim-80 mode-0 call with fake, aligned, non-null pointers; fields from kw."""
    from inklayer_amd import _lib
    p = _lib.InkAttn()
    p.Q = p.K = p.V = p.O = 4096
    p.ldq = p.ldk = p.ldv = 3 * 240 + 8
    p.ldo = 240
    p.n_batch, p.n_heads, p.n_q, p.n_k, p.head_dim, p.scale = 2, 3, 100, 100, 80, 0.1
    p.rel_h = p.rel_w = p.rel_aug = p.dense_bias = p.pad_k = p.pad_v = 4096
    for k, v in kw.items():
        setattr(p, k, v)
    return _lib.lib().ink_flash_attn(ctypes.byref(p), None)


WIN = dict(bias_mode=2, grid_w=14, n_q=196, n_k=196)
GLOB = dict(bias_mode=1, grid_w=64, n_q=320, n_k=1024)
REFUSED = {
    "pair_16_1": dict(head_dim=16, **GLOB), "pair_16_2": dict(head_dim=16, **WIN), "pair_32_1": dict(head_dim=32, **GLOB),
    "pair_32_2": dict(head_dim=32, **WIN), "pair_80_3": dict(head_dim=80, bias_mode=3, n_q=49, n_k=49),
    "pair_64_3": dict(head_dim=64, bias_mode=3, n_q=49, n_k=49), "pair_48_0": dict(head_dim=48),
    "tok_mode0": dict(tok_rows=4096), "tok_mode1": dict(tok_rows=4096, **GLOB),
    "tok_mode3": dict(head_dim=32, bias_mode=3, n_q=49, n_k=49, tok_rows=4096),
    "tok_nq_ne_nk": dict(**{**WIN, "n_q": 100}, tok_rows=4096),
    "mode3_nk": dict(head_dim=32, bias_mode=3, n_q=49, n_k=65), "mode3_nq": dict(head_dim=32, bias_mode=3, n_q=65, n_k=49),
    "win_nk_gt_grid": dict(**{**WIN, "n_k": 197}), "win_grid17": dict(bias_mode=2, grid_w=17, n_q=256, n_k=256),
    "win_nk257": dict(bias_mode=2, grid_w=16, n_q=100, n_k=257),
    "win64_nk_gt_grid": dict(head_dim=64, **{**WIN, "n_k": 197}),
    "relf16_streamed80": dict(rel_f16=1, **GLOB), "relf16_64": dict(head_dim=64, rel_f16=1, **GLOB),
    "glob_grid": dict(**{**GLOB, "grid_w": 32}), "glob_nk_ragged": dict(**{**GLOB, "n_k": 1000}),
    "glob80_nk_8192": dict(**{**GLOB, "n_k": 8192}), "glob64_nk_8192": dict(head_dim=64, **{**GLOB, "n_k": 8192}),
    "ldo_mod4": dict(ldo=242),
}


@pytest.mark.parametrize("name", sorted(REFUSED))
def test_refused_before_launch(name):
    """INK_ERR_ARG for each, with pointers that are never dereferenced on the host; instance_of() says None for the
    same numbers.  (Mode 3's limits with a mask, the pointer alignments and the missing tables / pad rows are asserted in
    test_swin_plan_cpu.py, test_cabi.py and test_sam_models_cpu.py.)"""
    kw = REFUSED[name]
    assert _call(**kw) == INK_ERR_ARG
    a = dict(head_dim=80, bias_mode=0, n_batch=2, n_q=100, n_k=100, grid_w=0, ldo=240, tok_rows=0, rel_f16=0)
    a.update({k: v for k, v in kw.items() if k in a})
    assert R.instance_of(a["head_dim"], a["bias_mode"], a["n_batch"], a["n_q"], a["n_k"], a["grid_w"], a["ldo"],
                         bool(a["tok_rows"]), bool(a["rel_f16"])) is None


def test_input_strides_refused():
    assert _call(ldq=3 * 240 + 4) == INK_ERR_ARG and _call(ldk=3 * 240 + 4) == INK_ERR_ARG and _call(ldv=3 * 240 + 4) == INK_ERR_ARG


def test_instance_of_accepts_the_supported_pairs():
    """The nine supported (head_dim, bias_mode) pairs of the header, and the shape thresholds between kernels."""
    hdr = (ROOT / "include" / "inklayer_hip.h").read_text()
    m = re.search(r"Supported \(head_dim, bias_mode\) pairs:(.*?);", hdr, re.S)
    pairs = {(int(a), int(b)) for a, b in re.findall(r"\((\d+), (\d+)\)", m.group(1))}
    assert pairs == {(i[0], i[1]) for i in GENERIC}
    f = R.instance_of
    assert f(32, 0, 1, 32, 9) == (32, 0, 1, False) and f(32, 0, 1, 33, 9) == (32, 0, 4, False)
    assert f(16, 0, 1, 32, 9) == (16, 0, 1, False) and f(16, 0, 1, 33, 9) == (16, 0, 4, False)
    assert f(80, 2, 1, 196, 192, 14) == (80, 2, 7, True) and f(80, 2, 1, 196, 193, 14) == "win4"
    assert f(80, 2, 1, 208, 208, 15, tok_rows=True) == "win4_tok" and f(80, 2, 1, 209, 209, 15) == (80, 2, 7, True)
    assert f(80, 2, 1, 257, 196, 14) == (80, 2, 7, True) and f(64, 2, 1, 196, 196, 14) == (64, 2, 7, True)
    assert f(80, 2, 4096, 256, 196, 14, ldo=1280) == (80, 2, 7, True)          # dense O beyond win4's 2 GiB descriptor
    assert f(80, 1, 1, 256, 256, 64) == "glob4" and f(80, 1, 1, 256, 192, 64) == (80, 1, 8, False)
    assert f(80, 1, 1, 255, 256, 64) == (80, 1, 8, False) and f(80, 1, 1, 4096, 4096, 64, rel_f16=True) == "glob4"
    assert f(64, 1, 1, 4096, 4096, 64) == (64, 1, 8, False)


def test_header_says_o_is_dense():
    """include/inklayer_hip.h on the row tables: they give the first row in Q and in K/V; O is dense unless tok_rows
    scatters it (the kernels' b * n_q + i; test_flash_attn_edges_gpu.py holds the behaviour)."""
    hdr = re.sub(r"\s*\n \*\s*", " ", (ROOT / "include" / "inklayer_hip.h").read_text())
    assert "first row of batch entry b in Q and in K/V" in hdr and "in Q/O" not in hdr
    assert "O is always dense: row b*n_q + i" in hdr
