"""CPU half of the depth-engine parity net (tests/test_depth_ops_gpu.py runs the kernels):
  * the GEMM dispatch table of every GEMM form of inklayer_amd/depth.py at 37 x 37 and 37 x 49 patches (host function of
    the shipped library);
  * the token counts N = 37 k + 1 of every input width, their ragged key tile and last query block, and that the GPU
    attention cases reach every kind of tail;
  * that every per-element bound of tests/depth_ops_ref.py puts the named mistakes at least 100x outside it, on the same
    data generators the GPU tests use (row / head slices of them, in float64 on the CPU)."""
import pytest
import torch

import depth_ops_ref as R
import vith_ref as V

# ink_gemm_query_variant per form, the same at 37 x 37 and 37 x 49: 0 = 128x128x64 tile, 32 = 128x128x32 (K % 64 != 0)
DISPATCH = {"pe": 32, "qkv": 0, "proj": 0, "fc1": 0, "fc2": 0, "up0": 32, "rn0": 32, "down3": 0, "rcu1": 0, "rcu2": 0,
            "oc1": 0, "oc2": 0, "oc3": 32}
# N -> (keys in the last 64-key tile, valid rows of the last 128-query block)
TAILS = {1370: (26, 90), 1814: (22, 22), 1407: (63, 127), 1518: (46, 110), 1888: (32, 96), 2369: (1, 65), 3072: (64, 128)}


def test_gemm_dispatch_table():
    """The variant the shape heuristic picks for every engine GEMM at both input sizes: only the two 128x128 families,
    the K step 32 one for pe (K = 1824), up0 (96), rn0 (864) and oc3 (32).  A change of the heuristic fails here until
    the GPU cases are revisited."""
    from inklayer_amd import _lib
    lib = _lib.lib()
    assert set(DISPATCH) == set(R.DEPTH_GEMMS)
    for ph, pw in R.DEPTH_SIZES:
        for name in R.DEPTH_GEMMS:
            M, N, K = R.gemm_shape(name, ph, pw)
            got = int(lib.ink_gemm_query_variant(M, N, K))
            assert got == DISPATCH[name], (name, (ph, pw), (M, N, K), got)
            assert K % 32 == 0 and R.gemm_bk(name) == (32 if got == 32 else 64)
    assert {n for n, v in DISPATCH.items() if v == 32} == {"pe", "up0", "rn0", "oc3"}
    assert R.gemm_shape("pe", 37, 37) == (1369, 768, 1824) and R.gemm_shape("oc3", 37, 37) == (268324, 4, 32)
    assert R.gemm_shape("rn0", 37, 37) == (21904, 128, 864) and R.gemm_shape("down3", 37, 37) == (361, 768, 6912)
    assert R.gemm_shape("oc1", 37, 37) == (87616, 64, 1152) and R.gemm_shape("oc2", 37, 49)[0] == 518 * 686


def test_token_count_table():
    """N = 37 k + 1 for k = 37..83 (input widths 518..1162): N is a multiple of 64 only at k = 83, so every realistic
    forward runs the ragged-key mask.  The GPU cases cover the two production sizes, a 63-key tail, a tail that masks
    both 32-key halves (46), a tail of exactly 32 (the second half all masked), a 1-key tail with a 65-row last query
    block, and no tail."""
    table = {37 * k + 1: R.token_tail(37 * k + 1) for k in range(37, 84)}
    assert [n for n, (tail, _) in table.items() if tail == 64] == [3072]
    assert set(R.ATTN_TOKENS) <= set(table) and set(R.ATTN_B2) <= set(R.ATTN_TOKENS)
    assert {n: table[n] for n in R.ATTN_TOKENS} == TAILS
    tails = {table[n][0] for n in R.ATTN_TOKENS}
    assert {1, 32, 63, 64} <= tails and any(32 < t < 63 for t in tails) and any(1 < t < 32 for t in tails)
    assert any(q == 65 for _, q in (table[n] for n in R.ATTN_TOKENS))


# ---------------------------------------------------------------------------------------------------------------
# discrimination of the bounds (float64, CPU)
# ---------------------------------------------------------------------------------------------------------------
def _attn_rows(N):
    return sorted(set(range(32)) | set(range(592, 608)) | set(range(N - 130, N)))


@torch.no_grad()
@pytest.mark.parametrize("N", R.ATTN_TOKENS)
def test_attention_bound_discriminates(N):
    """Heads 0..2 of one batch entry, the first 32, 16 middle and the last 130 query rows against all N keys: a dropped
    last key, an unmasked tail, the upper 32-key half of the last tile dropped, the V of the next head and an omitted
    scale each move some element >= 100x its bound.  Needed for that: the probe rows and the planted last key of
    depth_ops_ref.attn64_data (with Gaussian rows alone an unmasked tail stays within 3x the bound)."""
    qkv = R.attn64_data(N, 1, torch.Generator().manual_seed(N), "cpu")
    rows = _attn_rows(N)
    q, k, v = R.attn64_split(qkv, N, 0, heads=slice(0, 3), rows=rows)
    o, P, s = R.attn64_ref(q, k, v)
    tol = R.attn64_tol(q, k, v, P, s, o)
    for r in R.lastkey_rows(N):                 # the planted last key is the row maximum, by a margin
        sr = s[:, rows.index(r)]
        assert (sr.argmax(-1) == N - 1).all() and (sr[:, N - 1] - sr[:, :N - 1].amax(-1)).min() > 8
    names = []
    for what, wrong in R.attn64_mistakes(q, k, v, N):
        m = R.assert_discriminates(wrong, o, tol, what)
        print(f"  attention N={N}: {what}: {m:.0f}x the bound")
        names.append(what)
    tail = R.token_tail(N)[0]
    assert ("tail unmasked" in names) == (tail < 64) and ("keys 32..63 of the last tile dropped" in names) == (tail > 32)


@torch.no_grad()
@pytest.mark.parametrize("N", R.ATTN_B2)
def test_attention_batch_mixup_discriminates(N):
    """B = 2: the queries of entry 1 against the K / V of entry 0."""
    qkv = R.attn64_data(N, 2, torch.Generator().manual_seed(N + 1), "cpu")
    rows = _attn_rows(N)
    q, k, v = R.attn64_split(qkv, N, 1, heads=slice(0, 3), rows=rows)
    _, k0, v0 = R.attn64_split(qkv, N, 0, heads=slice(0, 3), rows=rows)
    o, P, s = R.attn64_ref(q, k, v)
    m = R.assert_discriminates(R.attn64_ref(q, k0, v0)[0], o, R.attn64_tol(q, k, v, P, s, o), "K / V of batch entry 0")
    print(f"  attention N={N}: K / V of batch entry 0 used for entry 1: {m:.0f}x the bound")


@torch.no_grad()
@pytest.mark.parametrize("name", sorted(R.DEPTH_GEMMS))
def test_gemm_bound_discriminates(name):
    """The first 256 rows of every engine GEMM form: the mistakes of depth_ops_ref.gemm_mistakes.  pe needed the coherent
    rounding errors of gemm_data's first 8 rows / columns for the plain-f16 product to leave the bound by 100x."""
    d = R.gemm_data(name, 256, torch.Generator().manual_seed(5), "cpu")
    ref, lin, mag = R.gemm_ref(name, d)
    tol = R.gemm_tol(name, d, ref, lin, mag)
    assert (tol > 0).all()
    for what, wrong, factor in R.gemm_mistakes(name, d):
        m = R.assert_discriminates(wrong, ref, tol, what, factor=factor)
        print(f"  {name}: {what}: {m:.0f}x the bound")


@torch.no_grad()
def test_layernorm_bound_discriminates_768():
    """vith_ref.layernorm_tol at C = 768 (3 float4 loads per lane instead of 5: the bound's 24 roundings still hold) on
    the hard rows of layernorm_data: a one-pass f32 variance and a dropped eps."""
    x, gamma, beta = V.layernorm_data(64, torch.Generator().manual_seed(7), "cpu", R.DD)
    assert x.shape == (64, 768)
    ref = V.layernorm_ref(x, gamma, beta)
    tol = V.layernorm_tol(x, gamma, beta, ref)
    for mistake, rows in (("one-pass", slice(20, 24)), ("no-eps", slice(16, 20))):
        V.assert_discriminates(V.layernorm_wrong(x, gamma, beta, mistake)[rows], ref[rows], tol[rows], mistake)


@torch.no_grad()
@pytest.mark.parametrize("f16_out", [False, True])
def test_resize_bound_discriminates(f16_out):
    """19 x 25 x 128 -> 37 x 49: align_corners = False leaves resize_tol by >= 100x; an f32 result rounded to f16 leaves
    the f32 bound."""
    h, w, H, W = 19, 25, 37, 49
    x = torch.randn(h * w, 128, generator=torch.Generator().manual_seed(3))
    ref = R.resize_ref(x, h, w, H, W)
    tol = R.resize_tol(x, h, w, H, W, ref, f16_out)
    R.assert_discriminates(R.resize_ref(x, h, w, H, W, align_corners=False), ref, tol, "align_corners = False")
    if not f16_out:
        R.assert_discriminates(ref.half().double(), ref, tol, "f32 result rounded to f16")
    # the float64 interpolation itself is within the f32 bound of its own f32 evaluation (the bound is not vacuous)
    y32 = torch.nn.functional.interpolate(x.view(1, h, w, 128).permute(0, 3, 1, 2), (H, W), mode="bilinear",
                                          align_corners=True).permute(0, 2, 3, 1).reshape(H * W, 128)
    R.assert_within((y32.half() if f16_out else y32).double(), ref, tol, "torch f32 bilinear")
