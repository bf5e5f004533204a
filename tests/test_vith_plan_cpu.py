"""CPU half of the ViT-H encoder parity net (tests/test_vith_ops_gpu.py runs the kernels):
  * the GEMM dispatch table of the four block projections at B = 1..8 (host functions of the shipped library), and that
    GEMM_BATCHES - the batch sizes the GPU tests run - reach every variant of it;
  * the window gather / scatter map the window kernels are driven by;
  * that every per-element bound of tests/vith_ref.py puts the named mistakes at least 100x outside it, on the
    same data generators the GPU tests use (row / window / head slices of them, in float64 on the CPU)."""
import pytest
import torch

import vith_ref as V

# ink_gemm_query_variant for M = 4096 B: B -> (qkv 3840x1280, proj 1280x1280, lin1 5120x1280, lin2 1280x5120):
# 10 = 16-wave 256x256, 0 = 128x128, 45 = ping-pong 256x320
DISPATCH = {1: (10, 0, 10, 0), 2: (45, 0, 45, 0), 3: (45, 10, 45, 10), 4: (45, 10, 45, 10),
            5: (45, 10, 45, 10), 6: (45, 45, 45, 45), 7: (45, 45, 45, 45), 8: (45, 45, 45, 45)}
GEMM_SHAPES = (("qkv", 3840, 1280), ("proj", 1280, 1280), ("lin1", 5120, 1280), ("lin2", 1280, 5120))
# the batch sizes of test_vith_ops_gpu.test_block_gemm_product_forms (imported there)
GEMM_BATCHES = (1, 3, 6, 8)


def test_gemm_dispatch_table():
    """The variant the shape heuristic picks for every block GEMM at every batch size the engine allows.  A change of
    the heuristic fails here until the GPU cases are revisited."""
    from inklayer_amd import _lib
    lib = _lib.lib()
    for B, variants in DISPATCH.items():
        M = 4096 * B
        got = tuple(int(lib.ink_gemm_query_variant(M, N, K)) for _, N, K in GEMM_SHAPES)
        assert got == variants, (B, got, variants)


def test_gemm_batches_reach_every_variant():
    """GEMM_BATCHES reach, for each of the four projections, every variant the table assigns it, and every row of the
    table's (qkv, proj) pair but B = 2's (45, 0), whose two halves B = 3 (qkv 45) and B = 1 (proj 0) run."""
    for i, (name, _, _) in enumerate(GEMM_SHAPES):
        every = {DISPATCH[B][i] for B in DISPATCH}
        tested = {DISPATCH[B][i] for B in GEMM_BATCHES}
        assert every == tested, (name, every, tested)


@pytest.mark.parametrize("B", [1, 8])
def test_window_map(B):
    """sam.window_rows (the engine's win_map): 25 windows of 196 per image, every token row exactly once, the 804
    padding entries of each image (70 x 70 - 64 x 64) at -1 and only on the right / bottom window edges."""
    from inklayer_amd import sam
    wm = sam.window_rows(B, 64, 14)
    assert wm.dtype == torch.int32 and wm.numel() == B * 4900
    valid = wm[wm >= 0].long()
    assert valid.numel() == B * 4096 and torch.equal(valid.sort().values, torch.arange(B * 4096))
    w = wm.view(B, 5, 5, 14, 14).long()                     # [image, window row, window col, y, x]
    y = (torch.arange(5)[:, None] * 14 + torch.arange(14)[None, :]).view(1, 5, 1, 14, 1)
    x = (torch.arange(5)[:, None] * 14 + torch.arange(14)[None, :]).view(1, 1, 5, 1, 14)
    want = torch.arange(B).view(B, 1, 1, 1, 1) * 4096 + y * 64 + x
    assert torch.equal(w, torch.where((y < 64) & (x < 64), want, torch.full_like(want, -1)))
    assert int((wm < 0).sum()) == 804 * B


# ---------------------------------------------------------------------------------------------------------------
# discrimination of the bounds (float64, CPU)
# ---------------------------------------------------------------------------------------------------------------
@torch.no_grad()
@pytest.mark.parametrize("form", sorted(V.GEMM_FORMS))
def test_gemm_bound_discriminates(form):
    """The first 512 rows (two 256-row tiles) of a block GEMM: a skipped 64-wide K slice, a 256x320 tile swapped with
    its grouped-order neighbour, a dropped bias, and for the in-place forms a residual dropped / added twice and the
    f32 output rounded to f16."""
    g = torch.Generator().manual_seed(1)
    a, w, b, r = V.gemm_data(form, 512, g, "cpu")
    ref, lin, mag = V.gemm_ref(form, a, w, b, r)
    tol = V.gemm_tol(form, ref, lin, mag)
    V.assert_discriminates(V.gemm_ref(form, a, w, b, r, skip_k=640)[0], ref, tol, "K slice 640..703 skipped")
    V.assert_discriminates(V.swap_tiles(ref), ref, tol, "tile (0,0) <-> (1,0)")
    V.assert_discriminates(V.gemm_ref(form, a, w, b, r, drop_bias=True)[0], ref, tol, "bias dropped")
    if r is not None:
        V.assert_discriminates(V.gemm_ref(form, a, w, b, r, res_times=0)[0], ref, tol, "residual dropped")
        V.assert_discriminates(V.gemm_ref(form, a, w, b, r, res_times=2)[0], ref, tol, "residual added twice")
        # an f32 stream rounded to f16 is caught, not by 100x: half an f16 ulp is 2^13 / (K/32 + 7) times the
        # accumulation term on a residual-dominated element (~49x at K = 5120), less where the products dominate
        V.assert_discriminates(V.f16_stream(ref), ref, tol, "f32 stream rounded to f16", factor=2)


@torch.no_grad()
def test_layernorm_bound_discriminates():
    """layernorm_tol on the hard rows of vith_ref.layernorm_data: a one-pass f32 variance (E[x^2] - mean^2) on the
    rows at |mean| / std = 3000, and eps left out of the sqrt on the constant rows (0 * inf: NaN)."""
    x, gamma, beta = V.layernorm_data(64, torch.Generator().manual_seed(7), "cpu")
    ref = V.layernorm_ref(x, gamma, beta)
    tol = V.layernorm_tol(x, gamma, beta, ref)
    for mistake, rows in (("one-pass", slice(20, 24)), ("no-eps", slice(16, 20))):
        wrong = V.layernorm_wrong(x, gamma, beta, mistake)
        V.assert_discriminates(wrong[rows], ref[rows], tol[rows], mistake)


def _relpos_case(S, f16_out):
    from inklayer_amd import sam
    g = torch.Generator().manual_seed(2)
    q = V.qkv_data(1, g, "cpu")[:, :V.D]
    Rh, Rw = V.rel_tables(S, g, "cpu")
    qrows = sam.window_rows(1, 64, 14).view(25, 196) if S == 14 else torch.arange(4096, dtype=torch.int32).view(1, 4096)
    rh, rw, mh, mw, qa = V.relpos_ref(q, Rh, Rw, S, qrows)
    tol_h, tol_w = V.relpos_tol(rh, mh, qa, f16_out), V.relpos_tol(rw, mw, qa, f16_out)
    return q, Rh, Rw, qrows, rh, rw, tol_h, tol_w


@torch.no_grad()
@pytest.mark.parametrize("S,f16_out", [(14, True), (64, False), (64, True)])
def test_relpos_bound_discriminates(S, f16_out):
    """relpos_bias, one image, all 16 heads: rel_h / rel_w swapped, k - q instead of q - k, the q of head h + 1, and
    the scale multiplied instead of divided / omitted each move some term by >= 100x its bound."""
    q, Rh, Rw, qrows, rh, rw, tol_h, tol_w = _relpos_case(S, f16_out)
    ref = torch.cat([rh, rw], -1)
    tol = torch.cat([tol_h, tol_w], -1)
    for what, kw in (("rel_h / rel_w swapped", dict(swap=True)), ("k - q indexing", dict(flip=True)),
                     ("q of head h + 1", dict(head_shift=1)), ("scale multiplied", dict(scale_mode="mul")),
                     ("scale omitted", dict(scale_mode="none"))):
        wr = V.relpos_ref(q, Rh, Rw, S, qrows, **kw)
        V.assert_discriminates(torch.cat([wr[0], wr[1]], -1), ref, tol, what)


@torch.no_grad()
def test_window_attention_bound_discriminates():
    """win4 at one image (25 windows x 16 heads): a key of the neighbouring window, zero instead of pad_k, the K / V
    of the previous (window, head) item and a dropped key, over the real query rows."""
    from inklayer_amd import sam
    g = torch.Generator().manual_seed(3)
    qkv = V.qkv_data(1, g, "cpu")
    Rh, Rw = V.rel_tables(14, g, "cpu")
    wm = sam.window_rows(1, 64, 14).view(25, 196)
    rh, rw, _, _, _ = V.relpos_ref(qkv[:, :V.D], Rh, Rw, 14, wm)
    aug = torch.cat([rh, rw, torch.zeros(*rh.shape[:-1], 4, dtype=V.F64)], -1).half()
    pad_k, pad_v = torch.randn(V.D, generator=g).half(), torch.randn(V.D, generator=g).half()
    win = torch.arange(25)
    q, k, v, bmag, P, s, o, valid = V.win_item_ref(qkv, aug, wm, pad_k, pad_v, win)
    tol = V.attn_tol(q, k, v, bmag, P, s, o)
    m = valid[:, None, :, None]
    for what, kw in (("key 0 of the neighbouring window", dict(neighbour_key=True)),
                     ("zero instead of pad_k", dict(zero_pad_k=True)), ("K / V of the previous item", dict(stale_kv=True)),
                     ("key 195 dropped", dict(drop_key=True))):
        wrong = V.win_item_ref(qkv, aug, wm, pad_k, pad_v, win, **kw)[6]
        V.assert_discriminates(torch.where(m, wrong, o), o, tol, what)


@torch.no_grad()
def test_global_attention_bound_discriminates():
    """glob4, head 0 of image 0 with f16 rel tables: a dropped 64-key tile, the last query tile with the rel rows of
    the one before, rel_h / rel_w swapped."""
    g = torch.Generator().manual_seed(4)
    qkv = V.qkv_data(1, g, "cpu")
    Rh, Rw = V.rel_tables(64, g, "cpu")
    rh, rw, _, _, _ = V.relpos_ref(qkv[:, :V.D], Rh, Rw, 64, torch.arange(4096).view(1, 4096))
    rh, rw = rh[0, 0].half().double(), rw[0, 0].half().double()
    q, k, v = (qkv[:, i * V.D:i * V.D + V.HD].double() for i in range(3))
    o, P, s, bmag = V.glob_ref(q, k, v, rh, rw)
    tol = V.attn_tol(q, k, v, bmag, P, s, o)
    for what, kw in (("key tile 37 dropped", dict(drop_tile=37)), ("last query tile: rel rows of the tile before",
                                                                    dict(last_tile_rows=True)),
                     ("rel_h / rel_w swapped", dict(swap=True))):
        V.assert_discriminates(V.glob_ref(q, k, v, rh, rw, **kw)[0], o, tol, what)

