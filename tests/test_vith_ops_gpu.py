"""float64 parity of the SAM ViT-H encoder kernels at the shapes production runs: the four block GEMMs at every
dispatch family (B = 1, 3, 6, 8), layernorm_rows at C = 1280, relpos_bias in its three forms, the window kernel's
persistent walk (B = 1 and 8, 16 heads), the global kernel (16 heads, f32 and f16 rel tables), the LayerNorm fold fed
by 20 statistics parts, and one encoder block of each kind through the engine.  References and per-element bounds are
in tests/vith_ref.py (tests/test_vith_plan_cpu.py shows on the CPU that named mistakes land >= 100x outside them; the
same checks are repeated here on the full data).  Outputs are NaN-prefilled with guard rows / columns.  GPU box only."""
import numpy as np
import pytest
import torch

import vith_ref as V
from test_vith_plan_cpu import DISPATCH, GEMM_BATCHES, GEMM_SHAPES

pytestmark = pytest.mark.gpu

NAN = float("nan")


def _gen(dev, seed):
    return torch.Generator(device=dev).manual_seed(seed)


def _report(what, worst):
    print(f"  {what}: worst error {worst:.3f}x the bound")


# ---------------------------------------------------------------------------------------------------------------
# block GEMMs in their product forms
# ---------------------------------------------------------------------------------------------------------------
@torch.no_grad()
@pytest.mark.parametrize("form", sorted(V.GEMM_FORMS))
@pytest.mark.parametrize("B", GEMM_BATCHES)
def test_block_gemm_product_forms(dev, B, form):
    """The block projection at M = 4096 B as SamEngine._blocks calls it (variant from DISPATCH): qkv f16 out at
    ld = 3840 with 256 NaN guard rows below; proj f32 with residual = out = x in place (NaN guard rows); lin1 GELU f16
    out at ldc = 5184 (64 NaN guard columns) + guard rows; lin2 K = 5120 in place.  Bound: vith_ref.gemm_tol."""
    from inklayer_amd import _lib, ops
    i = [n for n, _, _ in GEMM_SHAPES].index(form)
    N, K, act, f16, inplace = V.GEMM_FORMS[form]
    M = 4096 * B
    assert int(_lib.lib().ink_gemm_query_variant(M, N, K)) == DISPATCH[B][i]
    a, w, b, r = V.gemm_data(form, M, _gen(dev, 100 * B + i), dev)
    if inplace:
        buf = torch.full((M + 64, N), NAN, device=dev)
        buf[:M] = r
        out = buf[:M]
        ops.gemm(a, w, b, residual=out, out=out)
    else:
        ldc = N + 64 if form == "lin1" else N
        buf = torch.full((M + 256, ldc), NAN, dtype=V.F16, device=dev)
        out = buf[:M, :N]
        assert ops.gemm(a, w, b, act=act, out=out).data_ptr() == buf.data_ptr()
    assert buf[M:].isnan().all() and buf[:M, N:].isnan().all()
    ref, lin, mag = V.gemm_ref(form, a, w, b, r)
    tol = V.gemm_tol(form, ref, lin, mag)
    worst = V.assert_within(out.double(), ref, tol, f"{form} B={B}")
    _report(f"{form} B={B} variant {DISPATCH[B][i]}", worst)
    V.assert_discriminates(V.gemm_ref(form, a, w, b, r, skip_k=K // 2)[0], ref, tol, "K slice skipped")
    V.assert_discriminates(V.swap_tiles(ref), ref, tol, "tile swapped with its grouped neighbour")
    V.assert_discriminates(V.gemm_ref(form, a, w, b, r, drop_bias=True)[0], ref, tol, "bias dropped")
    if inplace:
        V.assert_discriminates(V.gemm_ref(form, a, w, b, r, res_times=0)[0], ref, tol, "residual dropped")
        V.assert_discriminates(V.gemm_ref(form, a, w, b, r, res_times=2)[0], ref, tol, "residual added twice")
        m = V.assert_discriminates(V.f16_stream(ref), ref, tol, "f32 stream rounded to f16", factor=2)
        print(f"  {form} B={B}: f32 stream rounded to f16 lands {m:.1f}x outside the bound")


# ---------------------------------------------------------------------------------------------------------------
# layernorm_rows at C = 1280 (the f16 operand of qkv and lin1)
# ---------------------------------------------------------------------------------------------------------------
@torch.no_grad()
def test_layernorm_rows_vith(dev):
    """layernorm_rows on 8192 rows of 1280 (B = 2) with the hard rows of vith_ref.layernorm_data (|mean| / std = 30,
    massive channels, constant rows, |mean| / std = 3000, f16-subnormal outputs), f16 out at ldo = 1344 with NaN guard columns / rows.
    Bound: vith_ref.layernorm_tol, which a one-pass f32 variance (rows at 3000) and a dropped eps (constant rows)
    leave by >= 100x.  The constant rows give exactly f16(beta): mean and x - mean are exact there."""
    from inklayer_amd import ops
    R = 8192
    x, gamma, beta = V.layernorm_data(R, _gen(dev, 7), dev)
    buf = torch.full((R + 4, V.D + 64), NAN, dtype=V.F16, device=dev)
    out = buf[:R, :V.D]
    ops.layernorm_rows(x, gamma, beta, 1e-6, out=out)
    assert buf[R:].isnan().all() and buf[:R, V.D:].isnan().all()
    ref = V.layernorm_ref(x, gamma, beta)
    tol = V.layernorm_tol(x, gamma, beta, ref)
    got = out.double()
    assert ((ref[:, :64].abs() < 2.0 ** -14) & (ref[:, :64] != 0)).sum() > 1000       # f16-subnormal outputs exercised
    assert torch.equal(out[16:20], beta.half()[None].expand(4, -1))
    worst = V.assert_within(got, ref, tol, "layernorm_rows C=1280")
    for rows, what in ((slice(0, 8), "|mean|/std = 30"), (slice(8, 16), "massive channels"),
                       (slice(20, 24), "|mean|/std = 3000")):
        _report(what, V.assert_within(got[rows], ref[rows], tol[rows], what))
    for mistake, rows in (("one-pass", slice(20, 24)), ("no-eps", slice(16, 20))):
        wrong = V.layernorm_wrong(x, gamma, beta, mistake)
        V.assert_discriminates(wrong[rows], ref[rows], tol[rows], mistake)
    _report("layernorm_rows C=1280, all rows", worst)


# ---------------------------------------------------------------------------------------------------------------
# relpos_bias
# ---------------------------------------------------------------------------------------------------------------
def _relpos_wrongs(q, Rh, Rw, S, qrows, ref, tol, valid=None):
    for what, kw in (("rel_h / rel_w swapped", dict(swap=True)), ("k - q indexing", dict(flip=True)),
                     ("q of head h + 1", dict(head_shift=1)), ("scale multiplied", dict(scale_mode="mul")),
                     ("scale omitted", dict(scale_mode="none"))):
        wr = V.relpos_ref(q, Rh, Rw, S, qrows, **kw)
        wrong = torch.cat([wr[0], wr[1]], -1)
        if valid is not None:
            wrong = torch.where(valid, wrong, ref)
        V.assert_discriminates(wrong, ref, tol, what)


@torch.no_grad()
@pytest.mark.parametrize("B", [1, 8])
def test_relpos_bias_windows(dev, B):
    """S = 14 rel_aug rows through the engine's 64 -> 70 win_map (tok_rows), 16 heads, q a column view of a packed
    [B*4096, 3840] qkv: per (window, head, query) 32 f16 = rel_h[0..13] | rel_w[0..13] | 4 zeros.  Only real query rows
    carry a requirement (padding rows are left untouched).  Bound: vith_ref.relpos_tol (f16 table in LDS, f16 out)."""
    from inklayer_amd import ops, sam
    g = _gen(dev, 20 + B)
    qkv = V.qkv_data(B, g, dev)
    q = qkv[:, :V.D]
    Rh, Rw = V.rel_tables(14, g, dev, std=0.3)
    wm = sam.window_rows(B, 64, 14).to(dev)
    nb = 25 * B
    n = nb * V.HEADS * 196
    buf = torch.full((n + 64, 32), NAN, dtype=V.F16, device=dev)
    ops.relpos_bias(q, Rh, Rw, S=14, n_batch=nb, n_heads=V.HEADS, head_dim=V.HD, scale=V.SCALE, out=buf[:n], tok_rows=wm)
    assert buf[n:].isnan().all()
    got = buf[:n].double().view(nb, V.HEADS, 196, 32)
    qrows = wm.view(nb, 196)
    rh, rw, mh, mw, qa = V.relpos_ref(q, Rh, Rw, 14, qrows)
    valid = (qrows >= 0)[:, None, :, None]
    ref = torch.cat([rh, rw], -1)
    tol = torch.cat([V.relpos_tol(rh, mh, qa, True), V.relpos_tol(rw, mw, qa, True)], -1)
    gv = torch.where(valid, got[..., :28], ref)
    worst = V.assert_within(gv, ref, tol, f"relpos_bias S=14 B={B}")
    assert (got[..., 28:][valid.expand(-1, V.HEADS, -1, 4)] == 0).all()
    _report(f"relpos_bias S=14 B={B}", worst)
    _relpos_wrongs(q, Rh, Rw, 14, qrows, ref, tol, valid)


@torch.no_grad()
@pytest.mark.parametrize("f16_tables", [False, True])
def test_relpos_bias_global(dev, f16_tables):
    """S = 64 tables [B*16*4096, 64] at B = 2, f32 (ink_relpos_bias) or f16 (ink_relpos_bias64_f16, the engine's
    setting), NaN guard rows.  Bound: vith_ref.relpos_tol."""
    from inklayer_amd import ops
    B = 2
    g = _gen(dev, 30 + f16_tables)
    qkv = V.qkv_data(B, g, dev)
    q = qkv[:, :V.D]
    Rh, Rw = V.rel_tables(64, g, dev, std=0.3)
    n = B * V.HEADS * 4096
    dt = V.F16 if f16_tables else V.F32
    bh, bw = (torch.full((n + 64, 64), NAN, dtype=dt, device=dev) for _ in range(2))
    oh, ow = ops.relpos_bias(q, Rh, Rw, S=64, n_batch=B, n_heads=V.HEADS, head_dim=V.HD, scale=V.SCALE,
                             out=(bh[:n], bw[:n]), f16_tables=f16_tables)
    assert oh.dtype == dt and bh[n:].isnan().all() and bw[n:].isnan().all()
    qrows = torch.arange(B * 4096, device=dev).view(B, 4096)
    rh, rw, mh, mw, qa = V.relpos_ref(q, Rh, Rw, 64, qrows)
    ref = torch.cat([rh, rw], -1)
    tol = torch.cat([V.relpos_tol(rh, mh, qa, f16_tables), V.relpos_tol(rw, mw, qa, f16_tables)], -1)
    got = torch.cat([bh[:n].double().view(B, V.HEADS, 4096, 64), bw[:n].double().view(B, V.HEADS, 4096, 64)], -1)
    worst = V.assert_within(got, ref, tol, f"relpos_bias S=64 f16_tables={f16_tables}")
    _report(f"relpos_bias S=64 {'f16' if f16_tables else 'f32'} tables", worst)
    _relpos_wrongs(q, Rh, Rw, 64, qrows, ref, tol)


# ---------------------------------------------------------------------------------------------------------------
# window attention (win4): the persistent walk at production
# ---------------------------------------------------------------------------------------------------------------
def _win_run(dev, qkv, Rh, Rw, pad_k, pad_v, B):
    """relpos_bias + flash_attn exactly as SamEngine._blocks runs a window block; out is a NaN-filled [B*4096, 1280]
    view of a [B*4096 + 64, 1344] buffer.  Returns (buffer, rel_aug)."""
    from inklayer_amd import ops, sam
    nb = 25 * B
    wm = sam.window_rows(B, 64, 14).to(dev)
    q, k, v = qkv[:, :V.D], qkv[:, V.D:2 * V.D], qkv[:, 2 * V.D:]
    aug = torch.full((nb * V.HEADS * 196, 32), NAN, dtype=V.F16, device=dev)
    ops.relpos_bias(q, Rh, Rw, S=14, n_batch=nb, n_heads=V.HEADS, head_dim=V.HD, scale=V.SCALE, out=aug, tok_rows=wm)
    buf = torch.full((B * 4096 + 64, V.D + 64), NAN, dtype=V.F16, device=dev)
    ops.flash_attn(q, k, v, n_batch=nb, n_heads=V.HEADS, head_dim=V.HD, scale=V.SCALE, n_q=196, n_k=196, rel_aug=aug,
                   grid_w=14, tok_rows=wm, pad_k=pad_k, pad_v=pad_v, out=buf[:B * 4096, :V.D])
    return buf, aug


@torch.no_grad()
@pytest.mark.parametrize("B", [1, 8])
def test_window_attention_persistent_walk(dev, B):
    """win4_attn_kernel at B = 1 (400 (window, head) items over the CUs: some workgroups take 2) and B = 8 (3200
    items, ~12.5 per workgroup), 16 heads, hd 80, q / k / v column views of the packed qkv, the engine's win_map and
    pad_k / pad_v.  The reference takes the kernel's f16 rel_aug as input (relpos_bias has its own test).  Every token
    row is written (no NaN left) and holds its own query's value, and the 64 guard rows and 64 guard columns stay NaN.
    That is all of "written exactly once" that an output can show: a second write of the right value leaves no trace,
    a stray write of another query's value fails the per-element bound of the row it lands in, and the win_map the
    kernel scatters through is a bijection onto the token rows (test_vith_plan_cpu.test_window_map).
    Bound: vith_ref.attn_tol.  At B = 8
    each image must equal, bit for bit, a B = 1 run on that image alone: items are independent, so state carried from
    one item of a workgroup to the next would show here."""
    from inklayer_amd import sam
    g = _gen(dev, 40 + B)
    qkv = V.qkv_data(B, g, dev)
    Rh, Rw = V.rel_tables(14, g, dev)
    pad_k, pad_v = torch.randn(V.D, generator=g, device=dev).half(), torch.randn(V.D, generator=g, device=dev).half()
    buf, aug = _win_run(dev, qkv, Rh, Rw, pad_k, pad_v, B)
    M = B * 4096
    assert buf[M:].isnan().all() and buf[:, V.D:].isnan().all()
    out = buf[:M, :V.D]
    assert not out.isnan().any()
    wm = sam.window_rows(B, 64, 14).to(dev).view(25 * B, 196)
    worst = 0.0
    for i in range(B):
        win = torch.arange(25 * i, 25 * i + 25, device=dev)
        q, k, v, bmag, P, s, o, valid = V.win_item_ref(qkv, aug, wm, pad_k, pad_v, win)
        tol = V.attn_tol(q, k, v, bmag, P, s, o)
        rows = wm[win].long()
        got = out[rows.clamp(min=0)].double().view(25, 196, V.HEADS, V.HD).permute(0, 2, 1, 3)
        m = valid[:, None, :, None]
        worst = max(worst, V.assert_within(torch.where(m, got, o), o, tol, f"win4 B={B} image {i}"))
        if i == 0:
            for what, kw in (("key 0 of the neighbouring window", dict(neighbour_key=True)),
                             ("zero instead of pad_k", dict(zero_pad_k=True)),
                             ("K / V of the previous item", dict(stale_kv=True)), ("key 195 dropped", dict(drop_key=True))):
                wrong = V.win_item_ref(qkv, aug, wm, pad_k, pad_v, win, **kw)[6]
                V.assert_discriminates(torch.where(m, wrong, o), o, tol, what)
        del q, k, v, bmag, P, s, o, tol
    _report(f"win4 B={B}", worst)
    if B > 1:
        for i in range(B):
            one = qkv[i * 4096:(i + 1) * 4096].clone()
            b1, aug1 = _win_run(dev, one, Rh, Rw, pad_k, pad_v, 1)
            n1 = 25 * V.HEADS * 196
            assert torch.equal(aug1.view(torch.int16), aug[i * n1:(i + 1) * n1].view(torch.int16))   # bits (NaN rows too)
            assert torch.equal(b1[:4096, :V.D], out[i * 4096:(i + 1) * 4096]), f"image {i}: B = 8 != B = 1"


# ---------------------------------------------------------------------------------------------------------------
# global attention (glob4)
# ---------------------------------------------------------------------------------------------------------------
def _glob_run(dev, qkv, Rh, Rw, B, f16_tables):
    from inklayer_amd import ops
    q, k, v = qkv[:, :V.D], qkv[:, V.D:2 * V.D], qkv[:, 2 * V.D:]
    rh, rw = ops.relpos_bias(q, Rh, Rw, S=64, n_batch=B, n_heads=V.HEADS, head_dim=V.HD, scale=V.SCALE,
                             f16_tables=f16_tables)
    buf = torch.full((B * 4096 + 64, V.D + 64), NAN, dtype=V.F16, device=dev)
    ops.flash_attn(q, k, v, n_batch=B, n_heads=V.HEADS, head_dim=V.HD, scale=V.SCALE, rel_h=rh, rel_w=rw, grid_w=64,
                   out=buf[:B * 4096, :V.D])
    return buf, rh, rw


def _glob_check(qkv, rh, rw, out, images, what, discriminate=False):
    worst = 0.0
    for b in images:
        for h in range(V.HEADS):
            q, k, v = (qkv[b * 4096:(b + 1) * 4096, j * V.D + h * V.HD:j * V.D + (h + 1) * V.HD].double() for j in range(3))
            bh = b * V.HEADS + h
            th, tw = rh.view(-1, 4096, 64)[bh].double(), rw.view(-1, 4096, 64)[bh].double()
            o, P, s, bmag = V.glob_ref(q, k, v, th, tw)
            tol = V.attn_tol(q, k, v, bmag, P, s, o)
            got = out[b * 4096:(b + 1) * 4096, h * V.HD:(h + 1) * V.HD].double()
            worst = max(worst, V.assert_within(got, o, tol, f"{what} image {b} head {h}"))
            if discriminate and h < 2:
                for wname, kw in (("key tile 37 dropped", dict(drop_tile=37)),
                                  ("last query tile: rel rows of the tile before", dict(last_tile_rows=True)),
                                  ("rel_h / rel_w swapped", dict(swap=True))):
                    V.assert_discriminates(V.glob_ref(q, k, v, th, tw, **kw)[0], o, tol, wname)
            del P, s, bmag, tol
    return worst


@torch.no_grad()
@pytest.mark.parametrize("f16_tables", [False, True])
def test_global_attention_b2(dev, f16_tables):
    """glob4_attn_kernel at B = 2, 16 heads, with f32 and with f16 rel tables from relpos_bias; logit std ~2 (peaked
    softmax) with every 16th query near uniform; NaN guard rows / columns.  Reference per (image, head) in float64
    on the kernel's own rel tables (relpos_bias has its own test).  Bound: vith_ref.attn_tol."""
    B = 2
    g = _gen(dev, 50 + f16_tables)
    qkv = V.qkv_data(B, g, dev)
    Rh, Rw = V.rel_tables(64, g, dev)
    buf, rh, rw = _glob_run(dev, qkv, Rh, Rw, B, f16_tables)
    M = B * 4096
    assert buf[M:].isnan().all() and buf[:, V.D:].isnan().all()
    worst = _glob_check(qkv, rh, rw, buf[:M, :V.D], range(B), "glob4", discriminate=True)
    _report(f"glob4 B=2 {'f16' if f16_tables else 'f32'} tables", worst)


@torch.no_grad()
def test_global_attention_b8_slice_equals_b1(dev):
    """The engine's setting (f16 tables) at B = 8: image 5 against float64, and bit for bit against a B = 1 run on
    image 5 alone (its rel tables too)."""
    B, i = 8, 5
    g = _gen(dev, 60)
    qkv = V.qkv_data(B, g, dev)
    Rh, Rw = V.rel_tables(64, g, dev)
    buf, rh, rw = _glob_run(dev, qkv, Rh, Rw, B, True)
    assert buf[B * 4096:].isnan().all() and buf[:, V.D:].isnan().all()
    out = buf[:B * 4096, :V.D]
    worst = _glob_check(qkv, rh, rw, out, [i], "glob4 B=8")
    _report("glob4 B=8 image 5, f16 tables", worst)
    b1, rh1, rw1 = _glob_run(dev, qkv[i * 4096:(i + 1) * 4096].clone(), Rh, Rw, 1, True)
    n1 = V.HEADS * 4096
    assert torch.equal(rh1, rh[i * n1:(i + 1) * n1]) and torch.equal(rw1, rw[i * n1:(i + 1) * n1])
    assert torch.equal(b1[:4096, :V.D], out[i * 4096:(i + 1) * 4096])


# ---------------------------------------------------------------------------------------------------------------
# one ViT-H block through the engine
# ---------------------------------------------------------------------------------------------------------------
BLOCK_ABS = 2.0 ** -12


@torch.no_grad()
@pytest.mark.parametrize("kind,B", [("window", 6), ("global", 2)])
def test_vith_block_matches_float64(dev, kind, B):
    """SamEngine._blocks(B, upto=1) of a depth-1 engine (product settings but bias_correction off: the reference has
    the checkpoint's biases) on random f32 tokens, against sam_ref.vit_block in float64: a window block at B = 6 (all
    four GEMMs variant 45), a global block at B = 2.  rel_pos tables scaled from std 0.2 to 0.5 so that a wrong bias is
    seen: the float64 block with rel_pos_h and rel_pos_w exchanged must miss the yardstick by >= 100x at every
    quantile.  Yardstick of test_swin_block_matches_float64: every error quantile, the maximum included, is at most 2x that
    of the float64 reference re-run with f16-rounded linear operands (sam_ref.f16_operands) plus BLOCK_ABS * max|block
    update|, for what that yardstick does not round (q, k, v, P and the rel terms inside the attention)."""
    from oracle import sam_ref
    from inklayer_amd import sam
    gi = (0,) if kind == "global" else ()
    oc = sam_ref.SamConfig(depth=1, global_attn_indexes=gi)
    sd = sam_ref.seeded_state_dict(sam_ref.sam_param_shapes(oc), 9)
    for k in sd:
        if "rel_pos" in k:
            sd[k] = sd[k] * 2.5
    eng = sam.SamEngine(sd, sam.SamConfig(depth=1, global_attn_indexes=gi), dev, max_batch=B, bias_correction=False)
    gen = torch.Generator().manual_seed(11 + B)
    x = torch.randn(B * 4096, V.D, generator=gen)
    eng.x[:B * 4096] = x.to(dev)
    got = eng._blocks(B, 1).reshape(B * 4096, V.D).double()
    p = "image_encoder.blocks.0."
    sd64 = {k: v.to(dev, torch.float64) for k, v in sd.items() if k.startswith(p)}
    x64 = x.to(dev, torch.float64).view(B, 64, 64, V.D)
    ref = sam_ref.vit_block(sd64, oc, 0, x64).reshape(-1, V.D)
    with sam_ref.f16_operands():
        emul = sam_ref.vit_block(sd64, oc, 0, x64).reshape(-1, V.D)
    # the same block with rel_pos_h and rel_pos_w exchanged: the yardstick has to reject it at every quantile
    swapped = dict(sd64)
    swapped[p + "attn.rel_pos_h"], swapped[p + "attn.rel_pos_w"] = sd64[p + "attn.rel_pos_w"], sd64[p + "attn.rel_pos_h"]
    wrong = sam_ref.vit_block(swapped, oc, 0, x64).reshape(-1, V.D)
    a = BLOCK_ABS * (ref - x64.reshape(-1, V.D)).abs().max().item()
    err = (got - ref).abs().flatten().cpu().numpy()
    eerr = (emul - ref).abs().flatten().cpu().numpy()
    werr = (wrong - ref).abs().flatten().cpu().numpy()
    del wrong, swapped
    assert np.isfinite(err).all()
    for qt in (0.5, 0.9, 0.99, 0.999, 1.0):
        hq, eq, wq = float(np.quantile(err, qt)), float(np.quantile(eerr, qt)), float(np.quantile(werr, qt))
        bound = 2 * eq + a
        print(f"  {kind} block B={B} q{qt}: HIP {hq:.2e}  emulated-f16 {eq:.2e}  -> {hq / bound:.3f}x the bound; "
              f"rel_h / rel_w swapped {wq / bound:.0f}x")
        assert hq <= bound, (qt, hq, eq, a)
        assert wq >= 100 * bound, ("rel_h / rel_w swapped passes the yardstick", qt, wq, bound)
