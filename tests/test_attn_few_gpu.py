"""Few-key / few-query attention (inklayer_amd/csrc/attn_few.hip) through ops.attn_fewkeys / ops.attn_fewq against the
float64 reference of tests/attn_few_ref.py: every n_k and n_q instantiation, rows passed as column slices of wider
buffers (as every product call does; the rest of the buffer is NaN), shared batch rows, the position constants, block
masks, the 64-key tile and key-range group boundaries, and planted keys that drive the online-softmax rescale factors
to exactly 0 and 1.  Bounds are the project's own for this family (attn_few_ref.TOL_*).  GPU box only."""
import pytest
import torch

import attn_few_ref as R

pytestmark = pytest.mark.gpu


def _lay(layout, q2, k2, v2):
    """The [rows, E] device matrices as the product passes them.
      contig    dense rows
      sam       attn_fewkeys in the SAM decoder: q the last third of a [*, 3E] buffer, k | v one [*, 2E] buffer
      det_self  the detector's text self-attention: q | k one [*, 2E] buffer (qk[:, :256], qk[:, 256:]), v = kv[:, :256]
      det_cross its text cross-attention: k | v one [*, 2E] buffer; q the second half of a poisoned buffer
      kvq       attn_fewq in the SAM decoder: k | v the first two thirds of a [*, 3E] buffer; q at column 8 of [*, E + 16]"""
    E = q2.shape[1]
    if layout == "contig":
        return q2, k2, v2
    if layout == "sam":
        k2 = R.strided(k2, 2 * E, 0)
        return R.strided(q2, 3 * E, 2 * E), k2, R.strided(v2, 2 * E, E, base=k2._base)
    if layout == "det_self":
        q2 = R.strided(q2, 2 * E, 0)
        return q2, R.strided(k2, 2 * E, E, base=q2._base), R.strided(v2, 2 * E, 0)
    if layout == "det_cross":
        k2 = R.strided(k2, 2 * E, 0)
        return R.strided(q2, 2 * E, E), k2, R.strided(v2, 2 * E, E, base=k2._base)
    assert layout == "kvq"
    k2 = R.strided(k2, 3 * E, 0)
    return R.strided(q2, E + 16, 8), k2, R.strided(v2, 3 * E, E, base=k2._base)


def _fewkeys(dev, layout, q, k, v, scale, *, shared=False, q_add=None, blocked=None):
    """q [n or 2 (shared), n_q, H, hd], k / v [n, n_k, H, hd] on the CPU -> ops.attn_fewkeys on views laid out as
    `layout`; shared: the entries read the q rows of image R.IMG_OF[b]."""
    from inklayer_amd import ops
    n, n_k, H, hd = k.shape
    n_q = q.shape[1]
    q2, k2, v2 = _lay(layout, *(R.rows2d(t).to(dev) for t in (q, k, v)))
    assert all(t.data_ptr() % 16 == 0 and t.stride(1) == 1 for t in (q2, k2, v2))
    out = ops.attn_fewkeys(q2, k2, v2, B=n, n_heads=H, head_dim=hd, scale=scale, n_q=n_q,
                           q_batch_rows=R.share_rows(n_q).to(dev) if shared else None,
                           q_add=None if q_add is None else q_add.to(dev),
                           blocked=None if blocked is None else blocked.to(dev))
    assert out.dtype == q.dtype and tuple(out.shape) == (n * n_q, H * hd)
    return out


def _fewq(dev, layout, q, k, v, scale, *, q_shared=False, kv_shared=False, k_add=None):
    """q [n or 2 (q_shared), n_q, H, 16], k / v [n or 2 (kv_shared), n_k, H, 16] on the CPU -> ops.attn_fewq."""
    from inklayer_amd import ops
    n = len(R.IMG_OF)
    n_q, H, hd = q.shape[1:]
    n_k = k.shape[1]
    q2, k2, v2 = _lay(layout, *(R.rows2d(t).to(dev) for t in (q, k, v)))
    assert all(t.data_ptr() % 16 == 0 and t.stride(1) == 1 for t in (q2, k2, v2))
    out = ops.attn_fewq(q2, k2, v2, n_batch=n, n_heads=H, head_dim=hd, scale=scale, n_q=n_q, n_k=n_k,
                        q_batch_rows=R.share_rows(n_q).to(dev) if q_shared else None,
                        kv_batch_rows=R.share_rows(n_k).to(dev) if kv_shared else None,
                        k_add=None if k_add is None else k_add.to(dev))
    assert out.dtype == torch.float32 and tuple(out.shape) == (n * n_q, H * hd)
    return out


def _check(tag, out, ref, tol, relative=True, e32=None, floor=0.0):
    """Finite, and max |out - ref| below tol (x max(1, |ref|max) when relative) or `floor`, whichever is larger."""
    assert bool(torch.isfinite(out).all()), f"{tag}: non-finite output"
    err, rmax = R.max_err(out, ref)
    bound = max(tol * max(1.0, rmax) if relative else tol, floor)
    vs32 = "" if e32 is None else f"  f32 reference {e32:.2e} (kernel / that = {err / max(e32, 1e-30):.2f})"
    print(f"{tag}: max err {err:.2e} (bound {bound:.2e}){vs32}")
    assert err < bound, f"{tag}: {err:.3e} >= {bound:.3e}"
    return err


def _e32(q, k, v, scale, ref, **kw):
    return (R.attn_ref(q, k, v, scale, dtype=torch.float32, **kw).double() - ref).abs().max().item()


# ---------------------------------------------------------------------------------------------------------------
# 1. few keys, f32 rows: the generic kernel below 7 keys at head_dim 16 and at head_dim 32, all ten NK instantiations
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hd,n_k,n_q", [(hd, n_k, 37) for hd in (16, 32) for n_k in range(1, 17)]
                         + [(hd, n_k, 512) for hd in (16, 32) for n_k in (7, 16)])
def test_fewkeys_f32_every_nk(dev, hd, n_k, n_q):
    """B = 3, 8 heads; n_q = 37 leaves the last workgroup partial (3 * 37 * 8 threads, x 4 for the quad kernel).  Dense
    and strided rows, with and without q_batch_rows (entries 0 and 2 read image 1's rows) and q_add, which is compared
    with float64 of (q + q_add)."""
    H, scale = 8, hd ** -0.5
    q_own, k, v = R.randn_inputs(hd, n_q, n_k, seed=100 * hd + n_k, H=H, k_gain=2.0)
    q_img = q_own[:2]
    g = torch.Generator(device="cpu").manual_seed(n_k)
    q_add = torch.randn(n_q, H * hd, generator=g)
    for shared in (False, True):
        q = q_img if shared else q_own
        q_ref = q_img[list(R.IMG_OF)] if shared else q_own
        for add in (None, q_add):
            ref = R.attn_ref(q_ref, k, v, scale, q_add=add)
            for layout in ("contig", "sam"):
                out = _fewkeys(dev, layout, q, k, v, scale, shared=shared, q_add=add)
                _check(f"hd={hd} n_k={n_k} n_q={n_q} {layout} shared={shared} q_add={add is not None}", out, ref,
                       R.TOL_FEWKEYS_F32)


# ---------------------------------------------------------------------------------------------------------------
# 2. few keys, f16 rows (attn_fewkeys_kernel<32, f16> / <64, f16>), with and without a block mask
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["cross", "self"])
@pytest.mark.parametrize("n_k", R.F16_NK)
@pytest.mark.parametrize("hd,H", R.F16_FORMS)
def test_fewkeys_f16(dev, hd, H, n_k, form):
    """The detector's text attentions: 37 queries against n_k keys (cross) and n_q = n_k (self), dense and as the
    detector slices its projection outputs."""
    n_q = R.FEWKEYS_NQ if form == "cross" else n_k
    q, k, v = R.f16_inputs(hd, H, n_q, n_k)
    ref = R.attn_ref(q, k, v, hd ** -0.5)
    for layout in ("contig", "det_" + form):
        out = _fewkeys(dev, layout, q, k, v, hd ** -0.5)
        _check(f"f16 hd={hd} n_k={n_k} n_q={n_q} {layout}", out, ref, R.TOL_F16, relative=False)


@pytest.mark.parametrize("name,n_q,n_k,blocked", R.blocked_cases(), ids=[c[0] for c in R.blocked_cases()])
@pytest.mark.parametrize("hd,H", R.F16_FORMS)
def test_fewkeys_f16_blocked(dev, hd, H, name, n_q, n_k, blocked):
    """Block-diagonal masks at 4, 5 and 16 keys and seeded random ones (every row keeps a key), head_dim 32 and 64."""
    q, k, v = R.f16_inputs(hd, H, n_q, n_k)
    ref = R.attn_ref(q, k, v, hd ** -0.5, blocked=blocked)
    for layout in ("contig", "det_self" if n_q == n_k else "det_cross"):
        out = _fewkeys(dev, layout, q, k, v, hd ** -0.5, blocked=blocked)
        _check(f"f16 hd={hd} blocked {name} {layout}", out, ref, R.TOL_F16, relative=False)


# ---------------------------------------------------------------------------------------------------------------
# 3. few queries: every n_q of both QW forms, the tile / group boundaries, every row table, k_add
# ---------------------------------------------------------------------------------------------------------------
FEWQ_MODES = (dict(), dict(kv_shared=True), dict(q_shared=True), dict(k_add=True),
              dict(q_shared=True, kv_shared=True, k_add=True))


def _fewq_case(dev, n_q, n_k, H):
    scale = 0.25
    q_own, k_own, v_own = R.randn_inputs(16, n_q, n_k, seed=31 * n_q + n_k + H, H=H, k_gain=2.0)
    g = torch.Generator(device="cpu").manual_seed(n_k + n_q)
    k_add = torch.randn(n_k, H * 16, generator=g)
    img = list(R.IMG_OF)
    for mode in FEWQ_MODES:
        qs, kvs, ka = mode.get("q_shared", False), mode.get("kv_shared", False), k_add if mode.get("k_add") else None
        q, k, v = (q_own[:2] if qs else q_own), (k_own[:2] if kvs else k_own), (v_own[:2] if kvs else v_own)
        # three entries read the rows of two blocks; the output is written at b * n_q all the same
        ref = R.attn_ref(q[img] if qs else q, k[img] if kvs else k, v[img] if kvs else v, scale, k_add=ka)
        for layout in ("contig", "kvq"):
            out = _fewq(dev, layout, q, k, v, scale, q_shared=qs, kv_shared=kvs, k_add=ka)
            _check(f"fewq n_q={n_q} n_k={n_k} H={H} {layout} {sorted(mode)}", out, ref, R.TOL_FEWQ)


@pytest.mark.parametrize("H", [4, 8])
@pytest.mark.parametrize("n_q", range(1, 17))
def test_fewq_every_nq(dev, n_q, H):
    """n_q 1..8 (QW = 2) and 9..16 (QW = 4) at 300 keys: every pattern of inactive query slots and idle waves; 4 heads
    is a single head group per entry."""
    _fewq_case(dev, n_q, 300, H)


@pytest.mark.parametrize("n_k", [1, 16, 63, 64, 65, 127, 128, 129, 191, 192, 193, 4097])
@pytest.mark.parametrize("n_q", R.FEWQ_NQ)
def test_fewq_key_range_boundaries(dev, n_q, n_k):
    """Group 1 has no keys up to 64; the last 64-key tile of each group is ragged to either side of 64, 128 and 192;
    4097 keys put one key past a tile boundary of group 0."""
    _fewq_case(dev, n_q, n_k, 8)


def test_fewq_row_tables_are_checked(dev):
    """ops.attn_fewq refuses a row table that is not int32 [n_batch] on the device before anything is launched."""
    from inklayer_amd import ops
    q, k, v = (R.rows2d(t).to(dev) for t in R.randn_inputs(16, 7, 40, seed=1))
    kw = dict(n_batch=3, n_heads=8, head_dim=16, scale=0.25, n_q=7, n_k=40)
    good = torch.tensor([0, 7, 14], dtype=torch.int32, device=dev)
    assert torch.equal(ops.attn_fewq(q, k, v, q_batch_rows=good, **kw), ops.attn_fewq(q, k, v, **kw))
    for bad in (good.long(), good[:2], good.cpu()):
        for name in ("q_batch_rows", "kv_batch_rows"):
            with pytest.raises(AssertionError):
                ops.attn_fewq(q, k, v, **{name: bad}, **kw)


# ---------------------------------------------------------------------------------------------------------------
# 4. planted keys: rescale factors of exactly 0 and 1 in the per-tile update, the 16-lane merge and the group fold
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_q", R.FEWQ_NQ)
@pytest.mark.parametrize("n_k,plant", R.FEWQ_PLANTS, ids=[f"{nk}-{'_'.join(f'{k}x{m}' for k, m in p)}" for nk, p in R.FEWQ_PLANTS])
def test_fewq_planted_keys(dev, n_k, plant, n_q):
    """A key (or tied keys) 20+ natural-log units above everything else (test_attn_few_ref_cpu.py), in the last ragged
    tile of group 1, in group 0 with group 1 empty, moving the running maximum several times, tied across the groups:
    the stale side of every rescale gets a factor of exactly 0, the -3.0e38 sentinels meet scores of 140."""
    q, k, v, scale = R.planted_inputs(16, n_k, plant, R.plant_seed(n_k, plant), n_q=n_q)
    ref = R.attn_ref(q, k, v, scale)
    e32 = _e32(q, k, v, scale, ref)
    for layout in ("contig", "kvq"):
        _check(f"fewq planted n_k={n_k} {plant} n_q={n_q} {layout}", _fewq(dev, layout, q, k, v, scale), ref, R.TOL_FEWQ,
               e32=e32)


@pytest.mark.parametrize("hd,H,dtype,n_k,plant,blocked_key", R.FEWKEYS_PLANTS,
                         ids=[f"hd{c[0]}-{str(c[2])[-7:]}-nk{c[3]}" for c in R.FEWKEYS_PLANTS])
def test_fewkeys_planted_keys(dev, hd, H, dtype, n_k, plant, blocked_key):
    """The same for the three few-key kernels; at head_dim 32 f16 a block mask takes the planted key away from every
    odd query."""
    n_q = R.FEWKEYS_NQ
    q, k, v, scale = R.planted_inputs(hd, n_k, plant, R.plant_seed(n_k, plant), H=H, n_q=n_q, dtype=dtype)
    blocked = None if blocked_key is None else R.block_key_for_odd_queries(n_q, n_k, blocked_key)
    ref = R.attn_ref(q, k, v, scale, blocked=blocked)
    e32 = _e32(q, k, v, scale, ref, blocked=blocked)
    f16 = dtype == torch.float16
    for layout in ("contig", "det_cross" if f16 else "sam"):
        out = _fewkeys(dev, layout, q, k, v, scale, blocked=blocked)
        _check(f"fewkeys planted hd={hd} {dtype} n_k={n_k} {plant} {layout}", out, ref,
               R.TOL_F16 if f16 else R.TOL_FEWKEYS_F32, relative=not f16, e32=e32)


@pytest.mark.parametrize("n_q", R.FEWQ_NQ)
def test_fewq_competing_keys(dev, n_q):
    """Keys 5 and 299 at scores of about 30 and 31, one per group: the weights are e / (1 + e) and 1 / (1 + e) up to
    the rounding of scores of 30..60 in f32 (an ulp of 4e-6 there moves a weight by as much).  Bound: the larger of the
    project's and 8 x the float32 reference's own error - the kernel folds scale * log2(e) into the query, uses the
    hardware exp2 and sums in another order, each worth a few ulp of the score.
    Measured on an MI355X (dense and strided rows alike): n_q 7 kernel 8.06e-6 against 4.17e-6 for the float32
    reference, ratio 1.93; n_q 12 kernel 5.98e-6 against 4.91e-6, ratio 1.22."""
    q, k, v, scale = R.competing_inputs(7, n_q)
    ref = R.attn_ref(q, k, v, scale)
    e32 = _e32(q, k, v, scale, ref)
    for layout in ("contig", "kvq"):
        _check(f"fewq competing n_q={n_q} {layout}", _fewq(dev, layout, q, k, v, scale), ref, R.TOL_FEWQ, e32=e32,
               floor=8 * e32)


# ---------------------------------------------------------------------------------------------------------------
# 5. a query gets the same bits from attn_fewq16_kernel<2> and <4>
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["planted", "strided"])
def test_fewq_forms_agree_bitwise(dev, case):
    """n_q = 9..16 (4 queries per wave, queries in LDS) against n_q = 8 (2 per wave, in registers) on the 8 queries both
    serve: the per-query arithmetic is the same text, so the outputs are equal bit for bit."""
    if case == "planted":
        plant = ((5, 1), (170, 2), (299, 3))
        q16, k, v, scale = R.planted_inputs(16, 300, plant, R.plant_seed(300, plant), n_q=16)
        kw = dict(layout="contig")
    else:
        q16, k, v = R.randn_inputs(16, 16, 1000, seed=6, k_gain=2.0)
        scale = 0.25
        g = torch.Generator(device="cpu").manual_seed(8)
        kw = dict(layout="kvq", k_add=torch.randn(1000, 128, generator=g) * 0.5)
    E = 128
    narrow = _fewq(dev, q=q16[:, :8].contiguous(), k=k, v=v, scale=scale, **kw).view(3, 8, E)
    for n_q in range(9, 17):
        wide = _fewq(dev, q=q16[:, :n_q].contiguous(), k=k, v=v, scale=scale, **kw).view(3, n_q, E)
        assert torch.equal(wide[:, :8], narrow), f"{case}: n_q={n_q} differs from the n_q=8 launch"
