"""Op-level parity of the GroundingDINO-side kernels against plain float64 references (oracle/gdino_ref.py where it
restates the operation).  Every output is pre-filled with NaN and every strided argument carries NaN in the columns a
kernel must not read.  The index-heavy tests also show, on the CPU, that a plausible indexing mistake moves the
reference by at least 100x the bound.  GPU box only."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

F16, F32, F64 = torch.float16, torch.float32, torch.float64
U = 2.0 ** -24            # f32 unit roundoff
NAN = float("nan")


def _plan(h, w, B):
    """The detector's host-built plan for an (h, w, B) input (what GDinoEngine.plan returns), built on the CPU: the
    plan reads only the config and the level embedding of its engine, and the latter only for `pos`."""
    from inklayer_amd import gdino
    eng = SimpleNamespace(cfg=gdino.GDinoConfig(), dev=torch.device("cpu"), level_embed_cpu=torch.zeros(4, 256))
    return gdino._Plan(eng, h, w, B)


def _strided(x: torch.Tensor, ld: int) -> torch.Tensor:
    """x [R, C] as the first C columns of an [R, ld] tensor whose other columns are NaN."""
    full = torch.full((x.shape[0], ld), NAN, dtype=x.dtype, device=x.device)
    full[:, :x.shape[1]] = x
    return full[:, :x.shape[1]]


def _nan_out(shape, dtype, dev) -> torch.Tensor:
    """An output buffer in which every element the kernel leaves unwritten stays NaN."""
    return torch.full(shape, NAN, dtype=dtype, device=dev)


def _assert_within(got, ref, tol, what):
    err = (got - ref).abs()
    bad = ~(err <= tol)                         # NaN-safe: a NaN output is out of bound
    if bad.any():
        i = int(bad.flatten().nonzero()[0])
        raise AssertionError(f"{what}: {int(bad.sum())} / {bad.numel()} elements out of bound; first at flat {i}: "
                             f"got {got.flatten()[i].item()!r}, ref {ref.flatten()[i].item()!r}, "
                             f"tol {tol.flatten()[i].item() if torch.is_tensor(tol) else tol!r}")


def _discriminates(wrong, ref, tol, what):
    m = ((wrong - ref).abs() / tol).max().item()
    assert m >= 100, f"the bound cannot tell the mistake '{what}' apart: max deviation {m:.1f}x the bound"


# ---------------------------------------------------------------------------------------------------------------
# msda_fused
# ---------------------------------------------------------------------------------------------------------------
M_, L_, P_ = 8, 4, 4


def _msda_inputs(rs, B, Q, shapes, ref_dim):
    """proj rows [B*Q, 384]: sampling offsets in pixel units of each level (half near the reference point, half
    anywhere in and around the level) and N(0, 30) logits; row 0 has 16 equal logits per head, row 1 one logit
    1000 above the rest."""
    off = np.empty((B * Q, M_, L_, P_, 2), np.float32)
    for l, (H, W) in enumerate(shapes):
        near = rs.normal(0, 2.0, size=(B * Q, M_, P_, 2))
        far = rs.uniform(-1, 1, size=(B * Q, M_, P_, 2)) * (np.array([W, H]) + 3.0)
        if ref_dim == 4:      # offsets are in units of box size / 8 here
            near, far = 4 * near, rs.uniform(-16, 16, size=(B * Q, M_, P_, 2))
        off[:, :, l] = np.where(rs.rand(B * Q, M_, P_, 1) < 0.5, far, near)
    lg = rs.normal(0, 30, size=(B * Q, M_, L_ * P_)).astype(np.float32)
    lg[0] = 7.25
    lg[1, :, 5] = lg[1].max() + 1000.5
    proj = np.concatenate([off.reshape(B * Q, 256), lg.reshape(B * Q, 128)], 1)
    return torch.from_numpy(proj)


def _msda_locations(proj, ref, shapes, B, Q, ref_batched, swap_xy=False):
    """The kernel's f32 location arithmetic (ms_deform_attn.py:309-322, op for op, no contraction), returned as
    float64 [B,Q,M,L,P,2] locations whose `loc * W - 0.5` in msda_core reproduces the kernel's f32 image coordinate,
    plus the f32 softmax of the logits in the kernel's order.  swap_xy: the (W, H) normaliser swapped (a mistake)."""
    f = np.float32
    pr = proj.numpy().reshape(B, Q, 384)
    off = pr[..., :256].reshape(B, Q, M_, L_, P_, 2)
    lg = pr[..., 256:].reshape(B, Q, M_, L_ * P_)
    e = np.exp(lg - lg.max(-1, keepdims=True))
    s = np.zeros(e.shape[:-1], np.float32)
    for i in range(L_ * P_):
        s = s + e[..., i]
    aw = (e * (f(1) / s)[..., None]).reshape(B, Q, M_, L_, P_)
    d = ref.shape[-1]
    rf = ref.numpy().reshape(B if ref_batched else 1, Q, 1, 1, d)
    loc = np.empty((B, Q, M_, L_, P_, 2), np.float64)
    regimes = np.zeros(3, np.int64)                # inside / partial border band / fully outside
    for l, (H, W) in enumerate(shapes):
        nx, ny = (f(H), f(W)) if swap_xy else (f(W), f(H))
        ox, oy = off[:, :, :, l, :, 0], off[:, :, :, l, :, 1]
        if d == 2:
            lx, ly = rf[..., 0] + ox / nx, rf[..., 1] + oy / ny
        else:
            rw, rh = (rf[..., 3], rf[..., 2]) if swap_xy else (rf[..., 2], rf[..., 3])
            lx = rf[..., 0] + ox / f(P_) * rw * f(0.5)
            ly = rf[..., 1] + oy / f(P_) * rh * f(0.5)
        him, wim = ly * f(H) - f(0.5), lx * f(W) - f(0.5)
        loc[:, :, :, l, :, 0] = (wim.astype(np.float64) + 0.5) / W
        loc[:, :, :, l, :, 1] = (him.astype(np.float64) + 0.5) / H
        live = (him > -1) & (wim > -1) & (him < H) & (wim < W)
        core = (him >= 0) & (wim >= 0) & (him <= H - 1) & (wim <= W - 1)
        regimes += [int(core.sum()), int((live & ~core).sum()), int((~live).sum())]
    return torch.from_numpy(loc), torch.from_numpy(aw.astype(np.float64)), regimes


def _msda_reference(value16, proj, ref, shapes, B, Q, ref_batched, **kw):
    from oracle import gdino_ref
    S = value16.shape[0] // B
    v = value16.double().view(B, S, M_, 32)
    loc, aw, regimes = _msda_locations(proj, ref, shapes, B, Q, ref_batched, **kw)
    return gdino_ref.msda_core(v, shapes, loc, aw), gdino_ref.msda_core(v.abs(), shapes, loc, aw), regimes


def _msda_tol(r, ra):
    """f16 output: half an f16 ulp of the reference (2^-11 |r|) plus the f32 path: each of the 64 (sample, corner) terms
    carries <= 16 u of weight error (softmax exp / sum / reciprocal, three weight products, 1 - frac) and each of the 64
    fma roundings adds <= u |partial sum| <= u * absref -> 80 u * absref; 1e-7 covers f16 subnormal spacing."""
    return 2.0 ** -11 * r.abs() + 80 * U * ra + 1e-7


def _run_msda(dev, value16, proj, ref, shapes, B, Q, ref_batched):
    from inklayer_amd import ops
    out = torch.full((B * Q, 256), NAN, dtype=F16, device=dev)
    p = _strided(proj.to(dev), 512)
    assert p.stride(0) == 512
    ops.msda_fused(value16.to(dev), p, ref.to(dev), shapes, B, Q, ref_batched=ref_batched, out=out)
    return out.double().cpu().view(B, Q, 256)


@torch.no_grad()
def test_msda_fused_encoder_form(dev):
    """Encoder form: ref [S, 2] shared by the batch, 2-d location arithmetic, at the plan of a non-square odd input
    (levels 40x59, 20x30, 10x15, 5x8); B = 2 gives 788 workgroups (partial last one, 788 % 8 != 0)."""
    from oracle import gdino_ref
    B = 2
    pl = _plan(320, 472, B)
    shapes, S = pl.shapes, pl.S
    assert torch.equal(pl.enc_ref, gdino_ref.enc_reference_points(shapes))
    rs = np.random.RandomState(11)
    value16 = torch.from_numpy(rs.standard_normal((B * S, 256)).astype(np.float16))
    proj = _msda_inputs(rs, B, S, shapes, 2)
    ref = pl.enc_ref
    r, ra, regimes = _msda_reference(value16, proj, ref, shapes, B, S, False)
    assert (regimes > 1000).all(), regimes
    tol = _msda_tol(r, ra)
    # the bound sees an x/y-swapped normaliser and level starts off by one
    _discriminates(_msda_reference(value16, proj, ref, shapes, B, S, False, swap_xy=True)[0], r, tol, "x/y swapped")
    vshift = torch.cat([value16[1:], value16[:1]])
    _discriminates(_msda_reference(vshift, proj, ref, shapes, B, S, False)[0], r, tol, "level starts + 1")
    got = _run_msda(dev, value16, proj, ref, shapes, B, S, False)
    _assert_within(got, r, tol, "msda_fused encoder form")


DEC_SHAPES = {"degenerate": [(1, 1), (1, 7), (5, 1), (2, 3)], "planlike": [(40, 59), (20, 30), (10, 15), (5, 8)]}


@torch.no_grad()
@pytest.mark.parametrize("shapes", sorted(DEC_SHAPES))
@pytest.mark.parametrize("B", [1, 2, 3])
@pytest.mark.parametrize("Q", [300, 900])
def test_msda_fused_decoder_form(dev, Q, B, shapes):
    """Decoder form: ref [B*Q, 4] boxes per image, 4-d location arithmetic; boxes with centres 0, 1 and near the
    borders, widths up to 1, and w = h = 1 at centre 1 (what a +inf proposal becomes)."""
    shapes = DEC_SHAPES[shapes]
    S = sum(h * w for h, w in shapes)
    rs = np.random.RandomState(100 * Q + 10 * B + S % 7)
    value16 = torch.from_numpy(rs.standard_normal((B * S, 256)).astype(np.float16))
    proj = _msda_inputs(rs, B, Q, shapes, 4)
    box = np.concatenate([rs.uniform(0, 1, (B * Q, 2)), rs.uniform(0.01, 1, (B * Q, 2))], 1).astype(np.float32)
    box[0::7, :2] = rs.choice([0.0, 1.0, 1e-3, 1 - 1e-3], size=(len(box[0::7]), 2))
    box[3::11] = 1.0
    box[5::13, 2:] = rs.choice([1.0, 1e-3], size=(len(box[5::13]), 2))
    ref = torch.from_numpy(box)
    r, ra, regimes = _msda_reference(value16, proj, ref, shapes, B, Q, True)
    assert (regimes > 0).all(), regimes
    tol = _msda_tol(r, ra)
    _discriminates(_msda_reference(value16, proj, ref, shapes, B, Q, True, swap_xy=True)[0], r, tol, "w/h swapped")
    if B > 1:
        shared = ref[:Q].contiguous()
        _discriminates(_msda_reference(value16, proj, shared, shapes, B, Q, False)[0], r, tol, "ref shared, not batched")
    got = _run_msda(dev, value16, proj, ref, shapes, B, Q, True)
    _assert_within(got, r, tol, "msda_fused decoder form")


def test_msda_fused_rejects_bad_arguments(dev):
    from inklayer_amd import ops
    from inklayer_amd._lib import InkLayerHipError
    shapes = DEC_SHAPES["degenerate"]
    v = torch.zeros((19, 256), dtype=F16, device=dev)
    ref4 = torch.zeros((8, 4), device=dev)
    for ld in (380, 386):                              # ldp < 384, ldp % 4 != 0
        with pytest.raises(InkLayerHipError):
            ops.msda_fused(v, torch.zeros((8, ld), device=dev), ref4, shapes, 1, 8, ref_batched=True)
    with pytest.raises(InkLayerHipError):             # ref_dim == 3
        ops.msda_fused(v, torch.zeros((8, 384), device=dev), torch.zeros((8, 3), device=dev), shapes, 1, 8,
                       ref_batched=True)
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------
# box_refine
# ---------------------------------------------------------------------------------------------------------------
def _box_refine_ref(delta, ref, ref_is_logit):
    from oracle import gdino_ref
    d, r = delta.double(), ref.double()
    return torch.sigmoid(d + (r if ref_is_logit else gdino_ref.inverse_sigmoid(r)))


def _run_box_refine(dev, delta, ref, ref_is_logit):
    from inklayer_amd import ops
    d = _strided(delta.to(dev), 12)
    out = _nan_out(tuple(ref.shape), F32, dev)
    got = ops.box_refine(d, ref.to(dev).contiguous(), ref_is_logit=ref_is_logit, out=out)
    assert got.data_ptr() == out.data_ptr()
    return out.cpu()


@torch.no_grad()
@pytest.mark.parametrize("ref_is_logit", [False, True])
def test_box_refine(dev, ref_is_logit):
    """sigmoid(delta + inverse_sigmoid(ref)) (or + ref for logits) vs float64.  Bound 1e-6 absolute: the f32 path
    rounds z with <= 2u |z|, and sigmoid'(z) * |z| <= 0.23, so z contributes <= 0.5 u; expf / 1 + e / reciprocal add
    <= 4 u of the output (<= 1): ~5e-7 < 1e-6.  Logits +-inf map exactly to 1 / 0."""
    rs = np.random.RandomState(5)
    N = 203                                               # 812 elements: 4 workgroups, the last one partial
    if ref_is_logit:
        refs = [float("inf"), float("-inf"), 0.0, 30.0, -30.0, 1e-6]
    else:
        refs = [0.0, 1.0, 1e-4, 1e-3, 1 - 1e-3, 1 - 1e-4, -0.1, 1.1]
    deltas = [0.0, 20.0, -20.0, 100.0, -100.0]
    grid = np.array([(r, d) for r in refs for d in deltas], np.float32)
    ref = (rs.normal(0, 4, N * 4) if ref_is_logit else rs.uniform(0, 1, N * 4)).astype(np.float32)
    delta = rs.normal(0, 3, N * 4).astype(np.float32)
    ref[:len(grid)], delta[:len(grid)] = grid[:, 0], grid[:, 1]
    ref, delta = torch.from_numpy(ref).view(N, 4), torch.from_numpy(delta).view(N, 4)
    got = _run_box_refine(dev, delta, ref, ref_is_logit)
    _assert_within(got.double(), _box_refine_ref(delta, ref, ref_is_logit), 1e-6, "box_refine")
    if ref_is_logit:
        assert (got[ref == float("inf")] == 1.0).all() and (got[ref == float("-inf")] == 0.0).all()


@torch.no_grad()
def test_box_refine_on_plan_proposals(dev):
    """The two-stage anchor step as gdino.py runs it: the plan's unsigmoided proposals (+inf where invalid) gathered
    per image with gather_rows(..., out_dtype=F32) (exact copy), then box_refine(ref_is_logit=True).  Bound as in
    test_box_refine; every +inf proposal component gives exactly 1.0."""
    from inklayer_amd import ops
    B, nq = 2, 900
    pl = _plan(320, 472, B)
    rs = np.random.RandomState(6)
    idx = np.stack([rs.choice(pl.S, nq, replace=False) for _ in range(B)]).astype(np.int32)
    idx[:, :20] = np.nonzero(~torch.isfinite(pl.props_unsig).all(1).numpy())[0][:20]
    props = pl.props_unsig
    assert (~torch.isfinite(props[torch.from_numpy(idx[:, :20]).long()])).all()
    prop = _nan_out((B * nq, 4), F32, dev)
    ops.gather_rows(props.to(dev), torch.from_numpy(idx).to(dev), B, nq, x_batch_rows=0, idx_batch_stride=nq,
                    out_dtype=F32, out=prop)
    want = props[torch.from_numpy(idx).long().view(-1)]
    assert torch.equal(prop.cpu(), want)
    delta = torch.from_numpy(rs.normal(0, 1, (B * nq, 4)).astype(np.float32))
    got = _run_box_refine(dev, delta, prop, True)
    _assert_within(got.double(), _box_refine_ref(delta, want, True), 1e-6, "box_refine on proposals")
    assert (got[want == float("inf")] == 1.0).all()


# ---------------------------------------------------------------------------------------------------------------
# sine_embed4
# ---------------------------------------------------------------------------------------------------------------
@torch.no_grad()
def test_sine_embed4(dev):
    """gen_sineembed_for_position of [N, 4] boxes vs gdino_ref.sine_embed_4d in float64.  Bound: half an f16 ulp
    (2^-11 |ref|) + 1e-6: the f32 argument 2pi*c/dim_t is off by <= 1.5 u |v| <= 5.7e-7 (|v| <= 2pi; the f32 2pi is
    one of the roundings) and sinf / cosf by <= 2 u, together < 1e-6."""
    from inklayer_amd import ops
    from oracle import gdino_ref
    N = 301
    rs = np.random.RandomState(7)
    box = rs.uniform(0, 1, (N, 4)).astype(np.float32)
    box[0], box[1], box[2], box[3] = (0, 1, 0.25, 0.75), (1, 0, 0.5, 0.125), (0, 0, 0, 0), (1, 1, 1, 1)
    box = torch.from_numpy(box)
    dt = torch.arange(128, dtype=torch.float32)          # as GDinoEngine builds w["dim_t"]
    dim_t = 10000 ** (2 * torch.div(dt, 2, rounding_mode="floor") / 128)
    r = gdino_ref.sine_embed_4d(box.double())
    tol = 2.0 ** -11 * r.abs() + 1e-6
    _discriminates(gdino_ref.sine_embed_4d(box[:, [1, 0, 2, 3]].double()), r, tol, "(x, y) blocks swapped")
    _discriminates(gdino_ref.sine_embed_4d(box.double()).view(N, 4, 64, 2).flip(-1).reshape(N, 512), r, tol,
                   "sin / cos interleave swapped")
    out = _nan_out((N, 512), F16, dev)
    ops.sine_embed4(box.to(dev), dim_t.to(dev), out=out)
    got = out.double().cpu()
    _assert_within(got, r, tol, "sine_embed4")


# ---------------------------------------------------------------------------------------------------------------
# layernorm_merge4
# ---------------------------------------------------------------------------------------------------------------
def _nv(C):
    nv = (C + 63) // 64
    return 2 if nv <= 2 else 3 if nv <= 3 else 6 if nv <= 6 else 12 if nv <= 12 else 16


def _merge_tol(xg, r, gamma, beta):
    """Two-pass f32 LayerNorm of one 4C row, f16 out.  The mean is off by dm <= K u mean|x| (K = NV + 10: two in-lane
    adds, NV lane accumulations, six wave levels, the division), which shifts y by |gamma| rstd dm and the variance by
    dm^2; the rest of the path (variance sum, sqrt, reciprocal, three products) is <= (K + 8) u relative to |y - beta|;
    + beta rounds once; the f16 store adds half an ulp (2^-11 |ref|, 1e-7 for subnormals)."""
    K = _nv(xg.shape[1] // 4) + 10
    rstd = 1.0 / torch.sqrt(xg.var(1, unbiased=False, keepdim=True) + 1e-5)
    dm = K * U * xg.abs().mean(1, keepdim=True)
    dev_ = (r - beta).abs()
    return (2.0 ** -11 * r.abs() + gamma.abs() * rstd * dm + ((K + 8) * U + 0.5 * (dm * rstd) ** 2) * dev_
            + U * r.abs() + 1e-7)


def _run_merge(dev, x, gamma, beta, g4):
    from inklayer_amd import ops
    xs = _strided(x.to(dev), x.shape[1] + 8)
    out = _nan_out((g4.shape[0], 4 * x.shape[1]), F16, dev)
    ops.layernorm_merge4(xs, gamma.to(dev), beta.to(dev), 1e-5, g4.to(dev).contiguous(), out=out)
    return out.double().cpu()


@torch.no_grad()
@pytest.mark.parametrize("stage", [0, 1, 2])
@pytest.mark.parametrize("hw", [(300, 412), (328, 468)])
def test_layernorm_merge4_plan(dev, hw, stage):
    """PatchMerging LayerNorm through the plan's host-built merge table, B = 2, at stage sizes from an odd x odd
    (75x103) and an even x odd (82x117) input; C = 96, 192, 384.  Reference: gdino_ref.patch_merging (pad, the
    x0..x3 concat, LayerNorm) in float64 with an identity reduction.  The table itself must equal the same concat
    applied to the token index image."""
    import torch.nn.functional as Fn
    from oracle import gdino_ref
    B = 2
    pl = _plan(hw[0], hw[1], B)
    H, W = pl.stage_hw[stage]
    C = 96 * 2 ** stage
    idx = torch.arange(B * H * W, dtype=F64).view(B, H, W, 1)
    idx = Fn.pad(idx, (0, 0, 0, W % 2, 0, H % 2), value=-1)
    table = torch.cat([idx[:, 0::2, 0::2], idx[:, 1::2, 0::2], idx[:, 0::2, 1::2], idx[:, 1::2, 1::2]], -1)
    assert torch.equal(pl.merge_map[stage], table.reshape(-1, 4).to(torch.int32))
    rs = np.random.RandomState(20 + stage)
    x = torch.from_numpy(rs.standard_normal((B * H * W, C)).astype(np.float32) * 2 + 0.5)
    gamma = torch.from_numpy((1 + 0.3 * rs.standard_normal(4 * C)).astype(np.float32))
    beta = torch.from_numpy((0.2 * rs.standard_normal(4 * C)).astype(np.float32))
    sd = {"m.norm.weight": gamma.double(), "m.norm.bias": beta.double(), "m.reduction.weight": torch.eye(4 * C, dtype=F64)}
    r = gdino_ref.patch_merging(sd, "m.", x.double().view(B, H * W, C), H, W).reshape(-1, 4 * C)
    g = pl.merge_map[stage].long()
    xg = torch.cat([torch.where(g[:, k:k + 1] >= 0, x.double()[g[:, k].clamp(min=0)], 0.0) for k in range(4)], 1)
    tol = _merge_tol(xg, r, gamma.double(), beta.double())
    swapped = sd.copy()
    perm = torch.cat([torch.arange(C), torch.arange(2 * C, 3 * C), torch.arange(C, 2 * C), torch.arange(3 * C, 4 * C)])
    swapped["m.reduction.weight"] = torch.eye(4 * C, dtype=F64)[perm]
    wrong = gdino_ref.patch_merging(swapped, "m.", x.double().view(B, H * W, C), H, W).reshape(-1, 4 * C)
    _discriminates(wrong, r, tol, "x1 / x2 concat order swapped")
    got = _run_merge(dev, x, gamma, beta, pl.merge_map[stage])
    _assert_within(got, r, tol, f"layernorm_merge4 stage {stage}")


@torch.no_grad()
@pytest.mark.parametrize("C", [4, 100, 700, 1000, 1024])
def test_layernorm_merge4_synthetic(dev, C):
    """Synthetic gather tables (every NV template branch together with the plan's C), 203 rows (not a multiple of 4),
    random -1 entries; row 0 has four -1 sources (output exactly f16(beta)); row 1 gathers four rows of 1e3 + a
    spread of 1e-2 (a one-pass variance loses it).  Bound: see _merge_tol."""
    import torch.nn.functional as Fn
    rs = np.random.RandomState(C)
    R, rows = 97, 203
    x = rs.standard_normal((R, C)).astype(np.float32)
    x[:4] = 1e3 + rs.uniform(-1e-2, 1e-2, (4, C))
    x = torch.from_numpy(x)
    g4 = rs.randint(4, R, (rows, 4))
    g4[rs.rand(rows, 4) < 0.2] = -1
    g4[0], g4[1] = -1, (0, 1, 2, 3)
    g4 = torch.from_numpy(g4.astype(np.int32))
    gamma = torch.from_numpy((1 + 0.3 * rs.standard_normal(4 * C)).astype(np.float32))
    beta = torch.from_numpy((0.2 * rs.standard_normal(4 * C)).astype(np.float32))
    g = g4.long()
    xg = torch.cat([torch.where(g[:, k:k + 1] >= 0, x.double()[g[:, k].clamp(min=0)], 0.0) for k in range(4)], 1)
    r = Fn.layer_norm(xg, (4 * C,), gamma.double(), beta.double(), 1e-5)
    tol = _merge_tol(xg, r, gamma.double(), beta.double())
    xw = torch.cat([xg[:, C:2 * C], xg[:, :C], xg[:, 2 * C:]], 1)
    _discriminates(Fn.layer_norm(xw, (4 * C,), gamma.double(), beta.double(), 1e-5), r, tol, "sources 0 / 1 swapped")
    got = _run_merge(dev, x, gamma, beta, g4)
    assert torch.equal(got[0].half(), beta.half())
    _assert_within(got, r, tol, f"layernorm_merge4 C={C}")


# ---------------------------------------------------------------------------------------------------------------
# swin_patchify
# ---------------------------------------------------------------------------------------------------------------
def _swin_unfold(x):
    """[3, h, w] normalised image -> [tokens, 64]: c*16 + ky*4 + kx, zero pad to multiples of 4, columns 48.. zero."""
    import torch.nn.functional as Fn
    _, h, w = x.shape
    gh, gw = -(-h // 4), -(-w // 4)
    x = Fn.pad(x, (0, 4 * gw - w, 0, 4 * gh - h))
    t = x.view(3, gh, 4, gw, 4).permute(1, 3, 0, 2, 4).reshape(gh * gw, 48)
    return torch.cat([t, torch.zeros(gh * gw, 16, dtype=t.dtype)], 1)


@torch.no_grad()
@pytest.mark.parametrize("hw", [(803, 1201), (5, 7)])
def test_swin_patchify(dev, hw):
    """load_image's ToTensor + Normalize and the 4x4 PatchEmbed gather.  The kernel does the same f32 operations in the
    same order ((u8 / 255 - mean) / std), so the result is bit-equal to that f32 computation rounded to f16; it is also
    within half an f16 ulp + 2^-22 relative (three f32 roundings) of the float64 value."""
    from inklayer_amd import gdino, ops
    h, w = hw
    rs = np.random.RandomState(h)
    img = rs.randint(0, 256, (h, w, 3)).astype(np.uint8)
    cfg = gdino.GDinoConfig()
    u8 = torch.from_numpy(img).permute(2, 0, 1)
    mean, std = torch.tensor(cfg.pixel_mean).view(3, 1, 1), torch.tensor(cfg.pixel_std).view(3, 1, 1)
    want = _swin_unfold((u8.float() / 255.0 - mean) / std).half()
    r64 = _swin_unfold((u8.double() / 255.0 - mean.double()) / std.double())
    tol = (2.0 ** -11 + 2.0 ** -22) * r64.abs() + 2.0 ** -25
    wrong = r64.view(-1, 4, 16)[:, :3].reshape(-1, 3, 4, 4).transpose(2, 3).reshape(-1, 48)
    _discriminates(wrong, r64[:, :48], tol[:, :48], "ky / kx swapped")
    gh, gw = -(-h // 4), -(-w // 4)
    out = torch.full((gh * gw, 64), NAN, dtype=F16, device=dev)
    ops.swin_patchify(torch.from_numpy(img).to(dev), cfg.pixel_mean, cfg.pixel_std, out)
    got = out.cpu()
    assert torch.equal(got.view(torch.int16), want.view(torch.int16))
    _assert_within(got.double(), r64, tol, "swin_patchify vs float64")


# ---------------------------------------------------------------------------------------------------------------
# gather_rows
# ---------------------------------------------------------------------------------------------------------------
GATHER_MODES = {   # (x_batch_rows, idx_batch_stride): shared source (proposals), shared index (valid_map), both batched
    "shared_x": (0, 1), "shared_idx": (1, 0), "batched": (1, 1)}


@torch.no_grad()
@pytest.mark.parametrize("out_dtype", [F16, F32], ids=["f16", "f32"])
@pytest.mark.parametrize("mode", sorted(GATHER_MODES))
@pytest.mark.parametrize("C", [4, 256])
def test_gather_rows(dev, C, mode, out_dtype):
    """out[b, r] = x[b * x_batch_rows + idx[b * idx_batch_stride + r]] (-1 -> zeros), exact: equal to x[idx] (f32) and
    to x[idx].half() (f16), incl. f16 overflow and subnormals.  C = 256, B = 3 x 5501 rows is past the 4096-workgroup
    grid-stride wrap."""
    from inklayer_amd import ops
    xb, ib = GATHER_MODES[mode]
    B, S, nq = 3, 9001, 5501
    rs = np.random.RandomState(C + len(mode))
    nsrc = B * S if xb else S
    x = rs.standard_normal((nsrc, C)).astype(np.float32)
    x[1, :4] = (70000.0, -1e-6, 3e-5, 65504.0)
    x = torch.from_numpy(x)
    nidx = B * nq if ib else nq
    idx = rs.randint(0, S, nidx).astype(np.int32)
    idx[rs.rand(nidx) < 0.1] = -1
    idx[:3] = (1, -1, S - 1)
    idx = torch.from_numpy(idx)
    x_batch_rows, idx_batch_stride = S * xb, nq * ib

    def reference(x_batch_rows):
        src = torch.stack([x_batch_rows * b + idx[b * idx_batch_stride: b * idx_batch_stride + nq].long()
                           for b in range(B)]).view(-1)
        keep = torch.stack([idx[b * idx_batch_stride: b * idx_batch_stride + nq] >= 0 for b in range(B)]).view(-1, 1)
        return torch.where(keep, x[src.clamp(min=0, max=nsrc - 1)], torch.zeros(()))
    want = reference(x_batch_rows)
    if xb:                                                     # a per-image source read as shared is seen
        assert not torch.equal(reference(0), want)
    out = _nan_out((B * nq, C), out_dtype, dev)
    got = ops.gather_rows(_strided(x.to(dev), C + 4), idx.to(dev), B, nq, x_batch_rows=x_batch_rows,
                          idx_batch_stride=idx_batch_stride, out_dtype=out_dtype, out=out)
    assert got.data_ptr() == out.data_ptr()
    got = got.cpu()
    want = want.to(out_dtype)
    itype = torch.int16 if out_dtype == F16 else torch.int32
    assert torch.equal(got.view(itype), want.view(itype))


# ---------------------------------------------------------------------------------------------------------------
# flash_attn bias_mode 3: Swin-T window attention
# ---------------------------------------------------------------------------------------------------------------
SWIN_HEADS = (3, 6, 12, 24)
SWIN_SCALE = 32 ** -0.5


def _swin_attn_ref(q, k, v, sb, sm, pad_keys=0):
    """float64 softmax(scale q k^T + sb + sm[window % nW]) v for q, k, v [Bw, nh, 49, 32], sb [nh, 49, 49] (logit
    units), sm [nW, 49, 49] or None.  pad_keys: that many extra keys of score 0 and value 0 (a mistake)."""
    s = SWIN_SCALE * (q @ k.transpose(-1, -2)) + sb[None]
    if sm is not None:
        s = s + sm[torch.arange(q.shape[0]) % sm.shape[0]][:, None]
    m = s.amax(-1, keepdim=True)
    e = torch.exp(s - m)
    den = e.sum(-1, keepdim=True) + pad_keys * torch.exp(-m)
    return (e / den) @ v, e / den, s


def _swin_attn_tol(q, k, v, sb, sm, P, s, o):
    """Bound of the HD = 32 bias_mode 3 path (one 64-key tile, no running-max rescale, LSUM_MFMA false).
    Scores: acc = bias (+ mask, one f32 add) + q.k (32 exact f16 products, f32 accumulation), then
    p = exp2(acc * c - m) with c = f32(scale log2 e); in natural-log units each p_k is off by a relative
    delta_k <= 40 u (scale sum|q k| + |sb| + |sm|) + 2 u |max_k s| + 4 u (accumulation, c, the fma and exp2 roundings),
    which moves o by <= sum_k P_k delta_k |v_k - o|.  P is rounded to f16 before the PV MFMA while l is summed in f32
    from the unrounded P, so the f16 rounding does not cancel: 2^-11 sum_k P_k |v_k| (2^-25 |v_k| absolute for P in the
    f16 subnormal range; sum p >= 1 since the max key has p = 1).  The PV accumulation adds 64 u sum P|v|, the l sum
    (33 terms), reciprocal and product 36 u |o|, the f16 store half an ulp (2^-11 |o|, 2^-25 subnormal)."""
    mag = SWIN_SCALE * (q.abs() @ k.abs().transpose(-1, -2)) + sb.abs()[None]
    if sm is not None:
        mag = mag + sm.abs()[torch.arange(q.shape[0]) % sm.shape[0]][:, None]
    delta = 40 * U * mag + 2 * U * s.amax(-1, keepdim=True).abs() + 4 * U
    Pd = P * delta
    va = v.abs()
    A = P @ va
    return (Pd @ va + Pd.sum(-1, keepdim=True) * o.abs() + (2.0 ** -11 + 64 * U) * A
            + 2.0 ** -25 * va.sum(-2, keepdim=True) + (2.0 ** -11 + 36 * U) * o.abs() + 2.0 ** -25)


def _swin_attn_inputs(pl, i, shifted, seed):
    """The packed qkv buffer as the engine hands it to flash_attn: f16 [B*nW*49, 3C + 8] in window order (plan.win_map),
    NaN in the 8 padding columns, one shared bias-only row where the map is -1; and the f32 dense bias of a std-1.0
    table, NaN in keys 49-63 (and the plan's mask, NaN in keys 49-63)."""
    from inklayer_amd import gdino
    nh = SWIN_HEADS[i]
    C = 32 * nh
    H, W = pl.stage_hw[i]
    g = torch.Generator().manual_seed(seed)
    tok = torch.randn(pl.B * H * W, 3 * C, generator=g).half()
    bias_row = (0.5 * torch.randn(3 * C, generator=g)).half()
    wm = pl.win_map[i][shifted].long()
    rows = torch.where(wm[:, None] >= 0, tok[wm.clamp(min=0)], bias_row[None])
    buf = torch.full((wm.numel(), 3 * C + 8), NAN, dtype=F16)
    buf[:, :3 * C] = rows
    dense = gdino.swin_dense_bias(torch.randn(169, nh, generator=g), 7, nh, SWIN_SCALE)
    mask = pl.shift_mask[i].clone() if shifted else None
    return buf, dense, mask


def _nan_keys(t):
    t = t.clone()
    t[:, :, 49:] = NAN
    return t


@torch.no_grad()
@pytest.mark.parametrize("shifted", [0, 1])
@pytest.mark.parametrize("stage", [0, 1, 2, 3])
@pytest.mark.parametrize("hw", [(800, 800), (800, 1066)])
def test_flash_attn_swin_windows(dev, hw, stage, shifted):
    """flash_attn_kernel<32, 3, 2> called as GDinoEngine._swin_block calls it, B = 2 (n_batch = 2 nW: up to 2262
    windows), the stage's heads, q / k / v column slices of one packed buffer, against float64 attention.  The NaN keys
    49-63 of dense_bias / dense_mask pin that the kernel overwrites keys >= n_k; `out` is a NaN-filled slice whose 64
    following rows must stay NaN.  Bound: _swin_attn_tol."""
    from oracle import gdino_ref
    from inklayer_amd import ops
    B = 2
    pl = _plan(hw[0], hw[1], B)
    nh, nW = SWIN_HEADS[stage], pl.nW[stage]
    C, Bw = 32 * nh, B * nW
    buf, dense, mask = _swin_attn_inputs(pl, stage, shifted, 1000 * stage + 10 * shifted + hw[1] % 7)
    qkv = buf[:, :3 * C].double().view(Bw, 49, 3, nh, 32).permute(2, 0, 3, 1, 4)
    q, k, v = qkv[0], qkv[1], qkv[2]
    sb = SWIN_SCALE * dense[:, :, :49].double()
    sm = SWIN_SCALE * mask[:, :, :49].double() if shifted else None
    o, P, s = _swin_attn_ref(q, k, v, sb, sm)
    tol = _swin_attn_tol(q, k, v, sb, sm, P, s, o)
    wrongs = {"bias transposed to [h, k, q]": _swin_attn_ref(q, k, v, sb.transpose(1, 2), sm)[0],
              "bias of head h + 1": _swin_attn_ref(q, k, v, sb.roll(-1, 0), sm)[0],
              "15 zero-score padding keys admitted": _swin_attn_ref(q, k, v, sb, sm, pad_keys=15)[0],
              "bias multiplied by scale": _swin_attn_ref(q, k, v, sb * SWIN_SCALE, sm)[0]}
    if shifted:
        H, W = pl.stage_hw[stage]
        Hp, Wp = -(-H // 7) * 7, -(-W // 7) * 7
        wrongs["mask of window (w + 1) % nW"] = _swin_attn_ref(q, k, v, sb, sm.roll(-1, 0))[0]
        wrongs["mask omitted"] = _swin_attn_ref(q, k, v, sb, None)[0]
        if Hp != Wp:
            smt = SWIN_SCALE * (gdino_ref.swin_shift_mask(Wp, Hp, 7) / SWIN_SCALE).double()
            wrongs["window grid transposed"] = _swin_attn_ref(q, k, v, sb, smt)[0]
    for what, wrong in wrongs.items():
        _discriminates(wrong, o, tol, what)
        print(f"  {what}: {((wrong - o).abs() / tol).max().item():.0f}x the bound")
    bd = buf.to(dev)
    full = _nan_out((Bw * 49 + 64, C), F16, dev)
    got = ops.flash_attn(bd[:, :C], bd[:, C:2 * C], bd[:, 2 * C:3 * C], n_batch=Bw, n_heads=nh, head_dim=32,
                         scale=SWIN_SCALE, n_q=49, n_k=49, dense_bias=_nan_keys(dense).to(dev),
                         dense_mask=_nan_keys(mask).to(dev) if shifted else None, out=full[:Bw * 49])
    assert got.data_ptr() == full.data_ptr()
    full = full.cpu()
    assert full[Bw * 49:].isnan().all()
    got = full[:Bw * 49].double().view(Bw, 49, nh, 32).permute(0, 2, 1, 3)
    print(f"{hw} stage {stage} shifted {shifted}: worst error {((got - o).abs() / tol).max().item():.3f}x the bound")
    _assert_within(got, o, tol, f"flash_attn bias_mode 3 {hw} stage {stage} shifted {shifted}")


# ---------------------------------------------------------------------------------------------------------------
# one Swin block through the engine
# ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def swin_engine(dev):
    """A 2-encoder / 2-decoder engine from seeded weights (as test_gdino_gpu.small_dino), with the relative-position
    bias tables scaled from std 0.2 to std 1.0 so that a wrong bias is seen."""
    from oracle import gdino_ref, sam_ref
    from inklayer_amd import gdino
    oc = gdino_ref.GDinoConfig(enc_layers=2, dec_layers=2, num_queries=300)
    sd = sam_ref.seeded_state_dict(gdino_ref.gdino_param_shapes(oc), 77)
    for k in sd:
        if k.endswith("relative_position_bias_table"):
            sd[k] = sd[k] * 5.0
    rs = np.random.RandomState(3)
    text = torch.from_numpy((0.5 * rs.standard_normal((4, 256))).astype(np.float32))
    eng = gdino.GDinoEngine(sd, gdino.GDinoConfig(enc_layers=2, dec_layers=2, num_queries=300), dev, encoded_text=text)
    return sd, eng


SWIN_BLOCK_ABS = 2.0 ** -12


@torch.no_grad()
@pytest.mark.parametrize("block", [0, 1])
@pytest.mark.parametrize("stage", [0, 3])
@pytest.mark.parametrize("hw", [(800, 800), (800, 1066)])
def test_swin_block_matches_float64(dev, swin_engine, hw, stage, block):
    """GDinoEngine._swin_block (block 0 unshifted, block 1 shifted) on random f32 tokens, B = 2, against
    gdino_ref.swin_block in float64.  Yardstick of test_detector_stages_match_oracle: every error quantile, the maximum
    included, is at most 2x that of the float64 oracle re-run with f16-rounded linear operands, plus
    SWIN_BLOCK_ABS * max|block update| (a quarter of an f16 ulp of the largest update), for what the yardstick does
    not round: q, k, v and P inside the attention, each to f16."""
    from oracle import gdino_ref
    sd, eng = swin_engine
    B = 2
    pl = eng.plan(hw[0], hw[1], B)
    H, W = pl.stage_hw[stage]
    C, nh = 96 * 2 ** stage, SWIN_HEADS[stage]
    g = torch.Generator().manual_seed(100 * stage + block)
    x = torch.randn(B * H * W, C, generator=g)
    xd = x.to(dev)
    eng._swin_block(xd, stage, block, pl)
    got = xd.double().cpu()
    p = f"backbone.0.layers.{stage}.blocks.{block}."
    sd64 = {k: v.double() for k, v in sd.items() if k.startswith(p)}
    Hp, Wp = -(-H // 7) * 7, -(-W // 7) * 7
    mask = gdino_ref.swin_shift_mask(Hp, Wp, 7).double()
    args = (p, x.double().view(B, H * W, C), H, W, nh, 7, 3 if block else 0, mask)
    ref = gdino_ref.swin_block(sd64, *args).reshape(-1, C)
    with gdino_ref.f16_operands():
        emul = gdino_ref.swin_block(sd64, *args).reshape(-1, C)
    a = SWIN_BLOCK_ABS * (ref - x.double()).abs().max().item()
    err = (got - ref).abs().flatten().numpy()
    eerr = (emul - ref).abs().flatten().numpy()
    assert np.isfinite(err).all()
    for qt in (0.5, 0.9, 0.99, 0.999, 1.0):
        hq, eq = float(np.quantile(err, qt)), float(np.quantile(eerr, qt))
        print(f"{hw} stage {stage} block {block} q{qt}: HIP {hq:.2e}  emulated-f16 {eq:.2e}  "
              f"-> {hq / (2 * eq + a):.3f}x the bound")
        assert hq <= 2 * eq + a, (qt, hq, eq, a)


# ---------------------------------------------------------------------------------------------------------------
# fusion_fold at production S
# ---------------------------------------------------------------------------------------------------------------
FOLD_CASES = [(13294, 1), (13294, 2), (13294, 3), (13294, 4), (17821, 4), (22223, 4)]   # 800x800 / x1066 / x1333
FOLD_PLANT = ((0, 5), (1, -3))          # (image, token): chunk 0 of image 0, the ragged last chunk of image 1
FOLD_COL = (1, 0)                       # (head, text token) of the planted column
FOLD_HEAVY = ((0, 2), (1, 3))           # (image, head) with a heavy column-statistics chunk in text token 0's column


def _fold_heavy_rows(S):
    """The first row of the heavy 512-row column-statistics chunk of each image: one in the middle of image 0, the first
    one of image 1."""
    return (S // 1024) * 512, 0
_FOLD = {}


def _fold_data(S):
    """Weights, text projections (T = 4; a case with T < 4 takes the first T tokens), image tokens with a +20 mean, and
    the float64 image side (vn, q, value_v: independent of T), for one S; only the latest S is kept.  The tokens of each
    128-token apply chunk share a random offset (the chunk's signature), and the tokens of one 512-row column-statistics
    chunk per image (_fold_heavy_rows) lean towards the folded query direction U of text token 0 of head FOLD_HEAVY, so
    that chunk holds about half of that column's sum-exp.  Token FOLD_PLANT of each image is aligned with the folded query direction U of column FOLD_COL, whose text key is 3x wider: it
    dominates that column's softmax over the image tokens (score ~30 against ~9 for the rest)."""
    if S in _FOLD:
        return _FOLD[S]
    _FOLD.clear()
    B, E, D = 2, 1024, 256
    g = torch.Generator().manual_seed(S)
    d = SimpleNamespace(B=B, S=S)
    d.Wqv = (torch.randn(2 * E, D, generator=g) / D ** 0.5).half()
    d.bqv = 0.1 * torch.randn(2 * E, generator=g)
    d.bqv[E:] *= 0.2                        # a small values_v bias: out_l is mostly the image tokens' contribution
    d.Wo = (torch.randn(D, E, generator=g) / E ** 0.5).half()
    d.bo = 0.1 * torch.randn(D, generator=g)
    d.lng, d.lnb = 1 + 0.1 * torch.randn(D, generator=g), 0.1 * torch.randn(D, generator=g)
    d.gam = 0.2 + 0.1 * torch.randn(D, generator=g)
    d.kl = torch.randn(B, 4, 2 * E, generator=g)
    h, t = FOLD_COL
    d.kl[:, t, h * 256:(h + 1) * 256] *= 3
    d.pos = torch.randn(S, D, generator=g)
    # every 128-token apply chunk has a signature of its own, so that each chunk moves the text side measurably
    sig = 1.5 * torch.randn(B, -(-S // 128), D, generator=g)
    v = torch.randn(B, S, D, generator=g) * 1.3 + 20 + sig.repeat_interleave(128, 1)[:, :S]
    udir = lambda b, h: d.Wqv[h * 256:(h + 1) * 256].double().t() @ d.kl[b, 0, h * 256:(h + 1) * 256].double()
    for (b, hh), lo in zip(FOLD_HEAVY, _fold_heavy_rows(S)):   # scores ~3 higher: ~half the column's sum-exp
        u = udir(b, hh)
        v[b, lo:lo + 512] += (6.4 * u / u.norm()).float()
    for b, s in FOLD_PLANT:
        u = udir(b, h)
        v[b, s] = (20 + 16 * u / u.norm()).float()
    d.v = v.view(B * S, D)
    d.vn = torch.nn.functional.layer_norm(d.v.double(), (D,), d.lng.double(), d.lnb.double(), 1e-5).view(B, S, D)
    d.q = (d.vn @ d.Wqv[:E].double().t() + d.bqv[:E].double()) * 256 ** -0.5
    d.vv = d.vn @ d.Wqv[E:].double().t() + d.bqv[E:].double()
    _FOLD[S] = d
    return d


def _fold_reference(d, T, num=None, den=None):
    """The reference's order of operations in float64 (test_folded_fusion_layer_equals_the_full_one).  num / den
    (mistakes): per-token multipliers [B, S] of the text side's weights exp(s - max) in the weighted sum of the image
    tokens and in the sum-exp, e.g. a chunk left out (0) or counted twice (2)."""
    B, S, E = d.B, d.S, 1024
    k, vl = d.kl[:, :T, :E].double(), d.kl[:, :T, E:].double()
    sp = lambda x: x.reshape(B, -1, 4, 256).transpose(1, 2)
    aw = sp(d.q) @ sp(k).transpose(-1, -2)                                # [B, 4, S, T]
    ov = (aw.softmax(-1) @ sp(vl)).transpose(1, 2).reshape(B, S, E)
    awl = aw.transpose(-1, -2)                                            # [B, 4, T, S]
    if num is None and den is None:
        ol = awl.softmax(-1) @ sp(d.vv)
    else:
        e = torch.exp(awl - awl.amax(-1, keepdim=True))
        one = torch.ones(B, S, dtype=F64)
        en = e * (one if num is None else num)[:, None, None]
        ed = e * (one if den is None else den)[:, None, None]
        ol = (en @ sp(d.vv)) / ed.sum(-1, keepdim=True)
    ol = ol.transpose(1, 2).reshape(B * T, E)
    want_v = (d.vn + d.gam.double() * (ov @ d.Wo.double().t() + d.bo.double())).view(B * S, 256)
    return want_v, ol, aw


def _fold_tol(d, T, aw, want_v, ol):
    """Per-element bounds of csrc/fusion_fold.hip (f32 throughout, f16 only for out_l).
    vn: two-pass LayerNorm, one wave per row: the mean is off by dm <= 10 u mean|x| (four in-lane adds, six wave levels,
      the scale), which moves vn by |g| rstd dm; the rest <= 18 u |vn - b| + u |vn| (as _merge_tol).
    scores s = vn . U + c with U = scale Wq_h^T k (256-term fma chain: <= 257 u Uabs, Uabs = scale |Wq_h|^T |k|) and a
      16-lane reduction (<= 12 u |vn| . Uabs); c = scale bq_h . k (<= 12 u scale |bq|.|k|): ds = dvn . Uabs +
      270 u |vn| . Uabs + 12 u cabs + u |s|.
    image side: p = softmax over the T tokens: relative error <= ds_t + max_t ds + 5 u; o = bo + sum_t p_t Z_t with
      Z = Wo_h vl (<= 257 u Zabs): do <= sum |dp| |Z| + sum p 257 u Zabs + 17 u (|bo| + sum p |Z|); the update
      v = vn + g o rounds twice.
    text side, per output e of column (h, t): out_l = bvv + Wvv_h m, m = sum_s w_s vn_s / sum_s w_s, w_s = exp(s - M),
      and the reference is ol = sum_s P_s vv_s, so a relative change x_s of token s's weight moves it by
      P_s x_s (vv_s - ol).  Terms: (1) each token's own score error, any sign: the 16-lane dot product (10 u),
      LayerNorm's element roundings (5 u), its mean error dm along the exact direction g . U and its rstd error along
      (vn - b) . U, with the exact U: sum_s P_s ds_s |vv_s - ol|; the error of c and of M shift every token alike and
      cancel.  (2) The kernel's U (a 256-step fma chain: <= u sum_n |partial_n| + u |U|) is common to all tokens: it
      moves ol by (sum_s P_s (vv_s - ol)(vn_s - m)^T) dU.  (3) The exp roundings (u |s - M| + 2 u) differ between the
      weighted sum and the sum-exp; the sum-exp is combined from 512-row chunks ((3 ncs + 40) u).  (4) The weighted sum
      runs 32 tokens per wave, 4 waves, the chunks: (40 + nchunk / 8) u |Wvv_h| sum_s P_s |vn_s|.  (5) vn's own errors
      in that sum: the mean error along Wvv_h g, the element roundings through |Wvv_h|.  (6) The output projection, a
      fma chain from bvv: u sum_n |partial_n|.  Then the f16 store (2^-11 |out_l|, 2^-25 subnormal)."""
    B, S, E = d.B, d.S, 1024
    vn = d.vn
    xs = d.v.double().view(B, S, 256)
    rstd = 1.0 / torch.sqrt(xs.var(-1, unbiased=False, keepdim=True) + 1e-5)
    dm = 10 * U * xs.abs().mean(-1, keepdim=True)
    dvn = d.lng.double().abs() * rstd * dm + 18 * U * (vn - d.lnb.double()).abs() + U * vn.abs()
    kabs = d.kl[:, :T, :E].double().abs().view(B, T, 4, 256)
    vlabs = d.kl[:, :T, E:].double().abs().view(B, T, 4, 256)
    Wq = d.Wqv[:E].double().abs().view(4, 256, 256)                       # [h, out, in]
    Uabs = 256 ** -0.5 * torch.einsum("hoi,btho->bhti", Wq, kabs)          # [B, 4, T, 256]
    cabs = 256 ** -0.5 * torch.einsum("ho,btho->bht", d.bqv[:E].double().abs().view(4, 256), kabs)
    s = aw                                                                 # [B, 4, S, T]
    ds = (torch.einsum("bsi,bhti->bhst", dvn + 270 * U * vn.abs(), Uabs) + 12 * U * cabs[:, :, None, :]
          + U * s.abs())
    # image side
    p = s.softmax(-1)
    dp = p * (ds + ds.amax(-1, keepdim=True) + 5 * U)
    Wo = d.Wo.double().view(256, 4, 256)                                   # [out, h, in]
    Z = torch.einsum("ohi,bthi->bhto", Wo, d.kl[:, :T, E:].double().view(B, T, 4, 256))
    Zabs = torch.einsum("ohi,bthi->bhto", Wo.abs(), vlabs)
    pZ = torch.einsum("bhst,bhto->bso", p, Z.abs())
    do = (torch.einsum("bhst,bhto->bso", dp, Z.abs()) + 257 * U * torch.einsum("bhst,bhto->bso", p, Zabs)
          + 17 * U * (d.bo.double().abs() + pZ))
    o = (want_v.view(B, S, 256) - vn) / d.gam.double()
    tol_v = dvn + d.gam.double().abs() * do + U * (d.gam.double() * o).abs() + U * want_v.view(B, S, 256).abs()
    # text side, per output e of column (h, t): the reference is ol = sum_s P_s vv_s with P = softmax over s and
    # vv_s = Wvv_h vn_s + bvv, so a change of token s's weight by a relative x_s moves ol by P_s x_s (vv_s - ol)
    nchunk, ncs = -(-S // 128), -(-S // 512)
    g, bb = d.lng.double(), d.lnb.double()
    Ws = d.Wqv[:E].double().view(4, 256, 256)
    Ue = 256 ** -0.5 * torch.einsum("hoi,btho->bhti", Ws, d.kl[:, :T, :E].double().view(B, T, 4, 256))   # exact U
    st = s.transpose(-1, -2)                                               # [B, 4, T, S]
    P = st.softmax(-1)
    rdm = (rstd * dm)[..., 0]                                              # [B, S]
    dss = (torch.einsum("bsi,bhti->bhts", 15 * U * vn.abs() + 5 * U * bb.abs(), Ue.abs())
           + rdm[:, None, None] * torch.einsum("i,bhti->bht", g, Ue).abs()[..., None]
           + 10 * U * torch.einsum("bsi,bhti->bhts", vn - bb, Ue).abs() + U * st.abs())
    eps = U * (st - st.amax(-1, keepdim=True)).abs() + 2 * U
    vvh = d.vv.view(B, S, 4, 256)
    bvv = d.bqv[E:].double().view(4, 256)
    Wvv = d.Wqv[E:].double().view(4, 256, 256)                             # [h, out, in]
    olh = ol.view(B, T, 4, 256)
    m = torch.einsum("bhts,bsi->bhti", P, vn)
    # U: a 256-step fma chain over d (from 0), then * scale: <= u sum_n |partial_n| + u |U|
    kt = d.kl[:, :T, :E].double().view(B, T, 4, 256)
    part = torch.cumsum(Ws.permute(0, 2, 1)[None, :, None] * kt.permute(0, 2, 1, 3)[..., None, :], -1)   # [B,4,T,i,d]
    dU = U * (256 ** -0.5 * part.abs().sum(-1) + Ue.abs())
    lnr = 12 * U * (vn - bb).abs() + U * vn.abs()
    tol_l = torch.empty(B, T, 4, 256, dtype=F64)
    for h in range(4):
        Wa = Wvv[h].abs()
        Wg = (Wvv[h] @ g).abs()
        for t in range(T):
            p_, r = P[:, h, t], vvh[:, :, h] - olh[:, t, h, None]          # [B, S], [B, S, 256]
            t1 = torch.einsum("bs,bse->be", p_ * dss[:, h, t], r.abs())   # per-token score errors, any signs
            G = torch.einsum("bse,bsi->bei", p_[..., None] * r, vn - m[:, h, t, None])
            t2 = (G.abs() @ dU[:, h, t, :, None])[..., 0]                  # the kernel's U, common to all tokens
            pe = p_ * eps[:, h, t]                                         # exp roundings, not shared by the two sums
            t3 = (torch.einsum("bs,bse->be", pe, (vvh[:, :, h] - bvv[h]).abs())
                  + (olh[:, t, h] - bvv[h]).abs() * (pe.sum(-1, keepdim=True) + (3 * ncs + 40) * U))
            pvn = torch.einsum("bs,bsi->bi", p_, vn.abs())
            t4 = (40 + nchunk / 8) * U * pvn @ Wa.t() + U * m[:, h, t].abs() @ Wa.t()
            t5 = (p_ * rdm).sum(-1, keepdim=True) * Wg + torch.einsum("bs,bsi->bi", p_, lnr) @ Wa.t()
            # out_l = fma chain over the 256 inputs from bvv: each step rounds its partial sum once
            part = bvv[h][None, :, None] + torch.cumsum(Wvv[h][None] * m[:, h, t, None, :], -1)
            t6 = U * part.abs().sum(-1)
            tol_l[:, t, h] = t1 + t2 + t3 + t4 + t5 + t6
    tol_l = tol_l.reshape(B * T, E) + 2.0 ** -11 * ol.abs() + 2.0 ** -25
    return tol_v.reshape(B * S, 256), tol_l


def _run_fold(dev, v, kl, T, d, B, S):
    from inklayer_amd import ops
    vd = v.to(dev).contiguous().clone()
    kl = kl.to(dev)
    o16 = _nan_out((B * S, 256), F16, dev)
    o16p = _nan_out((B * S, 256), F16, dev)
    out_l = ops.fusion_fold(vd, B, S, d.lng.to(dev), d.lnb.to(dev), 1e-5, kl, T, d.Wqv.to(dev), d.bqv.to(dev),
                            d.Wo.to(dev), d.bo.to(dev), d.gam.to(dev), 256 ** -0.5, pos=d.pos.to(dev), out16_pos=o16p,
                            out16=o16)
    return vd.cpu(), out_l.cpu(), o16.cpu(), o16p.cpu()


@torch.no_grad()
@pytest.mark.parametrize("S,T", FOLD_CASES)
def test_fusion_fold_production_sizes(dev, S, T):
    """ops.fusion_fold as the encoder calls it (pos, out16, out16_pos, text_kv with NaN padding columns), B = 2, at the
    production token counts (104-174 apply chunks, 26-44 column-statistics chunks), against the float64 layer;
    per-element bounds of _fold_tol.  The bound sees a wrong chunk combine: a 512-row column-statistics chunk left out
    of the sum-exp (the heavy ones of _fold_data, and the ragged last one of image 1, which holds a planted token), a 128-row
    apply chunk counted twice in the weighted sum or left out of both (in the middle of
    image 0 and in the ragged last chunk of image 1, never the planted token's), and the planted token left out.
    out16 / out16_pos equal f16(v) and f16(v + pos) of the kernel's own f32 output bit for bit."""
    d = _fold_data(S)
    B = d.B
    want_v, ol, aw = _fold_reference(d, T)
    tol_v, tol_l = _fold_tol(d, T, aw, want_v, ol)

    def tokens(b, lo, hi, val):
        x = torch.ones(B, S, dtype=F64)
        x[b, lo:hi] = val
        return x
    mid, last = (S // 384) * 128, (S - 1) // 128 * 128           # two apply chunks without a planted token
    cs0, cs1 = _fold_heavy_rows(S)
    wrongs = {"column-statistics chunk left out of the sum-exp (image 0)": dict(den=tokens(0, cs0, cs0 + 512, 0.0)),
              "first column-statistics chunk left out of the sum-exp (image 1)": dict(den=tokens(1, cs1, cs1 + 512, 0.0)),
              "ragged last column-statistics chunk left out of the sum-exp (image 1)":
                  dict(den=tokens(1, (S - 1) // 512 * 512, S, 0.0)),
              "apply chunk counted twice in the weighted sum (image 0)": dict(num=tokens(0, mid, mid + 128, 2.0)),
              "apply chunk left out of both sums (image 0)": dict(num=tokens(0, mid, mid + 128, 0.0),
                                                                  den=tokens(0, mid, mid + 128, 0.0)),
              "ragged last apply chunk left out of the weighted sum (image 1)": dict(num=tokens(1, last, S - 3, 0.0))}
    h, t = FOLD_COL
    if t < T:
        for b, s in FOLD_PLANT:
            col = aw[b, h, :, t]
            assert col.argmax().item() == s % S and col[s] > col.topk(2)[0][1] + 15     # the planted token dominates
            out = tokens(b, s % S, s % S + 1, 0.0)
            wrongs[f"planted token of image {b} left out of the text-side softmax"] = dict(num=out, den=out)
    for what, kw in wrongs.items():
        wrong = _fold_reference(d, T, **kw)[1]
        _discriminates(wrong, ol, tol_l, what)
        print(f"  {what}: {((wrong - ol).abs() / tol_l).max().item():.0f}x the bound")
    kl = _strided(d.kl[:, :T].reshape(B * T, 2048).to(dev), 2048 + 64)
    assert kl.stride(0) == 2048 + 64
    vout, out_l, o16, o16p = _run_fold(dev, d.v, kl, T, d, B, S)
    ev = ((vout.double() - want_v).abs() / tol_v).max().item()
    el = ((out_l.double() - ol).abs() / tol_l).max().item()
    print(f"S={S} T={T}: image update {ev:.3f}x, text-side output {el:.3f}x the bound")
    _assert_within(vout.double(), want_v, tol_v, f"fusion_fold v S={S} T={T}")
    _assert_within(out_l.double(), ol, tol_l, f"fusion_fold out_l S={S} T={T}")
    assert torch.equal(o16.view(torch.int16), vout.half().view(torch.int16))
    assert torch.equal(o16p.view(torch.int16), (vout.view(B, S, 256) + d.pos).half().view(B * S, 256).view(torch.int16))


@torch.no_grad()
def test_fusion_fold_images_are_independent(dev):
    """B = 8 at S = 13294, T = 4: every image's outputs (v, out_l, out16, out16_pos) are bitwise those of a B = 1 run on
    that image alone - no reduction crosses images."""
    d = _fold_data(13294)
    S, B, T = 13294, 8, 4
    g = torch.Generator().manual_seed(8)
    v = torch.randn(B * S, 256, generator=g) * 1.3 + 20
    kl = torch.randn(B * T, 2048, generator=g) * 0.7
    full = _run_fold(dev, v, kl, T, d, B, S)
    for b in range(B):
        one = _run_fold(dev, v[b * S:(b + 1) * S], kl[b * T:(b + 1) * T], T, d, 1, S)
        for name, a, o, rows in zip(("v", "out_l", "out16", "out16_pos"), full, one, (S, T, S, S)):
            assert torch.equal(a[b * rows:(b + 1) * rows], o), (b, name)


# ---------------------------------------------------------------------------------------------------------------
# groupnorm_nhwc through the plan
# ---------------------------------------------------------------------------------------------------------------
@torch.no_grad()
@pytest.mark.parametrize("hw", [(800, 800), (800, 1066)])
def test_groupnorm_nhwc_plan_levels(dev, hw):
    """GroupNorm(32, 256) of the four levels (T = 10000 / 2500 / 625 / 169 at 800x800), B = 2, each written at
    level_start[l] of one NaN-filled [B*S, 256] source with batch stride S*256, as GDinoEngine.neck does; group means
    20 + 3 N(0, 1), different per image.  Bound (two-pass f32 statistics, one workgroup per (image, group)): the mean
    is off by dm <= K u mean|x|, K = 2 ceil(T / 256) + 12 (per-thread chain of two 4-element chunks per token, the
    wave and workgroup reductions, the division); then as _merge_tol without the f16 store."""
    import torch.nn.functional as Fn
    from inklayer_amd import ops
    B = 2
    pl = _plan(hw[0], hw[1], B)
    S = pl.S
    out = _nan_out((B * S, 256), F32, dev)
    g = torch.Generator().manual_seed(hw[1])
    gm = 1 + 0.3 * torch.randn(256, generator=g)
    bt = 0.2 * torch.randn(256, generator=g)
    refs = []
    for l, (hh, ww) in enumerate(pl.shapes):
        T, ls = hh * ww, pl.level_start[l]
        cur = out.view(B, S, 256).cpu()
        assert cur[:, ls:].isnan().all(), f"level {l}: rows of levels not yet written are touched"
        mean = 20 + 3 * torch.randn(B, 1, 32, 1, generator=g)
        x = (mean + torch.randn(B, T, 32, 8, generator=g) * (0.5 + torch.rand(B, 1, 32, 1, generator=g))).view(B, T, 256)
        xd = x.double()
        r = Fn.group_norm(xd.transpose(1, 2), 32, gm.double(), bt.double(), 1e-5).transpose(1, 2)
        xg = xd.view(B, T, 32, 8)
        K = 2 * -(-T // 256) + 12
        dm = K * U * xg.abs().mean((1, 3), keepdim=True)
        rstd = 1.0 / torch.sqrt(xg.var((1, 3), unbiased=False, keepdim=True) + 1e-5)
        dev_ = (r - bt.double()).abs().view(B, T, 32, 8)
        tol = ((gm.double().abs().view(1, 1, 32, 8) * rstd * dm + ((K + 8) * U + 0.5 * (dm * rstd) ** 2) * dev_)
               .view(B, T, 256) + U * r.abs() + 1e-7)
        ilv = Fn.group_norm(xd.view(B, T, 8, 32).transpose(2, 3).reshape(B, T, 256).transpose(1, 2), 32).transpose(1, 2)
        ilv = ilv.reshape(B, T, 32, 8).transpose(2, 3).reshape(B, T, 256) * gm.double() + bt.double()
        _discriminates(ilv, r, tol, "channel c in group c % 32")
        mo = xg.mean((1, 3), keepdim=True).flip(0)
        wrong = ((xg - mo) * rstd.flip(0)).view(B, T, 256) * gm.double() + bt.double()
        _discriminates(wrong, r, tol, "statistics of the other image")
        ops.groupnorm_nhwc(x.view(B * T, 256).to(dev), B, T, 32, gm.to(dev), bt.to(dev), 1e-5, out[ls:], S * 256)
        got = out.view(B, S, 256)[:, ls:ls + T].double().cpu()
        print(f"{hw} level {l} (T={T}): worst error {((got - r).abs() / tol).max().item():.3f}x the bound")
        _assert_within(got, r, tol, f"groupnorm_nhwc level {l}")
        refs.append((ls, T, r, tol))
    final = out.view(B, S, 256).double().cpu()
    for l, (ls, T, r, tol) in enumerate(refs):             # no later level overwrote an earlier one
        _assert_within(final[:, ls:ls + T], r, tol, f"groupnorm_nhwc level {l} after all levels")
