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
