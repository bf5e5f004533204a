"""float64 parity of the kernels under inklayer_amd/depth.py (Depth-Anything-V2 ViT-B + DPT head) at the shapes
production runs: flash attention at head_dim 64 over ragged key tiles (seven token counts, B = 1 and 2), every GEMM
form of the engine on the two 128x128 tile families, layernorm_rows at C = 768, im2col / bilinear resize at production
sizes, one ViT-B block and the DPT head through the engine.  References and per-element bounds are in
tests/depth_ops_ref.py (tests/test_depth_plan_cpu.py shows on the CPU that named mistakes land >= 100x outside them;
the same checks are repeated here on the full data).  Outputs are NaN-prefilled with guard rows / columns.  GPU box only."""
import numpy as np
import pytest
import torch

import depth_ops_ref as R
import vith_ref as V
from test_depth_plan_cpu import DISPATCH, TAILS

pytestmark = pytest.mark.gpu

NAN = float("nan")
QUANTILES = (0.5, 0.9, 0.99, 0.999, 1.0)
STAGE_ABS = 2.0 ** -12
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


def _gen(dev, seed):
    return torch.Generator(device=dev).manual_seed(seed)


def _report(what, worst):
    print(f"  {what}: worst error {worst:.3f}x the bound")


# ---------------------------------------------------------------------------------------------------------------
# a. flash_attn at head_dim 64
# ---------------------------------------------------------------------------------------------------------------
def _attn_run(dev, qkv, N, B):
    """ops.flash_attn as DepthEngine.encode calls it: q / k / v column slices of the packed qkv (ld 2304); the output is
    a [B*N, 768] view of a NaN-filled [B*N + 64, 832] buffer."""
    from inklayer_amd import ops
    buf = torch.full((B * N + 64, R.DD + 64), NAN, dtype=V.F16, device=dev)
    ops.flash_attn(qkv[:, :R.DD], qkv[:, R.DD:2 * R.DD], qkv[:, 2 * R.DD:], n_batch=B, n_heads=R.DHEADS, head_dim=R.DHD,
                   scale=R.SCALE64, n_q=N, n_k=N, out=buf[:B * N, :R.DD])
    return buf


@torch.no_grad()
@pytest.mark.parametrize("N,B", [(n, 1) for n in R.ATTN_TOKENS] + [(n, 2) for n in R.ATTN_B2])
def test_flash_attn_hd64_ragged_tiles(dev, N, B):
    """flash_attn_kernel<64, 0, 4> (the depth engine is its only user) at N = 37 k + 1 tokens, 12 heads: the ragged-key
    mask of the last 64-key tile (tails 26, 22, 63, 46, 32, 1, none), the zero-filled tail of load_tile, a partly valid
    last 128-query block.  Data: depth_ops_ref.attn64_data (peaked rows, near-uniform rows, probe rows that a phantom
    key takes over, the last key planted as a row maximum).  Every element of all 12 heads within attn64_tol; guard
    rows / columns untouched; the mistakes of attn64_mistakes re-checked on the full data; at B = 2 entry 1 equals, bit
    for bit, a B = 1 run on its rows."""
    assert R.token_tail(N) == TAILS[N]
    qkv = R.attn64_data(N, B, _gen(dev, 70 + N + B), dev)
    buf = _attn_run(dev, qkv, N, B)
    assert buf[B * N:].isnan().all() and buf[:, R.DD:].isnan().all()
    out = buf[:B * N, :R.DD]
    assert not out.isnan().any()
    worst = 0.0
    for b in range(B):
        q, k, v = R.attn64_split(qkv, N, b)
        o, P, s = R.attn64_ref(q, k, v)
        tol = R.attn64_tol(q, k, v, P, s, o)
        del P, s
        got = out[b * N:(b + 1) * N].double().unflatten(1, (R.DHEADS, R.DHD)).permute(1, 0, 2)
        worst = max(worst, V.assert_within(got, o, tol, f"flash_attn hd64 N={N} B={B} entry {b}"))
        if b == 0:
            for what, wrong in R.attn64_mistakes(q, k, v, N):
                V.assert_discriminates(wrong, o, tol, what)
        else:
            _, k0, v0 = R.attn64_split(qkv, N, 0)
            V.assert_discriminates(R.attn64_ref(q, k0, v0)[0], o, tol, "K / V of batch entry 0 used for entry 1")
        del q, k, v, o, tol
    tail, lastq = TAILS[N]
    _report(f"flash_attn hd64 N={N} B={B} (key tail {tail}, last query block {lastq} rows)", worst)
    if B > 1:
        one = _attn_run(dev, qkv[N:2 * N].clone(), N, 1)
        assert torch.equal(one[:N, :R.DD], out[N:2 * N]), "entry 1 of B = 2 != the B = 1 run on its rows"


# ---------------------------------------------------------------------------------------------------------------
# b. the engine's GEMM forms
# ---------------------------------------------------------------------------------------------------------------
@torch.no_grad()
@pytest.mark.parametrize("name,hw", [(n, (37, 37)) for n in sorted(R.DEPTH_GEMMS)] + [(n, (37, 49)) for n in R.GEMM_AT_37x49])
def test_depth_gemm_forms(dev, name, hw):
    """ops.gemm as DepthEngine calls it, at the production M / N / K (variant from DISPATCH), 64 NaN guard rows below the
    output: pe with split-f16 operands, residual = pos and out a view one row into the token buffer (row 0 a guard);
    proj / fc2 with col_scale and the residual in place (late-residual epilogue); rcu2 with a separate linear residual;
    oc3 at N = 4, ldc = 4.  Bound: depth_ops_ref.gemm_tol, every element; the mistakes of gemm_mistakes re-checked on
    the full data."""
    from inklayer_amd import _lib, ops
    f = R.DEPTH_GEMMS[name]
    M, N, K = R.gemm_shape(name, *hw)
    assert int(_lib.lib().ink_gemm_query_variant(M, N, K)) == DISPATCH[name]
    d = R.gemm_data(name, M, _gen(dev, 200 + sorted(R.DEPTH_GEMMS).index(name) + hw[1]), dev)
    top = 1 if f.kind == "pe" else 0
    buf = torch.full((top + M + 64, N), NAN, dtype=V.F16 if f.f16 else V.F32, device=dev)
    out = buf[top:top + M]
    if f.kind == "late":
        out.copy_(d["r"])
        ops.gemm(d["a"], d["w"], d["b"], col_scale=d["cs"], residual=out, out=out)
    elif f.kind:
        ops.gemm(d["a"], d["w"], d["b"], residual=d["r"], out=out)
    else:
        assert ops.gemm(d["a"], d["w"], d["b"], act=f.act, out=out).stride(0) == N
    assert buf[:top].isnan().all() and buf[top + M:].isnan().all()
    ref, lin, mag = R.gemm_ref(name, d)
    tol = R.gemm_tol(name, d, ref, lin, mag)
    worst = V.assert_within(out.double(), ref, tol, f"{name} {hw}")
    _report(f"{name} {hw[0]}x{hw[1]} M={M} N={N} K={K} variant {DISPATCH[name]}", worst)
    del lin, mag
    for what, wrong, factor in R.gemm_mistakes(name, d):
        V.assert_discriminates(wrong, ref, tol, what, factor=factor)
        del wrong


# ---------------------------------------------------------------------------------------------------------------
# c. layernorm_rows at C = 768
# ---------------------------------------------------------------------------------------------------------------
@torch.no_grad()
def test_layernorm_rows_768(dev):
    """layernorm_rows on 1370 rows of 768, eps 1e-6 (norm1 / norm2 / the final norm of the engine), with the hard rows of
    vith_ref.layernorm_data, f16 out at ldo = 832 with NaN guard columns / rows.  Bound: vith_ref.layernorm_tol."""
    from inklayer_amd import ops
    Rr, C = 1370, R.DD
    x, gamma, beta = V.layernorm_data(Rr, _gen(dev, 8), dev, C)
    buf = torch.full((Rr + 4, C + 64), NAN, dtype=V.F16, device=dev)
    out = buf[:Rr, :C]
    ops.layernorm_rows(x, gamma, beta, 1e-6, out=out)
    assert buf[Rr:].isnan().all() and buf[:Rr, C:].isnan().all()
    ref = V.layernorm_ref(x, gamma, beta)
    tol = V.layernorm_tol(x, gamma, beta, ref)
    got = out.double()
    assert ((ref[:, :64].abs() < 2.0 ** -14) & (ref[:, :64] != 0)).sum() > 1000       # f16-subnormal outputs exercised
    assert torch.equal(out[16:20], beta.half()[None].expand(4, -1))
    worst = V.assert_within(got, ref, tol, "layernorm_rows C=768")
    for rows, what in ((slice(0, 8), "|mean|/std = 30"), (slice(8, 16), "massive channels"),
                       (slice(20, 24), "|mean|/std = 3000")):
        _report(what, V.assert_within(got[rows], ref[rows], tol[rows], what))
    for mistake, rows in (("one-pass", slice(20, 24)), ("no-eps", slice(16, 20))):
        V.assert_discriminates(V.layernorm_wrong(x, gamma, beta, mistake)[rows], ref[rows], tol[rows], mistake)
    _report("layernorm_rows C=768, all rows", worst)


# ---------------------------------------------------------------------------------------------------------------
# d. pixel ops at production sizes
# ---------------------------------------------------------------------------------------------------------------
@torch.no_grad()
@pytest.mark.parametrize("H,W,C,stride,relu", [(518, 686, 64, 1, False), (37, 49, 768, 2, False), (148, 148, 128, 1, True)])
def test_im2col3x3_production_sizes(dev, H, W, C, stride, relu):
    """im2col3x3 on the output_conv2 input (518 x 686 x 64: 204 M output elements, 64-bit flat indices), the stride-2
    resize_layers.3 input at odd sizes, and an RCU input with the ReLU on the way; the input holds -0.0, zeros and
    negative values.  Bit-exact (sign of zero included) against F.unfold; the ReLU maps -0.0 and negatives to +0."""
    from inklayer_amd import ops
    x = torch.randn(H * W, C, generator=_gen(dev, 300 + C), device=dev).half()
    x.view(-1)[5::97] = -0.0
    x.view(-1)[11::89] = 0.0
    assert (x < 0).any() and (x.view(torch.int16) == -32768).any()
    got = ops.im2col3x3(x, 1, H, W, stride=stride, relu=relu)
    src = x.float().view(1, H, W, C).permute(0, 3, 1, 2)
    if relu:
        src = torch.where(src > 0, src, torch.zeros((), device=dev))
    u = torch.nn.functional.unfold(src, 3, padding=1, stride=stride)                    # [1, C*9, L], (c, ky, kx) order
    L = u.shape[-1]
    assert L == ((H - 1) // stride + 1) * ((W - 1) // stride + 1) and tuple(got.shape) == (L, 9 * C)
    ref = u.view(C, 9, L).permute(2, 1, 0).reshape(L, 9 * C).half()
    del u, src
    assert torch.equal(got.view(torch.int16), ref.view(torch.int16))
    print(f"  im2col3x3 {H}x{W}x{C} stride {stride} relu {relu}: {got.numel()} elements bit-exact")


@torch.no_grad()
@pytest.mark.parametrize("h,w,C,H,W,f16", [(19, 25, 128, 37, 49, False), (296, 392, 64, 518, 686, True), (518, 686, 1, 600, 800, False)])
def test_resize_bilinear_production_sizes(dev, h, w, C, H, W, f16):
    """resize_bilinear_ac as the engine runs it: a fusion block's upsample to the next stage's (odd) size, the 518 x 686
    upsample in front of output_conv2 (f16 out), and the final 1-channel resize to the sketch size.  Against float64
    F.interpolate(align_corners=True); bound depth_ops_ref.resize_tol (f32 source coordinate, two lerps), which
    align_corners = False leaves by >= 100x."""
    from inklayer_amd import ops
    x = torch.randn(h * w, C, generator=_gen(dev, 400 + C), device=dev)
    got = ops.resize_bilinear_ac(x, 1, h, w, H, W, out_dtype=V.F16 if f16 else V.F32)
    assert tuple(got.shape) == (H * W, C)
    ref = R.resize_ref(x, h, w, H, W)
    tol = R.resize_tol(x, h, w, H, W, ref, f16)
    worst = V.assert_within(got.double(), ref, tol, f"resize {h}x{w}x{C} -> {H}x{W}")
    _report(f"resize_bilinear_ac {h}x{w}x{C} -> {H}x{W} {'f16' if f16 else 'f32'} out", worst)
    V.assert_discriminates(R.resize_ref(x, h, w, H, W, align_corners=False), ref, tol, "align_corners = False")


# ---------------------------------------------------------------------------------------------------------------
# e / f. one ViT-B block and the DPT head through the engine
# ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def engine1(dev):
    """A depth-1 engine (one ViT-B block, the whole DPT head) on seeded weights, and the oracle's view of them."""
    from oracle import depth_ref
    from inklayer_amd import depth
    cfg = depth_ref.DepthConfig(depth=1, layer_idx=(0,))
    sd = depth_ref.seeded_state_dict(cfg, 17)
    for leaf in ("weight", "bias"):          # see test_vitb_block_matches_float64
        sd[f"pretrained.blocks.0.attn.proj.{leaf}"] = sd[f"pretrained.blocks.0.attn.proj.{leaf}"] * 2
    return sd, cfg, depth.DepthEngine(sd, depth.DepthConfig(depth=1, layer_idx=(0,)), dev)


def _quantiles(t):
    return [float(x) for x in np.quantile(t.abs().flatten().cpu().numpy(), QUANTILES)]


def check_yardstick(what, got, ref, emul, scale, wrongs, wrong_from=0.0):
    """Every error quantile of got (the maximum included) is at most 2x that of emul (the float64 reference re-run with
    f16-rounded GEMM operands) plus STAGE_ABS * scale; every (name, tensor) of wrongs misses that bound >= 100x at
    every quantile from wrong_from up.  got None: only the wrongs are checked (the CPU side of the argument)."""
    a = STAGE_ABS * scale
    eq = _quantiles(emul - ref)
    hq = _quantiles(got - ref) if got is not None else None
    wq = [(n, _quantiles(w - ref)) for n, w in wrongs]
    for i, qt in enumerate(QUANTILES):
        bound = 2 * eq[i] + a
        line = f"  {what} q{qt}: emulated-f16 {eq[i]:.2e}"
        if hq is not None:
            line += f"  HIP {hq[i]:.2e} -> {hq[i] / bound:.3f}x the bound"
        print(line + "".join(f"; {n} {w[i] / bound:.0f}x" for n, w in wq))
        if hq is not None:
            assert np.isfinite(hq[i]) and hq[i] <= bound, (what, qt, hq[i], eq[i], a)
        for n, w in wq:
            assert qt < wrong_from or w[i] >= 100 * bound, (f"'{n}' passes the yardstick", what, qt, w[i], bound)


def block_refs(sd, cfg, rec, nh, nw, dev):
    """float64 references of DepthEngine.encode at depth 1 for the patch rows rec [T, 588] (f64, what the split-f16
    patch operand represents): tokens = patch embedding + pos in float64; ref = norm(block(tokens)) without the class
    token; emul = the same with the BLOCK under depth_ref.f16_operands (not the split-precision embedding) and its
    result rounded to f16: encode() returns the operand of the head's projection GEMMs, which the engine stores in f16
    (layernorm_rows, f16 out) and which f16_operands would round at that GEMM; without it the yardstick has no term for
    half an f16 ulp of a feature in [4, 8), 2^-9, four times its own largest error.  Then the block with ls1.gamma
    dropped and with the q scale omitted; max |block update|."""
    from oracle import depth_ref
    sd64 = {k: v.to(dev, torch.float64) for k, v in sd.items()}
    D = cfg.embed_dim
    t = rec @ sd64["pretrained.patch_embed.proj.weight"].reshape(D, -1).t() + sd64["pretrained.patch_embed.proj.bias"]
    pos = depth_ref.interpolate_pos_encoding(sd, cfg, rec.shape[0], nh, nw).to(dev, torch.float64)
    tok = torch.cat([sd64["pretrained.cls_token"][0], t], 0)[None] + pos

    def run(w):
        return depth_ref._ln(depth_ref.vit_block(w, cfg, 0, tok), w, "pretrained.norm")[0, 1:]

    blk = depth_ref.vit_block(sd64, cfg, 0, tok)
    ref = depth_ref._ln(blk, sd64, "pretrained.norm")[0, 1:]
    with depth_ref.f16_operands():
        emul = run(sd64).half().double()      # the features are the f16 operand of the head's first GEMMs
    p = "pretrained.blocks.0."
    no_ls = dict(sd64)
    no_ls[p + "ls1.gamma"] = torch.ones_like(sd64[p + "ls1.gamma"])
    no_scale = dict(sd64)
    for leaf in ("attn.qkv.weight", "attn.qkv.bias"):                 # q rows times head_dim^0.5: the scale cancelled
        x = sd64[p + leaf].clone()
        x[:D] *= (D // cfg.num_heads) ** 0.5
        no_scale[p + leaf] = x
    wrongs = [("ls1.gamma dropped", run(no_ls)), ("q scale omitted", run(no_scale))]
    return ref, emul, wrongs, (blk - tok).abs().max().item()


@torch.no_grad()
@pytest.mark.parametrize("hw,size", [((37, 37), (750, 750)), ((37, 49), (600, 800))])
def test_vitb_block_matches_float64(dev, engine1, hw, size):
    """DepthEngine.encode at depth 1 (patch embedding on split-f16 operands, one block with LayerScale, the final norm,
    the class-token drop) on the patches ops.depth_patchify makes of a synthetic sketch, against block_refs.  Yardstick
    of the Swin / ViT-H block tests (check_yardstick), which the float64 block with ls1.gamma dropped, and with the q
    scale omitted, miss >= 100x at every quantile.  For that at the median the seeded attn.proj weight and bias are
    doubled (engine1): with the seeded ones a dropped ls1.gamma is 96x the bound at the median (float64, CPU).  encode([p0, p1]) equals encode([p0]) and encode([p1]) bit for
    bit (the view(B, N, D)[:, 1:] token drop; every GEMM on variant 0 or 32 at both M)."""
    from inklayer_amd import _lib, ops, synthetic
    sd, cfg, eng = engine1
    ph, pw = hw
    T = ph * pw
    for B in (1, 2):
        for name in ("qkv", "proj", "fc1", "fc2"):
            _, N, K = R.gemm_shape(name, ph, pw)
            assert int(_lib.lib().ink_gemm_query_variant(B * (T + 1), N, K)) == 0
    assert int(_lib.lib().ink_gemm_query_variant(T, R.DD, 3 * eng.KP)) == 32 and eng.KP == R.KP
    nh, nw = 14 * ph, 14 * pw
    pts = []
    for seed in (4, 5):
        bgr = np.ascontiguousarray(synthetic.synthetic_sketch(seed, size[0], size[1])[..., ::-1])
        pts.append(ops.depth_patchify(torch.from_numpy(bgr).to(dev), nh, nw, 14, eng.KP, MEAN, STD, chan_reverse=True))
    assert tuple(pts[0].shape) == (T, 3 * eng.KP)
    outs = eng.encode([pts[0]], ph, pw)
    assert len(outs) == 1 and tuple(outs[0].shape) == (T, R.DD) and outs[0].dtype == V.F16
    rec = pts[0][:, :588].double() + pts[0][:, eng.KP:eng.KP + 588].double() / 64
    ref, emul, wrongs, upd = block_refs(sd, cfg, rec, nh, nw, dev)
    check_yardstick(f"ViT-B block {ph}x{pw}", outs[0].double(), ref, emul, upd, wrongs)
    both = eng.encode(pts, ph, pw)[0]
    assert tuple(both.shape) == (2 * T, R.DD)
    assert torch.equal(both[:T], outs[0]) and torch.equal(both[T:], eng.encode([pts[1]], ph, pw)[0])
    assert not torch.equal(both[:T], both[T:])


def head_refs(sd, cfg, feats16, ph, pw, dev, mistakes=True):
    """float64 depth_ref.dpt_head on the f16 features: (ref, emul, {name: wrong}) each a dict of NHWC stages rn0..3,
    path0..3 (path_1..path_4) and 'out' (the depth map, flat).  Mistakes: the ReLU in front of conv1 of every
    ResidualConvUnit dropped; align_corners = False in the fusion blocks' resize."""
    from oracle import depth_ref
    import torch.nn.functional as F
    sd64 = {k: v.to(dev, torch.float64) for k, v in sd.items()}
    feats = [(f.double()[None], None) for f in feats16]

    def run():
        st = {}
        o = depth_ref.dpt_head(sd64, cfg, feats, ph, pw, st)
        res = {"out": o.reshape(-1)}
        for i in range(4):
            res[f"rn{i}"] = st["rn"][i][0].permute(1, 2, 0).reshape(-1, cfg.features)
            res[f"path{i}"] = st["path"][i][0].permute(1, 2, 0).reshape(-1, cfg.features)
        return res

    ref = run()
    with depth_ref.f16_operands():
        emul = run()
    wrongs = {}
    if mistakes:
        rcu, fusion = depth_ref._rcu, depth_ref._fusion

        def rcu_no_relu(x, sd_, p):
            out = depth_ref._conv(x, sd_, p + ".conv1", padding=1)
            return depth_ref._conv(F.relu(out), sd_, p + ".conv2", padding=1) + x

        def fusion_no_ac(sd_, p, x0, x1=None, size=None):
            out = x0 if x1 is None else x0 + rcu(x1, sd_, p + ".resConfUnit1")
            out = rcu(out, sd_, p + ".resConfUnit2")
            kw = dict(scale_factor=2) if size is None else dict(size=size)
            return depth_ref._conv(F.interpolate(out, mode="bilinear", align_corners=False, **kw), sd_, p + ".out_conv")

        try:
            depth_ref._rcu = rcu_no_relu
            wrongs["RCU input ReLU dropped"] = run()
            depth_ref._rcu, depth_ref._fusion = rcu, fusion_no_ac
            wrongs["fusion resize align_corners=False"] = run()
        finally:
            depth_ref._rcu, depth_ref._fusion = rcu, fusion
    return ref, emul, wrongs


HEAD_STAGES = [f"rn{i}" for i in range(4)] + [f"path{i}" for i in (3, 2, 1, 0)] + ["out"]


@torch.no_grad()
def test_dpt_head_matches_float64(dev, engine1):
    """DepthEngine.head at 37 x 37 on random f16 features (std 1, the final norm's output) against depth_ref.dpt_head in
    float64 on the same features, stage by stage: layer_rn 1..4, path_4..path_1, the depth map.  Yardstick per stage:
    check_yardstick with the float64 head under depth_ref.f16_operands and STAGE_ABS * max |stage|.  On every path stage
    and on the depth map the head without the RCU input ReLU, and with align_corners = False in the fusion resize, miss
    it >= 100x at the quantiles 0.9 and above (the rn stages come before both).  Not at the median: the median pixel of
    the depth map is 0 after the final ReLU whatever the head does, and the resize shift, zero at the map centre and
    growing towards the borders, is 67x .. 89x the bound at the median of the path stages (float64, CPU)."""
    sd, cfg, eng = engine1
    ph = pw = 37
    g = _gen(dev, 500)
    feats16 = [torch.randn(ph * pw, R.DD, generator=g, device=dev).half() for _ in range(4)]
    st = {}
    d = eng.head(feats16, ph, pw, st)
    assert tuple(d.shape) == (14 * ph, 14 * pw)
    got = {"out": d.reshape(-1).double().cpu()}
    for i in range(4):
        got[f"rn{i}"], got[f"path{i}"] = st["rn"][i].double().cpu(), st["path"][i].double().cpu()
    # (the four float64 heads run on the host: seconds there, and float64 convolutions are native to it)
    ref, emul, wrongs = head_refs(sd, cfg, [f.cpu() for f in feats16], ph, pw, torch.device("cpu"))
    for name in HEAD_STAGES:
        assert got[name].shape == ref[name].shape, name
        ws = [] if name.startswith("rn") else [(n, w[name]) for n, w in wrongs.items()]
        check_yardstick(f"DPT head {name}", got[name], ref[name], emul[name], ref[name].abs().max().item(), ws, wrong_from=0.9)
