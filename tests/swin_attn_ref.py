"""float64 reference, error bound and inputs for ops.swin_attn (csrc/attention_swin.hip), shared by
tests/test_swin_attn_gpu.py (runs the kernel) and tests/test_gdino_models_cpu.py (holds the yardstick on the CPU)."""
from types import SimpleNamespace

import torch

F16, F64 = torch.float16, torch.float64
U = 2.0 ** -24            # f32 unit roundoff
NAN = float("nan")
SCALE = 32 ** -0.5
HEADS = (4, 8, 16, 32)    # Swin-B: heads of stage i (head width 32)


def plan(h, w, B, ws):
    """The detector's host-built plan for an (h, w, B) input and window size ws, built on the CPU (the plan reads only
    the config and the level embedding of its engine)."""
    from inklayer_amd import gdino
    cfg = gdino.GDinoConfig(embed_dim=128, depths=(2, 2, 2, 2), num_heads=HEADS, window_size=ws)
    eng = SimpleNamespace(cfg=cfg, dev=torch.device("cpu"), level_embed_cpu=torch.zeros(4, 256))
    return gdino._Plan(eng, h, w, B)


def padded(ws):
    """Key slots of the kernel: ws^2 rounded up to whole 32-key MFMA tiles."""
    return -(-ws * ws // 32) * 32


def attn_ref(q, k, v, sb, sm, pad_keys=0):
    """float64 softmax(scale q k^T + sb + sm[window % nW]) v for q, k, v [Bw, nh, N, 32], sb [nh, N, N] (logit units),
    sm [nW, N, N] or None.  pad_keys: that many extra keys of value 0 admitted (a mistake) with the score this kernel
    would give them were they not overwritten: their K rows are zero and their table offset is that of key 0, so the
    score is the accumulator init sb[h, q, 0].  -> (o, P, s)."""
    s = SCALE * (q @ k.transpose(-1, -2)) + sb[None]
    if sm is not None:
        s = s + sm[torch.arange(q.shape[0]) % sm.shape[0]][:, None]
    m = s.amax(-1, keepdim=True)
    e = torch.exp(s - m)
    den = e.sum(-1, keepdim=True) + pad_keys * torch.exp(sb[None, :, :, :1] - m)
    return (e / den) @ v, e / den, s


def tol(q, k, v, sb, sm, P, s, o, ws):
    """Bound of swin_attn_kernel<ws> on |got - o|, from the kernel's own arithmetic (u = 2^-24, KP = padded(ws) key
    slots: 160 at ws = 12 for 144 keys, 64 at ws = 7 for 49).

    Scores.  The accumulator starts at f32(table / scale) (the table is multiplied by f32(1 / scale) on its way into
    LDS: two roundings) plus, in a shifted block, f32(-100 / scale) (one f32 add), and the MFMAs add q.k: 32 exact f16
    products summed in f32 in an order the hardware chooses, 33 terms with the init.  Then p = exp2(fma(acc, c, -m c))
    with c = f32(scale log2 e) and m the row maximum of acc: one rounding each for c, m c and the fma, exp2 to 2 ulp.
    There is NO running maximum and no rescale: all KP scores of a query are in registers before the one maximum is
    taken.  In natural-log units each p_k is therefore off by a relative
        delta_k <= 40 u (scale sum|q k| + |sb| + |sm|) + 2 u |max_k s| + 4 u
    (33 + 3 + 1 + 1 <= 40 roundings on the score's magnitude, 2 on the maximum's, 4 u for fma and exp2), which moves o
    by <= sum_k P_k delta_k |v_k - o| <= (P delta) |v| + sum(P delta) |o|.
    P is rounded to f16 before the P V MFMA while l is summed in f32 from the unrounded p, so that rounding does not
    cancel: 2^-11 sum_k P_k |v_k| (2^-25 |v_k| absolute for p in the f16 subnormal range; l >= 1 since the maximum key
    has p = 1).  The P V accumulation over KP slots adds KP u sum P |v|; the l sum (KP / 2 terms in the lane, one across
    the half-waves), the reciprocal and the product (KP / 2 + 4) u |o|; the f16 store half an ulp (2^-11 |o|, 2^-25 in
    the subnormal range)."""
    KP = padded(ws)
    mag = SCALE * (q.abs() @ k.abs().transpose(-1, -2)) + sb.abs()[None]
    if sm is not None:
        mag = mag + sm.abs()[torch.arange(q.shape[0]) % sm.shape[0]][:, None]
    delta = 40 * U * mag + 2 * U * s.amax(-1, keepdim=True).abs() + 4 * U
    Pd = P * delta
    va = v.abs()
    A = P @ va
    return (Pd @ va + Pd.sum(-1, keepdim=True) * o.abs() + (2.0 ** -11 + KP * U) * A
            + 2.0 ** -25 * va.sum(-2, keepdim=True) + (2.0 ** -11 + (KP // 2 + 4) * U) * o.abs() + 2.0 ** -25)


def inputs(pl, i, shifted, ws, seed):
    """The packed qkv buffer as the engine hands it to the attention: f16 [B*nW*ws^2, 3C + 8] in window order
    (plan.win_map), NaN in the 8 padding columns, one shared bias-only row where the map is -1; and a std-1.0
    relative-position table [(2 ws - 1)^2, nh] as the checkpoint holds it."""
    nh = HEADS[i]
    C = 32 * nh
    H, W = pl.stage_hw[i]
    g = torch.Generator().manual_seed(seed)
    tok = torch.randn(pl.B * H * W, 3 * C, generator=g).half()
    bias_row = (0.5 * torch.randn(3 * C, generator=g)).half()
    wm = pl.win_map[i][shifted].long()
    rows = torch.where(wm[:, None] >= 0, tok[wm.clamp(min=0)], bias_row[None])
    buf = torch.full((wm.numel(), 3 * C + 8), NAN, dtype=F16)
    buf[:, :3 * C] = rows
    table = torch.randn((2 * ws - 1) ** 2, nh, generator=g)
    return buf, table


def case(hw, stage, shifted, ws, B=2):
    """One test case: inputs, the float64 result, its bound and the named mistakes.  The bias and the mask of the
    reference come from oracle/gdino_ref.py (relative_position_index, the dense 0 / -100 mask), not from the plan's
    region ids or the kernel's index formula."""
    from oracle import gdino_ref
    from inklayer_amd import gdino
    pl = plan(hw[0], hw[1], B, ws)
    nh, nW, N = HEADS[stage], pl.nW[stage], ws * ws
    C, Bw = 32 * nh, B * nW
    buf, table = inputs(pl, stage, shifted, ws, 1000 * stage + 10 * shifted + hw[1] % 7 + ws)
    qkv = buf[:, :3 * C].double().view(Bw, N, 3, nh, 32).permute(2, 0, 3, 1, 4)
    q, k, v = qkv[0], qkv[1], qkv[2]
    sb = table.double()[gdino_ref.swin_rel_index(ws).view(-1)].view(N, N, nh).permute(2, 0, 1)
    H, W = pl.stage_hw[stage]
    Hp, Wp = -(-H // ws) * ws, -(-W // ws) * ws
    sm = gdino_ref.swin_shift_mask(Hp, Wp, ws).double() if shifted else None
    o, P, s = attn_ref(q, k, v, sb, sm)
    bound = tol(q, k, v, sb, sm, P, s, o, ws)
    wrongs = {"bias transposed to [h, k, q]": attn_ref(q, k, v, sb.transpose(1, 2), sm)[0],
              "bias of head h + 1": attn_ref(q, k, v, sb.roll(-1, 0), sm)[0],
              f"{padded(ws) - N} padding keys admitted": attn_ref(q, k, v, sb, sm, pad_keys=padded(ws) - N)[0]}
    if shifted:
        if nW > 1:
            wrongs["mask of window (w + 1) % nW"] = attn_ref(q, k, v, sb, sm.roll(-1, 0))[0]
        wrongs["mask omitted"] = attn_ref(q, k, v, sb, None)[0]
        if Hp != Wp:
            wrongs["window grid transposed"] = attn_ref(q, k, v, sb, gdino_ref.swin_shift_mask(Wp, Hp, ws).double())[0]
    region = gdino.swin_regions(Hp, Wp, ws).to(torch.uint8) if shifted else None
    return SimpleNamespace(pl=pl, nh=nh, nW=nW, N=N, C=C, Bw=Bw, buf=buf, table=table, sb=sb, sm=sm, o=o, tol=bound,
                           wrongs=wrongs, region=region, q=q, k=k, v=v, P=P, s=s)
