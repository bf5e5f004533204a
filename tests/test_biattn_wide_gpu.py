"""ops.biattn_wide (inklayer_amd/csrc/biattn_wide.hip: the fusion layer's bi-attention for captions of up to 256
tokens, three f16 MFMA products) against float64.  GPU box only.

The bound follows the kernel's own arithmetic, per output element, with u = 2^-24:
  scores      256 exact f16 x f16 products accumulated in f32 by the MFMA unit; every accumulation step is allowed one
              f32 ulp (2 u, which also covers a truncating adder), then one multiply by the scale:
              ds <= 256 * 2u * scale * |q|.|k| + u |s|.
  weights     w = exp(s - m) <= 1 with m the row maximum (image side) or the chunk's column maximum (text side):
              relative error ds + u |s - max| (the subtraction) + 4 u (expf, the 2^14 scaling is exact) + 2^-11 (the
              rounding to f16); a weight below f16's smallest normal after the 2^14 scaling, i.e. below 2^-28, may be
              flushed: absolute error 2^-28.  The text side's merge multiplies a chunk by exp(m_c - M): u |m_c - M| +
              2 u more, and |m_c - M| <= |s - M| for every row of the chunk.
  normaliser  the sum of the SAME rounded weights, so the weights stay a convex combination: a weight error eps_i moves
              the output by at most  sum p_i eps_i |v_i|  +  (sum p_i eps_i) |out|.  The sum itself: image side 16
              sequential adds per lane for T = 256 and a 4-step shuffle tree, 1 / sum, one multiply; text side at
              most 512 sequential adds per lane (16 rows of each of a chunk's 32 tiles), one shuffle, the merge's
              sum over the chunks, one division.
  value sums  exact f16 x f16 products accumulated in f32: Tp steps (image side), at most 1024 rows of a chunk plus the
              chunks of the merge (text side), each step one f32 ulp of the running sum <= sum p |v|.
  store       f16: 2^-11 relative, 2^-25 absolute below the normal range.

Shapes: the kernel works on tiles of 32 image rows, image-side workgroups of 128 rows (4 tiles), text-side chunks of
1024 rows (8 workgroups' column maxima), and pads T to a multiple of 32 (one MFMA column tile).  So S = 70 is two tiles
and six rows, 257 two workgroups and one row, 300 a ragged third workgroup, 1025 one chunk and one row, 1100 a ragged
second chunk, and T sits at, just below and just above the column-tile edges 32 and 256.  T = 1 .. 4 (at most four live
columns of the one column tile, the captions the engine folds unless fold_fusion is off) run at the same row edges and,
for T = 4, at the production token counts 13294 and 22223."""
import pytest
import torch

pytestmark = pytest.mark.gpu

F16, F64 = torch.float16, torch.float64
U = 2.0 ** -24
E, H, HD = 1024, 4, 256
SCALE = 256 ** -0.5
TILE, GROUP, CHUNK = 32, 128, 1024


def _assert_within(got, ref, tol, what):
    err = (got - ref).abs()
    bad = ~(err <= tol)                         # NaN-safe: a NaN output is out of bound
    if bad.any():
        i = int(bad.flatten().nonzero()[0])
        raise AssertionError(f"{what}: {int(bad.sum())} / {bad.numel()} elements out of bound; first at flat {i}: "
                             f"got {got.flatten()[i].item()!r}, ref {ref.flatten()[i].item()!r}, "
                             f"tol {tol.flatten()[i].item()!r}")


def _discriminates(wrong, ref, tol, what):
    """The bound rejects `wrong` (a float64 result with one plausible mistake) with an order of magnitude to spare.  Ten
    rather than the hundred of the index-heavy op tests: with a thousand image tokens of comparable weight both the right
    and the wrong text-side result are averages near zero, so the mistake itself is only tens of f16 ulps of |v|."""
    m = ((wrong - ref).abs() / tol).max().item()
    print(f"    mistake '{what}': {m:.0f}x the bound")
    assert m >= 10, f"the bound cannot tell the mistake '{what}' apart: max deviation {m:.1f}x the bound"


def _heads(x):
    return x.double().view(-1, H, HD).transpose(0, 1)                    # [4, n, 256]


def _reference(qv1, kl1, S, T):
    """One image: float64 results and bounds, each [4, n, 256], and the pieces the discrimination cases need."""
    q, vv = _heads(qv1[:, :E]), _heads(qv1[:, E:])
    k, vl = _heads(kl1[:, :E]), _heads(kl1[:, E:])
    s = SCALE * (q @ k.transpose(-1, -2))                                # [4, S, T]
    ds = 256 * 2 * U * SCALE * (q.abs() @ k.abs().transpose(-1, -2)) + U * s.abs()
    Tp, NC = -(-T // 32) * 32, -(-S // CHUNK)
    # image side
    p = s.softmax(-1)
    rv = p @ vl
    eps = ds + U * (s - s.amax(-1, keepdim=True)).abs() + 4 * U + 2.0 ** -11
    pe = p * eps
    tv = (pe @ vl.abs() + pe.sum(-1, keepdim=True) * rv.abs()
          + 2.0 ** -28 * (vl.abs().sum(1, keepdim=True) + T * rv.abs())
          + Tp * 2 * U * (p @ vl.abs())
          + ((Tp // 16 + 4 + 3) * U + 2.0 ** -11) * rv.abs() + 2.0 ** -25)
    # text side
    st, dst = s.transpose(-1, -2), ds.transpose(-1, -2)                  # [4, T, S]
    P = st.softmax(-1)
    rl = P @ vv
    e2 = dst + 2 * U * (st - st.amax(-1, keepdim=True)).abs() + 8 * U + 2.0 ** -11
    Pe = P * e2
    tl = (Pe @ vv.abs() + Pe.sum(-1, keepdim=True) * rl.abs()
          + 2.0 ** -28 * (vv.abs().sum(1, keepdim=True) + S * rl.abs())
          + (CHUNK * 2 * U + (NC + 2) * U) * (P @ vv.abs())
          + ((512 + 1 + NC + 3) * U + 2.0 ** -11) * rl.abs() + 2.0 ** -25)
    return dict(s=s, p=p, vl=vl, vv=vv, rv=rv, tv=tv, rl=rl, tl=tl)


def _run(dev, qv, kl, B, S, T):
    from inklayer_amd import ops
    ov, ol = ops.biattn_wide(qv.to(dev), kl.to(dev), B, S, T, SCALE)
    torch.cuda.synchronize()
    return ov.cpu(), ol.cpu()


def _check(dev, qv, kl, B, S, T, what, discriminate=False):
    ov, ol = _run(dev, qv, kl, B, S, T)
    worst_v = worst_l = 0.0
    refs = [_reference(qv[b * S:(b + 1) * S], kl[b * T:(b + 1) * T], S, T) for b in range(B)]
    for b, r in enumerate(refs):
        gv = ov[b * S:(b + 1) * S].double().view(S, H, HD).transpose(0, 1)
        gl = ol[b * T:(b + 1) * T].double().view(T, H, HD).transpose(0, 1)
        worst_v = max(worst_v, ((gv - r["rv"]).abs() / r["tv"]).max().item())
        worst_l = max(worst_l, ((gl - r["rl"]).abs() / r["tl"]).max().item())
        if discriminate and b == 0:
            pw = r["p"].transpose(-1, -2)
            _discriminates((pw / pw.sum(-1, keepdim=True)) @ r["vv"], r["rl"], r["tl"],
                           "text side weighted by the image-side softmax over T")
            Tp = -(-T // 32) * 32
            if Tp - T >= Tp // 4:   # one pad column of 256 weighs what f16 rounding weighs: no bound can reject that
                e = (r["s"] - r["s"].amax(-1, keepdim=True)).exp()
                pad0 = (Tp - T) * (-r["s"].amax(-1, keepdim=True)).exp()          # pad columns scored 0, values 0
                _discriminates((e @ r["vl"]) / (e.sum(-1, keepdim=True) + pad0), r["rv"], r["tv"],
                               "pad columns scored 0 instead of -inf")
    print(f"{what}: out_v worst / bound = {worst_v:.3f}, out_l worst / bound = {worst_l:.3f}")
    for b, r in enumerate(refs):
        gv = ov[b * S:(b + 1) * S].double().view(S, H, HD).transpose(0, 1)
        gl = ol[b * T:(b + 1) * T].double().view(T, H, HD).transpose(0, 1)
        _assert_within(gv, r["rv"], r["tv"], f"{what} out_v image {b}")
        _assert_within(gl, r["rl"], r["tl"], f"{what} out_l image {b}")
    return ov, ol


def _data(B, S, T, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(B * S, 2 * E, generator=g).half(), torch.randn(B * T, 2 * E, generator=g).half()


EDGES = [(70, 1), (257, 2), (300, 3), (1100, 4),        # the caption lengths the folded path serves by default
         (70, 5), (257, 17), (257, 32), (300, 33), (1025, 31), (1100, 100), (1100, 255), (1100, 256)]


@torch.no_grad()
@pytest.mark.parametrize("S,T", EDGES)
def test_biattn_wide_edge_shapes(dev, S, T):
    """B = 2 (the batch offset is live) at the tile, workgroup, chunk and column-tile edges; the bound rejects a text
    side weighted by the image-side softmax and pad columns scored 0."""
    qv, kl = _data(2, S, T, 1000 * S + T)
    _check(dev, qv, kl, 2, S, T, f"S={S} T={T}", discriminate=True)


@torch.no_grad()
def test_biattn_wide_production_size(dev):
    S, T = 13294, 256
    qv, kl = _data(1, S, T, 7)
    _check(dev, qv, kl, 1, S, T, f"S={S} T={T}")


@torch.no_grad()
@pytest.mark.parametrize("S", [13294, 22223])
def test_biattn_wide_production_sizes_four_tokens(dev, S):
    """The default caption's T = 4 at the token counts of an 800 x 1199 and a 1024 x 1365 input, B = 2: what the
    unfolded layer (fold_fusion = False) runs.  22223 rows are 22 chunks, the last ragged."""
    T = 4
    qv, kl = _data(2, S, T, 1000 * S + T)
    _check(dev, qv, kl, 2, S, T, f"S={S} T={T}", discriminate=True)


@torch.no_grad()
def test_biattn_wide_planted_extremes(dev):
    """An image token of the last, ragged chunk whose score for one text column is far above everything (the column's
    softmax lives in one chunk: the merge must scale the others away), and a text token that dominates an image row of
    the first chunk (row softmax with pad columns present).  q = c k gives the score c |k|^2 / 16, about 16 c."""
    S, T = 1100, 37
    qv, kl = _data(2, S, T, 99)
    for b in range(2):
        qv[b * S + S - 3, :E] = (3.0 * kl[b * T + 11, :E].float()).half()       # score about 48 in every head
        qv[b * S + 5, :E] = (2.0 * kl[b * T + 30, :E].float()).half()           # score about 32
    r = _reference(qv[:S], kl[:T], S, T)
    assert (r["s"][:, S - 3, 11] > r["s"][:, :, 11].topk(2, dim=-1).values[:, 1] + 20).all()
    assert (r["s"][:, 5, 30] > r["s"][:, 5].topk(2, dim=-1).values[:, 1] + 15).all()
    _check(dev, qv, kl, 2, S, T, "planted extremes S=1100 T=37", discriminate=True)


@torch.no_grad()
def test_biattn_wide_is_deterministic_and_batch_independent(dev):
    """No atomics: B = 1 equals the same image as entry 3 of B = 4 bit for bit, and a repeated run equals itself."""
    S, T = 1100, 23
    qv, kl = _data(4, S, T, 5)
    full = _run(dev, qv, kl, 4, S, T)
    again = _run(dev, qv, kl, 4, S, T)
    one = _run(dev, qv[3 * S:].clone(), kl[3 * T:].clone(), 1, S, T)
    assert torch.equal(full[0], again[0]) and torch.equal(full[1], again[1])
    assert torch.equal(full[0][3 * S:], one[0]) and torch.equal(full[1][3 * T:], one[1])
    assert not torch.isnan(full[0].float()).any() and not torch.isnan(full[1].float()).any()
