"""float64 restatement of GroundingDINO's text branch (BertModelWarper.forward, GD/.../bertwarper.py:31-166, then
feat_map, groundingdino.py:277-279) for a list of captions, the captions the text-encoder tests share, and per-element
bounds for the two kernels of inklayer_amd/csrc/text_bert.hip.  tests/test_text_encoder_ref_cpu.py ties it to
inklayer_amd.text_branch.bert_encode, which tests/test_text_branch_cpu.py pins to HuggingFace's BertModel.  CPU-only:
nothing here touches the library."""
import math

import torch

U = 2.0 ** -24
F64 = torch.float64
HEADS, HD = 12, 64

# the two captions of tests/test_text_branch_cpu.py (ids up to 4937: their BERT needs a vocabulary beyond them)
BRANCH_CAPTIONS = ((101, 4874, 1012, 102), (101, 4874, 3899, 1012, 4937, 1012, 102))
IDS4 = (101, 1999, 1012, 102)                                   # every other caption: ordinary ids below 2048
IDS9 = (101, 1100, 1101, 1012, 1102, 1012, 1103, 1012, 102)
IDS1 = (101,)


def caption_ids(n, first=200):
    """[CLS] w w . w . w w w . ... [SEP]: n >= 2 token ids below 2048 with phrases of growing length."""
    ids, size = [101], 2
    while len(ids) < n - 1:
        ids += [first + (7 * (len(ids) + i)) % 1500 for i in range(min(size, n - 2 - len(ids)))]
        if len(ids) < n - 1:
            ids.append(1012)
        size = size % 5 + 1
    return tuple((ids + [102])[:n - 1] + [102])


IDS23, IDS256 = caption_ids(23), caption_ids(256, first=300)


def _g(sd, name):
    return sd["bert." + name].detach().to(F64)


def _ln(x, g, b, eps=1e-12):
    mu = x.mean(-1, keepdim=True)
    var = ((x - mu) ** 2).mean(-1, keepdim=True)
    return (x - mu) / torch.sqrt(var + eps) * g + b


def masks_and_pos(ids):
    from inklayer_amd.gdino import text_masks_and_position_ids
    return text_masks_and_position_ids(list(ids))


def embed64(sd, ids):
    _, pos = masks_and_pos(ids)
    e = "embeddings."
    x = _g(sd, e + "word_embeddings.weight")[list(ids)] + _g(sd, e + "token_type_embeddings.weight")[0] \
        + _g(sd, e + "position_embeddings.weight")[pos]
    return _ln(x, _g(sd, e + "LayerNorm.weight"), _g(sd, e + "LayerNorm.bias"))


def layer64(sd, i, x, allowed):
    """One BertLayer on x [T, 768] float64 with the boolean allowed [T, T] mask."""
    p = f"encoder.layer.{i}."
    lin = lambda t, n: t @ _g(sd, p + n + ".weight").T + _g(sd, p + n + ".bias")
    T, D = x.shape
    sp = lambda t: t.view(T, HEADS, HD).transpose(0, 1)
    q, k, v = (sp(lin(x, "attention.self." + n)) for n in ("query", "key", "value"))
    s = (q @ k.transpose(-1, -2)) / math.sqrt(HD)
    s = s.masked_fill(~allowed[None], float("-inf"))
    ctx = (s.softmax(-1) @ v).transpose(0, 1).reshape(T, D)
    x = _ln(lin(ctx, "attention.output.dense") + x, _g(sd, p + "attention.output.LayerNorm.weight"),
            _g(sd, p + "attention.output.LayerNorm.bias"))
    h = lin(x, "intermediate.dense")
    h = 0.5 * h * (1.0 + torch.erf(h / math.sqrt(2.0)))
    return _ln(lin(h, "output.dense") + x, _g(sd, p + "output.LayerNorm.weight"), _g(sd, p + "output.LayerNorm.bias"))


def n_layers(sd):
    return 1 + max(int(k.split(".")[3]) for k in sd if k.startswith("bert.encoder.layer."))


def hidden64(sd, ids):
    allowed, _ = masks_and_pos(ids)
    x = embed64(sd, ids)
    for i in range(n_layers(sd)):
        x = layer64(sd, i, x, allowed)
    return x


def encode64(sd, ids, hidden=None):
    h = hidden64(sd, ids) if hidden is None else hidden
    return h @ sd["feat_map.weight"].detach().to(F64).T + sd["feat_map.bias"].detach().to(F64)


def encode64_batch(sd, id_lists):
    """-> (list of hidden [T_b, 768], list of features [T_b, 256]), float64, each distinct caption computed once."""
    memo = {}
    for ids in id_lists:
        if tuple(ids) not in memo:
            h = hidden64(sd, ids)
            memo[tuple(ids)] = (h, encode64(sd, ids, h))
    return [memo[tuple(i)][0] for i in id_lists], [memo[tuple(i)][1] for i in id_lists]


# ---------------------------------------------------------------------------------------------------------------
# ink_text_embed_ln
# ---------------------------------------------------------------------------------------------------------------
def embed_ln_ref(ids, pos_ids, word, pos, type_row, gamma, beta, eps):
    """float64 result [R, C] and a per-element bound for the kernel's f32 arithmetic.  With z = (w + t) + p the kernel
    rounds twice per element: dz <= 2 u (|w| + |t| + |p|).  The mean and the variance are sums of C terms as four-term
    groups, <= 8 sequential partials and six butterfly levels, <= 14 roundings each: the mean moves by <= 14 u mean|z|,
    rstd by <= 20 u relative (half of the variance's 2 x (14 + 3) u, and the division, square root and eps add).
    LayerNorm's Jacobian turns an input perturbation d into g rstd (d_i - mean(d) - yhat_i mean(yhat d)); the four
    operations of (z - mean) rstd g + b add 4 u of the terms they form."""
    w, p, t = word.to(F64)[ids], pos.to(F64)[pos_ids], type_row.to(F64)
    g, b = gamma.to(F64), beta.to(F64)
    z = w + t + p
    mu = z.mean(-1, keepdim=True)
    rstd = 1.0 / torch.sqrt(((z - mu) ** 2).mean(-1, keepdim=True) + eps)
    yhat = (z - mu) * rstd
    ref = yhat * g + b
    dz = 2 * U * (w.abs() + t.abs() + p.abs()) + 14 * U * z.abs().mean(-1, keepdim=True) + U * (z.abs() + mu.abs())
    tol = g.abs() * rstd * (dz + dz.mean(-1, keepdim=True) + yhat.abs() * (yhat.abs() * dz).mean(-1, keepdim=True)) \
        + 20 * U * (g * yhat).abs() + 4 * U * ((g * yhat).abs() + b.abs()) + 1e-30
    return ref, tol


# ---------------------------------------------------------------------------------------------------------------
# ink_attn_text_f32
# ---------------------------------------------------------------------------------------------------------------
TILE = 64            # keys per LDS tile of attn_text_f32_kernel: one rescale of the running state per tile


def attn_text_ref(q, k, v, lens, blocked, scale, *, ignore_mask=False, shift_keys=0):
    """Packed rows q / k / v [R, H, 64]; caption b owns lens[b] rows; blocked[b] u8 [T_b, T_b] (1 = not allowed) or
    None.  -> (float64 result [R, H, 64], per-element bound of the kernel's arithmetic).  A row with no allowed key is
    zeros.  The two named mistakes: ignore_mask drops the mask; shift_keys = 1 reads the keys and values of the NEXT
    caption (cyclically) instead of the caption's own, as a wrong row base would.

    Bound, u = 2^-24, in the style of tests/test_attn_midkeys_gpu.py::_tol for this kernel's arithmetic:
      scores   sixteen fma chains of four products, joined by a tree of four additions, then one multiply by the
               scale: ds <= (4 + 4 + 1) u scale |q|.|k|;
      weights  exp(s - m): relative ds + u |s - max| + 4 u, and one rescale by exp(m_old - m_new) (3 u) per tile of 64
               keys that follows: eps = ds + u |s - max| + (4 + 3 n_tiles) u;
      sums     the value sum and the normaliser are sequential over the ALLOWED keys of a tile (a blocked key adds
               nothing; c = the largest such count among the row's tiles, <= 64) and merged once per tile:
               (c + n_tiles) u each, then one division and one multiply; the f32 store is exact."""
    R, H, hd = q.shape
    ref, tol = torch.zeros(R, H, hd, dtype=F64), torch.zeros(R, H, hd, dtype=F64)
    starts = [0]
    for n in lens:
        starts.append(starts[-1] + n)
    for b, n in enumerate(lens):
        rows = slice(starts[b], starts[b + 1])
        kb = b
        if shift_keys:
            kb = (b + shift_keys) % len(lens)
        qq = q[rows].double()
        kk, vv = k[starts[kb]:starts[kb + 1]].double(), v[starts[kb]:starts[kb + 1]].double()
        if shift_keys:                                     # the neighbour's rows at this caption's key positions
            idx = torch.arange(n) % kk.shape[0]
            kk, vv = kk[idx], vv[idx]
        nt = -(-n // TILE)
        s = torch.einsum("qhd,khd->hqk", qq, kk) * scale
        ds = (4 + 4 + 1) * U * scale * torch.einsum("qhd,khd->hqk", qq.abs(), kk.abs())
        if blocked is not None and blocked[b] is not None and not ignore_mask:
            s = s.masked_fill(blocked[b].bool()[None], float("-inf"))
        dead = torch.isinf(s).all(-1)                      # [H, n]
        p = s.masked_fill(dead[..., None], 0.0).softmax(-1).masked_fill(dead[..., None], 0.0)
        out = torch.einsum("hqk,khd->qhd", p, vv)
        gap = (s - s.amax(-1, keepdim=True)).abs().masked_fill(p == 0, 0.0)
        pe = p * (ds + U * gap + (4 + 3 * nt) * U)
        av = vv.abs()
        ref[rows] = out
        live = torch.nn.functional.pad(~torch.isinf(s), (0, nt * TILE - n))
        c = live.view(H, n, nt, TILE).sum(-1).amax(-1).transpose(0, 1)[..., None].double()      # [n, H, 1]
        tol[rows] = (torch.einsum("hqk,khd->qhd", pe, av) + pe.sum(-1).transpose(0, 1)[..., None] * out.abs()
                     + (c + nt + 2) * U * torch.einsum("hqk,khd->qhd", p, av) + (c + nt + 3) * U * out.abs() + 1e-30)
    return ref, tol
