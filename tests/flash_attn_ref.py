"""float64 reference, per-element error bound, data generator, named mistakes and the case table of ink_flash_attn as
a whole: every instance of flash_attn_kernel<HD, MODE, NW, ALLKV> (inklayer_amd/csrc/attention.hip) and the two
dedicated kernels it dispatches to (win4: attention_win.hip, glob4: attention_glob.hip), at the smallest shapes that
drive every path of each.  Shared by tests/test_flash_attn_edges_gpu.py (the kernels) and
tests/test_flash_attn_plan_cpu.py (that the case table reaches every instance and branch, that the bound tells the
named mistakes apart, and the argument contract, on the CPU).  Nothing here touches the package under test; every
function runs on whatever device its inputs live on.

Everything is compared in BUFFER form: a float64 image of the O buffer, [rows of O, H * hd], NaN where the kernel must
not write (place()).  Mistakes of placement ("O written at the shared Q rows", "padded query stored") are wrong
buffers like any other."""
import math
import zlib
from collections import namedtuple
from types import SimpleNamespace

import torch

from attn_few_ref import IMG_OF, share_rows, strided
from vith_ref import F16, F32, F64, H16, SUB16, U, assert_discriminates, assert_within, discrimination  # noqa: F401

N_CUS = 256                   # compute units of an MI355X: the persistent kernels launch min(blocks, N_CUS) workgroups
PROBE_COL = 3
V_SHIFT = slice(8, 16)
MAP_EXTRA = 6                 # tok_rows cases: a token map of (S + 6)^2 tokens per image, 2 x 2 windows of S x S


# ---------------------------------------------------------------------------------------------------------------
# the dispatcher, restated
# ---------------------------------------------------------------------------------------------------------------
def instance_of(head_dim, bias_mode, n_batch, n_q, n_k, grid_w=0, ldo=None, tok_rows=False, rel_f16=False):
    """The `if` chain of ink_flash_attn for well-formed pointers, tables and input strides: "glob4", "win4_tok", "win4",
    a tuple (HD, MODE, NW, ALLKV) of flash_attn_kernel, or None where the C code returns INK_ERR_ARG.  ldo defaults to
    the dense width of one head (only its divisibility by 4 and win4's 2 GiB limit depend on it); mode 3 is taken with
    dense_bias present and, if a mask is given, n_mask > 0."""
    if ldo is None:
        ldo = 4 * head_dim
    if min(n_batch, n_q, n_k) <= 0 or ldo % 4:
        return None
    if tok_rows and bias_mode != 2:
        return None
    if bias_mode == 1 and head_dim in (80, 64):
        if grid_w != 64 or n_k % 64 or n_k > 64 * 64:
            return None
        if head_dim == 80 and n_q % 256 == 0 and n_k % 128 == 0 and 256 <= n_k <= 4096:
            return "glob4"
        return None if rel_f16 else (head_dim, 1, 8, False)
    if rel_f16 and bias_mode != 1:
        rel_f16 = False                                  # (the field is read in mode 1 only)
    if bias_mode == 2 and head_dim in (80, 64):
        if not (0 < grid_w <= 16 and n_k <= grid_w * grid_w and n_k <= 256):
            return None
        if tok_rows and n_q != n_k:
            return None
        if head_dim == 80 and 193 <= n_k <= 208 and n_q <= 256 and (tok_rows or n_batch * n_q * ldo * 2 < 2 ** 31):
            return "win4_tok" if tok_rows else "win4"
        return (head_dim, 2, 7, True)
    if bias_mode == 0 and head_dim in (80, 64):
        return (head_dim, 0, 4, False)
    if bias_mode == 0 and head_dim in (32, 16):
        return (head_dim, 0, 1 if n_q <= 32 else 4, False)
    if bias_mode == 3 and head_dim == 32:
        return (32, 3, 2, False) if n_k <= 64 and n_q <= 64 else None
    return None


# ---------------------------------------------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------------------------------------------
Case = namedtuple("Case", "name hd mode B H n_q n_k grid_w q_share kv_share packed tok yard gcols")


def _c(hd, mode, B, H, n_q, n_k, grid_w=0, *, q_share=False, kv_share=False, packed=False, tok=False, yard=False, tag="",
       gcols=64):
    """gcols: guard columns beside O (ldo = H hd + gcols); 68 makes ldo an odd multiple of 4, the least the contract asks."""
    name = f"hd{hd}m{mode}_{n_q}x{n_k}" + (f"g{grid_w}" if mode == 2 else "") + tag + (f"_ldo{gcols}" if gcols != 64 else "")
    return Case(name, hd, mode, B, H, n_q, n_k, grid_w, q_share, kv_share, packed, tok, yard, gcols)


def _tok(hd, S, n_img, H=3, yard=False, gcols=64):
    """tok_rows case: n_img token maps of (S + 6)^2 tokens, each cut into 2 x 2 windows of S x S (B = 4 n_img windows):
    windows 1..3 of every image have padded keys, and their rows y >= 6 are padding only."""
    return _c(hd, 2, 4 * n_img, H, S * S, S * S, S, tok=True, yard=yard, tag=f"_tok{n_img}", gcols=gcols)


def _mode1(hd):
    return [_c(hd, 1, 2, 3, 1, 64, 64, yard=True), _c(hd, 1, 3, 3, 255, 192, 64), _c(hd, 1, 3, 3, 257, 1024, 64),
            _c(hd, 1, 3, 3, 320, 192, 64, gcols=68), _c(hd, 1, 3, 3, 255, 64, 64, kv_share=True, tag="_kvs")]


def _mode2(hd):
    return [_c(hd, 2, 2, 3, 144, 144, 12), _c(hd, 2, 2, 3, 192, 192, 14), _c(hd, 2, 2, 3, 209, 209, 15),
            _c(hd, 2, 2, 3, 225, 225, 15, gcols=68), _c(hd, 2, 2, 3, 256, 256, 16),
            _c(hd, 2, 2, 3, 1, 144, 12), _c(hd, 2, 2, 3, 100, 209, 15, yard=True),
            _c(hd, 2, 43, 6, 144, 144, 12, tag="_walk")]


CASES = tuple(
    [_c(16, 0, 2, 2, 7, 40, yard=True), _c(16, 0, 2, 2, 32, 64), _c(16, 0, 2, 2, 1, 1),
     _c(16, 0, 2, 2, 33, 65), _c(16, 0, 3, 2, 100, 77, kv_share=True, yard=True, tag="_kvs"), _c(16, 0, 2, 2, 129, 192),
     _c(32, 0, 2, 2, 32, 65, yard=True), _c(32, 0, 2, 2, 5, 1), _c(32, 0, 2, 2, 20, 129),
     _c(32, 0, 2, 2, 33, 33, yard=True), _c(32, 0, 2, 8, 900, 900), _c(32, 0, 3, 2, 130, 31, q_share=True, tag="_qs"),
     _c(80, 0, 2, 2, 70, 33, yard=True), _c(80, 0, 2, 2, 129, 192, gcols=68), _c(80, 0, 2, 3, 196, 196, packed=True, tag="_packed"),
     _c(64, 0, 2, 3, 70, 33, yard=True), _c(64, 0, 2, 3, 129, 130, gcols=68)]
    + _mode1(80) + _mode1(64) + _mode2(80) + _mode2(64)
    # tok_rows: the generic window kernel at head_dim 80 (S = 12, and S = 16 with two query blocks per window), at
    # head_dim 64 (S = 14, and S = 16), the dedicated kernel at head_dim 80, S = 14; 25 (13 at nqb = 2) images make
    # more (window, head, query block) items than workgroups, with 3 heads: a workgroup's walk crosses windows
    + [_tok(80, 12, 25, yard=True), _tok(80, 16, 13), _tok(64, 14, 25, yard=True), _tok(64, 16, 13, gcols=68), _tok(80, 14, 25, yard=True), _tok(80, 14, 1, gcols=68)]
    + [_c(80, 2, 2, 3, 1, 193, 14), _c(80, 2, 2, 3, 100, 208, 15, yard=True, gcols=68), _c(80, 2, 2, 3, 256, 193, 14),
       _c(80, 2, 3, 3, 100, 196, 14, q_share=True, tag="_qs"), _c(80, 2, 3, 3, 256, 208, 15, kv_share=True, tag="_kvs"),
       _c(80, 1, 3, 3, 256, 256, 64, q_share=True, kv_share=True, yard=True, tag="_qs_kvs"),
       _c(80, 1, 2, 3, 256, 384, 64, gcols=68)])
assert len({c.name for c in CASES}) == len(CASES)


def ldo_of(case):
    return case.H * case.hd + case.gcols  # every output is a view with guard columns beside it


def case_instance(case, n_batch=None):
    return instance_of(case.hd, case.mode, n_batch or case.B, case.n_q, case.n_k, case.grid_w, ldo_of(case), case.tok)


def tok_table(case):
    """int32 tok_rows [B, S*S] of a tok case (CPU) and the number of token rows: window b = (image, wy, wx), token
    i = (y, x) is row image * W*W + (wy S + y) W + (wx S + x) of the token buffer, or -1 outside the map."""
    S = case.grid_w
    W = S + MAP_EXTRA
    n_img = case.B // 4
    img, wy, wx = (t.reshape(-1, 1, 1) for t in torch.meshgrid(torch.arange(n_img), torch.arange(2), torch.arange(2), indexing="ij"))
    y, x = torch.arange(S).view(1, S, 1), torch.arange(S).view(1, 1, S)
    Y, X = wy * S + y, wx * S + x
    rows = torch.where((Y < W) & (X < W), img * W * W + Y * W + X, torch.full((), -1))
    return rows.reshape(case.B, S * S).to(torch.int32), n_img * W * W


def _walks(total, n_wg):
    return [(w * total // n_wg, (w + 1) * total // n_wg) for w in range(n_wg)]


def branches(case, n_cus=N_CUS):
    """The branch names a case drives, from its numbers alone (tests/test_flash_attn_plan_cpu.py lists, per instance, the
    ones that must be reached)."""
    inst = case_instance(case)
    out = set()
    nq, nk = case.n_q, case.n_k
    T = -(-nk // 64)
    tail = nk - (T - 1) * 64
    if inst in ("win4", "win4_tok"):
        NW, allkv, T, tail = 8, True, 4, nk - 192            # 3 full tiles + a 16-slot tail tile; 8 subtiles of 32 queries
    elif inst == "glob4":
        NW, allkv = 8, False
    else:
        NW, allkv = inst[2], inst[3]
    out.add("tiles=1" if T == 1 else "tiles=2" if T == 2 else "tiles>=3")
    if allkv and isinstance(inst, tuple):
        out.add("half_tail" if tail <= 32 else "full_tail")
    else:
        out.add("tail=1" if tail == 1 else "tail<=32" if tail <= 32 else "tail=33..63" if tail < 64 else "tail=full")
    nqb = -(-nq // (NW * 32))
    out.add("nqb=1" if nqb == 1 else "nqb>1")
    last = nq - (nqb - 1) * NW * 32
    if nq % 32:
        out.add("ragged_q")
    if last <= (NW - 1) * 32:
        out.add("idle_waves")
    if nq == 1:
        out.add("n_q=1")
    if nk == 1:
        out.add("n_k=1")
    if T >= 2:
        out.add("rescale_late")                               # make_data plants a late maximum in every tile after the first
    total = case.B * case.H * (nqb if isinstance(inst, tuple) else 1)
    if allkv:
        if total > n_cus:
            out.add("persistent_multi_block")
        per_win = total // case.B
        if any(e > s and (e - 1) // per_win != s // per_win for s, e in _walks(total, min(total, n_cus))):
            out.add("window_change_in_walk")
    if case.mode == 1 and (case.B * case.H * nqb) % 8:
        out.add("grid_not_multiple_of_8")
    if case.q_share:
        out.add("q_rows_shared")
    if case.kv_share:
        out.add("kv_rows_shared")
    if case.packed or case.tok:
        out.add("packed_qkv")
    if ldo_of(case) > case.H * case.hd:
        out.add("ldo>width")
    if ldo_of(case) % 8 == 4:
        out.add("ldo%8=4")                                    # O rows 8-byte, not 16-byte aligned
    if case.tok:
        rows, _ = tok_table(case)
        out.add("tok_rows")
        if (rows < 0).any():
            out.add("pad_keys")
        pad = (rows < 0)
        waves = torch.nn.functional.pad(pad, (0, -nq % 32), value=True).view(case.B, -1, 32)
        if waves.all(-1).any():
            out.add("all_pad_wave")
    return out


# ---------------------------------------------------------------------------------------------------------------
# data
# ---------------------------------------------------------------------------------------------------------------
def roles(n_q, T, b):
    """Query rows with a planted role in Q block b: lastkey (set to the planted last key), probe (a phantom zero key
    takes the row), late {tile t >= 1: row set to the key planted in tile t}.  A single query alternates between
    lastkey (even b) and probe (odd b)."""
    if n_q == 1:
        return ([0], [], {}) if b % 2 == 0 else ([], [0], {})
    lastkey = sorted({5 % n_q, n_q - 1})
    used = set(lastkey)
    probe = []
    for r in (9 % n_q, (2 * n_q) // 3, n_q - 2):
        if r >= 0 and r not in used:
            probe.append(r)
            used.add(r)
    late = {}
    for t in range(1, T):
        r = (13 + 7 * t) % n_q
        if r not in used and r % 16:
            late[t] = r
            used.add(r)
    return lastkey, probe, late


def late_key(t, n_k):
    """Index of the key planted as a late maximum in tile t (None where the tile has no room beside the last key)."""
    k = 64 * t + 5
    return k if k < n_k - 1 else None


def make_data(case, dev="cpu"):
    """Inputs of a case in the style of depth_ops_ref.attn64_data, at any size; generated on the CPU from a seed derived
    from the case name, rounded to f16 and moved to `dev`.  q, k ~ N(0, 1.4^2) (logit std ~2: peaked rows), v ~ N(0, 1),
    every 16th query scaled by 1/40 (near-uniform rows).  Per head: column 3 of every key (and of pad_k) is the constant
    4 and the probe queries are 0.1 N(0, 1) with -24 there: every real key's logit moves by -96 scale, a zero phantom
    key keeps logit 0 and takes the row.  V columns 8..15 get +1.  The last key is a planted vector (x 1.5) and the
    lastkey queries equal it: the running max rises in the last tile and a dropped last key takes the row's weight.
    In every tile t >= 1 key 64 t + 5 is a planted vector (x 1.25) and one query equals it: the running max rises in
    that tile (rescale_late).  The planted vectors are the same in every K/V block, so that shared row tables keep the roles.
    Layout: Q, K, V are column slices of wider buffers filled with 65504 (attn_few_ref.strided): separate ones, one
    packed qkv (packed), or one packed token buffer that tok_rows gathers from.  Buffers hold B blocks each; a shared row
    table (attn_few_ref.share_rows: 3 entries over 2 images) only redirects entries.
    Bias: mode 1 rel_h / rel_w f32 [B*H, n_q, 64] ~ N(0, (0.8 / scale)^2); mode 2 rel_aug f16 [B*H, n_q, 32] built by
    hand in the kernel's layout from rel tables of std 0.1 and the entry's own f16 queries (query i sits at ((i // S) % S,
    i % S)): columns 0..S-1 = q.Rh[qy - j + S - 1] / scale, S..2S-1 the same for w; rows of padded queries are NaN."""
    g = torch.Generator().manual_seed(zlib.crc32(case.name.encode()))
    rn = lambda *s: torch.randn(*s, generator=g)                                   # noqa: E731
    hd, H, B, nq, nk = case.hd, case.H, case.B, case.n_q, case.n_k
    D = H * hd
    T = -(-nk // 64)
    scale = float(torch.tensor(hd ** -0.5, dtype=F32))
    q, k, v = 1.4 * rn(B, nq, H, hd), 1.4 * rn(B, nk, H, hd), rn(B, nk, H, hd)
    q[:, ::16] /= 40
    k[..., PROBE_COL] = 4.0
    v[..., V_SHIFT] += 1.0
    klast = 1.5 * 1.4 * rn(H, hd)
    klast[:, PROBE_COL] = 4.0
    k[:, nk - 1] = klast
    klate = {}
    for t in range(1, T):
        if late_key(t, nk) is not None:
            klate[t] = 1.25 * 1.4 * rn(H, hd)
            klate[t][:, PROBE_COL] = 4.0
            k[:, late_key(t, nk)] = klate[t]
    d = SimpleNamespace(case=case, scale=scale, q_rows=None, kv_rows=None, tok_rows=None, pad_k=None, pad_v=None,
                        rel_h=None, rel_w=None, rel_aug=None)
    valid = torch.ones(B, nq, dtype=torch.bool)
    if case.tok:
        tok, d.n_out = tok_table(case)
        valid = tok >= 0
        pad_k, pad_v = 1.4 * rn(H, hd), rn(H, hd)
        pad_k[:, PROBE_COL] = 4.0
        pad_v[:, V_SHIFT] += 1.0
        k = torch.where(valid[:, :, None, None], k, pad_k)               # what the last key / late keys are where padded
    else:
        d.n_out = B * nq
    for b in range(B):
        lastkey, probe, late = roles(nq, T, b)
        for r in probe:
            q[b, r] = 0.1 * rn(H, hd)
            q[b, r, :, PROBE_COL] = -24.0
        for r in lastkey:
            q[b, r] = k[b, nk - 1]
        for t, r in late.items():
            if t in klate:
                q[b, r] = k[b, late_key(t, nk)]
    q, k, v = q.half(), k.half(), v.half()
    # ---- layout ----
    if case.tok:
        buf = torch.full((d.n_out, 3 * D + 8), 65504.0, dtype=F16)
        rows = tok[valid].long()
        for i, t in enumerate((q, k, v)):
            buf[rows, i * D:(i + 1) * D] = t.reshape(B, nq, D)[valid]
        buf = buf.to(dev)
        d.q, d.k, d.v = (buf[:, i * D:(i + 1) * D] for i in range(3))
        d.tok_rows = tok.to(dev)
        d.pad_k, d.pad_v = pad_k.half().reshape(D).to(dev), pad_v.half().reshape(D).to(dev)
    elif case.packed:
        assert nq == nk
        d.q = strided(q.reshape(B * nq, D).to(dev), 3 * D + 8, 0)
        d.k = strided(k.reshape(B * nk, D).to(dev), 3 * D + 8, D, base=d.q._base)
        d.v = strided(v.reshape(B * nk, D).to(dev), 3 * D + 8, 2 * D, base=d.q._base)
    else:
        d.q = strided(q.reshape(B * nq, D).to(dev), D + 24, 8)
        d.k = strided(k.reshape(B * nk, D).to(dev), D + 8, 0)
        d.v = strided(v.reshape(B * nk, D).to(dev), D + 24, 16)
    if case.q_share:
        d.q_rows = share_rows(nq).to(dev)
    if case.kv_share:
        d.kv_rows = share_rows(nk).to(dev)
    # ---- bias (from the entry's own f16 queries) ----
    if case.mode == 1:
        d.rel_h = ((0.8 / scale) * rn(B * H, nq, 64)).to(dev)
        d.rel_w = ((0.8 / scale) * rn(B * H, nq, 64)).to(dev)
    elif case.mode == 2:
        S = case.grid_w
        Rh, Rw = 0.1 * rn(2 * S - 1, hd), 0.1 * rn(2 * S - 1, hd)
        qe = q if not case.q_share else q[list(IMG_OF)]
        d.rel_aug = hand_rel_aug(qe.double(), Rh.double(), Rw.double(), S, scale, valid).to(dev)
        d.Rh, d.Rw = Rh.to(dev), Rw.to(dev)           # (S = 14: the GPU test takes rel_aug from ops.relpos_bias instead)
    return d


def hand_rel_aug(q, Rh, Rw, S, scale, valid):
    """rel_aug f16 [B*H, n_q, 32] in the kernel's layout from q [B, n_q, H, hd] (float64); rows of padded queries NaN."""
    B, nq, H, _ = q.shape
    i, j = torch.arange(nq), torch.arange(S)
    aug = torch.zeros(B, H, nq, 32, dtype=F64)
    for col0, R, pos in ((0, Rh, (i // S) % S), (S, Rw, i % S)):
        tab = R[pos[:, None] - j[None, :] + S - 1]                               # [n_q, S, hd]
        aug[..., col0:col0 + S] = torch.einsum("bqhd,qjd->bhqj", q, tab) / scale
    aug = torch.where(valid[:, None, :, None], aug, torch.full((), math.nan, dtype=F64))
    return aug.half().reshape(B * H * nq, 32)


# ---------------------------------------------------------------------------------------------------------------
# reference
# ---------------------------------------------------------------------------------------------------------------
def _starts(table, B, n):
    return [int(r) for r in table.tolist()] if table is not None else [b * n for b in range(B)]


def operands(d, *, ignore_q_rows=False, ignore_kv_rows=False, zero_pad_k=False):
    """float64 q [B, H, n_q, hd], k, v [B, H, n_k, hd] as entry b must see them, read back out of the buffers through the
    row tables / tok_rows (padded keys: pad_k / pad_v, padded queries: zero), and the query mask valid [B, n_q]."""
    c = d.case
    B, H, hd, nq, nk = c.B, c.H, c.hd, c.n_q, c.n_k
    dev = d.q.device
    if c.tok:
        rows = d.tok_rows.long()
        valid = rows >= 0
        rc = rows.clamp(min=0)

        def gather(t, pad):
            x = torch.where(valid[..., None], t[rc].double(), pad.double())
            return x.view(B, nq, H, hd).permute(0, 2, 1, 3)
        zero = torch.zeros(H * hd, dtype=F64, device=dev)
        return gather(d.q, zero), gather(d.k, zero if zero_pad_k else d.pad_k), gather(d.v, d.pad_v), valid
    qs = _starts(None if ignore_q_rows else d.q_rows, B, nq)
    ks = _starts(None if ignore_kv_rows else d.kv_rows, B, nk)
    blk = lambda t, s, n: torch.stack([t[r:r + n] for r in s]).double().view(B, n, H, hd).permute(0, 2, 1, 3)  # noqa: E731
    return blk(d.q, qs, nq), blk(d.k, ks, nk), blk(d.v, ks, nk), torch.ones(B, nq, dtype=torch.bool, device=dev)


def bias_terms(d, *, swap=False):
    """(rel_h term, rel_w term) [B, H, n_q, n_k] in score units (before the scale), or (None, None) in mode 0."""
    c = d.case
    if c.mode == 0:
        return None, None
    kk = torch.arange(c.n_k, device=d.q.device)
    if c.mode == 1:
        th, tw = (t.double().view(c.B, c.H, c.n_q, 64) for t in (d.rel_h, d.rel_w))
        kh, kw = kk // 64, kk % 64
    else:
        S = c.grid_w
        ra = d.rel_aug.double().view(c.B, c.H, c.n_q, 32).nan_to_num(nan=0.0)      # padded queries: no requirement
        th, tw = ra[..., :S], ra[..., S:2 * S]
        kh, kw = kk // S, kk % S
    if swap:
        th, tw = tw, th
    return th[..., kh], tw[..., kw]


def reference(d, *, drop=None, phantom=0, no_scale=False, v_next_head=False, kv_of_entry0=False, swap=False, **op_kw):
    """float64 softmax(scale q k^T + bias) v of every batch entry and head: (o [B, H, n_q, hd], P, s, q, k, v, bias
    magnitude, |rel_h term| in logits, valid).  Mistakes: drop (key slice left out), phantom (that many zero K / V rows
    with logit 0 after the last key: an unmasked tail), no_scale, v_next_head, kv_of_entry0 (entry 1 reads the K / V of
    entry 0), swap (rel_h / rel_w exchanged), and those of operands()."""
    q, k, v, valid = operands(d, **op_kw)
    if v_next_head:
        v = v.roll(-1, 1)
    if kv_of_entry0:
        k, v = k.clone(), v.clone()
        k[1], v[1] = k[0], v[0]
    sc = 1.0 if no_scale else d.scale
    raw = q @ k.transpose(-1, -2)
    mag = d.scale * (q.abs() @ k.abs().transpose(-1, -2))
    bh, bw = bias_terms(d, swap=swap)
    hmag = None
    if bh is not None:
        raw = raw + bh + bw
        mag = mag + d.scale * (bh.abs() + bw.abs())
        hmag = d.scale * bh.abs()
    s = sc * raw
    vv = v
    if phantom:
        s = torch.cat([s, s.new_zeros(*s.shape[:-1], phantom)], -1)
        vv = torch.cat([v, v.new_zeros(*v.shape[:-2], phantom, v.shape[-1])], -2)
    if drop is not None:
        s = s.clone()
        s[..., drop] = -math.inf
    P = torch.softmax(s, -1)
    return P @ vv, P, s, q, k, v, mag, hmag, valid


def tolerance(inst, d, P, s, q, k, v, mag, hmag, o):
    """Bound per output element [B, H, n_q, hd] for the kernel `inst` (a value of instance_of); logit units, u = 2^-24.

    Scores.  q.k (+ the rel terms in mode 2, as two extra k-steps against one-hot columns) are NQK = hd/16 (+2) MFMA
    32x32x16 steps of 16 exact f16 products, <= 6 roundings each: 6 NQK u mag_k with mag_k = scale (|q|.|k| + |rel_h| +
    |rel_w|).  In mode 1 rel_w is the f32 accumulator init of the same chain (its magnitude is in mag_k) and rel_h is
    added in the exponent, below.
    Exponent.  p_k = exp2(fma(s_k, c, -m)), c = f32(scale) * f32(log2 e) off by <= 2 u relative (2 u |s_k|), the fma
    rounds once (u (|s_k| + |m|)), v_exp_f32 is good to 1 ulp (2 u), and 2 u for the reference's own scale product:
    delta_k <= 6 NQK u mag_k + 4 u (|s_k| + M) + 4 u relative on p_k, M >= |m|.  The generic kernel rescales at EVERY
    rise of the running max, so m is the true running max and M = max_j |s_j|.  win4 / glob4 defer the rescale until a
    row's max has grown by more than 2^12: m sits up to 12 log2 units = 8.4 logits below the row max, M = max_j |s_j| + 9.
    Mode 1: the exponent is fma(s_k, c, rel_h c - m): rel_h c rounds once and carries c's 2 u (3 u |h_k|, h_k = scale
    |rel_h[q, k/64]|), the subtraction rounds once (u (|h_k| + M)): + 4 u |h_k| + u M.  An error of m, or of a rescale
    factor alpha = exp2(m_old - m_new), is common to a row's numerator and denominator and cancels.
    delta_k moves o by sum_k P_k delta_k |v_k - o|.
    P is rounded to f16 for the P.V MFMA: relative 2^-11, absolute 2^-25 in the subnormal range; l >= 1 at the end (the
    row max has p >= 1 up to roundings).  Row sum, two forms:
      * ones-column (head_dim 80 and 16, win4, glob4: V's padded width leaves room): l is summed by the same MFMA from
        the same rounded P, so the rounding e_k is common and moves o by sum_k P_k e_k (v_k - o):
        2^-11 sum_k P_k |v_k - o| + 2^-25 sum_k |v_k - o|;
      * VALU (head_dim 64 and 32: padded width == head width): l is summed from the UNROUNDED p, the rounding is in the
        numerator alone: 2^-11 sum_k P_k |v_k| + 2^-25 sum_k |v_k|.
    Accumulation.  4 P.V MFMA steps per 64-key tile, <= 6 roundings each, and at most one rescale per tile: 25 T u
    sum_k P_k |v_k|, T = ceil(n_k / 64).  l by the ones-column: the same chain, 25 T u |o|; on the VALU: 32 adds per tile
    and lane, one add per tile into the running sum, one rescale per tile, one cross-half add: (34 + 2 T) u |o|.
    o = O * (1 / l): 3 u |o|; the f16 store: 2^-11 |o| + 2^-25.  |v_k - o| <= |v_k| + |o| throughout, so every term is a
    matrix product."""
    c = d.case
    nk = c.n_k
    T = -(-nk // 64)
    dedicated = not isinstance(inst, tuple)
    hd_k, mode = (80, c.mode) if dedicated else inst[:2]
    nqk = hd_k // 16 + (2 if mode == 2 else 0)
    ones_column = dedicated or hd_k in (80, 16)
    M = s.abs().amax(-1, keepdim=True) + (9 if dedicated else 0)
    delta = 6 * nqk * U * mag + 4 * U * (s.abs() + M) + 4 * U
    if mode == 1:
        delta = delta + 4 * U * hmag + U * M
    Pd = P * delta
    va, oa = v.abs(), o.abs()
    A = P @ va
    vsum = va.sum(-2, keepdim=True)
    tol = Pd @ va + Pd.sum(-1, keepdim=True) * oa + 25 * T * U * A + (3 * U + H16) * oa + SUB16
    if ones_column:
        return tol + H16 * (A + oa) + SUB16 * (vsum + nk * oa) + 25 * T * U * oa
    return tol + H16 * A + SUB16 * vsum + (34 + 2 * T) * U * oa


def place(d, x, *, at_q_rows=False, valid=None):
    """[B, H, n_q, hd] -> the float64 image of the O buffer [rows of O, H * hd], NaN where nothing is written: dense
    (row b n_q + i), or scattered to token order by tok_rows (padded queries nowhere).  Mistake at_q_rows: entry b is
    written at q_batch_rows[b] + i (later entries overwrite earlier ones)."""
    c = d.case
    rowsx = x.permute(0, 2, 1, 3).reshape(c.B, c.n_q, c.H * c.hd)
    buf = torch.full((d.n_out, c.H * c.hd), math.nan, dtype=F64, device=x.device)
    if c.tok:
        buf[d.tok_rows.long()[valid]] = rowsx[valid]
    elif at_q_rows:
        for b, r in enumerate(_starts(d.q_rows, c.B, c.n_q)):
            buf[r:r + c.n_q] = rowsx[b]
    else:
        buf[:] = rowsx.reshape(c.B * c.n_q, -1)
    return buf


def expected(d):
    """(reference buffer, bound buffer) of a case: what O must hold, NaN where it must stay untouched."""
    o, P, s, q, k, v, mag, hmag, valid = reference(d)
    tol = tolerance(case_instance(d.case), d, P, s, q, k, v, mag, hmag, o)
    return place(d, o, valid=valid), place(d, tol, valid=valid)


def buf_within(got, ref, tol, what):
    """Every written element within the bound, every other element still NaN; returns the worst error / bound."""
    w = ~ref.isnan()
    assert got[~w].isnan().all(), f"{what}: an element of O that must stay untouched was written"
    z, one = torch.zeros((), dtype=F64, device=ref.device), torch.ones((), dtype=F64, device=ref.device)
    return assert_within(torch.where(w, got, z), torch.where(w, ref, z), torch.where(w, tol, one), what)


def buf_discrimination(wrong, ref, tol):
    """max |wrong - ref| / tol over the buffer; an element written by only one of the two counts as infinitely far."""
    both_nan = wrong.isnan() & ref.isnan()
    r = ((wrong - ref).abs() / tol).nan_to_num(nan=math.inf)
    return torch.where(both_nan, torch.zeros((), dtype=F64, device=ref.device), r).max().item()


def mistakes(d):
    """(name, wrong O buffer) of every named mistake that applies to the case."""
    c = d.case
    inst = case_instance(c)
    nk = c.n_k
    T = -(-nk // 64)
    tail = nk - (T - 1) * 64
    slots = 64 * T
    if inst in ("win4", "win4_tok"):
        tail, slots = nk - 192, 208                           # the tail tile of the window kernel has 16 key slots
    have_probe = any(roles(c.n_q, T, b)[1] for b in range(c.B))
    valid = operands(d)[3]
    P_ = lambda **kw: place(d, reference(d, **kw)[0], valid=valid)     # noqa: E731
    out = []
    if nk > 1:
        out.append(("last key dropped", P_(drop=slice(nk - 1, nk))))
        out.append(("scale omitted", P_(no_scale=True)))
    if slots > nk and have_probe:
        out.append(("tail unmasked", P_(phantom=slots - nk)))
    if tail > 32:
        out.append(("keys 32..63 of the last tile dropped", P_(drop=slice(nk - tail + 32, nk))))
    out.append(("V of head h+1", P_(v_next_head=True)))
    out.append(("K/V of batch entry 0 used for entry 1", P_(kv_of_entry0=True)))
    if c.q_share:
        out.append(("q_batch_rows ignored", P_(ignore_q_rows=True)))
        out.append(("O written at the shared Q rows instead of densely", place(d, reference(d)[0], at_q_rows=True)))
    if c.kv_share:
        out.append(("kv_batch_rows ignored", P_(ignore_kv_rows=True)))
    if c.mode in (1, 2):
        out.append(("rel_h and rel_w swapped", P_(swap=True)))
    if c.tok:
        out.append(("pad_k zero instead of the bias row", P_(zero_pad_k=True)))
        # a padded query computes on the stand-in row 0 of Q; stored, it lands on row 0 of O
        o = reference(d)[0]
        b, i = (~valid).nonzero()[-1].tolist()
        q0 = d.q[0].double().view(c.H, 1, c.hd)
        k, v = operands(d)[1:3]
        bh, bw = bias_terms(d)
        s = d.scale * (q0 @ k[b].transpose(-1, -2) + (bh + bw)[b, :, i:i + 1])
        wrong = place(d, o, valid=valid)
        wrong[0] = (torch.softmax(s, -1) @ v[b]).reshape(-1)
        out.append(("padded query stored", wrong))
    return out
