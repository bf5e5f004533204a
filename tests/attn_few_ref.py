"""float64 reference, input generators and case tables for the few-key / few-query attention family
(inklayer_amd/csrc/attn_few.hip: attn_fewkeys_kernel<HD, T>, attn_fewkeys16_f32_kernel<NK>, attn_fewq16_kernel<QW>).
Shared by tests/test_attn_few_gpu.py (the kernels) and tests/test_attn_few_ref_cpu.py (that the reference is right and
the generated inputs do what they claim, on the CPU).  CPU-only: nothing here touches the package under test; every
function runs on whatever device its inputs live on."""
import torch

G = 30.0                     # score of a planted key with mult 1, in natural-log units
IMG_OF = (1, 0, 1)           # batch entry -> image when three entries share the rows of two images

# the project's bounds for this family (tests/test_precision_gpu.py, tests/test_gdino_gpu.py)
TOL_FEWKEYS_F32 = 2e-6       # x max(1, |ref|max)
TOL_FEWQ = 5e-6              # x max(1, |ref|max)
TOL_F16 = 2e-3               # absolute: half an f16 ulp is 9.8e-4 below 4 (every f16 case keeps |ref| < 4)


def attn_ref(q, k, v, scale, *, blocked=None, q_add=None, k_add=None, dtype=torch.float64):
    """softmax(scale (q + q_add)(k + k_add)^T [blocked -> -inf]) v per batch entry and head, evaluated in `dtype`.
    q [n, n_q, H, hd], k / v [n, n_k, H, hd]; q_add [n_q, H * hd] and k_add [n_k, H * hd] are added by position;
    blocked [n_q, n_k], nonzero = not allowed.  -> [n, n_q, H, hd]."""
    n, n_q, H, hd = q.shape
    q, k, v = q.to(dtype), k.to(dtype), v.to(dtype)
    if q_add is not None:
        q = q + q_add.to(dtype).view(1, n_q, H, hd)
    if k_add is not None:
        k = k + k_add.to(dtype).view(1, k.shape[1], H, hd)
    s = torch.einsum("bqhd,bkhd->bhqk", q, k) * scale
    if blocked is not None:
        s = s.masked_fill(blocked.bool()[None, None], float("-inf"))
    return torch.einsum("bhqk,bkhd->bqhd", s.softmax(-1), v)


def scores64(q, k, scale):
    """float64 scores [n, H, n_q, n_k] of rows laid out as in attn_ref."""
    return torch.einsum("bqhd,bkhd->bhqk", q.double(), k.double()) * scale


def rows2d(t):
    """[n, r, H, hd] -> the [n * r, H * hd] row matrix the ops take."""
    return t.reshape(t.shape[0] * t.shape[1], -1)


def strided(t, ld, col0, base=None):
    """The rows of t [rows, w] as the column slice [col0, col0 + w) of a buffer of width ld filled with NaN (65504 for
    f16): a read outside the slice shows in the result.  col0 and ld are multiples of 8 elements, so every row of the
    view stays 16-byte aligned.  base: embed into this buffer (view._base of an earlier call) instead of a new one."""
    rows, w = t.shape
    assert ld % 8 == 0 and col0 % 8 == 0 and col0 + w <= ld
    if base is None:
        fill = 65504.0 if t.dtype == torch.float16 else float("nan")
        base = torch.full((rows, ld), fill, dtype=t.dtype, device=t.device)
    assert base.shape == (rows, ld) and base.dtype == t.dtype and base.is_contiguous()
    view = base[:, col0:col0 + w]
    view.copy_(t)
    return view


def share_rows(rows_per_image, img_of=IMG_OF):
    """int32 table: first row of each batch entry when entry b reads the rows of image img_of[b]."""
    return torch.tensor([i * rows_per_image for i in img_of], dtype=torch.int32)


def randn_inputs(hd, n_q, n_k, seed, n=3, H=8, n_q_blocks=None, n_kv_blocks=None, k_gain=1.0, dtype=torch.float32,
                 clamp=None):
    """Seeded standard-normal q [n_q_blocks or n, n_q, H, hd], k / v [n_kv_blocks or n, n_k, H, hd] (k times k_gain),
    rounded to dtype.  clamp bounds |v| (the f16 cases: keeps every output below 4, see TOL_F16)."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    q = torch.randn(n_q_blocks or n, n_q, H, hd, generator=g)
    k = torch.randn(n_kv_blocks or n, n_k, H, hd, generator=g) * k_gain
    v = torch.randn(n_kv_blocks or n, n_k, H, hd, generator=g)
    if clamp is not None:
        v = v.clamp(-clamp, clamp)
    return q.to(dtype), k.to(dtype), v.to(dtype)


def planted_inputs(hd, n_k, plant, seed, n=3, H=8, n_q=7, dtype=torch.float32):
    """q = 1 + 0.25 randn, k / v = randn; for each (key, mult) of plant the key row `key` of every batch entry and head
    is the constant mult * G / (scale * hd), scale = hd^-0.5: its score is mult * G * mean(q row), about mult * 30
    natural-log units for every query, far above the few units of the other keys.  -> q, k, v, scale."""
    scale = hd ** -0.5
    g = torch.Generator(device="cpu").manual_seed(seed)
    q = 1 + 0.25 * torch.randn(n, n_q, H, hd, generator=g)
    k = torch.randn(n, n_k, H, hd, generator=g)
    v = torch.randn(n, n_k, H, hd, generator=g)
    for key, mult in plant:
        k[:, key] = mult * G / (scale * hd)
    return q.to(dtype), k.to(dtype), v.to(dtype), scale


def competing_inputs(seed, n_q, n_k=300, n=3, H=8):
    """Keys 5 and 299 planted at G and G + 1 (key 299's constant times (G + 1) / G: not bit-equal): two dominant keys
    one natural-log unit apart, one per key-range group, so the f32 rounding of scores of 30..60 moves both weights."""
    q, k, v, scale = planted_inputs(16, n_k, [(5, 1), (n_k - 1, 1)], seed, n=n, H=H, n_q=n_q)
    k[:, n_k - 1] *= (G + 1) / G
    return q, k, v, scale


# ---------------------------------------------------------------------------------------------------------------
# block masks of attn_fewkeys (u8 [n_q, n_k], 1 = not allowed); every one keeps at least one key per query row
# ---------------------------------------------------------------------------------------------------------------
def block_diagonal(n):
    """The detector's text self-attention mask: tokens see their own phrase only.  Phrase lengths 1, 2, 1, 3, 1, 4, ...
    cut at n (n = 4 gives the [1, 2, 1] pattern of the fixed caption)."""
    m = torch.ones(n, n, dtype=torch.uint8)
    lo, i = 0, 0
    while lo < n:
        size = 1 if i % 2 == 0 else 2 + i // 2
        hi = min(n, lo + size)
        m[lo:hi, lo:hi] = 0
        lo, i = hi, i + 1
    return m


def random_blocked(n_q, n_k, seed):
    """Half of the pairs blocked at random, key q % n_k of query q kept (the diagonal when n_q = n_k)."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    m = (torch.rand(n_q, n_k, generator=g) < 0.5).to(torch.uint8)
    m[torch.arange(n_q), torch.arange(n_q) % n_k] = 0
    return m


def block_key_for_odd_queries(n_q, n_k, key):
    """`key` blocked for every odd query: half of the queries lose a planted key."""
    m = torch.zeros(n_q, n_k, dtype=torch.uint8)
    m[1::2, key] = 1
    return m


F16_FORMS = ((32, 8), (64, 4))               # (head_dim, n_heads) of the f16 kernels: the detector's two text attentions
F16_NK = (1, 2, 4, 5, 15, 16)
F16_CLAMP = 3.5                              # |v| of the f16 cases: outputs stay below 4 (TOL_F16)


def f16_inputs(hd, H, n_q, n_k):
    """q, k, v of the f16 GPU case (hd, H, n_q, n_k), rounded to f16."""
    return randn_inputs(hd, n_q, n_k, seed=1000 * hd + 20 * n_q + n_k, H=H, dtype=torch.float16, clamp=F16_CLAMP)


def blocked_cases():
    """(name, n_q, n_k, matrix) of every block mask the f16 GPU cases run, for either form."""
    cases = [(f"diag{n}", n, n, block_diagonal(n)) for n in (4, 5, 16)]
    cases += [(f"rand{nq}x{nk}", nq, nk, random_blocked(nq, nk, 100 * nq + nk)) for nq, nk in ((5, 5), (16, 16), (37, 15))]
    return cases


# ---------------------------------------------------------------------------------------------------------------
# the planted cases of the GPU tests (tests/test_attn_few_ref_cpu.py checks the claims on each)
# ---------------------------------------------------------------------------------------------------------------
FEWQ_NQ = (7, 12)            # one n_q of each attn_fewq16_kernel<QW> form, both with inactive query slots
FEWQ_PLANTS = (              # (n_k, plant)
    (300, ((5, 1),)),
    (300, ((5, 1), (170, 2), (299, 3))),             # the running maximum moves up twice, the last time in the last tile
    (300, ((299, 3), (170, 2), (5, 1))),             # ... the dominant key is in the first tile of group 0
    (300, ((5, 2), (299, 2))),                       # a tie across the two groups: the mean of two value rows
    (129, ((128, 1),)),                              # the only key of group 1's last tile dominates
    (40, ((39, 1),)),                                # group 1 has no keys
    (4096, ((70, 1), (2047, 2), (2048, 3), (4095, 4))),
    (4096, ((63, 3), (4095, 3))),
)
FEWKEYS_NQ = 37
FEWKEYS_PLANTS = (           # (head_dim, n_heads, dtype, n_k, plant, blocked key or None)
    (16, 8, torch.float32, 7, ((6, 1),), None),
    (16, 8, torch.float32, 16, ((0, 1), (15, 1)), None),
    (16, 8, torch.float32, 5, ((4, 1),), None),
    (32, 8, torch.float32, 16, ((3, 1),), None),
    (64, 4, torch.float16, 16, ((15, 1), (2, 2)), None),
    (32, 8, torch.float16, 4, ((0, 1),), 0),
)


def plant_seed(n_k, plant):
    return 1000 + n_k + sum(17 * key + mult for key, mult in plant)


def top_gap(s, plant, blocked=None):
    """Smallest margin, over (entry, head, query), between the top planted score and every key outside the top set (the
    keys planted with the largest mult).  s: float64 scores [n, H, n_q, n_k].  Blocked pairs leave: a query whose top
    keys are all blocked is not counted."""
    top_mult = max(mult for _, mult in plant)
    top = [key for key, mult in plant if mult == top_mult]
    s = s.clone()
    if blocked is not None:
        s = s.masked_fill(blocked.bool()[None, None], float("-inf"))
    best = s[..., top].min(-1).values
    rest = s.clone()
    rest[..., top] = float("-inf")
    gap = best - rest.max(-1).values
    return gap[torch.isfinite(best)].min().item()


def max_err(got, ref):
    """(largest |got - ref|, |ref|max) with got moved to the CPU in float64."""
    got = got.detach().double().cpu().reshape(ref.shape)
    return (got - ref.double()).abs().max().item(), ref.abs().max().item()
