"""Case builders for the edge suites of the automatic mask generator's kernels (csrc/amg.hip): pure numpy / torch, no GPU
and no inklayer_amd import.  tests/test_amg_edges_ref_cpu.py shows on the CPU that the lists have power (a planted
variant of tests/amg_ref.py differs on at least one case of each), tests/test_amg_edges_gpu.py runs them through the
ops.  Also the plane packers and the noise that tests/test_amg_gpu.py uses."""
import numpy as np
import torch


# ------------------------------------------------------------------------------------------------ planes, noise
def smooth_noise(seed, n, h, w, k=9, scale=14.0, bias=1.5):
    """Box-filtered noise scaled to a few units minus a bias: each mask a handful of blobs that both stability
    thresholds cut through."""
    rs = np.random.RandomState(seed)
    x = torch.from_numpy(rs.standard_normal((n, 1, h, w)).astype(np.float32))
    ker = torch.ones(1, 1, k, k) / (k * k)
    return (torch.nn.functional.conv2d(x, ker, padding=k // 2)[:, 0] * scale - bias).contiguous()


def unpack_planes(planes, H):
    """column-major bit planes int64 [m, W, ceil(H / 64)] -> bool [m, H, W]"""
    p = planes.cpu().numpy().view(np.uint64)
    bits = (p[..., None] >> np.arange(64, dtype=np.uint64)) & np.uint64(1)
    m, W, hp, _ = bits.shape
    full = bits.reshape(m, W, hp * 64)
    assert not full[:, :, H:].any(), "bits of rows >= H must be zero"
    return torch.from_numpy(full[:, :, :H].astype(bool).transpose(0, 2, 1).copy())


def pack_planes(masks, dev=None):
    """bool [m, H, W] -> column-major bit planes, on the device when one is given (test-side construction of hand-made
    planes)"""
    m, H, W = masks.shape
    hp = -(-H // 64)
    pad = np.zeros((m, W, hp * 64), dtype=np.uint64)
    pad[:, :, :H] = masks.numpy().transpose(0, 2, 1)
    words = (pad.reshape(m, W, hp, 64) << np.arange(64, dtype=np.uint64)).sum(-1, dtype=np.uint64)
    out = torch.from_numpy(words.view(np.int64))
    return out if dev is None else out.to(dev)


# ------------------------------------------------------------------------------------------------ stats op
# (crop_hw, xy0 = (x0, y0), orig_hw or None for the full frame).  The stats kernel's rows form serves crop_w % 4 == 0, a
# thread owns 4 columns and steps 256 threads (a second trip above 1024 columns); a workgroup owns one band of 64 frame
# rows.
_FRAME = (200, 40)
STATS_GEOMS = [
    ((5, 1028), (0, 0), None),               # rows form, second trip of the column loop
    ((6, 1032), (3, 61), (70, 1040)),        # the same inside a frame, across the 63/64 band line
    ((7, 3), (0, 0), None),                  # one-pixel form below 4 columns
    ((1, 1), (0, 0), None),
    ((9, 1), (0, 0), None),
    ((9, 4), (0, 0), None),                  # rows form with one thread
    ((63, 8), (0, 0), None),
    ((64, 8), (0, 0), None),
    ((65, 8), (0, 0), None),
    ((128, 12), (0, 0), None),
    ((129, 7), (0, 0), None),
    # crops in a 200 x 40 frame; x0 == 0 and x0 + cw == orig_w occur in both forms
    ((64, 8), (0, 64), _FRAME),              # exactly one aligned band
    ((64, 7), (33, 64), _FRAME),
    ((2, 12), (28, 63), _FRAME),             # one row on each side of a band line
    ((2, 5), (0, 63), _FRAME),
    ((62, 8), (0, 1), _FRAME),               # inside one band, touching neither end
    ((62, 7), (33, 1), _FRAME),
    ((100, 12), (28, 100), _FRAME),          # y0 + ch == orig_h
    ((100, 5), (0, 100), _FRAME),
]


def stats_input_hw(crop_hw, L=1024):
    """ResizeLongestSide.get_preprocess_shape, as oracle.sam_ref.preprocess_shape states it"""
    sc = L * 1.0 / max(crop_hw)
    return int(crop_hw[0] * sc + 0.5), int(crop_hw[1] * sc + 0.5)


def stats_corner_is_shared(crop_hw):
    """Where the crop is about as large as the model's input (scale ~ 1 in both stages' composition), the clamped first
    two and last two rows and columns of the virtual 1024 frame are copies of one low-res row / column, so the pixels
    next to a corner repeat the corner's value whatever the logits: no threshold turns on the corner pixel alone."""
    return max(crop_hw) > 512


RAMP_CORNERS = [(0, 0), (0, 1), (1, 0), (1, 1)]        # (bottom?, right?)


def ramp(bottom, right, S=256):
    """Integer-valued low-res ramp with its one maximum at a corner of the plane; the crop occupies the plane's top-left
    part, so the maximum over the crop lies at the crop's corner of the same name.  Integer values keep the blends of
    equal neighbours exact (l v + (1 - l) v == v), so structural ties are exact ties."""
    yy, xx = torch.meshgrid(torch.arange(float(S)), torch.arange(float(S)), indexing="ij")
    return -((yy - (S - 1) * bottom).abs() + (xx - (S - 1) * right).abs())


def stats_low(content, seed):
    """low-res logits [5, 256, 256].  "noise": three noise masks, an all-negative and an all-positive one; "ramps": the
    four corner ramps and one noise mask."""
    if content == "noise":
        nz = smooth_noise(seed, 3, 256, 256)
        return torch.cat([nz[:2], torch.full((1, 256, 256), -3.0), torch.full((1, 256, 256), 3.0), nz[2:]]).contiguous()
    assert content == "ramps"
    return torch.cat([torch.stack([ramp(b, r) for b, r in RAMP_CORNERS]), smooth_noise(seed, 1, 256, 256)]).contiguous()


def second_largest(logits):
    """the second-largest distinct value of a mask's logits (the largest when there is only one)"""
    u = torch.unique(logits)
    return float(u[-2] if len(u) > 1 else u[-1])


def tie_thresholds(logits):
    """(thr, offset) as Python floats with float32(thr + offset) == a and float32(thr - offset) == b for two logits
    a >= b that occur: a the second-largest distinct value, b the first distinct value from the median downwards for
    which both sums are exact in double (values of very different magnitude can round)."""
    u = torch.unique(logits).double()
    a = float(u[-2] if len(u) > 1 else u[-1])
    for i in range(len(u) // 2, -1, -1):
        b = float(u[i])
        thr, off = (a + b) / 2, (a - b) / 2
        if thr + off == a and thr - off == b:
            return thr, off, a, b
    raise AssertionError("no exact pair")


# ------------------------------------------------------------------------------------------------ RLE
RLE_SHAPES = [(64, 255), (64, 256), (64, 257), (64, 513), (65, 128), (65, 129), (1, 300), (1, 1), (63, 260),
              (128, 130), (129, 90)]                   # T = W * ceil(H / 64) words over 256 threads


def rle_masks(H, W):
    """bool [k, H, W] and the names of the patterns"""
    names = ["empty", "full", "px00", "px0W", "pxH0", "pxHW", "last_row", "bern50", "columns", "alt0", "alt1", "bern02"]
    hand = torch.zeros(len(names) + 1, H, W, dtype=torch.bool)
    hand[1] = True
    hand[2, 0, 0] = True
    hand[3, 0, W - 1] = True
    hand[4, H - 1, 0] = True
    hand[5, H - 1, W - 1] = True
    hand[6, H - 1, :] = True                      # the last row: a run that ends each column
    hand[6, 0, 1:] = True                         # ... and continues into the next one
    rs = np.random.RandomState(1000 * H + W)
    hand[7] = torch.from_numpy(rs.uniform(size=(H, W)) < 0.5)
    hand[8, :, ::2] = True                        # whole columns
    p = torch.arange(W)[None, :] * H + torch.arange(H)[:, None]      # position in the column-major order
    hand[9] = p % 2 == 1                          # every position a change; starts with a zero
    hand[10] = p % 2 == 0                         # ... starts with a one
    hand[11] = torch.from_numpy(rs.uniform(size=(H, W)) < 0.02)
    if W >= 8:                                    # one long run: many consecutive chunks without a change
        hand[12, :, 3:W - 3] = True
        names.append("one_run")
    return hand[:len(names)].contiguous(), names


def rle_select(k):
    """reverse order with a repeated index"""
    return [k - 1] + list(range(k - 1, -1, -1))


# ------------------------------------------------------------------------------------------------ small regions
RSR_SHAPES = [(1, 1), (1, 70), (70, 1), (63, 5), (64, 5), (65, 5), (129, 66), (5, 300)]
RSR_MIN_AREAS = (0, 1, 2, 5, 10 ** 6)                  # for the general patterns
RSR_A = 4                                              # rectangles of area RSR_A - 1, RSR_A, RSR_A + 1
RSR_MODES = (("holes",), ("islands",), ("holes", "islands"))


def _zeros(H, W):
    return torch.zeros(H, W, dtype=torch.bool)


def rsr_general(H, W):
    """[(name, bool [H, W])]: the patterns that go through every min_area of RSR_MIN_AREAS, where the shape has room"""
    out = [("empty", _zeros(H, W)), ("full", ~_zeros(H, W))]
    m = _zeros(H, W)
    m[H // 2, W // 2] = True
    out.append(("one_pixel", m))
    yy, xx = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    out.append(("checker0", (yy + xx) % 2 == 0))       # at odd H column 0 holds (H + 1) / 2 runs: the run bound
    out.append(("checker1", (yy + xx) % 2 == 1))
    L = min(W, 5)
    if L >= 2 and H >= L:                              # one-pixel-wide diagonals through rows 62 .. 66 where H allows
        r0 = min(62, H - L)
        d, a = _zeros(H, W), _zeros(H, W)
        for i in range(L):
            d[r0 + i, i] = True
            a[r0 + i, L - 1 - i] = True
        out += [("diagonal", d), ("antidiagonal", a)]
    if H >= 65 and W >= 4:                             # two blobs that touch only corner to corner across rows 63 / 64
        m = _zeros(H, W)
        m[62:64, 0:2] = True
        m[64:66, 2:4] = True
        out.append(("corner_touch", m))
        out.append(("corner_touch_flipped", m.flip(1)))
    rs = np.random.RandomState(7 * H + W)
    for p in (0.1, 0.5, 0.9):
        out.append((f"bern{int(p * 100)}", torch.from_numpy(rs.uniform(size=(H, W)) < p)))
    return out


def _along(H, W, cells):
    """a mask from cells (position along the long axis, position across it)"""
    m = _zeros(H, W)
    for u, v in cells:
        if H >= W:
            m[u, v] = True
        else:
            m[v, u] = True
    return m


def rsr_areas(H, W, a=RSR_A):
    """[(name, mask)] for min_area = a: one-pixel-thick rectangles of area a - 1, a and a + 1 along the long axis, as
    islands (together, and each alone: alone, the small one is also the largest) and, where the short axis has three
    pixels, as enclosed holes of a block."""
    long, short = max(H, W), min(H, W)
    if long < 3 * a + 8:
        return []
    out, pos, spans = [], 1, []
    for n in (a - 1, a, a + 1):
        spans.append((pos, n))
        pos += n + 2
    v = short // 2
    out.append(("islands_all", _along(H, W, [(s + i, v) for s, n in spans for i in range(n)])))
    for s, n in spans:
        out.append((f"island_{n}", _along(H, W, [(s + i, v) for i in range(n)])))
    if short >= 3:
        block = [(u, vv) for u in range(0, pos) for vv in (v - 1, v, v + 1)]
        holes = {(s + i, v) for s, n in spans for i in range(n)}
        out.append(("holes_all", _along(H, W, [c for c in block if c not in holes])))
        for s, n in spans:
            one = {(s + i, v) for i in range(n)}
            out.append((f"hole_{n}", _along(H, W, [c for c in block if c not in one])))
    return out


def rsr_ties(H, W):
    """[(name, mask)] for min_area above every area, mode islands: the first of the equal largest components in raster
    order of their first pixels stays.  Each mask also holds a smaller island."""
    out = []
    if W >= 6:                                         # same top row, different x
        y = min(1, H - 1)
        m = _zeros(H, W)
        m[y, 0:2] = True
        m[y, 3:5] = True
        m[H - 1, W - 1] = True
        out.append(("same_row", m))
    if W >= 6 and H >= 5:                              # the smaller y on the larger x
        m = _zeros(H, W)
        m[0:2, 4] = True
        m[2:4, 0] = True
        m[H - 1, 2] = True
        out.append(("upper_right_first", m))
    if H >= 12:                                        # three equal, one above the other (and shifted where W allows)
        m = _zeros(H, W)
        for i, y in enumerate((6, 3, 9)):
            m[y:y + 2, min(W - 1, 2 * (2 - i))] = True
        m[0, 0] = True
        out.append(("three_equal", m))
    elif W >= 12:
        m = _zeros(H, W)
        for x in (3, 6, 9):
            m[0, x:x + 2] = True
        m[H - 1, 0] = True
        out.append(("three_equal", m))
    return out


def rsr_cases(H, W):
    """[(min_area, names, bool [k, H, W])] for one shape"""
    gen = rsr_general(H, W)
    out = [(a, [n for n, _ in gen], torch.stack([m for _, m in gen])) for a in RSR_MIN_AREAS]
    for a, lst in ((RSR_A, rsr_areas(H, W)), (10 ** 6, rsr_ties(H, W))):
        if lst:
            out.append((a, [n for n, _ in lst], torch.stack([m for _, m in lst])))
    return out


# ------------------------------------------------------------------------------------------------ NMS
def cluster_boxes(rs, n):
    """heavy overlap: a few dozen clusters of jittered copies"""
    c = rs.uniform(0, 800, (40, 2))
    s = rs.uniform(20, 200, (40, 2))
    k = rs.randint(0, 40, n)
    xy = c[k] + rs.uniform(-6, 6, (n, 2))
    wh = s[k] * rs.uniform(0.85, 1.15, (n, 2))
    return torch.from_numpy(np.concatenate([xy, xy + wh], 1).astype(np.float32))


CHAIN = torch.tensor([[0., 0., 10., 10.], [4., 0., 14., 10.], [8., 0., 18., 10.]])   # iou(A,B) = iou(B,C) = 3/7, iou(A,C) = 1/9
CHAIN_THR = 0.3
CHAIN_POSITIONS = [(62, 63, 64), (63, 64, 65), (0, 64, 128)]


def chain_case(positions, n=200, seed=0):
    """A > B > C in score at the given positions of the sorted order: A suppresses B, B alone would suppress C, so C
    survives.  The other boxes lie far away and apart; the original order is a permutation of the sorted one."""
    far = torch.tensor([[1000. + 30 * i, 500., 1020. + 30 * i, 520.] for i in range(n)])
    boxes = far.clone()
    for p, b in zip(positions, CHAIN):
        boxes[p] = b
    scores = torch.tensor([1.0 - i / 1024.0 for i in range(n)])          # exact in float32, strictly descending
    perm = torch.from_numpy(np.random.RandomState(seed).permutation(n))
    return boxes[perm].contiguous(), scores[perm].contiguous(), perm


def nms_cases():
    """[(name, boxes f32 [n, 4], scores f32 [n], thr)]"""
    rs = np.random.RandomState(17)
    out = []
    for n in (127, 128, 192, 193):
        b = cluster_boxes(rs, n)
        s = torch.from_numpy((rs.randint(0, 20, n) / 20.0).astype(np.float32))          # many ties
        for thr in (0.7, 0.3):
            out.append((f"clusters_{n}_{thr}", b, s, thr))
        out.append((f"equal_scores_{n}", b, torch.full((n,), 0.5), 0.5))
    # thr == 0: boxes that share an edge have intersection 0 and are kept; a sliver of overlap suppresses
    grid = torch.tensor([[10. * i, 10. * j, 10. * i + 10, 10. * j + 10] for j in range(9) for i in range(15)])
    sliver = grid.clone()
    sliver[1::2, 0] -= 0.125                                                             # every second box reaches into its left neighbour
    sg = torch.from_numpy(rs.permutation(len(grid)).astype(np.float32))
    out.append(("edges_thr0", grid, sg, 0.0))
    out.append(("slivers_thr0", sliver, sg, 0.0))
    out.append(("edges_equal_scores_thr0", grid, torch.zeros(len(grid)), 0.0))
    for pos in CHAIN_POSITIONS:
        b, s, _ = chain_case(pos)
        out.append((f"chain_{pos[0]}_{pos[1]}_{pos[2]}", b, s, CHAIN_THR))
    b = cluster_boxes(rs, 150) - 400.0                                                   # negative coordinates
    out.append(("negative", b, torch.from_numpy(rs.uniform(size=150).astype(np.float32)), 0.5))
    b = cluster_boxes(rs, 150)                                                           # x2 < x1 / y2 < y1: computed as given
    b[::3] = b[::3][:, [2, 1, 0, 3]]
    b[1::7] = b[1::7][:, [0, 3, 2, 1]]
    s = torch.from_numpy((rs.randint(0, 50, 150) / 50.0).astype(np.float32))
    for thr in (0.5, 0.0, -0.5):
        out.append((f"inverted_{thr}", b.contiguous(), s, thr))
    # iou == thr exactly is kept: 1 / 2 and 1 / 4 are exact
    out.append(("iou_equals_thr", torch.tensor([[0., 0., 2., 1.], [0., 0., 1., 1.], [0., 0., 4., 1.]]),
                torch.tensor([0.9, 0.8, 0.7]), 0.5))
    return out
