"""Reference for the device entry points of csrc/refine_stage.hip (ink_refine_*, ink_bitplane_pack), one function per
entry point, in plain numpy on UNPACKED arrays: bool [H, W] planes, uint8 label images, python ints.  Everything is
integer / bit work, so every comparison made with these is exact equality.

The operations themselves are the ones oracle/refine4_ref.py states (disk, sk_dilate, sk_erode, ...); what is added here
is the CONTRACT of each launch (which plane it reads, what the tables hold, raster order, caps) - and
tests/test_refine_stage_ref_cpu.py pins every function below to the oracle's function of the same step, so this file is
no truth of its own.  `wrong=` selects a deliberately wrong variant of a restatement; the CPU test shows that the chosen
inputs tell each of them apart from the right one.

Also here: the generators of the inputs tests/test_refine_stage_ops_gpu.py feeds to the kernels (the CPU test asserts
that they contain what they are meant to contain)."""
import numpy as np
from scipy import ndimage

from oracle import refine4_ref as O

INT_MAX = 0x7FFFFFFF
# one and two row-scan carries (H > 1024, > 2048), Wp = 65 (W > 4096), widths around the 64-pixel word
EDGE_SIZES = [(1, 1), (3, 63), (5, 64), (4, 65), (7, 129), (1030, 70), (2051, 3), (2, 4100)]
CROSS = ndimage.generate_binary_structure(2, 1)
SQUARE3 = np.ones((3, 3), bool)


# ---------------------------------------------------------------------------------------------------------------
# row-aligned little-endian bit planes
# ---------------------------------------------------------------------------------------------------------------
def pack(b: np.ndarray) -> np.ndarray:
    """bool [..., H, W] -> uint64 [..., H, ceil(W / 64)]: bit k of word w of a row = pixel 64 w + k, tail bits 0."""
    b = np.asarray(b, bool)
    W = b.shape[-1]
    p = np.zeros(b.shape[:-1] + (((W + 63) // 64) * 64,), np.uint8)
    p[..., :W] = b
    return np.ascontiguousarray(np.packbits(p, axis=-1, bitorder="little")).view("<u8")


def _bits(words: np.ndarray) -> np.ndarray:
    w = np.ascontiguousarray(np.asarray(words).view("<u8"))
    return np.unpackbits(w.view(np.uint8), axis=-1, bitorder="little")


def unpack(words: np.ndarray, W: int) -> np.ndarray:
    """uint64 / int64 [..., H, Wp] -> bool [..., H, W]."""
    return _bits(words)[..., :W].astype(bool)


def tail_is_clear(words: np.ndarray, W: int) -> bool:
    """No bit at a position >= W is set in any row."""
    return not _bits(words)[..., W:].any()


# ---------------------------------------------------------------------------------------------------------------
# the entry points
# ---------------------------------------------------------------------------------------------------------------
def sketch_planes(rgb: np.ndarray, wrong=None) -> np.ndarray:
    """ink_refine_sketch_planes: bool [4, H, W] = blue <= max(all bytes) / 2, PIL luma < 250, PIL luma <= 250,
    libpng gray < 250."""
    r, g, b = (rgb[..., i].astype(np.int64) for i in range(3))
    luma = (r * 19595 + g * 38470 + b * 7471 + 0x8000) >> 16
    gray = (r * 9798 + g * 19235 + b * 3735 + 16384) >> 15
    le = luma < 250 if wrong == "luma_lt_250" else luma <= 250
    return np.stack([2 * b <= int(rgb.max()), luma < 250, le, gray < 250])


def bitplane_pack(img: np.ndarray, thresh: int) -> np.ndarray:
    """ink_bitplane_pack: pixel > thresh."""
    return np.asarray(img).astype(np.int64) > thresh


def depth_samples(masks: np.ndarray, depth: np.ndarray, pts_yx: np.ndarray):
    """ink_refine_depth_samples: (vals [P] = depth at the points, bit for bit; inside bool [n, P])."""
    y, x = pts_yx[:, 0], pts_yx[:, 1]
    return depth[y, x], np.asarray(masks).reshape(-1, *depth.shape)[:, y, x]


def pair_tables(masks, planes: np.ndarray, rect: np.ndarray, wrong=None):
    """ink_refine_pair_tables: (dil bool [n, H, W], pair [n, n, 2], per [n, 3], sketch_area).
    dil[m] = cross dilation of mask m & plane 0; pair[i, j] = (|M_i & M_j|, |D_i & D_j| inside rows [y0, y1) x columns
    [x0, x1) of rect[i, j]), symmetric, rect[i, j] read for i <= j; per[i] = (|M_i|, |D_i|, |M_i & plane 1|);
    sketch_area = |plane 1|."""
    M = [np.asarray(m, bool) for m in masks]
    n = len(M)
    D = [O.sk_dilate(m & planes[0], CROSS) for m in M]
    pair, per = np.zeros((n, n, 2), np.int64), np.zeros((n, 3), np.int64)
    for i in range(n):
        per[i] = (M[i].sum(), D[i].sum(), (M[i] & planes[1]).sum())
        for j in range(i, n):
            y0, y1, x0, x1 = (int(v) for v in rect[i, j])
            if wrong == "inclusive_right":
                x1 += 1
            pair[i, j] = pair[j, i] = ((M[i] & M[j]).sum(), (D[i] & D[j])[y0:max(y1, y0), x0:max(x1, x0)].sum())
    return (np.stack(D) if n else np.zeros((0,) + planes.shape[1:], bool)), pair, per, int(planes[1].sum())


def composite(masks, order, shape):
    """ink_refine_composite: label = 1 + the first rank r with order[r] >= 0 whose mask covers the pixel;
    (label uint8 [H, W], bincount [256])."""
    label = np.zeros(shape, np.uint8)
    for r in range(len(order) - 1, -1, -1):
        if order[r] >= 0:
            label[np.asarray(masks[order[r]], bool)] = r + 1
    return label, np.bincount(label.ravel(), minlength=256)


def relabel_clean(label: np.ndarray, lut: np.ndarray, wrong=None) -> np.ndarray:
    """ink_refine_relabel_clean: L = lut[label]; a pixel with at most one 8-neighbour of its own L becomes 0."""
    L = np.asarray(lut, np.uint8)[label]
    H, W = L.shape
    p = np.pad(L.astype(np.int32), 1, constant_values=-1)
    cnt = np.zeros(L.shape, np.int32)
    for dy in range(3):
        for dx in range(3):
            if (dy, dx) != (1, 1):
                cnt += p[dy:dy + H, dx:dx + W] == L
    drop = cnt < 1 if wrong == "cnt_lt_1" else cnt <= 1
    return np.where(drop, 0, L).astype(np.uint8)


def same_label_neighbours(L: np.ndarray) -> np.ndarray:
    """8-neighbours carrying the pixel's own label (0 for unlabeled pixels)."""
    H, W = L.shape
    p = np.pad(L.astype(np.int32), 1, constant_values=-1)
    cnt = np.zeros(L.shape, np.int32)
    for dy in range(3):
        for dx in range(3):
            if (dy, dx) != (1, 1):
                cnt += p[dy:dy + H, dx:dx + W] == L
    return np.where(L > 0, cnt, 0)


def pixel_list(plane: np.ndarray, cap=None, wrong=None):
    """The raster-order list the growth returns, built the way the contract describes it: per-row counts, an exclusive
    scan over the rows in passes of 1024 with a carry, then every row writes its pixels at its offset, entries at or
    past `cap` dropped.  -> (full count, int32 [min(count, cap), 2] (y, x))."""
    H = plane.shape[0]
    counts = plane.sum(1).astype(np.int64)
    rowoff, carry = np.zeros(H, np.int64), 0
    for y0 in range(0, H, 1024):
        blk = counts[y0:y0 + 1024]
        base = 0 if wrong == "no_carry" else carry
        rowoff[y0:y0 + 1024] = base + np.cumsum(blk) - blk
        carry = base + int(blk.sum())
    yx = np.full((int(counts.sum()), 2), -1, np.int32)
    for y in np.nonzero(counts)[0]:
        xs = np.nonzero(plane[y])[0]
        yx[rowoff[y]:rowoff[y] + len(xs), 0] = y
        yx[rowoff[y]:rowoff[y] + len(xs), 1] = xs
    return carry, yx[:min(carry, carry if cap is None else cap)]


def grow(label: np.ndarray, planes: np.ndarray, cap=None, wrong=None) -> dict:
    """ink_refine_grow.  unlabeled = plane 2 & label == 0; its closing by disk(3); 4-connected components of more than
    50 pixels are `large`; flags[L] = a pixel of L lies within disk(3) of `large`; a labelled pixel keeps its label on
    plane 2 and loses it elsewhere; an unlabeled stroke pixel takes the LARGEST label with a pixel inside disk(3 if
    flags[L] else 2) around it.  bbox[L] = (xmin, ymin, xmax, ymax) of the grown label, (W, H, -1, -1) if absent;
    count / yx = the still unlabeled stroke pixels in raster order."""
    H, W = label.shape
    sk = planes[2]
    unl = sk & (label == 0)
    cc, _ = ndimage.label(O.sk_closing(unl, O.disk(3)))
    sizes = np.bincount(cc.ravel())
    big = sizes >= 50 if wrong == "ge_50" else sizes > 50
    big[0] = False
    near = O.sk_dilate(big[cc], O.disk(3))
    present = [int(l) for l in np.unique(label) if l]
    flags = np.zeros(256, np.int64)
    if wrong != "disk2_always":
        flags[np.unique(label[(label > 0) & near])] = 1
    out = np.where(sk, label, 0).astype(np.uint8)
    for L in (present[::-1] if wrong == "smallest_wins" else present):
        out[O.sk_dilate(label == L, O.disk(3 if flags[L] else 2)) & unl] = L
    bbox = np.tile(np.array([W, H, -1, -1], np.int64), (256, 1))
    for L in np.unique(out):
        if L:
            m = out == L
            ys, xs = np.nonzero(m.any(1))[0], np.nonzero(m.any(0))[0]
            bbox[L] = (xs[0], ys[0], xs[-1], ys[-1])
    count, yx = pixel_list(sk & (out == 0), cap)
    return {"grown": out, "flags": flags, "bbox": bbox, "count": count, "yx": yx, "closed_sizes": sizes[1:], "unl": unl}


def query_dists(label: np.ndarray, q_yx: np.ndarray) -> np.ndarray:
    """ink_refine_query_dists for EVERY label: int64 [Q, 256], the smallest squared distance from q to a pixel of the
    label, INT_MAX where the label has none (the kernel owes only the candidates' entries)."""
    d2 = np.full((len(q_yx), 256), INT_MAX, np.int64)
    qy, qx = q_yx[:, 0].astype(np.int64), q_yx[:, 1].astype(np.int64)
    for L in np.unique(label):
        if L:
            ys, xs = np.nonzero(label == L)
            d2[:, L] = ((qy[:, None] - ys[None]) ** 2 + (qx[:, None] - xs[None]) ** 2).min(1)
    return d2


def candidate_words(cands) -> np.ndarray:
    """list of label lists -> uint64 [Q, 4], the 256-bit sets."""
    out = np.zeros((len(cands), 4), np.uint64)
    for q, ls in enumerate(cands):
        for l in ls:
            out[q, l >> 6] |= np.uint64(1) << np.uint64(l & 63)
    return out


def finalize(label: np.ndarray, assign_yxl: np.ndarray, planes: np.ndarray, wrong=None):
    """ink_refine_finalize: the assignments written into the label image; plane 3 minus the labelled pixels, opened
    with the 3x3 square (erosion: outside = set, dilation: outside = clear), then every pixel also takes its upper,
    left and upper-left neighbour.  -> (label, extra bool [H, W], its pixel count)."""
    lab = label.copy()
    for y, x, l in np.asarray(assign_yxl).reshape(-1, 3):
        lab[y, x] = l
    un = planes[3] & (lab == 0)
    op = O.sk_dilate(O.sk_erode(un, SQUARE3), SQUARE3)
    d = op.copy()
    if wrong == "anchor_down_right":
        d[:-1, :] |= op[1:, :]
        d[:, :-1] |= op[:, 1:]
        d[:-1, :-1] |= op[1:, 1:]
    else:
        d[1:, :] |= op[:-1, :]
        d[:, 1:] |= op[:, :-1]
        d[1:, 1:] |= op[:-1, :-1]
    return lab, d, int(d.sum())


# ---------------------------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------------------------
def threshold_palette() -> np.ndarray:
    """RGB triples on both sides of every threshold of the sketch planes: PIL luma 249 / 250 / 251 and libpng gray 249 /
    250 / 251, blues 126 / 127 / 128 around half of an even and an odd maximum, and the two brightest triples for which
    the two grays disagree (247 against 248; over all 2^24 triples they never fall on different sides of 250)."""
    v = np.arange(225, 256)
    c = np.stack(np.meshgrid(v, v, v, indexing="ij"), -1).reshape(-1, 3).astype(np.uint8)
    luma, gray = O.pil_luma(c[None])[0], O.png_gray(c[None])[0]
    out = [[200, 200, 126], [200, 200, 127], [200, 200, 128], [0, 0, 0], [255, 255, 255], [255, 243, 251], [254, 242, 250]]
    for l in (249, 250, 251):
        for g in (249, 250, 251):
            sel = np.nonzero((luma == l) & (gray == g))[0]
            out += [c[k].tolist() for k in sel[[0, len(sel) // 2, -1]]] if len(sel) else []
    return np.array(out, np.uint8)


def random_rgb(H: int, W: int, seed: int, top: int = 255) -> np.ndarray:
    """A sketch of threshold triples, dark strokes and white paper; `top`: the largest byte, which occurs."""
    rs = np.random.RandomState(seed)
    pal = threshold_palette()
    rgb = pal[rs.randint(0, len(pal), (H, W))]
    dark = rs.rand(H, W) < 0.45
    rgb[dark] = rs.randint(0, 120, (int(dark.sum()), 3))
    rgb = np.minimum(rgb, top).astype(np.uint8)
    rgb[rs.randint(H), rs.randint(W), rs.randint(3)] = top
    return np.ascontiguousarray(rgb)


def random_planes(H: int, W: int, seed: int) -> np.ndarray:
    """Four sketch planes with blobs of stroke wide enough to survive an opening, and noise."""
    rs = np.random.RandomState(seed)
    base = ndimage.binary_dilation(rs.rand(H, W) < 0.08, structure=np.ones((3, 3), bool), iterations=1)
    return np.stack([base ^ (rs.rand(H, W) < 0.02 * (k + 1)) for k in range(4)])


def random_masks(n: int, H: int, W: int, seed: int) -> np.ndarray:
    """bool [n, H, W]: noisy rectangles that overlap each other."""
    rs = np.random.RandomState(seed)
    out = np.zeros((n, H, W), bool)
    for m in out:
        y0, x0 = rs.randint(0, H), rs.randint(0, W)
        y1, x1 = rs.randint(y0, H) + 1, rs.randint(x0, W) + 1
        if rs.rand() < 0.5:
            y0, x0 = 0, 0
        m[y0:y1, x0:x1] = rs.rand(y1 - y0, x1 - x0) < 0.8
    return out


def random_labels(H: int, W: int, seed: int, labels) -> np.ndarray:
    """uint8 label image: noisy rectangles of the given labels over a background of 0."""
    rs = np.random.RandomState(seed)
    out = np.zeros((H, W), np.uint8)
    for l in labels:
        y0, x0 = rs.randint(0, H), rs.randint(0, W)
        y1, x1 = min(H, y0 + rs.randint(1, 9)), min(W, x0 + rs.randint(1, 9))
        out[y0:y1, x0:x1] = np.where(rs.rand(y1 - y0, x1 - x0) < 0.85, l, out[y0:y1, x0:x1])
    return out


def random_rects(n: int, H: int, W: int, seed: int) -> np.ndarray:
    """int32 [n, n, 4] (y0, y1, x0, x1), symmetric, half open, inside the image."""
    rs = np.random.RandomState(seed)
    rect = np.zeros((n, n, 4), np.int32)
    for i in range(n):
        for j in range(i, n):
            y0, x0 = rs.randint(0, H), rs.randint(0, W)
            rect[i, j] = rect[j, i] = (y0, rs.randint(y0, H + 1), x0, rs.randint(x0, W + 1))
    return rect


PAIR_RECTS_HW = (10, 200)
PAIR_RECTS = [(0, 0, 0, 0), (0, 10, 0, 200), (3, 4, 77, 78), (1, 9, 70, 100), (0, 10, 60, 130), (2, 8, 63, 64),
              (2, 8, 64, 65), (2, 8, 65, 128), (0, 10, 63, 128), (1, 7, 0, 63), (0, 10, 64, 128), (0, 10, 128, 200),
              (4, 9, 63, 65), (0, 3, 128, 129), (5, 6, 0, 200)]


def pair_rects_case():
    """6 dense masks on a 10 x 200 sketch; the 15 pairs i < j take PAIR_RECTS in order, the diagonal random ones."""
    H, W = PAIR_RECTS_HW
    rs = np.random.RandomState(11)
    masks = rs.rand(6, H, W) < 0.7
    planes = rs.rand(4, H, W) < 0.8
    rect = random_rects(6, H, W, 12)
    k = 0
    for i in range(6):
        for j in range(i + 1, 6):
            rect[i, j] = rect[j, i] = PAIR_RECTS[k]
            k += 1
    return masks, planes, rect


def relabel_case():
    """(label [12, 70], a LUT that drops labels, a LUT that maps two labels onto one).  Isolated pixels, pairs and
    three-pixel lines of one label, inside and on the border, one line across x = 63 / 64, labels up to 254."""
    L = np.zeros((12, 70), np.uint8)
    L[5, 5] = L[0, 10] = 3                              # isolated: inside, on the top border
    L[0, 0] = L[11, 69] = 4                             # isolated in two corners
    L[5, 20:22] = 5                                     # pairs: inside, on the bottom border
    L[11, 30:32] = 5
    L[8, 40:43] = 6                                     # lines: inside, on the right border, across the word boundary
    L[3:6, 69] = 6
    L[2, 62:67] = 9
    L[0, 50:53] = 9                                     # a line on the top border
    L[5, 50] = 7                                        # 7 beside three pixels of 8: only a merging LUT joins them
    L[5, 51] = L[5, 52] = L[4, 51] = 8
    L[9, 10:13] = 254
    L[10, 10] = 200                                     # 200 under a line of 254
    L[7:10, 0] = 253                                    # a line on the left border
    L[9:12, 56:60] = 100                                # a block that survives whole
    drop = np.arange(256, dtype=np.uint8)
    drop[[3, 9, 200]] = 0
    drop[254] = 1
    merge = np.arange(256, dtype=np.uint8)
    merge[7] = merge[8] = 2
    merge[200] = merge[254] = 17
    return L, drop, merge


def grow_case():
    """(label [48, 200], planes [4, 48, 200]) with, all verified by the CPU test: an unlabeled 3 x 17 block (51 pixels:
    a large component) and a 5 x 10 one (50: not large), each across a word boundary; label 3 three columns left of
    the large block (flagged: grows by disk(3), reaching a pixel at distance^2 = 9), label 7 three columns left of the
    small one (not flagged: disk(2) does not reach it); a 3 x 3 block of stroke between labels 200 and 254 (the larger
    label wins); label 1 partly off the strokes (loses those pixels)."""
    H, W = 48, 200
    lab, sk = np.zeros((H, W), np.uint8), np.zeros((H, W), bool)
    sk[10:13, 60:77] = True                             # 51 unlabeled pixels, columns 60 .. 76
    lab[10:13, 53:58] = 3
    sk[30:35, 120:130] = True                           # 50 unlabeled pixels, columns 120 .. 129
    lab[30:35, 113:118] = 7
    sk[40:43, 23:26] = True
    lab[40:43, 20:23] = 200
    lab[40:43, 26:29] = 254
    lab[2:5, 2:7] = 1
    sk |= lab > 0
    sk[2:5, 5:7] = False
    sk[20, 150:190] = True                              # a long thin stroke nothing reaches: stays in the list
    sk[47, 0] = sk[0, 199] = True
    planes = np.stack([sk, sk, sk, sk])
    planes[[0, 1, 3]] ^= np.random.RandomState(5).rand(3, H, W) < 0.3        # the growth reads plane 2 alone
    return lab, planes


QUERY_HW = (40, 300)
QUERY_ABSENT = 100


def query_case():
    """(label [40, 300] holding every label 1 .. 254 but QUERY_ABSENT, q_yx int32 [300, 2], candidate lists).
    Query 0 has candidates in all four 64-bit words, among them the absent label and label 250, whose nearest pixel is
    five rows below it while its own row holds a far one; query 1 has no candidates."""
    H, W = QUERY_HW
    rs = np.random.RandomState(21)
    lab = np.zeros((H, W), np.uint8)
    for l in range(1, 255):
        if l in (QUERY_ABSENT, 250):
            continue
        for _ in range(rs.randint(1, 4)):
            lab[rs.randint(H), rs.randint(W)] = l
    lab[20, 140:161] = 0
    lab[25, 150] = lab[20, 290] = 250
    present = set(np.unique(lab).tolist())
    for l in range(1, 255):                              # a later label may have overwritten an earlier one's only pixel
        if l != QUERY_ABSENT and l not in present:
            y, x = np.argwhere(lab == 0)[rs.randint(1000)]
            lab[y, x] = l
    q = np.stack([rs.randint(0, H, 300), rs.randint(0, W, 300)], 1).astype(np.int32)
    q[0] = (20, 150)
    q[2], q[3], q[4], q[5] = (0, 0), (H - 1, W - 1), (0, W - 1), (H - 1, 0)
    cands = [sorted(set(rs.randint(1, 255, rs.randint(1, 7)).tolist())) for _ in range(300)]
    cands[0] = [5, 70, QUERY_ABSENT, 150, 250, 254]
    cands[1] = []
    cands[2] = [1, 63, 64, 127, 128, 191, 192, 254]
    return lab, q, cands


def dark_sketch(H: int = 300, W: int = 300) -> np.ndarray:
    """A sketch that is stroke everywhere: H * W > 65536 unlabeled stroke pixels, more than the growth's first cap."""
    rgb = np.full((H, W, 3), 20, np.uint8)
    rgb[..., 2] = 0
    return rgb


def small_masks(n: int, H: int, W: int, seed: int) -> np.ndarray:
    """bool [n, H, W]: small noisy patches that overlap now and then, so that late ranks of a composite keep pixels."""
    rs = np.random.RandomState(seed)
    out = np.zeros((n, H, W), bool)
    for m in out:
        y0, x0 = rs.randint(0, H), rs.randint(0, W)
        y1, x1 = min(H, y0 + rs.randint(1, 12)), min(W, x0 + rs.randint(1, 12))
        m[y0:y1, x0:x1] = rs.rand(y1 - y0, x1 - x0) < 0.8
    return out


def finalize_case():
    """(label [12, 130], planes [4, 12, 130]): unclaimed strokes on plane 3 whose opening touches the corner (0, 0), the
    bottom border and ends at x = 63, so that the 2 x 2 dilation carries a bit from word 0 into word 1; a 2-wide stroke
    the opening removes; a block under a label."""
    H, W = 12, 130
    p3 = np.zeros((H, W), bool)
    p3[0:3, 0:3] = True
    p3[4:8, 60:64] = True
    p3[9:12, 100:110] = True
    p3[5:7, 20:40] = True                              # two rows only: opened away
    p3[0:4, 124:130] = True                            # the top right corner
    p3[3:9, 80:90] = True
    lab = np.zeros((H, W), np.uint8)
    lab[3:9, 84:90] = 2                                # claimed: not part of the extra mask
    rs = np.random.RandomState(9)
    planes = np.stack([rs.rand(H, W) < 0.5, rs.rand(H, W) < 0.5, rs.rand(H, W) < 0.5, p3])
    return lab, planes
