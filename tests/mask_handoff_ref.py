"""Independent statement of the mask hand-off kernels of csrc/refine.hip (TEST INFRASTRUCTURE ONLY) with every
parameter explicit, and the inputs tests/test_mask_handoff_ops_gpu.py feeds them.

  cleanup(mask_u8, k, area_threshold, aspect_threshold)   = ink_mask_cleanup for one mask: threshold > 127, k x k closing
      (clipped-window counts; no scipy morphology, so that it can be pinned AGAINST scipy), 8-connected components,
      keep iff area > area_threshold or (aspect_threshold > 0 and max(w, h) / (min(w, h) + 1e-5) > aspect_threshold).
  sketch_iou_counts(masks_u8, rgb_u8)                     = ink_mask_sketch_iou_counts: r_i = (mask_i != 0) & (Pillow luma
      < 250); counts[i, j] = (|r_i & r_j|, |r_i | r_j|).

Both take `wrong=<name>` (MISTAKES_CLEANUP / MISTAKES_COUNTS): the classic mistakes, planted on purpose, so that
tests/test_mask_handoff_ref_cpu.py can show that the case lists below tell each of them from the right answer.

Everything is exact (bytes, integer counts).  The cases are built on demand by name (CLEANUP_CASES holds the builders;
count_sketch / count_masks make the count inputs per shape), so that importing this module costs nothing."""
from __future__ import annotations

from typing import Callable, Dict, NamedTuple, Optional, Tuple

import numpy as np

MISTAKES_CLEANUP = ("conn4", "area_ge", "aspect_no_eps", "aspect_min_max_swapped", "threshold_ge_127",
                    "erode_outside_is_background", "open_not_close", "close_r_plus_1", "horizontal_only")
MISTAKES_COUNTS = ("luma_le_250", "luma_truncated", "mask_gt_127", "union_without_strokes")


def run_bound(W: int, k: int) -> int:
    """The per-row run bound that sizes the components workspace of ink_mask_cleanup (refine.hip, cleanup_rm)."""
    return W // ((k + 1) // 2 + 1) + 2


# ---------------------------------------------------------------------------------------------------------------
# cleanup
# ---------------------------------------------------------------------------------------------------------------
def _window_counts(b: np.ndarray, r: int, axis: int) -> Tuple[np.ndarray, np.ndarray]:
    """Along `axis` of a 2-D bool image: the number of set pixels in [x - r, x + r] clipped to the image, and the
    number of pixels of that clipped window."""
    a = np.moveaxis(b, axis, -1)
    L = a.shape[-1]
    pre = np.zeros(a.shape[:-1] + (L + 1,), np.int64)
    pre[..., 1:] = np.cumsum(a, axis=-1)
    x = np.arange(L)
    lo, hi = np.maximum(x - r, 0), np.minimum(x + r, L - 1)
    return np.moveaxis(pre[..., hi + 1] - pre[..., lo], -1, axis), np.moveaxis(np.broadcast_to(hi - lo + 1, a.shape), -1, axis)


def dilate(b: np.ndarray, r: int, axes=(1, 0)) -> np.ndarray:
    """Box dilation by +-r per axis; pixels outside the image never win (cv2's default morphology border)."""
    for ax in axes:
        b = _window_counts(b, r, ax)[0] > 0
    return b


def erode(b: np.ndarray, r: int, axes=(1, 0), outside_is_background: bool = False) -> np.ndarray:
    """Box erosion by +-r per axis; pixels outside the image never lose (they count as foreground)."""
    for ax in axes:
        cnt, size = _window_counts(b, r, ax)
        b = cnt == (2 * r + 1 if outside_is_background else size)
    return b


def close(b: np.ndarray, k: int, wrong: Optional[str] = None) -> np.ndarray:
    """cv2.morphologyEx(MORPH_CLOSE, k x k rectangle, default border) of a 2-D bool image, k odd."""
    assert k >= 1 and k % 2 == 1 and b.ndim == 2 and b.dtype == bool
    r = k // 2 + (1 if wrong == "close_r_plus_1" else 0)
    axes = (1,) if wrong == "horizontal_only" else (1, 0)
    if wrong == "open_not_close":
        return dilate(erode(b, r, axes), r, axes)
    return erode(dilate(b, r, axes), r, axes, outside_is_background=wrong == "erode_outside_is_background")


def keep_rule(area, bw, bh, area_threshold, aspect_threshold, wrong: Optional[str] = None) -> np.ndarray:
    """area > thr, or (aspect_threshold > 0 and max(w, h) / (min(w, h) + 1e-5) > aspect_threshold), in float64.
    aspect_threshold <= 0 switches the aspect rule off; area_threshold = -1 keeps every component (area >= 1)."""
    area, bw, bh = (np.asarray(v, np.int64) for v in (area, bw, bh))
    keep = area >= area_threshold if wrong == "area_ge" else area > area_threshold
    if aspect_threshold > 0:
        big, small = np.maximum(bw, bh).astype(np.float64), np.minimum(bw, bh).astype(np.float64)
        if wrong == "aspect_min_max_swapped":
            big, small = small, big
        keep = keep | (big / (small + (0.0 if wrong == "aspect_no_eps" else 1e-5)) > float(aspect_threshold))
    return keep


def components(b: np.ndarray, conn8: bool = True):
    """labels (0 = background), area[n + 1], bbox width[n + 1], bbox height[n + 1] (entry 0 unused)."""
    from scipy import ndimage
    labels, n = ndimage.label(b, structure=np.ones((3, 3), bool) if conn8 else None)
    area = np.bincount(labels.ravel(), minlength=n + 1)
    bw, bh = np.ones(n + 1, np.int64), np.ones(n + 1, np.int64)
    for i, sl in enumerate(ndimage.find_objects(labels), start=1):
        bh[i], bw[i] = sl[0].stop - sl[0].start, sl[1].stop - sl[1].start
    return labels, area, bw, bh


def cleanup(mask_u8: np.ndarray, k: int, area_threshold: int = 500, aspect_threshold: float = 1.1,
            wrong: Optional[str] = None) -> np.ndarray:
    """uint8 [H, W] or [n, H, W] -> uint8 0 / 255 of the same shape."""
    assert mask_u8.dtype == np.uint8 and wrong in (None,) + MISTAKES_CLEANUP
    if mask_u8.ndim == 3:
        return np.stack([cleanup(m, k, area_threshold, aspect_threshold, wrong) for m in mask_u8])
    b = mask_u8 >= 127 if wrong == "threshold_ge_127" else mask_u8 > 127
    labels, area, bw, bh = components(close(b, k, wrong), conn8=wrong != "conn4")
    keep = keep_rule(area, bw, bh, area_threshold, aspect_threshold, wrong)
    keep[0] = False
    return np.where(keep[labels], 255, 0).astype(np.uint8)


def max_runs_per_row(b: np.ndarray) -> int:
    """The largest number of horizontal runs of set pixels in a row of a 2-D bool image."""
    starts = b.copy()
    starts[:, 1:] &= ~b[:, :-1]
    return int(starts.sum(1).max()) if b.size else 0


# ---------------------------------------------------------------------------------------------------------------
# sketch IoU counts
# ---------------------------------------------------------------------------------------------------------------
def pil_luma(rgb: np.ndarray, truncated: bool = False) -> np.ndarray:
    """Pillow's Image.convert("L"): (19595 r + 38470 g + 7471 b + 0x8000) >> 16."""
    r, g, b = (rgb[..., i].astype(np.int64) for i in range(3))
    return (r * 19595 + g * 38470 + b * 7471 + (0 if truncated else 0x8000)) >> 16


def sketch_iou_counts(masks_u8: np.ndarray, rgb_u8: np.ndarray, wrong: Optional[str] = None) -> np.ndarray:
    assert masks_u8.dtype == np.uint8 and rgb_u8.dtype == np.uint8 and wrong in (None,) + MISTAKES_COUNTS
    assert masks_u8.ndim == 3 and rgb_u8.shape == masks_u8.shape[1:] + (3,)
    luma = pil_luma(rgb_u8, truncated=wrong == "luma_truncated")
    strokes = luma <= 250 if wrong == "luma_le_250" else luma < 250
    on = masks_u8 > 127 if wrong == "mask_gt_127" else masks_u8 != 0
    n = len(masks_u8)
    out = np.zeros((n, n, 2), np.int64)
    for i in range(n):
        for j in range(n):
            out[i, j, 0] = np.count_nonzero(on[i] & on[j] & strokes)
            union = on[i] | on[j]
            out[i, j, 1] = np.count_nonzero(union if wrong == "union_without_strokes" else union & strokes)
    return out


# ---------------------------------------------------------------------------------------------------------------
# cleanup cases
# ---------------------------------------------------------------------------------------------------------------
class Case(NamedTuple):
    masks: np.ndarray            # uint8 [n, H, W]
    k: int
    area_threshold: int
    aspect_threshold: float


CLOSE_SHAPES = [(1, 8), (5, 9), (33, 64), (40, 65), (127, 71), (128, 128), (129, 130), (130, 257)]
CLOSE_KS = [1, 3, 5, 11, 31]                 # r = 0, 1, 2, 5, 15: r >= H at (1, 8), (5, 9); r >= W at k = 31 and W <= 9
CLOSE_DENSITIES = [0.02, 0.3, 0.9]
GAP_KS = [3, 5, 9]
MASK_BYTES = np.array([0, 1, 127, 128, 255], np.uint8)
CLOSE_ONLY = dict(area_threshold=-1, aspect_threshold=1.1)     # every component is kept: the output is the closed image


def _u8(b) -> np.ndarray:
    return np.asarray(b, bool).astype(np.uint8) * 255


def noise_masks(H: int, W: int, k: int) -> np.ndarray:
    """One mask per density of CLOSE_DENSITIES."""
    rs = np.random.RandomState(1000 * H + 10 * W + k)
    return np.stack([_u8(rs.rand(H, W) < d) for d in CLOSE_DENSITIES])


def edge_masks(H: int, W: int, k: int) -> np.ndarray:
    """An empty mask, a full one, and noise in the five byte levels around the threshold (0, 1, 127, 128, 255)."""
    rs = np.random.RandomState(77 + 1000 * H + 10 * W + k)
    return np.stack([np.zeros((H, W), np.uint8), np.full((H, W), 255, np.uint8), MASK_BYTES[rs.randint(0, 5, (H, W))]])


def gap_line(k: int) -> np.ndarray:
    """A 1-D pattern with the four gap widths cv2's border rule makes special, r = k / 2: a gap of r against the left
    border (closes), an interior gap of 2 r (closes), an interior gap of 2 r + 1 (stays open), a gap of r + 1 against
    the right border (stays open).  The runs between them are 3 pixels long."""
    r = k // 2
    parts = [(0, r), (1, 3), (0, 2 * r), (1, 3), (0, 2 * r + 1), (1, 3), (0, r + 1)]
    return np.concatenate([np.full(n, v, bool) for v, n in parts])


def gap_line_closed(k: int) -> np.ndarray:
    """What the closing makes of gap_line(k), stated by hand."""
    r = k // 2
    parts = [(1, r + 3 + 2 * r + 3), (0, 2 * r + 1), (1, 3), (0, r + 1)]
    return np.concatenate([np.full(n, v, bool) for v, n in parts])


def gap_masks(k: int) -> np.ndarray:
    """gap_line(k) and its mirror image along x (rows constant), along y, and along both axes (outer product)."""
    p = gap_line(k)
    L = len(p)
    ms = []
    for q in (p, p[::-1]):
        ms += [np.broadcast_to(q[None, :], (L, L)), np.broadcast_to(q[:, None], (L, L)), np.outer(q, q[::-1])]
    return np.stack([_u8(m) for m in ms])


def seam_pixel_masks() -> np.ndarray:
    """Single pixels at rows 127 and 128 of a 129-row image: the windows of the rows around them straddle the 128-row
    segment seam of the vertical passes (k = 5: r = 2)."""
    H, W = 129, 71
    ms = []
    for y in (127, 128):
        m = np.zeros((H, W), bool)
        m[y, [0, 35, 70]] = True
        ms.append(m)
    both = np.zeros((H, W), bool)
    both[127, 10] = both[128, 13] = True                          # close enough to merge under the dilation
    both[123, 40] = both[128, 40] = True                          # a vertical gap of 2 r = 4 across the seam: closes
    both[122, 60] = both[128, 60] = True                          # a gap of 2 r + 1: stays open
    return np.stack([_u8(m) for m in ms + [both]])


def corner_masks(H: int, W: int) -> np.ndarray:
    ms = []
    for ys, xs in (([0], [0]), ([0], [W - 1]), ([H - 1], [0]), ([H - 1], [W - 1]), ([0, 0, H - 1, H - 1], [0, W - 1, 0, W - 1])):
        m = np.zeros((H, W), bool)
        m[ys, xs] = True
        ms.append(m)
    return np.stack([_u8(m) for m in ms])


# --- keep rule -------------------------------------------------------------------------------------------------
KEEP_HW = (96, 128)
# name -> (top, left, height, width, pixels removed from the inside); every block is at least 2 pixels from the next
KEEP_BLOCKS = {
    "22x23": (0, 0, 22, 23, 0),                 # area 506: kept by the area rule; touches the top and the left border
    "22x23-5": (0, 105, 22, 23, 5),             # area 501: kept; touches the top and the right border
    "22x23-6": (74, 0, 22, 23, 6),              # area 500: dropped (aspect 23 / 22.00001 < 1.1); bottom and left border
    "20x22": (76, 106, 20, 22, 0),              # area 440, aspect 22 / 20.00001 < 1.1: dropped; bottom and right border
    "22x20": (30, 108, 22, 20, 0),              # the same on its side; right border
    "10x11": (0, 40, 10, 11, 0),                # aspect 11 / 10.00001 < 1.1: dropped; top border
    "11x10": (40, 0, 11, 10, 0),                # left border
    "10x12": (86, 40, 10, 12, 0),               # aspect 1.2: kept; bottom border
    "12x10": (30, 40, 12, 10, 0),
    "1x1": (50, 60, 1, 1, 0),                   # dropped
    "1x2": (50, 70, 1, 2, 0),                   # aspect 2 / 1.00001: kept at 1.1, dropped at 2.0 and at 1.99999
    "2x1": (60, 60, 2, 1, 0),
    "1x1 corner": (95, 80, 1, 1, 0),
}
HOLES = [(5, 5), (5, 9), (9, 5), (9, 9), (13, 13), (16, 17)]    # inside a 22 x 23 block, never on its bounding box
# aspect_threshold = 1.99999: the one setting where the 1e-5 decides (2 / 1.00001 = 1.99998 < 1.99999 < 2 / 1); at 1.1
# it never can: max / min > 1.1 needs max >= 1.1 min + 0.1, far more than the 1.1e-5 the term moves the bound by
KEEP_PARAMS = {"default": (500, 1.1), "aspect_0": (500, 0.0), "aspect_2": (500, 2.0), "area_0": (0, 1.1),
               "area_1e9": (10 ** 9, 1.1), "aspect_1.99999": (500, 1.99999)}


def keep_block(name: str) -> np.ndarray:
    top, left, h, w, holes = KEEP_BLOCKS[name]
    m = np.zeros(KEEP_HW, bool)
    m[top:top + h, left:left + w] = True
    for dy, dx in HOLES[:holes]:
        m[top + dy, left + dx] = False
    return m


def keep_mask() -> np.ndarray:
    return np.any([keep_block(b) for b in KEEP_BLOCKS], axis=0)


# --- labelling -------------------------------------------------------------------------------------------------
def staircase() -> Tuple[np.ndarray, int]:
    """Two components of 70 pixels, each three vertical bars that meet only diagonally at the rows 31/32 and 63/64
    (one stepping right, one stepping left) -> (mask, area threshold that keeps only a fully merged component)."""
    m = np.zeros((70, 64), bool)
    for x0, step in ((10, 1), (40, -1)):
        m[0:32, x0] = m[32:64, x0 + step] = m[64:70, x0 + 2 * step] = True
    return m, 69


def comb(H: int) -> Tuple[np.ndarray, int]:
    """Teeth in every second column that meet only in the last row."""
    m = np.zeros((H, 41), bool)
    m[:, ::2] = True
    m[H - 1, :] = True
    return m, int(m.sum()) - 1


def checkerboard() -> Tuple[np.ndarray, int]:
    """(66, 130): 65 runs per row, one component under 8-connectivity, none of more than one pixel under 4."""
    y, x = np.mgrid[0:66, 0:130]
    m = (y + x) % 2 == 0
    return m, int(m.sum()) - 1


def stripes257() -> np.ndarray:
    """(34, 257), vertical stripes of period 2: 129 runs per row (the bound is 130), 129 components of 34 pixels."""
    m = np.zeros((34, 257), bool)
    m[:, ::2] = True
    return m


def spiral() -> Tuple[np.ndarray, int]:
    """A one-pixel-wide square spiral with one clear pixel between its turns: one component, through a long chain of
    unions that crosses the row-block seams many times."""
    H, W = 41, 45
    m = np.zeros((H, W), bool)
    y, x, dy, dx = 0, 0, 0, 1
    m[0, 0] = True
    while True:
        moved = False
        while True:                                   # straight on until the border or one pixel before an older turn
            ny, nx, ay, ax = y + dy, x + dx, y + 2 * dy, x + 2 * dx
            if not (0 <= ny < H and 0 <= nx < W) or m[ny, nx] or (0 <= ay < H and 0 <= ax < W and m[ay, ax]):
                break
            y, x, moved = ny, nx, True
            m[y, x] = True
        if not moved:
            return m, int(m.sum()) - 1
        dy, dx = dx, -dy                              # turn right


# --- wide and tall ---------------------------------------------------------------------------------------------
def wide_masks() -> np.ndarray:
    """(6, 4161): 66 words per row.  Stripes of period 2 (2081 runs per row, the bound is 2082); the same with runs
    that cross x = 4095/4096 (the words 63/64, the carry of the second pass of the run kernel); both phases mixed."""
    H, W = 6, 4161
    a = np.zeros((H, W), bool)
    a[:, ::2] = True
    b = np.zeros((H, W), bool)
    b[:, 1::2] = True
    b[1, 4095:4097] = b[2, 4090:4100] = b[4, 4032:4161] = True
    b[5, 4096] = True
    c = np.zeros((H, W), bool)
    c[0::3, ::2] = c[1::3, 1::2] = True                   # two-row checkerboard bands; rows 2 and 5 stay clear
    c[3, 4094:4098] = True
    return np.stack([_u8(a), _u8(b), _u8(c)])


def long_row_masks() -> np.ndarray:
    """(3, 16383), for k = 3: noise, stripes of period k + 1 = 4 (the gaps of 3 stay open: 4096 runs per row), stripes
    of period (k + 1) / 2 + 1 = 3 (the gaps of 2 close: one run)."""
    H, W = 3, 16383
    rs = np.random.RandomState(16383)
    s4, s3 = np.zeros((H, W), bool), np.zeros((H, W), bool)
    s4[:, 1::4] = True
    s3[:, ::3] = True
    return np.stack([_u8(rs.rand(H, W) < 0.3), _u8(s4), _u8(s3)])


def tall_masks() -> np.ndarray:
    """(16383, 8), for k = 3: noise at two densities and a full-height line with isolated pixels beside it."""
    H, W = 16383, 8
    rs = np.random.RandomState(8)
    line = np.zeros((H, W), bool)
    line[:, 1] = True
    line[::7, 6] = True
    return np.stack([_u8(rs.rand(H, W) < 0.3), _u8(rs.rand(H, W) < 0.05), _u8(line)])


def _build_cleanup_cases() -> Dict[str, Callable[[], Case]]:
    c: Dict[str, Callable[[], Case]] = {}
    for H, W in CLOSE_SHAPES:
        for k in CLOSE_KS:
            c[f"close noise {H}x{W} k={k}"] = lambda H=H, W=W, k=k: Case(noise_masks(H, W, k), k, **CLOSE_ONLY)
            c[f"close edge {H}x{W} k={k}"] = lambda H=H, W=W, k=k: Case(edge_masks(H, W, k), k, **CLOSE_ONLY)
    for k in GAP_KS:
        c[f"close gaps k={k}"] = lambda k=k: Case(gap_masks(k), k, **CLOSE_ONLY)
    c["close seam pixels k=5"] = lambda: Case(seam_pixel_masks(), 5, **CLOSE_ONLY)
    for H, W in ((33, 64), (129, 130)):
        for k in (5, 11):
            c[f"close corners {H}x{W} k={k}"] = lambda H=H, W=W, k=k: Case(corner_masks(H, W), k, **CLOSE_ONLY)
    for name, (area, aspect) in KEEP_PARAMS.items():
        c[f"keep {name}"] = lambda area=area, aspect=aspect: Case(_u8(keep_mask())[None], 1, area, aspect)
    c["label staircase"] = lambda: Case(_u8(staircase()[0])[None], 1, staircase()[1], 0.0)
    for H in (33, 65):
        c[f"label comb H={H}"] = lambda H=H: Case(_u8(comb(H)[0])[None], 1, comb(H)[1], 0.0)
    c["label checkerboard"] = lambda: Case(_u8(checkerboard()[0])[None], 1, checkerboard()[1], 0.0)
    c["label stripes257 whole"] = lambda: Case(_u8(stripes257())[None], 1, 33, 0.0)      # 34 > 33: every stripe is kept
    c["label stripes257 merged"] = lambda: Case(_u8(stripes257())[None], 1, 34, 0.0)     # kept only if two were merged
    c["label spiral"] = lambda: Case(_u8(spiral()[0])[None], 1, spiral()[1], 0.0)
    c["wide 6x4161 k=1 all"] = lambda: Case(wide_masks(), 1, **CLOSE_ONLY)
    c["wide 6x4161 k=1 area 6"] = lambda: Case(wide_masks(), 1, 6, 0.0)                  # a lone stripe has 6 pixels
    c["wide 3x16383 k=3"] = lambda: Case(long_row_masks(), 3, **CLOSE_ONLY)
    c["tall 16383x8 k=3"] = lambda: Case(tall_masks(), 3, 500, 1.1)
    return c


CLEANUP_CASES = _build_cleanup_cases()
SMALL_CLEANUP_CASES = [n for n in CLEANUP_CASES if not n.startswith(("wide", "tall"))]


def cleanup_case(name: str) -> Case:
    return CLEANUP_CASES[name]()


def cleanup_want(case: Case, wrong: Optional[str] = None) -> np.ndarray:
    return cleanup(case.masks, case.k, case.area_threshold, case.aspect_threshold, wrong)


# ---------------------------------------------------------------------------------------------------------------
# sketch IoU count cases
# ---------------------------------------------------------------------------------------------------------------
COUNT_NS = [1, 2, 5, 33]
# (H, W): 1, 1, 1, 2, 256, 256, 256 words of 64 pixels, and 257 words of which the last holds one pixel
COUNT_SHAPES = [(1, 1), (1, 63), (1, 64), (5, 13), (128, 128), (127, 129), (129, 127), (1, 16385)]
TRUNCATION_COLOUR = (237, 255, 254)            # Pillow luma 250 (no stroke); 249 if the luma is truncated


def sketch_palette() -> np.ndarray:
    """uint8 [P, 3]: found by searching pil_luma: four colours each of luma exactly 249, 250 and 251 that are no greys,
    the greys 249 and 250, TRUNCATION_COLOUR, white, black and a mid grey.  The first two have luma 249 and 250."""
    found = {249: [], 250: [], 251: []}
    for r in range(255, 199, -5):
        for g in range(255, 229, -1):
            for b in range(255, 149, -7):
                l = int(pil_luma(np.array([r, g, b], np.uint8)))
                if l in found and len(found[l]) < 4 and not r == g == b:
                    found[l].append((r, g, b))
    assert all(len(v) == 4 for v in found.values())
    cols = [found[249][0], found[250][0]] + found[249][1:] + found[250][1:] + found[251]
    cols += [(249, 249, 249), (250, 250, 250), TRUNCATION_COLOUR, (255, 255, 255), (0, 0, 0), (128, 128, 128)]
    return np.array(cols, np.uint8)


def count_sketch(H: int, W: int, rot: int = 0) -> np.ndarray:
    """uint8 [H, W, 3] drawn from the palette; its first pixels walk through the palette (from entry `rot`) so that a
    tiny image still holds the threshold colours."""
    pal = np.roll(sketch_palette(), -rot, axis=0)
    rs = np.random.RandomState(H * 131 + W)
    idx = rs.randint(0, len(pal), H * W)
    m = min(len(pal), H * W)
    idx[:m] = np.arange(m)
    return pal[idx].reshape(H, W, 3)


def count_masks(n: int, H: int, W: int) -> np.ndarray:
    """uint8 [n, H, W] drawn from MASK_BYTES; the last pixel of the image is set in mask 0 (the lone bit of a tail word)."""
    rs = np.random.RandomState(n * 7919 + H * 131 + W)
    m = MASK_BYTES[rs.randint(0, 5, (n, H, W))]
    m[0, H - 1, W - 1] = 1
    return m


# ---------------------------------------------------------------------------------------------------------------
# end to end: one small sketch NMS
# ---------------------------------------------------------------------------------------------------------------
NMS_HW = (96, 120)
NMS_THRESHOLDS = (0.05, 0.2, 0.5)


def nms_case():
    """rgb uint8 [96, 120, 3], raw masks uint8 [6, 96, 120], boxes [7, 4] (normalised), scores [7].  Box 2 covers the
    whole page: filter_full_or_empty_bbox drops it, so from there on the filtered index (which also selects the mask,
    the reference's quirk) is the original index minus one."""
    H, W = NMS_HW
    rs = np.random.RandomState(96120)
    rgb = np.full((H, W, 3), 255, np.uint8)
    rgb[rs.rand(H, W) < 0.35] = (20, 20, 20)
    boxes = np.array([[0.1, 0.1, 0.6, 0.6], [0.1, 0.1, 0.35, 0.4], [0.0, 0.0, 1.0, 1.0], [0.1, 0.1, 0.6, 0.58],
                      [0.5, 0.5, 0.9, 0.9], [0.7, 0.1, 0.9, 0.3], [0.52, 0.5, 0.9, 0.88]])
    scores = np.array([0.61, 0.83, 0.95, 0.42, 0.77, 0.30, 0.55])
    masks = np.zeros((6, H, W), np.uint8)
    for i in range(6):                                           # mask i belongs to the FILTERED box i
        x0, y0, x1, y1 = boxes[i if i < 2 else i + 1] * np.array([W, H, W, H])
        masks[i, int(y0):int(y1), int(x0):int(x1)] = 255
        masks[i][rs.rand(H, W) < 0.1] ^= 255
    return rgb, masks, boxes, scores
