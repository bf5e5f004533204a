"""Synthetic inputs for the layer-assembly tests (tests/test_layers_ref_cpu.py, tests/test_layers_gpu.py): the rules
the reference's committed outputs do not separate, each on the two shapes the kernels are tested at.  70 x 130 and
130 x 70: two plane words per row with a ragged tail / one ragged word, more rows than one 32-row band, a chamfer
tile edge inside the image in one direction only.  Below them, the inputs of the edge suite (EDGE_SHAPES onwards)."""
import numpy as np
from scipy import ndimage

import layers_ref as R

SHAPES = [(70, 130), (130, 70)]


def _blank(shape):
    return np.zeros(shape, bool)


def holes_image(shape):
    """Foreground slab with holes: A 6x7 = 42 pixels, contour area 7x8 - 2 = 54 (filled by the rule although its pixel
    count is below 50); B 5x6 = 30 pixels, contour area 40 (stays); C large but one pixel from the image edge
    (stays); D a 1-pixel ring hole of 24 pixels around a 5x5 island, contour area 62 (filled, island included: the
    component pass leaves it undecided); E a large hole holding an island that holds a small hole (all filled)."""
    H, W = shape
    a = _blank(shape)
    a[2:H - 2, 0:W - 2] = True
    t = (H >= W)                                         # transpose the layout on the tall shape

    def cut(y0, y1, x0, x1, v=False):
        if t:
            a[x0:x1, y0:y1] = v
        else:
            a[y0:y1, x0:x1] = v
    cut(5, 11, 5, 12)                                    # A
    cut(5, 10, 16, 22)                                   # B
    a[(90 if t else 20):(110 if t else 40), 1:9] = False   # C: one pixel from x = 0 on either shape
    cut(14, 21, 26, 33)                                  # D ring ...
    cut(15, 20, 27, 32, True)                            # ... around its island
    cut(26, 60, 40, 64)                                  # E
    cut(32, 54, 45, 60, True)                            # island in E
    cut(36, 40, 48, 52)                                  # small hole in the island
    return a


def two_components(shape):
    """A 1-pixel-wide line of 60 pixels (contour area 0) and a 7x7 block of 49 pixels (contour area 36): the pixel count
    ranks the line first, the contour area the block.  A 1-pixel spur on the block adds only the two half cells where it joins."""
    H, W = shape
    a = _blank(shape)
    if W >= H:
        a[5, 5:65] = True
    else:
        a[5:65, 5] = True
    a[20:27, 20:27] = True
    a[23, 27:33] = True                                  # the spur
    return a


def equal_components(shape):
    """Two 5x5 blocks of equal contour area: the one met last in raster order is kept."""
    a = _blank(shape)
    a[4:9, 4:9] = True
    a[40:45, 30:35] = True
    return a


def diagonal_gap(shape):
    """Pixel (0, 0) walled in by an anti-diagonal line with 1-pixel diagonal steps: the 4-connected flood from the
    corner stays inside, an 8-connected one would leak through the steps."""
    a = _blank(shape)
    for k in range(12):
        a[11 - k, k] = True
    a[30:40, 30:40] = True
    return a


def blob(shape):
    """One blob wider than a 64-pixel chamfer tile plus its 16-pixel halo, with a notch and a few zero pixels inside."""
    H, W = shape
    a = _blank(shape)
    a[3:H - 3, 4:W - 4] = True
    a[H // 2 - 2:H // 2 + 2, 0:W // 3] = False
    a[H // 3, 2 * W // 3] = False
    return a


def blob_strokes(shape):
    H, W = shape
    s = _blank(shape)
    s[H // 2 + 9:H // 2 + 11, W // 2 - 20:W // 2 + 20] = True
    s[H // 4:H // 4 + 12, W // 2] = True
    return s


def closed_sketch(shape):
    """Grey sketch (dark strokes on white) of a closed ring well inside the image, with a second, smaller ring."""
    H, W = shape
    g = np.full(shape, 255, np.uint8)
    g[20:H - 20, 20] = g[20:H - 20, W - 21] = 30
    g[20, 20:W - 20] = g[H - 21, 20:W - 20] = 30
    g[28:34, 28:34] = 90
    g[30:32, 30:32] = 255
    return g


def open_sketch(shape):
    """Grey sketch whose strokes (three sides of a frame) come close to the image edge (open-curve branch), with two
    rings inside: after the 1-step dilation their holes are 8 x 8 (contour area 79) and 5 x 5 (contour area 34)."""
    H, W = shape
    g = np.full(shape, 255, np.uint8)
    g[6:H - 6, 6] = g[6:H - 6, W - 7] = 10
    g[6, 6:W - 6] = 10
    g[20:32, 20] = g[20:32, 31] = 60                      # ring with a 10 x 10 interior
    g[20, 20:32] = g[31, 20:32] = 60
    g[40:49, 40] = g[40:49, 48] = 60                      # ring with a 7 x 7 interior
    g[40, 40:49] = g[48, 40:49] = 60
    return g


def overlap_masks(shape):
    """Four 0 / 255 masks: 1 touches 0's box only in its last column, 2 only in its last row (no overlap by the exclusive
    slicing), 3 lies inside 0's box (overlap)."""
    H, W = shape
    m = np.zeros((4,) + shape, np.uint8)
    m[0, 10:31, 10:41] = 255                             # box x 10..40, y 10..30 (inclusive)
    m[0, 12:29, 12:39] = 0                               # an outline, so that its background mask is a filled silhouette
    m[1, 15:25, 40:50] = 255                             # column 40 = x2: dropped
    m[2, 30:45, 15:25] = 255                             # row 30 = y2: dropped
    m[3, 14:24, 14:24] = 255                             # an L: its own box holds pixels that are not its own
    m[3, 16:24, 16:24] = 0
    return m


def coloured_sketch(shape):
    H, W = shape
    rgb = np.full(shape + (3,), 255, np.uint8)
    rgb[10:31, 10:41] = (20, 20, 20)
    rgb[15, 18] = (200, 30, 90)                          # inside mask 3: R and B must come out swapped
    rgb[15:25, 40:50] = (0, 0, 0)
    rgb[30:45, 15:25] = (0, 0, 0)
    return rgb


# ---- the edge suite (tests/test_layers_cases_cpu.py, tests/test_layers_edges_gpu.py) ------------------------------------------
# Shapes chosen for one named edge of the kernels each; seeded random planes; constructed planes, each of which returns
# None on a shape it does not fit (the callers drop it there, see `fitting`); and, per GPU test, the list of planes it
# runs, so that the CPU test of the inputs and the GPU test look at the same arrays.
EDGE_SHAPES = [
    (1, 1),        # a single pixel: RM = 1, one live wave in a workgroup of 4 rows
    (1, 70),       # a single row, two plane words with a 6-bit tail
    (33, 2),       # two columns: RM = 2; one seam (row 32) whose band holds one row
    (64, 64),      # exactly one plane word (no tail bits, the start run at x0 = -1 has no `hi` word) and one chamfer tile
    (128, 128),    # exact multiples everywhere: Wp = 2 without tail, 2 x 2 tiles, last seam at row 96, last block ends at H
    (65, 129),     # one past the word, the tile and two seams: Wp = 3 with a 1-bit tail, tiles 1 pixel thick at the end
    (161, 200),    # wave 0 of the seam launch takes its second seam (row 160); 3 x 4 tiles, one with its halo inside; Wp = 4
    (200, 161),    # the same transposed: seams up to row 192, Wp = 3
    (3, 4200),     # Wp = 66: the second 64-word chunk of the run kernel; hundreds of runs per row; H < 4
]


def fitting(*planes):
    """The planes that exist on this shape (a constructed plane that does not fit is None)."""
    return [p for p in planes if p is not None]


def noise(shape, density, seed):
    return np.random.default_rng(seed).random(shape) < density


def blobs(shape, seed, margin=0):
    """Sparse seeds (and the centre pixel) dilated 2 - 5 times by the cross; no seed within `margin` of the edge."""
    H, W = shape
    a = np.random.default_rng(1000 + seed).random(shape) < 0.004
    if margin:
        keep = _blank(shape)
        keep[margin:H - margin, margin:W - margin] = True
        a &= keep
    a[H // 2, W // 2] = True
    return ndimage.binary_dilation(a, structure=R.CROSS, iterations=2 + seed % 4)


def rings(shape, seed):
    """A solid plane with carved rectangles and 6 % speckle inside them: holes with many small islands."""
    H, W = shape
    rng = np.random.default_rng(2000 + seed)
    a = np.ones(shape, bool)
    for _ in range(max(1, H * W // 700)):
        h, w = (int(v) for v in rng.integers(3, 15, 2))
        y, x = int(rng.integers(0, max(1, H - h))), int(rng.integers(0, max(1, W - w)))
        a[y:y + h, x:x + w] = False
    return a | (~a & (rng.random(shape) < 0.06))


def corner_flood_complement(plane):
    """What the engine hands to mode 'largest': everything but the 4-connected background component of pixel (0, 0)."""
    if plane[0, 0]:
        return np.ones(plane.shape, bool)
    lab, _ = ndimage.label(~plane, structure=R.CROSS)
    return ~(lab == lab[0, 0])


def comb(shape, closed=False):
    """A spine in row 0 with one-pixel teeth in every second column below it: W / 2 runs per tooth row, and one component
    made by W / 2 unions.  closed: a second spine under the teeth turns the slots into W / 2 one-pixel-wide holes."""
    H, W = shape
    if H < (3 if closed else 2) or W < 3:
        return None
    a = _blank(shape)
    t = min(6, H - 1 - int(closed))
    a[0] = True
    a[1:1 + t, ::2] = True
    if closed:
        a[1 + t] = True
    return a


def checkerboard(shape, phase=0):
    """One 8-connected component, H W / 2 4-connected ones; as a complement, holes that meet only at corners."""
    y, x = np.indices(shape)
    return (y + x + phase) % 2 == 0


def serpentine(shape, x0=0, x1=None):
    """A 1-pixel boustrophedon path over columns [x0, x1): full lines in the even rows, joined at alternating ends in the
    odd ones.  One component, linked across every row and so across every seam; its first run is in row 0."""
    H, W = shape
    x1 = W if x1 is None else x1
    if H < 3 or x1 - x0 < 3:
        return None
    a = _blank(shape)
    a[0::2, x0:x1] = True
    for y in range(1, H - 1, 2):
        a[y, x1 - 1 if (y // 2) % 2 == 0 else x0] = True
    return a


def serpentine_with_rival(shape):
    """The serpentine (contour area: one cell per turn) and, right of it, a 2-pixel-wide bar of the same contour area that
    starts in row 1: the bar is kept, unless the serpentine's root is not its first run."""
    H, W = shape
    if H < 3 or W < 16:
        return None
    a = serpentine(shape, 0, W - 6)
    turns = len(range(1, H - 1, 2))
    a[1:turns + 2, W - 3:W - 1] = True
    return a


def _stamp(a, y, x, shape_bits, value=False):
    h, w = shape_bits.shape
    a[y:y + h, x:x + w][shape_bits] = value


def _rect(h, w, extra=()):
    """h x w rectangle in a frame one row higher, plus the pixels `extra` (row, col)."""
    b = np.zeros((h + 1, w), bool)
    b[:h] = True
    for p in extra:
        b[p] = True
    return b


def nested_rings(shape):
    """Two nests of depth 4 in a solid plane: an 11 x 11 ring hole, a 9 x 9 ring island in it, a 7 x 7 ring hole in that
    (24 pixels, contour area 62: undecided) around a 5 x 5 island.  The nest at (2, 2) has its outer hole filled by the rule,
    so the undecided hole lies inside a filled one; the nest in the bottom right corner has its outer hole one pixel from
    the edge, which stays, and the undecided hole inside it is filled on its own."""
    H, W = shape
    if H < 26 or W < 26:
        return None
    a = np.ones(shape, bool)
    for y, x in ((2, 2), (H - 12, W - 12)):
        a[y:y + 11, x:x + 11] = False
        a[y + 1:y + 10, x + 1:x + 10] = True
        a[y + 2:y + 9, x + 2:x + 9] = False
        a[y + 3:y + 8, x + 3:x + 8] = True
    return a


# holes by (twice the contour area, pixels): 2 (h + 1) (w + 1) - 4 for a rectangle, + 3 for a pixel added flush with a
# corner, + 2 for one added in the middle of a side; a 2 x 2 island takes 2 off the hole's OWN cells
THRESHOLD_HOLES = [
    ("100 / 36 px", 3, _rect(3, 12), None),
    ("99 / 37 px", 8, _rect(4, 9, [(4, 0)]), None),                  # more pixels, less area than the one above
    ("100 / 25 px", 15, _rect(1, 25), None),
    ("99 / 25 px", 18, _rect(1, 24, [(1, 0)]), None),
    ("100 with island", 22, _rect(4, 9, [(4, 3), (4, 6)]), (1, 3)),    # own cells 98: undecided, filled by the host
    ("99 with island", 29, _rect(4, 9, [(4, 0)]), (1, 3)),            # own cells 97: undecided, stays
]


def threshold_holes(shape):
    """Pairs of holes at the threshold: contour areas 50 and 49.5, as rectangles and as 1-pixel strips, and a pair with a
    2 x 2 island each, which the kernel leaves to the host."""
    H, W = shape
    if H < 36 or W < 30:
        return None
    a = np.ones(shape, bool)
    for _, y, bits, island in THRESHOLD_HOLES:
        _stamp(a, y, 3, bits)
        if island:
            a[y + island[0]:y + island[0] + 2, 3 + island[1]:3 + island[1] + 2] = True
    return a


def edge_hole_boxes(shape):
    """(x0, x1, y0, y1, distance from its side) of eight 8 x 8 holes (contour area 79): per side one at distance 1, which
    stays, and one at distance 2, which is filled."""
    H, W = shape
    out = []
    for d, y, x in ((1, 10, 20), (2, 24, 34)):
        out += [(d, d + 7, y, y + 7, d), (W - 1 - d - 7, W - 1 - d, y, y + 7, d),
                (x, x + 7, d, d + 7, d), (x, x + 7, H - 1 - d - 7, H - 1 - d, d)]
    return out


def edge_holes(shape):
    H, W = shape
    if H < 64 or W < 64:
        return None
    a = np.ones(shape, bool)
    for x0, x1, y0, y1, _ in edge_hole_boxes(shape):
        a[y0:y1 + 1, x0:x1 + 1] = False
    return a


def diag_islands(shape):
    """Two holes of fewer than 50 own cells in boxes that allow 50, with islands of two and of three pixels that touch only
    at corners: a 4 x 4 block with two 1-pixel tails, a 5 x 5 block with one."""
    H, W = shape
    if H < 22 or W < 15:
        return None
    a = np.ones(shape, bool)
    a[3:7, 3:7] = False
    a[3, 7:12] = False
    a[7:12, 3] = False
    a[4, 4] = a[5, 5] = True
    a[14:19, 3:8] = False
    a[14, 8:12] = False
    a[15, 4] = a[16, 5] = a[15, 6] = True
    return a


RING_GRID_SHAPE = (100, 120)


def ring_grid(k, shape=RING_GRID_SHAPE):
    """k copies of case D of holes_image (a 24-pixel ring hole around a 5 x 5 island: undecided) on a grid of pitch 10."""
    H, W = shape
    per_row = (W - 4) // 10
    assert k <= per_row * ((H - 4) // 10)
    a = np.ones(shape, bool)
    for i in range(k):
        y, x = 3 + 10 * (i // per_row), 3 + 10 * (i % per_row)
        a[y:y + 7, x:x + 7] = False
        a[y + 1:y + 6, x + 1:x + 6] = True
    return a


def tie_components(shape):
    """Three components of contour area 12: a 2 x 13 bar (26 pixels), below it a U of 34 pixels (1-pixel arms, 2-pixel
    bottom) and, inside the U's opening and starting in the U's first row, a 4 x 5 block (20 pixels).  In raster order the
    bar comes first, then the U's left arm, then the block, then the U's right arm: the block is kept, and a U whose root
    were its right arm would win instead."""
    H, W = shape
    if H < 18 or W < 20:
        return None
    a = _blank(shape)
    a[3:5, 4:17] = True
    a[8:15, 4:16] = True
    a[8:13, 5:15] = False
    a[8:12, 7:12] = True
    return a


# ---- chamfer inputs -------------------------------------------------------------------------------------------------------
def solid3(shape):
    """All ones but three pixels: distances of half the image, far more than the 8 moves one launch can see."""
    H, W = shape
    a = np.ones(shape, bool)
    for y, x in ((1, 2), (H // 2, W // 2), (H - 2, W - 2)):
        a[min(max(y, 0), H - 1), min(max(x, 0), W - 1)] = False
    return a


def zero_tile(shape):
    """Noise of density 0.8 around one all-zero 64 x 64 chamfer tile (the interior tile where there is one)."""
    H, W = shape
    if H < 64 or W < 64:
        return None
    a = noise(shape, 0.8, 11)
    o = 64 if H >= 128 and W >= 128 else 0
    a[o:o + 64, o:o + 64] = False
    return a


def chamfer_masks(shape):
    if shape == (3, 4200):                                 # 527 launches per call: one plane only
        return [("solid3", solid3(shape))]
    named = [("solid3", solid3(shape)), ("noise 0.8", noise(shape, 0.8, 7)), ("ones", np.ones(shape, bool)),
             ("zeros", _blank(shape)), ("zero tile", zero_tile(shape))]
    return [(k, v) for k, v in named if v is not None]


def chamfer_strokes(masks, kind):
    """Stroke planes for a stack of masks.  'subset': a random 2 % of the mask; 'empty'; 'on_zero': the subset and one
    stroke pixel on a zero of the mask (where it has one)."""
    rng = np.random.default_rng(77)
    out = np.zeros(masks.shape, bool)
    if kind == "empty":
        return out
    for k, m in enumerate(masks):
        out[k] = m & (rng.random(m.shape) < 0.02)
        if kind == "on_zero" and not m.all():
            ys, xs = np.nonzero(~m)
            out[k, ys[len(ys) // 2], xs[len(ys) // 2]] = True
    return out


# ---- per GPU test: the planes it runs ---------------------------------------------------------------------------------------
def _big(shape):
    return min(shape) >= 64


def corner_pixels(shape):
    """Single pixels at every corner and on both sides of every word boundary (rows spread over the image)."""
    H, W = shape
    xs = sorted({0, W - 1} | {x for b in range(64, W, 64) for x in (b - 1, b)})
    pts = [(y, x) for y in sorted({0, H - 1}) for x in (0, W - 1)]
    pts += [((7 * i) % H, x) for i, x in enumerate(xs)]
    return sorted(set(pts))


def dilate_planes(shape):
    H, W = shape
    pix = _blank(shape)
    for p in corner_pixels(shape):
        pix[p] = True
    ends = _blank(shape)                                   # a row's last pixel and a row's first: nothing may wrap
    ends[0, W - 1] = True
    if H >= 5:                                             # far enough apart for each to show its own wrap
        ends[H - 1, 0] = True
    return [noise(shape, 0.05, 60), pix, ends]


def band_planes(shape, band):
    """Single pixels at distance band - 1 (inside the band) and band (outside it) from each side, clipped into the image,
    and an empty plane."""
    H, W = shape
    pts = []
    for d in (band - 1, band):
        pts += [(d, W // 2), (H - 1 - d, W // 2), (H // 2, d), (H // 2, W - 1 - d)]
    stack = np.zeros((len(pts) + 1,) + shape, bool)
    for k, (y, x) in enumerate(pts):
        stack[k, min(max(y, 0), H - 1), min(max(x, 0), W - 1)] = True
    return stack


def flood_planes(shape):
    empty, corner = _blank(shape), noise(shape, 0.3, 21)
    corner[0, 0] = True
    clear = [noise(shape, d, 20 + i) for i, d in enumerate((0.3, 0.5, 0.62))]
    for c in clear:
        c[0, 0] = False
    s = serpentine(shape)
    return fitting(*clear, checkerboard(shape, 1), checkerboard(shape, 0), None if s is None else ~s, corner, empty)


def fill_all_planes(shape):
    return fitting(noise(shape, 0.3, 30), noise(shape, 0.5, 31), noise(shape, 0.62, 32), rings(shape, 0),
                   comb(shape, closed=True), comb(shape), nested_rings(shape), checkerboard(shape, 0))


def fill_rule_calls(shape):
    """Batches of at most 3 planes: the undecided holes of a call share one table of 64 records."""
    if _big(shape):
        calls = [[noise(shape, 0.5, s) for s in (0, 1, 2)],
                 [noise(shape, 0.3, 3), noise(shape, 0.62, 4), diag_islands(shape)],
                 [threshold_holes(shape), edge_holes(shape), rings(shape, 1)],
                 fitting(nested_rings(shape), rings(shape, 2))]
    else:
        calls = [[noise(shape, 0.5, 0), noise(shape, 0.3, 3), rings(shape, 1)]]
    return [np.stack(c) for c in calls if c]


def largest_planes(shape):
    return fitting(corner_flood_complement(_corner_clear(noise(shape, 0.3, 40))),
                   corner_flood_complement(_corner_clear(noise(shape, 0.5, 41))),
                   corner_flood_complement(_corner_clear(blobs(shape, 2))),
                   corner_flood_complement(_corner_clear(blobs(shape, 3))),
                   tie_components(shape), comb(shape), serpentine(shape), serpentine_with_rival(shape), _blank(shape))


def _corner_clear(a):
    a = a.copy()
    a[0, 0] = False
    return a


def sketch_planes(shape):
    """Stroke planes for background_masks: noise and blobs (strokes near the edge: open curve) and, on the shapes that have
    room, blobs kept 26 pixels off the edge (closed silhouette under every parameter set).  Each has a stroke pixel."""
    out = [noise(shape, 0.3, 50), blobs(shape, 1)]
    if _big(shape):
        out.append(blobs(shape, 0, margin=28))
    for a in out:
        a[shape[0] // 2, shape[1] // 2] = True
    return out


def grey_of(plane):
    return np.where(plane, 30, 255).astype(np.uint8)


BG_PARAM_SETS = [{}, dict(safety_margin=10), dict(dilate_iter=10, kernel_size=5, safety_margin=1, stroke_thick=2, border_band=3),
                 dict(kernel_size=5, dilate_iter=2, border_band=3)]


def object_masks(shape, n, seed):
    """n 0 / 255 masks: random rectangles and L shapes, with (for n >= 8) an empty mask, a 1-pixel-high and a 1-pixel-wide
    one, and two that touch only the dropped last column / row of mask 0's box."""
    H, W = shape
    rng = np.random.default_rng(3000 + seed)
    m = np.zeros((n,) + shape, np.uint8)
    for i in range(n):
        h, w = int(rng.integers(1, max(2, H // 2 + 1))), int(rng.integers(1, max(2, W // 2 + 1)))
        y, x = int(rng.integers(0, H - h + 1)), int(rng.integers(0, W - w + 1))
        m[i, y:y + h, x:x + w] = 255
        if i % 2 and h > 2 and w > 2:                     # an L: its box holds pixels that are not its own
            m[i, y:y + h // 2, x + w // 2:x + w] = 0
    if n >= 8:
        x1, y1, x2, y2 = R.mask_to_bbox(m[0])
        m[3] = 0
        m[4] = 0
        m[4, H // 2, :] = 255
        m[5] = 0
        m[5, :, W // 2] = 255
        m[6] = 0
        m[6, :, x2] = 255                                  # only column x2 of mask 0's box
        m[7] = 0
        m[7, y2, :] = 255                                  # only row y2
    return m


def layer_masks(shape, seed=0):
    """6 overlapping object masks (filled rectangles and ellipses, none empty) and a random RGB sketch."""
    H, W = shape
    rng = np.random.default_rng(4000 + seed)
    y, x = np.indices(shape)
    m = np.zeros((6,) + shape, np.uint8)
    for i in range(6):
        cy, cx = int(rng.integers(H // 4, 3 * H // 4)), int(rng.integers(W // 4, 3 * W // 4))
        ry, rx = int(rng.integers(4, H // 5)), int(rng.integers(4, W // 5))
        if i % 2:
            m[i][((y - cy) / ry) ** 2 + ((x - cx) / rx) ** 2 <= 1.0] = 255
        else:
            m[i, cy - ry:cy + ry, cx - rx:cx + rx] = 255
    rgb = rng.integers(0, 256, shape + (3,), dtype=np.uint8)
    rgb[rng.random(shape) < 0.5] = 255
    return m, rgb


# ---- the kernel's hole rule, restated --------------------------------------------------------------------------------------
def hole_table(mask):
    """Per enclosed 4-connected hole of `mask`: dict(first=(y, x) of its first pixel in raster order, box=(x0, x1, y0, y1) of
    its own pixels, own2=twice the contour area of its own cells (R.cells_area2), islands=it surrounds foreground,
    region2=twice the contour area with what it surrounds, off_edge=the box is two pixels off every side, undecided=the
    kernel leaves it to the host: off_edge, own2 < 100, islands, and a box that allows 50, pixels=its pixel count,
    window / region=the box as slices and the hole with what it surrounds inside it)."""
    H, W = mask.shape
    lab, n = ndimage.label(~mask, structure=R.CROSS)
    out = []
    for l, sl in enumerate(ndimage.find_objects(lab), 1):
        y0, y1, x0, x1 = sl[0].start, sl[0].stop - 1, sl[1].start, sl[1].stop - 1
        if x0 == 0 or y0 == 0 or x1 == W - 1 or y1 == H - 1:
            continue
        own = np.pad(lab[sl] == l, 1)
        region = ndimage.binary_fill_holes(own, structure=R.ONES3)
        ys, xs = np.nonzero(own)
        islands = bool((region & ~own).any())
        own2 = R.cells_area2(own, True)
        off_edge = x0 > 1 and y0 > 1 and x1 < W - 2 and y1 < H - 2
        out.append(dict(first=(y0 + int(ys[0]) - 1, x0 + int(xs[0]) - 1), box=(x0, x1, y0, y1), own2=own2, islands=islands,
                        region2=R.cells_area2(region, True), off_edge=off_edge, pixels=int(own.sum()),
                        window=(slice(y0, y1 + 1), slice(x0, x1 + 1)), region=region[1:-1, 1:-1],
                        undecided=off_edge and own2 < 100 and islands and 2 * (x1 - x0 + 2) * (y1 - y0 + 2) >= 100))
    return out
