"""Synthetic inputs for the layer-assembly tests (tests/test_layers_ref_cpu.py, tests/test_layers_gpu.py): the rules
the reference's committed outputs do not separate, each on the two shapes the kernels are tested at.  70 x 130 and
130 x 70: two plane words per row with a ragged tail / one ragged word, more rows than one 32-row band, a chamfer
tile edge inside the image in one direction only."""
import numpy as np

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
