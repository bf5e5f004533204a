"""numpy / scipy restatement of the reference's layer-assembly stage (InkLayer/inpainting/util.py,
fill_object_bg_mask.py, runner.py:79-84), written from the arithmetic and from the published algorithms it relies on,
without cv2.  The test-side oracle of inklayer_amd/layers.py and csrc/layers.hip.

Pinned by the reference's committed outputs (tests/golden/layers_<set>.npz): the grey conversion, the Otsu decision,
the ellipse shapes, both branches of get_mask, the chamfer constants, the bbox slicing and the channel swap.
Pinned HERE and not by cv2 (the fixtures do not separate it from cruder rules): `contour_area`, i.e. Suzuki-Abe border
following (CVGIP 30, 1985, algorithm 1) plus the shoelace sum over the followed pixel centres, and the order in which
equal areas are ranked (`largest_component`).
"""
import numpy as np
from scipy import ndimage

CROSS = np.array([[0, 1, 0], [1, 1, 1], [0, 1, 0]], bool)
ONES3 = np.ones((3, 3), bool)
FIX_A, FIX_B, FIX_C = 65536, 91750, 143976        # round(w * 2^16) for w = 1, 1.4, 2.1969
DIST_INF = (2 ** 31 - 1) >> 2


def png_gray(rgb):
    """cv2.imread(path, IMREAD_GRAYSCALE) of an 8-bit RGB PNG."""
    r, g, b = (rgb[..., i].astype(np.uint32) for i in range(3))
    return ((r * 9798 + g * 19235 + b * 3735 + 16384) >> 15).astype(np.uint8)


def histogram(gray):
    return np.bincount(np.asarray(gray, np.uint8).ravel(), minlength=256).astype(np.int64)


def otsu_from_hist(h):
    """Otsu's threshold from 256 counts, in float64 and in the order cv2 evaluates it; first maximum wins."""
    n = float(h.sum())
    scale = 1.0 / n
    mu = 0.0
    for i in range(256):
        mu += float(i) * float(h[i])
    mu *= scale
    mu1 = q1 = 0.0
    best, best_t = 0.0, 0
    eps = float(np.finfo(np.float32).eps)
    for i in range(256):
        p = float(h[i]) * scale
        mu1 *= q1
        q1 += p
        q2 = 1.0 - q1
        if min(q1, q2) < eps or max(q1, q2) > 1.0 - eps:
            continue
        mu1 = (mu1 + float(i) * p) / q1
        mu2 = (mu - q1 * mu1) / q2
        sigma = q1 * q2 * (mu1 - mu2) * (mu1 - mu2)
        if sigma > best:
            best, best_t = sigma, i
    return best_t


def ellipse(k):
    if k == 3:
        return CROSS
    assert k == 5
    e = np.zeros((5, 5), bool)
    e[1:4, :] = True
    e[:, 2] = True
    return e


def dilate(a, k, iterations):
    if iterations <= 0:
        return a.copy()
    return ndimage.binary_dilation(a, structure=ellipse(k), iterations=iterations, border_value=0)


def touches_band(a, band):
    return bool(a[:band].any() or a[-band:].any() or a[:, :band].any() or a[:, -band:].any())


# ---- border following and contour area -------------------------------------------------------------------------------
_CW = [(0, 1), (1, 1), (1, 0), (1, -1), (0, -1), (-1, -1), (-1, 0), (-1, 1)]     # clockwise on the screen (row down)


def follow_border(f, start, first_bg):
    """Suzuki-Abe steps 3.1 - 3.5: the border of the 1-component through `start` (row, col) next to the 0-pixel
    `first_bg` (a 4-neighbour of start).  f: bool image, taken as 0 outside.  -> list of (row, col)."""
    H, W = f.shape

    def on(p):
        return 0 <= p[0] < H and 0 <= p[1] < W and f[p[0], p[1]]

    def direction(a, b):
        return _CW.index((b[0] - a[0], b[1] - a[1]))

    i0 = start
    d = direction(i0, first_bg)
    p1 = None
    for s in range(8):                                    # 3.1 clockwise from first_bg
        q = (i0[0] + _CW[(d + s) % 8][0], i0[1] + _CW[(d + s) % 8][1])
        if on(q):
            p1 = q
            break
    if p1 is None:
        return [i0]
    out = []
    p2, p3 = p1, i0
    while True:
        d = direction(p3, p2)
        p4 = None
        for s in range(1, 9):                             # 3.3 counterclockwise from the element after p2
            dd = _CW[(d - s) % 8]
            q = (p3[0] + dd[0], p3[1] + dd[1])
            if on(q):
                p4 = q
                break
        out.append(p3)
        if p4 == i0 and p3 == p1:                         # 3.5
            return out
        p2, p3 = p3, p4


def shoelace2(pts):
    """|twice the polygon area| through the points (row, col), an integer."""
    s = 0
    n = len(pts)
    for k in range(n):
        y0, x0 = pts[k]
        y1, x1 = pts[(k + 1) % n]
        s += x0 * y1 - x1 * y0
    return abs(s)


def outer_contour(f, comp):
    """Border of the 8-connected component `comp` (bool) of f that faces the outside."""
    ys, xs = np.nonzero(comp)
    y, x = int(ys[0]), int(xs[0])                          # first pixel in raster order: its left neighbour is 0
    return follow_border(f, (y, x), (y, x - 1))


def hole_contour(f, hole):
    """Border that surrounds the 4-connected 0-component `hole` (bool, not touching the image edge): it runs on
    the 1-pixels around it."""
    ys, xs = np.nonzero(hole)
    y, x = int(ys[0]), int(xs[0])                          # its left neighbour is a 1-pixel
    return follow_border(f, (y, x - 1), (y, x))


def contour_area(pts):
    return shoelace2(pts) / 2.0


def holes_of(mask):
    """label image and count of the 4-connected 0-components that do not reach the image edge."""
    lab, n = ndimage.label(~mask, structure=CROSS)
    edge = np.unique(np.concatenate([lab[0], lab[-1], lab[:, 0], lab[:, -1]]))
    keep = [l for l in range(1, n + 1) if l not in set(edge.tolist())]
    return lab, keep


def fill_enclosed_regions(mask):
    return ndimage.binary_fill_holes(mask, structure=CROSS)


def fill_holes_not_touching_border(mask, min_area=50):
    """Every hole whose contour's bounding rect stays off the image edge and whose contour area is >= min_area is
    filled as a polygon: the hole and everything it surrounds."""
    H, W = mask.shape
    out = mask.copy()
    lab, keep = holes_of(mask)
    for l in keep:
        hole = lab == l
        pts = hole_contour(mask, hole)
        ys = [p[0] for p in pts]
        xs = [p[1] for p in pts]
        touches = min(xs) == 0 or min(ys) == 0 or max(xs) + 1 == W or max(ys) + 1 == H
        if not touches and contour_area(pts) >= min_area:
            out |= ndimage.binary_fill_holes(hole, structure=ONES3)
    return out


def largest_component(sil):
    """The 8-connected component with the largest outer contour area, with what it surrounds.  Equal areas: the one
    whose first pixel comes LAST in raster order (contours are listed newest first and max() keeps the first)."""
    lab, n = ndimage.label(sil, structure=ONES3)
    first = {}
    flat = lab.ravel()
    idx = np.nonzero(flat)[0]
    for l, p in zip(flat[idx][::-1], idx[::-1]):
        first[int(l)] = int(p)
    best, best_key = None, None
    for l in range(1, n + 1):
        comp = lab == l
        key = (shoelace2(outer_contour(sil, comp)), first[l])
        if best_key is None or key > best_key:
            best, best_key = comp, key
    return ndimage.binary_fill_holes(best, structure=CROSS)


# ---- chamfer distance --------------------------------------------------------------------------------------------------
_MOVES = ([(0, 1, FIX_A), (0, -1, FIX_A), (1, 0, FIX_A), (-1, 0, FIX_A)]
          + [(a, b, FIX_B) for a in (-1, 1) for b in (-1, 1)]
          + [(a * sa, b * sb, FIX_C) for a, b in ((1, 2), (2, 1)) for sa in (-1, 1) for sb in (-1, 1)])


def chamfer_fixed(mask):
    """5x5 chamfer distance to the nearest 0-pixel INSIDE the image, int32 in 16.16 fixed point (weights 1, 1.4,
    2.1969); the fixed point of the relaxation, which the two raster passes reach on a rectangle."""
    H, W = mask.shape
    out = np.zeros((H, W), np.int64)
    if not mask.any():
        return out.astype(np.int32)
    if mask.all():
        return np.full((H, W), DIST_INF, np.int32)
    ys, xs = np.nonzero(mask)
    y0, y1 = max(0, ys.min() - 2), min(H, ys.max() + 3)
    x0, x1 = max(0, xs.min() - 2), min(W, xs.max() + 3)
    m = mask[y0:y1, x0:x1]
    h, w = m.shape
    d = np.full((h + 4, w + 4), DIST_INF, np.int64)
    d[2:-2, 2:-2] = np.where(m, DIST_INF, 0)
    while True:
        c = d[2:-2, 2:-2]
        new = c.copy()
        for dy, dx, wgt in _MOVES:
            np.minimum(new, d[2 + dy:2 + dy + h, 2 + dx:2 + dx + w] + wgt, out=new)
        if np.array_equal(new, c):
            break
        d[2:-2, 2:-2] = new
    out[y0:y1, x0:x1] = d[2:-2, 2:-2]
    return out.astype(np.int32)


def dist_float(d_fixed):
    """The float32 image cv2 hands out: the integers converted to float32 and scaled by 2^-16."""
    return d_fixed.astype(np.float32) * np.float32(1.0 / 65536.0)


# ---- get_mask ------------------------------------------------------------------------------------------------------------
def get_mask(gray, dilate_iter=5, kernel_size=3, safety_margin=0, stroke_thick=1, border_band=2):
    """-> (bool mask, 'open-curve' | 'closed-silhouette', shrink_by).  gray: what IMREAD_GRAYSCALE gives."""
    inv = 255 - np.asarray(gray, np.uint8)
    strokes = inv > otsu_from_hist(histogram(inv))
    thick = dilate(strokes, kernel_size, dilate_iter)
    if touches_band(thick, border_band):
        m = dilate(strokes, kernel_size, stroke_thick)
        return fill_holes_not_touching_border(m, 50), "open-curve", 0
    lab, _ = ndimage.label(~thick, structure=CROSS)
    flooded = thick | (lab == lab[0, 0])
    sil = ~flooded | thick
    mask = largest_component(sil)
    dist = chamfer_fixed(mask)
    min_pad = int(np.floor(dist_float(dist)[strokes].min()))
    shrink_by = max(0, min_pad - safety_margin)
    if shrink_by > 0:
        mask = dist_float(dist) >= np.float32(shrink_by)
    return fill_enclosed_regions(mask), "closed-silhouette", shrink_by


BG_PARAMS = dict(dilate_iter=10, kernel_size=5, safety_margin=1, stroke_thick=2, border_band=3)


# ---- util.py ---------------------------------------------------------------------------------------------------------------
def mask_to_bbox(mask_u8):
    ys, xs = np.nonzero(np.asarray(mask_u8) > 127)
    return [int(xs.min()), int(ys.min()), int(xs.max()), int(ys.max())]       # inclusive maxima


def mask_within_bbox(mask, bbox):
    x1, y1, x2, y2 = bbox
    m = mask.copy()
    m[:y1] = False
    m[y2:] = False                                         # exclusive: the last row and column drop out
    m[:, :x1] = False
    m[:, x2:] = False
    return m


def overlap_list(masks_u8, i):
    mi = masks_u8[i] > 0
    return [j for j in range(i) if mask_within_bbox(mi, mask_to_bbox(masks_u8[j])).any()]


def assemble(input_rgb, masks_u8, i, bg_cache=None):
    """assemble_inpaint_input_at_index for layer i.  masks_u8: [n, H, W] uint8 in masks_final order.
    -> dict(sketch_layer (the array the reference holds: B, G, R), overlaps, edit_mask | None, debug_vis | None,
    original_sketch_mask | None)."""
    mask = masks_u8[i] > 0
    layer = np.ascontiguousarray(input_rgb[..., ::-1]).copy()
    layer[~mask] = 255
    out = dict(sketch_layer=layer, overlaps=[], edit_mask=None, debug_vis=None, original_sketch_mask=None)
    if i == 0:
        return out
    ov = overlap_list(masks_u8, i)
    out["overlaps"] = ov
    if not ov:
        out["debug_vis"] = mask
        return out
    bg = np.zeros_like(mask)
    for j in ov:
        if bg_cache is not None and j in bg_cache:
            b = bg_cache[j]
        else:
            b = get_mask(255 - masks_u8[j], **BG_PARAMS)[0]
            if bg_cache is not None:
                bg_cache[j] = b
        bg |= b
    edit = mask_within_bbox(bg, mask_to_bbox(masks_u8[i]))
    edit[mask] = False
    vis = np.zeros(mask.shape + (3,), np.uint8)
    vis[mask] = 255
    vis[edit] = (0, 0, 255)
    out.update(edit_mask=edit, debug_vis=vis, original_sketch_mask=(layer < 255).any(axis=2))
    return out


def composite(inpainted_rgb, sketch_layer, original_sketch_mask):
    final = np.array(inpainted_rgb, copy=True)
    final[original_sketch_mask] = sketch_layer[..., ::-1][original_sketch_mask]
    return final


def rgba_layer(layer_rgb):
    """create_rgba_with_background_mask on the pixels of complete_layers/layer_i.png -> uint8 [H, W, 4]."""
    gray = png_gray(layer_rgb)
    bg = get_mask(gray)[0]
    sketch = gray < 240
    out = np.zeros(gray.shape + (4,), np.uint8)
    out[..., 3] = np.where(sketch | bg, 255, 0)
    out[bg, :3] = 255
    out[sketch, :3] = gray[sketch][:, None]
    return out


# ---- closed forms the product uses, checked against the border following in tests/test_layers_ref_cpu.py -------------------
def cells_area2(region, hole):
    """Twice the contour area by 2x2 cells of pixel centres.  hole=False: `region` is an 8-connected component
    with what it surrounds; a cell counts 1 when all four corners lie in it and 1/2 when three do.  hole=True:
    `region` is a hole with what it surrounds; a cell counts 1 when two or more corners lie in it and 1/2 when one."""
    r = np.pad(region.astype(np.int64), 1)
    c = r[:-1, :-1] + r[:-1, 1:] + r[1:, :-1] + r[1:, 1:]
    if hole:
        return int(2 * (c >= 2).sum() + (c == 1).sum())
    return int(2 * (c == 4).sum() + (c == 3).sum())
