"""An independent numpy statement of the evaluation stage's counting (csrc/evaluate.hip, inklayer_amd/evaluate.py), and
the inputs the CPU and GPU tests share.

The table is stated mask by mask with boolean indexing and np.unique(return_counts=True) - not with the package's
rank image and bincount.  `mistake=` plants one of the errors a tiled counting kernel can make, so that a test can show
that its inputs would expose it:
  "last_strip"     the last strip of 1024 pixels (in raster order) is not counted
  "cols64"         the columns from 64 * (W // 64) on are not counted
  "mask32_row0"    mask 32 is counted into row 0
  "totals_tile"    the launch has ceil(n / 32) row tiles instead of ceil((n + 1) / 32): row n stays empty when n % 32 == 0
  "stroke249"      the stroke test is grey < 249
"""
from functools import lru_cache
from pathlib import Path

import numpy as np

GOLDEN = Path(__file__).resolve().parent / "golden"
SETS = ["Clipasso_brushpen_0249", "animal_hike_sketch", "bunny_cook_sketch", "clock_lamp_plant", "fscoco_animals",
        "mario_bunny", "office_sketch"]
MISTAKES = ["last_strip", "cols64", "mask32_row0", "totals_tile", "stroke249"]
STRIP = 1024


def gray(sketch):
    """cv2's COLOR_RGB2GRAY for uint8 (fixed point, 14 bits); a single channel is taken as it is."""
    a = np.asarray(sketch)
    if a.ndim == 2:
        return a.astype(np.int64)
    a = a.astype(np.int64)
    return (4899 * a[..., 0] + 9617 * a[..., 1] + 1868 * a[..., 2] + 8192) >> 14


def planes_of(pred, n_labels=None):
    """bool [n, H, W] of a stack / sequence of masks (non-zero = inside) or, with n_labels, of a label image."""
    if n_labels is not None:
        lab = np.asarray(pred)
        return np.stack([lab == l for l in range(1, n_labels + 1)]) if n_labels else np.zeros((0,) + lab.shape, bool)
    return np.stack([np.asarray(m) != 0 for m in pred]) if len(pred) else None


def contingency(pred, labels, sketch=None, stroke_only=False, n_labels=None, mistake=None):
    """-> (T int64 [n + 1, U], values int64 [U])."""
    labels = np.asarray(labels)
    H, W = labels.shape
    values = np.unique(labels).astype(np.int64)
    planes = planes_of(pred, n_labels)
    n = 0 if planes is None else len(planes)
    counted = np.ones((H, W), bool)
    if stroke_only:
        counted = gray(sketch) < (249 if mistake == "stroke249" else 250)
    if mistake == "last_strip":
        counted = counted.copy()
        counted.reshape(-1)[STRIP * ((H * W - 1) // STRIP):] = False
    if mistake == "cols64":
        counted = counted.copy()
        counted[:, 64 * (W // 64):] = False
    T = np.zeros((n + 1, len(values)), np.int64)

    def count_into(row, sel):
        vals, cnt = np.unique(labels[sel], return_counts=True)
        T[row, np.searchsorted(values, vals)] += cnt

    for i in range(n):
        count_into(0 if (mistake == "mask32_row0" and i == 32) else i, planes[i] & counted)
    if not (mistake == "totals_tile" and n % 32 == 0):
        count_into(n, counted)
    return T, values


def ranks(labels):
    """-> (values, rank image)."""
    values, inv = np.unique(np.asarray(labels), return_inverse=True)
    return values.astype(np.int64), inv.reshape(np.shape(labels))


def boxes(labels):
    """int64 [U, 4]: xmin, ymin, xmax, ymax (inclusive) per distinct value."""
    labels = np.asarray(labels)
    out = []
    for v in np.unique(labels):
        ys, xs = np.nonzero(labels == v)
        out.append((xs.min(), ys.min(), xs.max(), ys.max()))
    return np.asarray(out, np.int64)


def picture(labels, colors):
    """read_GT_mat_file.py:40-70 given its colour list: white, then colors[idx] for the idx-th distinct value but 0."""
    labels = np.asarray(labels)
    out = np.full(labels.shape + (3,), 255, np.uint8)
    for idx, v in enumerate(np.unique(labels)):
        if v != 0:
            out[labels == v] = colors[idx]
    return out


# ----------------------------------------------------------------------------------------------------------------------
# shared inputs
# ----------------------------------------------------------------------------------------------------------------------
SHAPES = [(1, 1), (5, 67), (33, 256), (64, 129)]
MASK_COUNTS = [0, 1, 31, 32, 33, 65]
VALUE_COUNTS = [1, 2, 256]
DTYPES = [np.uint8, np.uint16, np.int32]


def make_labels(rs, H, W, U, dtype):
    """A per-pixel random label image with min(U, H W) distinct values, sparse over the dtype's range (up to 65535) and
    holding its largest value; 0 is among them for every second seed."""
    U = min(U, H * W)
    top = 255 if dtype == np.uint8 else 65535
    zero = U > 1 and (bool(rs.randint(2)) or U == top + 1)
    pool = rs.permutation(top - 1) + 1                                       # 1 .. top - 1 in random order
    values = np.sort(np.concatenate([[top], [0] if zero else [], pool[:U - 1 - int(zero)]])).astype(np.int64)
    assert len(np.unique(values)) == U
    lab = values[rs.randint(0, U, size=H * W)]
    lab[rs.permutation(H * W)[:U]] = values                                  # every value occurs
    return lab.reshape(H, W).astype(dtype)


def make_masks(rs, n, H, W):
    """uint8 [n, H, W]: overlapping random rectangles with holes; inside values 1, 7 and 255 in turn."""
    out = np.zeros((n, H, W), np.uint8)
    for k in range(n):
        y0, x0 = rs.randint(0, H), rs.randint(0, W)
        y1, x1 = rs.randint(y0, H) + 1, rs.randint(x0, W) + 1
        if k % 4 == 0:
            y0, x0, y1, x1 = 0, 0, H, W                                      # reaches the last row and column
        out[k, y0:y1, x0:x1] = (rs.rand(y1 - y0, x1 - x0) < 0.8) * (1, 7, 255)[k % 3]
    return out


def make_sketch(rs, H, W, channels):
    """uint8 sketch whose greys straddle the stroke bound: 248 .. 251 on most pixels, anything on the rest; the last
    pixel is 249."""
    g = rs.randint(248, 252, size=(H, W))
    other = rs.rand(H, W) < 0.3
    g[other] = rs.randint(0, 256, size=int(other.sum()))
    g[H - 1, W - 1] = 249
    g = g.astype(np.uint8)
    if channels == 1:
        return g
    rgb = np.repeat(g[..., None], 3, axis=2)
    tint = rs.rand(H, W) < 0.3                                               # not only grey pixels
    rgb[tint, 1] = rs.randint(240, 256, size=int(tint.sum()))
    rgb[H - 1, W - 1] = 249
    return rgb


def small_case(shape, n, U, dtype, channels=3):
    """(masks, labels, sketch) of one small case, seeded by its parameters."""
    H, W = shape
    rs = np.random.RandomState(100000 * H + 100 * W + 7 * n + U + np.dtype(dtype).itemsize)
    return make_masks(rs, n, H, W), make_labels(rs, H, W, U, dtype), make_sketch(rs, H, W, channels)


def small_cases():
    """Every (shape, n, U, dtype) of the GPU test's grid."""
    for shape in SHAPES:
        for n in MASK_COUNTS:
            for U in VALUE_COUNTS:
                for dtype in DTYPES:
                    yield shape, n, U, dtype


@lru_cache(maxsize=None)
def load_set(name):
    """One committed refinement fixture at its real size: input uint8 [H, W, 3]; masks bool [n, H, W] (the segmentor's);
    final bool [m, H, W] with final_indices (the files of masks_final/); label = the label image of masks_final (mask i
    of the stack -> i + 1); scores / final_scores / final_kept as in the JSON files.  Read-only, loaded once."""
    z = np.load(GOLDEN / f"refine_{name}.npz")
    inp = z["input"]
    W = inp.shape[1]
    unpack = lambda key: np.unpackbits(z[key][z[key + "_present"]], axis=-1)[..., :W].astype(bool)
    final = unpack("masks_final")
    label = np.zeros(inp.shape[:2], np.uint8)
    for i, m in enumerate(final):
        label[m] = i + 1
    out = {"input": inp, "masks": unpack("masks"), "final": final, "label": label,
           "final_indices": np.flatnonzero(z["masks_final_present"]), "scores": z["scores"],
           "final_scores": z["final_scores"], "final_kept": z["final_kept"], "bboxes": z["bboxes"],
           "final_bboxes": z["final_bboxes"]}
    for a in out.values():
        a.setflags(write=False)
    return out


@lru_cache(maxsize=None)
def set_table(name, stroke_only):
    """The reference table of a set: its `masks` against its final label image.  Computed once, shared."""
    s = load_set(name)
    T, values = contingency(s["masks"], s["label"], s["input"], stroke_only)
    T.setflags(write=False)
    return T, values
