"""The numpy / scipy restatement of the layer-assembly stage (tests/layers_ref.py) against the reference's own
committed outputs (tests/golden/layers_<set>.npz, every pixel of every set), and its rules on the synthetic cases that
those outputs do not separate.  No GPU."""
import glob
import os

import numpy as np
import pytest
from scipy import ndimage

import layers_cases as K
import layers_ref as R

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
SETS = sorted(os.path.basename(f)[len("layers_"):-4] for f in glob.glob(os.path.join(GOLDEN, "layers_*.npz")))


def load_set(name):
    L = np.load(os.path.join(GOLDEN, f"layers_{name}.npz"))
    Z = np.load(os.path.join(GOLDEN, f"refine_{name}.npz"))
    inp = Z["input"]
    W = inp.shape[1]
    masks = np.unpackbits(Z["masks_final"], axis=-1)[..., :W][Z["masks_final_present"]].astype(np.uint8) * 255
    n = int(L["n_layers"])
    assert n == len(masks)
    return dict(input=inp, masks=masks, n=n, need=L["need_inpaint"],
                edit=np.unpackbits(L["edit_mask"], axis=-1)[..., :W].astype(bool), sketch=L["sketch_layer"],
                index=L["inpaint_index"].tolist(), inpainted=L["inpainted"], final=L["inpainted"] ^ L["final_xor"],
                alpha=np.unpackbits(L["rgba_alpha"], axis=-1)[..., :W].astype(bool), rgb=L["rgba_rgb"],
                gray_ok=bool(L["rgba_gray_ok"]))


def test_six_sets_are_packed():
    assert len(SETS) == 6 and "fscoco_animals" in SETS and "Clipasso_brushpen_0249" in SETS


@pytest.mark.parametrize("name", SETS)
def test_restatement_reproduces_every_fixture_pixel(name):
    S = load_set(name)
    assert S["gray_ok"] and sorted(S["index"]) == [i for i in range(S["n"]) if S["need"][i]]   # nothing left out
    cache, branches = {}, set()
    for i in range(S["n"]):
        a = R.assemble(S["input"], S["masks"], i, cache)
        assert np.array_equal(a["sketch_layer"], S["sketch"][i]), ("sketch_layer", i)
        assert (a["edit_mask"] is not None) == bool(S["need"][i]), ("need_inpaint", i)
        layer_file = a["sketch_layer"]
        if a["edit_mask"] is not None:
            assert np.array_equal(a["edit_mask"], S["edit"][i]), ("edit_mask", i)
            k = S["index"].index(i)
            layer_file = R.composite(S["inpainted"][k], a["sketch_layer"], a["original_sketch_mask"])
            assert np.array_equal(layer_file, S["final"][k]), ("final_composited", i)
        rgba = R.rgba_layer(layer_file)
        assert np.array_equal(rgba[..., 3] > 0, S["alpha"][i]), ("rgba alpha", i)
        assert np.array_equal(rgba[..., 0], S["rgb"][i]) and np.array_equal(rgba[..., 1], S["rgb"][i]), ("rgba colour", i)
        assert set(np.unique(rgba[..., 3]).tolist()) <= {0, 255}


# ---- synthetic cases ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", K.SHAPES)
def test_hole_rule_uses_the_contour_area_not_the_pixel_count(shape):
    a = K.holes_image(shape)
    lab, keep = R.holes_of(a)
    facts = {}
    for l in keep:
        hole = lab == l
        pts = R.hole_contour(a, hole)
        facts[int(hole.sum())] = R.contour_area(pts)
    assert facts[42] == 54.0 and facts[30] == 40.0 and facts[24] == 62.0       # A, B, D: the box of ring pixels less 4 cut corners
    out = R.fill_holes_not_touching_border(a)
    filled = out & ~a
    flab, fn = ndimage.label(filled, structure=R.CROSS)
    sizes = sorted(int((flab == l).sum()) for l in range(1, fn + 1))
    # A (42), D's ring (24), E's hole (34 x 24 minus its 22 x 15 island) and the small hole in E's island (16)
    assert sizes == sorted([42, 24, 34 * 24 - 22 * 15, 16])
    assert not out[np.nonzero(lab == [l for l in keep if (lab == l).sum() == 30][0])].any()      # B stays
    c = [l for l in keep if (lab == l).sum() == 160][0]                                          # C: one pixel from the edge
    assert not out[lab == c].any()
    assert np.array_equal(R.fill_enclosed_regions(a), ndimage.binary_fill_holes(a))
    assert R.fill_enclosed_regions(a)[lab == c].all()


@pytest.mark.parametrize("shape", K.SHAPES)
def test_largest_component_ranks_by_contour_area(shape):
    a = K.two_components(shape)
    lab, n = ndimage.label(a, structure=R.ONES3)
    assert n == 2
    by_count = max(range(1, 3), key=lambda l: (lab == l).sum())
    got = R.largest_component(a)
    assert not got[lab == by_count].any() and got[20:27, 20:27].all() and int(got.sum()) == 49 + 6
    block = np.zeros_like(a)
    block[20:27, 20:27] = True
    assert R.shoelace2(R.outer_contour(block, block)) == 72
    # the spur adds the two half cells where it joins the block and nothing along its length
    assert R.shoelace2(R.outer_contour(a, lab == lab[20, 20])) == 74
    longer = a.copy()
    longer[23, 27:60] = True
    assert R.shoelace2(R.outer_contour(longer, ndimage.label(longer, structure=R.ONES3)[0] == lab[20, 20])) == 74
    e = K.equal_components(shape)
    assert R.largest_component(e)[40:45, 30:35].all() and int(R.largest_component(e).sum()) == 25


@pytest.mark.parametrize("shape", K.SHAPES)
def test_closed_forms_agree_with_border_following(shape):
    rng = np.random.default_rng(shape[0])
    imgs = [K.holes_image(shape), K.two_components(shape), K.diagonal_gap(shape), K.blob(shape)]
    imgs += [rng.random((12, 15)) < p for p in (0.4, 0.5, 0.6, 0.75) for _ in range(6)]
    seen = 0
    for a in imgs:
        lab, n = ndimage.label(a, structure=R.ONES3)
        for l in range(1, n + 1):
            comp = lab == l
            assert R.shoelace2(R.outer_contour(a, comp)) == R.cells_area2(ndimage.binary_fill_holes(comp, structure=R.CROSS), False)
        hl, keep = R.holes_of(a)
        for l in keep:
            hole = hl == l
            assert R.shoelace2(R.hole_contour(a, hole)) == R.cells_area2(ndimage.binary_fill_holes(hole, structure=R.ONES3), True)
            seen += 1
    assert seen > 10


@pytest.mark.parametrize("shape", K.SHAPES)
def test_flood_is_four_connected(shape):
    a = K.diagonal_gap(shape)
    lab4, _ = ndimage.label(~a, structure=R.CROSS)
    lab8, _ = ndimage.label(~a, structure=R.ONES3)
    assert (lab4 == lab4[0, 0]).sum() == 66 and (lab8 == lab8[0, 0]).sum() > 1000


def test_chamfer_is_the_two_pass_result_on_a_small_image():
    rng = np.random.default_rng(5)
    m = rng.random((17, 23)) < 0.8
    d = R.chamfer_fixed(m).astype(np.int64)
    ref = np.where(m, R.DIST_INF, 0).astype(np.int64)
    H, W = m.shape
    fwd = [(dy, dx, w) for dy, dx, w in R._MOVES if dy < 0 or (dy == 0 and dx < 0)]
    for moves, ys, xs in ((fwd, range(H), range(W)),
                          ([(-dy, -dx, w) for dy, dx, w in fwd], range(H - 1, -1, -1), range(W - 1, -1, -1))):
        for y in ys:
            for x in xs:
                for dy, dx, w in moves:
                    if 0 <= y + dy < H and 0 <= x + dx < W:
                        ref[y, x] = min(ref[y, x], ref[y + dy, x + dx] + w)
    assert np.array_equal(d, ref)
    assert R.dist_float(np.array([[3 * 65536 - 1]], np.int32))[0, 0] < 3.0


@pytest.mark.parametrize("shape", K.SHAPES)
def test_get_mask_branches(shape):
    m, branch, shrink = R.get_mask(K.closed_sketch(shape))
    assert branch == "closed-silhouette" and shrink == 4
    m0, branch0, shrink0 = R.get_mask(K.closed_sketch(shape), safety_margin=10)
    assert branch0 == "closed-silhouette" and shrink0 == 0 and m0.sum() > m.sum()
    mo, brancho, _ = R.get_mask(K.open_sketch(shape))
    assert brancho == "open-curve"
    assert mo[24:28, 24:28].all() and not mo[44, 44]           # the 8 x 8 hole is filled, the 5 x 5 one is not
    lab, keep = R.holes_of(R.dilate(K.open_sketch(shape) < 128, 3, 1))
    areas = sorted(R.contour_area(R.hole_contour(R.dilate(K.open_sketch(shape) < 128, 3, 1), lab == l)) for l in keep)
    assert areas[0] < 50 <= areas[1]


@pytest.mark.parametrize("shape", K.SHAPES)
def test_bbox_slicing_and_channel_swap(shape):
    masks, rgb = K.overlap_masks(shape), K.coloured_sketch(shape)
    assert R.mask_to_bbox(masks[0]) == [10, 10, 40, 30]
    assert [R.overlap_list(masks, i) for i in range(4)] == [[], [], [], [0]]
    a = R.assemble(rgb, masks, 3)
    assert tuple(a["sketch_layer"][15, 18]) == (90, 30, 200)                   # saved as it is: R and B swapped
    assert tuple(R.composite(np.zeros_like(rgb), a["sketch_layer"], a["original_sketch_mask"])[15, 18]) == (200, 30, 90)
    assert a["edit_mask"].any() and not a["edit_mask"][masks[3] > 0].any()
    x1, y1, x2, y2 = R.mask_to_bbox(masks[3])
    ys, xs = np.nonzero(a["edit_mask"])
    assert xs.max() < x2 and ys.max() < y2                                     # mask 3's own box is sliced the same way
    assert a["debug_vis"][a["edit_mask"]].tolist() == [[0, 0, 255]] * int(a["edit_mask"].sum())
