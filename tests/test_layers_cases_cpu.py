"""The inputs of the layer-assembly edge suite (tests/layers_cases.py, run on the GPU by tests/test_layers_edges_gpu.py)
on the CPU: that each generated plane reaches the branch it is named for, at the very seeds and shapes the GPU tests use,
and that exact equality against tests/layers_ref.py tells the listed mistakes apart.  A later edit of a generator that
loses an edge fails here.  No GPU."""
import numpy as np
import pytest
from scipy import ndimage

import layers_cases as K
import layers_ref as R

BIG = [s for s in K.EDGE_SHAPES if min(s) >= 64]
SEAM2 = [(161, 200), (200, 161)]


def _runs(row):
    r = np.concatenate([[False], row, [False]])
    return np.nonzero(r[1:] & ~r[:-1])[0]                  # the start columns


def _max_runs(plane):
    return max(len(_runs(row)) for row in plane)


# ---- the shapes and where each constructed plane exists ---------------------------------------------------------------------
def test_edge_shapes_are_the_named_edges():
    assert K.EDGE_SHAPES == [(1, 1), (1, 70), (33, 2), (64, 64), (128, 128), (65, 129), (161, 200), (200, 161), (3, 4200)]
    assert K.SHAPES == [(70, 130), (130, 70)]
    wp = {s: (s[1] + 63) // 64 for s in K.EDGE_SHAPES}
    assert wp[(3, 4200)] == 66 and wp[(64, 64)] == 1 and wp[(128, 128)] == 2 and wp[(65, 129)] == 3
    assert [s for s in K.EDGE_SHAPES if s[1] % 64 == 0] == [(64, 64), (128, 128)]           # no tail bits
    assert [s for s in K.EDGE_SHAPES if s[0] >= 161] == SEAM2                               # a wave's second seam: row 160
    assert [s for s in K.EDGE_SHAPES if s[0] > 128 and s[1] > 128] == SEAM2                 # an interior chamfer tile


def test_constructed_planes_exist_where_they_fit():
    fits = {name: [s for s in K.EDGE_SHAPES if f(s) is not None] for name, f in dict(
        comb=K.comb, comb_closed=lambda s: K.comb(s, True), serpentine=K.serpentine, rival=K.serpentine_with_rival,
        nested=K.nested_rings, threshold=K.threshold_holes, edge=K.edge_holes, diag=K.diag_islands, tie=K.tie_components,
        zero_tile=K.zero_tile).items()}
    wide = BIG + [(3, 4200)]
    assert fits["comb"] == fits["comb_closed"] == fits["serpentine"] == fits["rival"] == wide
    assert fits["nested"] == fits["threshold"] == fits["edge"] == fits["diag"] == fits["tie"] == fits["zero_tile"] == BIG


# ---- coverage facts -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_noise_planes_hold_rule_filled_holes_with_islands(seed):
    a = K.noise((161, 200), 0.5, seed)
    t = K.hole_table(a)
    filled_with_islands = [h for h in t if h["off_edge"] and h["islands"] and h["region2"] >= 100]
    assert len(filled_with_islands) >= 20
    assert 1 <= sum(h["undecided"] for h in t) <= 21                    # three such planes stay inside the 64 records


@pytest.mark.parametrize("shape", K.EDGE_SHAPES)
def test_every_fill_rule_call_has_undecided_holes_within_the_cap(shape):
    for call in K.fill_rule_calls(shape):
        assert 1 <= len(call) <= 3
        count = sum(h["undecided"] for p in call for h in K.hole_table(p))
        if shape in BIG:
            assert 1 <= count <= 64
        else:                                                # no room for a hole with an island two pixels off every edge
            assert count == 0 and min(shape) < 7


def test_hole_table_is_the_rule_of_the_restatement():
    """Filling every hole of the table that is off the edge with region2 >= 100 is fill_holes_not_touching_border."""
    for shape in [(64, 64), (65, 129)]:
        for call in K.fill_rule_calls(shape):
            for p in call:
                assert np.array_equal(_rule(p), R.fill_holes_not_touching_border(p))


def test_lane_strides_and_word_chunks_are_reached():
    for W in list(range(130, 260)) + [4200]:
        c = K.comb((3, W))
        assert _max_runs(c) > 64 and _max_runs(c) == (W + 1) // 2
        assert _max_runs(~K.comb((3, W), closed=True)) > 64
    for d, seed in ((0.3, 30), (0.5, 31), (0.62, 32)):
        a = K.noise((3, 4200), d, seed)
        for row in a:
            s = _runs(row)
            assert (s < 4096).sum() > 64 and (s >= 4096).sum() >= 10     # runs on both sides of word 64
    assert any(row[4095] and row[4096] for a in K.fill_all_planes((3, 4200)) + [~p for p in K.fill_all_planes((3, 4200))]
               for row in a)                                            # a run that crosses from chunk 0 into chunk 1
    # one component across every seam, first run in row 0
    for shape in BIG + [(3, 4200)]:
        s = K.serpentine(shape)
        assert ndimage.label(s, structure=R.CROSS)[1] == 1 and s[0, 0] and s[:shape[0] - 1].sum(axis=1).min() >= 1


@pytest.mark.parametrize("shape", BIG)
def test_threshold_edge_and_island_holes_are_what_they_claim(shape):
    H, W = shape
    a = K.threshold_holes(shape)
    lab, keep = R.holes_of(a)
    by_row = {}
    for l in keep:
        hole = lab == l
        by_row[int(np.nonzero(hole)[0][0])] = (R.contour_area(R.hole_contour(a, hole)), int(hole.sum()))
    want = {3: (50.0, 36), 8: (49.5, 37), 15: (50.0, 25), 18: (49.5, 25), 22: (50.0, 34), 29: (49.5, 33)}
    assert by_row == want
    t = {h["first"][0]: h for h in K.hole_table(a)}
    assert [t[r]["undecided"] for r in sorted(t)] == [False] * 4 + [True] * 2
    assert (t[22]["own2"], t[22]["region2"], t[29]["own2"], t[29]["region2"]) == (98, 100, 97, 99)
    out = R.fill_holes_not_touching_border(a)
    assert [bool(out[r, 4]) for r in sorted(want)] == [True, False, True, False, True, False]
    # the edges: a box at distance 1 from its side stays, at distance 2 it is filled
    e = K.edge_holes(shape)
    got = {h["box"]: h for h in K.hole_table(e)}
    boxes = K.edge_hole_boxes(shape)
    assert len(got) == len(boxes) == 8
    oe = R.fill_holes_not_touching_border(e)
    for x0, x1, y0, y1, d in boxes:
        assert min(x0, y0, W - 1 - x1, H - 1 - y1) == d and got[(x0, x1, y0, y1)]["region2"] == 158
        assert bool(oe[y0, x0]) == (d == 2) and got[(x0, x1, y0, y1)]["off_edge"] == (d == 2)
    assert sorted(b[4] for b in boxes) == [1] * 4 + [2] * 4
    for side in (lambda b: b[0], lambda b: W - 1 - b[1], lambda b: b[2], lambda b: H - 1 - b[3]):
        assert sorted(side(b) for b in boxes)[:2] == [1, 2]             # each side has its own pair
    # islands of two and three pixels that touch only at corners
    d = K.diag_islands(shape)
    td = K.hole_table(d)
    assert len(td) == 2 and all(h["undecided"] and h["own2"] == h["region2"] < 100 for h in td)
    counts = ndimage.label(_islands(d), structure=R.CROSS)[1], ndimage.label(_islands(d), structure=R.ONES3)[1]
    assert counts == (5, 2) and int(_islands(d).sum()) == 5              # five pixels, two islands
    # nested rings: an undecided hole inside a hole the rule fills, and one inside a hole that stays
    n = K.nested_rings(shape)
    tn = sorted(K.hole_table(n), key=lambda h: h["first"])
    assert [(h["pixels"], h["undecided"], h["off_edge"]) for h in tn] == [(40, False, True), (24, True, True),
                                                                          (40, False, False), (24, True, True)]
    assert tn[0]["own2"] >= 100 and tn[1]["own2"] == 92 and tn[1]["region2"] == 124
    on = R.fill_holes_not_touching_border(n)
    assert on[2:13, 2:13].all() and not on[H - 12, W - 12] and on[H - 10:H - 3, W - 10:W - 3].all()
    # ring_grid: k undecided holes, nothing else
    for k in (40, 64, 65):
        tk = K.hole_table(K.ring_grid(k))
        assert len(tk) == k and all(h["undecided"] and h["own2"] == 92 for h in tk)


def _islands(mask):
    """Foreground pixels enclosed by a hole."""
    lab, keep = R.holes_of(mask)
    out = np.zeros_like(mask)
    for l in keep:
        hole = lab == l
        out |= ndimage.binary_fill_holes(hole, structure=R.ONES3) & ~hole
    return out


@pytest.mark.parametrize("shape", BIG)
def test_tie_components_have_equal_contour_areas(shape):
    a = K.tie_components(shape)
    lab, n = ndimage.label(a, structure=R.ONES3)
    assert n == 3
    facts = sorted((int(np.flatnonzero(lab == l)[0]), R.shoelace2(R.outer_contour(a, lab == l)), int((lab == l).sum()))
                   for l in range(1, 4))
    assert [f[1] for f in facts] == [24, 24, 24] and [f[2] for f in facts] == [26, 34, 20]
    W = shape[1]
    assert facts[1][0] // W == facts[2][0] // W == 8 and facts[1][0] < facts[2][0]      # the U, then the block, in one row
    assert a[8, 15] and not a[8, 12:15].any()                                            # the U's right arm comes after the block
    got = R.largest_component(a)
    assert got[8:12, 7:12].all() and int(got.sum()) == 20
    r = K.serpentine_with_rival(shape)
    lab, n = ndimage.label(r, structure=R.ONES3)
    assert n == 2
    areas = [R.shoelace2(R.outer_contour(r, lab == l)) for l in (1, 2)]
    assert areas[0] == areas[1] == 2 * len(range(1, shape[0] - 1, 2)) and lab[0, 0] == 1
    assert np.array_equal(R.largest_component(r), lab == 2)


@pytest.mark.parametrize("shape", K.EDGE_SHAPES)
def test_largest_inputs_have_no_enclosed_background(shape):
    planes = K.largest_planes(shape)
    assert len(planes) >= 5 and not planes[-1].any()
    for p in planes:
        assert R.holes_of(p)[1] == []
    if shape in SEAM2:                                     # many components, and rows of more than 64 runs
        assert ndimage.label(planes[0], structure=R.ONES3)[1] > 50 and _max_runs(K.comb(shape)) > 64


def test_chamfer_inputs_reach_their_branches():
    for shape in SEAM2:
        names = [k for k, _ in K.chamfer_masks(shape)]
        assert names == ["solid3", "noise 0.8", "ones", "zeros", "zero tile"]
        m = dict(K.chamfer_masks(shape))
        assert R.chamfer_fixed(m["solid3"]).max() > 56 * 65536            # more than 7 launches of 8 moves
        assert m["ones"].all() and not m["zeros"].any() and not m["zero tile"][64:128, 64:128].any()
        assert m["zero tile"][48:64, 48:144].any() and m["zero tile"][128:144, 48:144].any()
        masks = np.stack(list(m.values()))
        sub, none, zero = (K.chamfer_strokes(masks, k) for k in ("subset", "empty", "on_zero"))
        assert not none.any() and not (sub & ~masks).any() and sub[0].sum() > 100 and not sub[3].any()
        assert [(z & ~mk).sum() for z, mk in zip(zero, masks)] == [1, 1, 0, 1, 1]
    assert [k for k, _ in K.chamfer_masks((3, 4200))] == ["solid3"]
    assert R.chamfer_fixed(K.solid3((3, 4200))).max() > 1000 * 65536


def test_sketches_reach_both_branches():
    for shape in [(64, 64), (161, 200)]:
        for params in K.BG_PARAM_SETS:
            branches = [R.get_mask(K.grey_of(p), **params)[1] for p in K.sketch_planes(shape)]
            assert branches == ["open-curve", "open-curve", "closed-silhouette"], (shape, params)
    for shape in [(1, 1), (33, 2), (3, 4200)]:
        assert [R.get_mask(K.grey_of(p))[1] for p in K.sketch_planes(shape)] == ["open-curve"] * 2


def test_object_masks_hold_the_box_edges():
    for shape in K.EDGE_SHAPES:
        H, W = shape
        m = K.object_masks(shape, 40, 0)
        assert not m[3].any() and (m[4] > 0).sum() == W and (m[5] > 0).sum() == H and len(K.object_masks(shape, 1, 1)) == 1
        x1, y1, x2, y2 = R.mask_to_bbox(m[0])
        assert not R.mask_within_bbox(m[6] > 0, (x1, y1, x2, y2)).any() and (m[6, y1:y2 + 1, x1:x2 + 1] > 0).any()
        assert not R.mask_within_bbox(m[7] > 0, (x1, y1, x2, y2)).any() and (m[7, y1:y2 + 1, x1:x2 + 1] > 0).any()
    masks, rgb = K.layer_masks((64, 64))
    assert all(m.any() for m in masks) and sum(len(R.overlap_list(masks, i)) for i in range(6)) >= 3


# ---- discrimination: each mistake changes the expected result of a GPU case ----------------------------------------------------
def _rule(mask, by_pixels=False, off=2, strict=False, islands=True):
    """The hole rule from K.hole_table, with the mistakes as switches."""
    H, W = mask.shape
    out = mask.copy()
    for h in K.hole_table(mask):
        x0, x1, y0, y1 = h["box"]
        a2 = 2 * h["pixels"] if by_pixels else (h["region2"] if islands else h["own2"])
        clear = x0 >= off and y0 >= off and x1 <= W - 1 - off and y1 <= H - 1 - off
        if clear and (a2 > 100 if strict else a2 >= 100):
            out[h["window"]] |= h["region"]
    return out


def _differs(wrong, right, planes):
    return any(not np.array_equal(wrong(p), right(p)) for p in planes)


def _rule_planes(shape):
    return [p for call in K.fill_rule_calls(shape) for p in call]


def test_hole_mistakes_change_an_expected_result():
    shape = (64, 64)
    planes = _rule_planes(shape)
    right = R.fill_holes_not_touching_border
    assert not _differs(_rule, right, planes)
    th, ed, ne = K.threshold_holes(shape), K.edge_holes(shape), K.nested_rings(shape)
    assert _differs(lambda p: _rule(p, by_pixels=True), right, [th])
    assert _differs(lambda p: _rule(p, off=1), right, [ed])
    assert not np.array_equal(_rule(th, strict=True), right(th))
    assert _differs(lambda p: _rule(p, islands=False), right, [ne]) and _differs(lambda p: _rule(p, islands=False), right, [th])
    # holes taken 8-connected
    fa = K.fill_all_planes(shape)
    assert _differs(lambda p: ndimage.binary_fill_holes(p, structure=R.ONES3), R.fill_enclosed_regions, fa)
    assert not np.array_equal(ndimage.binary_fill_holes(K.checkerboard(shape), structure=R.ONES3),
                              R.fill_enclosed_regions(K.checkerboard(shape)))

    def rule8(p):                                          # the rule on 8-connected holes
        lab, n = ndimage.label(~p, structure=R.ONES3)
        out = p.copy()
        for l in range(1, n + 1):
            hole = np.pad(lab == l, 1)
            if hole[1].any() or hole[-2].any() or hole[:, 1].any() or hole[:, -2].any():
                continue
            ys, xs = np.nonzero(hole[1:-1, 1:-1])
            region = ndimage.binary_fill_holes(hole, structure=R.ONES3)
            if min(xs.min(), ys.min()) > 1 and xs.max() < p.shape[1] - 2 and ys.max() < p.shape[0] - 2 \
                    and R.cells_area2(region, True) >= 100:
                out |= region[1:-1, 1:-1]
        return out
    assert _differs(rule8, right, planes[:3])


def test_tie_break_mistake_changes_an_expected_result():
    def first_wins(sil):
        lab, n = ndimage.label(sil, structure=R.ONES3)
        best, best_area = None, -1
        for l in range(1, n + 1):                         # labels come in raster order of their first pixels
            area = R.shoelace2(R.outer_contour(sil, lab == l))
            if area > best_area:
                best, best_area = lab == l, area
        return ndimage.binary_fill_holes(best, structure=R.CROSS)
    for shape in BIG:
        assert not np.array_equal(first_wins(K.tie_components(shape)), R.largest_component(K.tie_components(shape)))
        assert not np.array_equal(first_wins(K.serpentine_with_rival(shape)), R.largest_component(K.serpentine_with_rival(shape)))
    plain = K.largest_planes((64, 64))[0]
    assert np.array_equal(first_wins(plain), R.largest_component(plain))       # the variant is wrong in the tie only


def _flood(a):
    lab, _ = ndimage.label(~a, structure=R.CROSS)
    return ~(lab == lab[0, 0]) if not a[0, 0] else np.ones(a.shape, bool)


@pytest.mark.parametrize("shape", SEAM2)
def test_missing_seam_link_changes_an_expected_result(shape):
    def unlinked(a):                                       # rows 0 .. 159 and 160 .. never joined
        out = np.ones(a.shape, bool)
        out[:160] = _flood(a[:160])
        return out
    planes = K.flood_planes(shape)
    assert _differs(unlinked, _flood, planes)
    snake = ~K.serpentine(shape)
    assert not np.array_equal(unlinked(snake), _flood(snake)) and (~_flood(snake))[160:].any()

    def unlinked_largest(sil):
        top = sil.copy()
        top[160:] = False
        return R.largest_component(top)
    assert _differs(unlinked_largest, R.largest_component, [K.serpentine(shape), K.largest_planes(shape)[0]])


def test_chamfer_mistakes_change_an_expected_result():
    shape = (161, 200)
    m = dict(K.chamfer_masks(shape))

    def eight_moves(mask):
        d = np.pad(np.where(mask, R.DIST_INF, 0).astype(np.int64), 2, constant_values=R.DIST_INF)
        H, W = mask.shape
        for _ in range(8):
            new = d[2:-2, 2:-2].copy()
            for dy, dx, w in R._MOVES:
                np.minimum(new, d[2 + dy:2 + dy + H, 2 + dx:2 + dx + W] + w, out=new)
            d[2:-2, 2:-2] = new
        return d[2:-2, 2:-2].astype(np.int32)

    def outside_zero(mask):
        return R.chamfer_fixed(np.pad(mask, 2))[2:-2, 2:-2]
    assert not np.array_equal(eight_moves(m["solid3"]), R.chamfer_fixed(m["solid3"]))
    assert np.array_equal(eight_moves(m["noise 0.8"]), R.chamfer_fixed(m["noise 0.8"]))      # right where 8 moves suffice
    for k in ("solid3", "noise 0.8", "ones", "zero tile"):
        assert not np.array_equal(outside_zero(m[k]), R.chamfer_fixed(m[k])), k
    for s in K.EDGE_SHAPES:                                # even on the single pixel: INF, not 1
        assert not np.array_equal(outside_zero(np.ones(s, bool)), R.chamfer_fixed(np.ones(s, bool)))


@pytest.mark.parametrize("shape", [s for s in K.EDGE_SHAPES if s[0] > 1])
def test_wrapping_dilation_changes_an_expected_result(shape):
    def wrapped(a, k, it):                                 # the row end taken as joined to the next row's start
        assert k == 3
        H, W = a.shape
        for _ in range(it):
            f = np.concatenate([[False], a.ravel(), [False]])
            a = (f[1:-1] | f[:-2] | f[2:]).reshape(H, W) | np.pad(a, ((1, 0), (0, 0)))[:-1] | np.pad(a, ((0, 1), (0, 0)))[1:]
        return a
    noise, pix, ends = K.dilate_planes(shape)
    assert not np.array_equal(wrapped(ends, 3, 1), R.dilate(ends, 3, 1))
    mid = np.zeros(shape, bool)
    mid[shape[0] // 2, shape[1] // 2] = True
    if shape[1] > 2:
        assert np.array_equal(wrapped(mid, 3, 1), R.dilate(mid, 3, 1))
    for p in K.corner_pixels(shape):
        assert pix[p]
    H, W = shape
    assert {(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1)} <= set(K.corner_pixels(shape))
    cols = {x for _, x in K.corner_pixels(shape)}
    assert all({b - 1, b} <= cols for b in range(64, W, 64))


def test_band_pixels_sit_on_both_sides_of_the_band():
    for shape in BIG:
        for band in (1, 2, 3):
            flags = [R.touches_band(p, band) for p in K.band_planes(shape, band)]
            assert flags == [True] * 4 + [False] * 4 + [False]
        wide = min(shape) // 2 + 1                           # wider than half the image: every pixel lies in the band
        assert [R.touches_band(p, wide) for p in K.band_planes(shape, wide)] == [True] * 8 + [False]
