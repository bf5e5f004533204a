"""tests/refine_stage_ref.py on the CPU: (a) every restatement of an entry point of csrc/refine_stage.hip equals the
function of the same step in oracle/refine4_ref.py on random inputs, (b) the inputs tests/test_refine_stage_ops_gpu.py
feeds to the kernels contain what they are meant to contain, (c) on those inputs the reference tells the classic
mistakes apart from the right answer."""
import numpy as np
import pytest

import refine_stage_ref as R
from oracle import refine4_ref as O


def _label_masks(label, n):
    return [label == l for l in range(1, n + 1)]


# ---------------------------------------------------------------------------------------------------------------
# (a) pinned to the oracle
# ---------------------------------------------------------------------------------------------------------------
def test_pack_unpack_round_trip_and_layout():
    for W in (1, 63, 64, 65, 129):
        b = np.random.RandomState(W).rand(2, 3, W) < 0.5
        p = R.pack(b)
        assert p.shape == (2, 3, (W + 63) // 64) and p.dtype == np.uint64
        assert np.array_equal(R.unpack(p, W), b) and R.tail_is_clear(p, W)
        assert np.array_equal(R.unpack(p.view(np.int64), W), b)
    one = np.zeros((1, 130), bool)
    one[0, [0, 65, 129]] = True
    assert R.pack(one).tolist() == [[1, 2, 2]]
    assert not R.tail_is_clear(np.array([[1 << 40]], np.uint64), 40) and R.tail_is_clear(np.array([[1 << 39]], np.uint64), 40)


@pytest.mark.parametrize("seed", range(6))
def test_composite_and_relabel_clean_equal_composite_and_parse_masks(seed):
    rs = np.random.RandomState(seed)
    H, W, n = 37, 90, 7
    masks = list(R.random_masks(n, H, W, seed))
    masks[3] = masks[1] & (rs.rand(H, W) < 0.98)                 # nearly hidden behind an earlier mask: merged away
    masks[0][:2] = False                                         # the page is never covered completely
    order = [int(v) for v in rs.permutation(n)]
    if seed % 2:
        order[2] = -1
    by_rank = [masks[m] if m >= 0 else np.zeros((H, W), bool) for m in order]
    want, info = O.composite_and_parse_masks(by_rank, [[0, 0, 1, 1]] * n)
    label, hist = R.composite(masks, order, (H, W))
    assert hist.sum() == H * W and hist[0] > 0
    lut = np.zeros(256, np.uint8)
    for k, (pm, inf) in enumerate(zip(want, info)):
        r = inf["original_indices"][0]
        assert np.array_equal(label == r + 1, pm) and hist[r + 1] == pm.sum()
        lut[r + 1] = k + 1
    assert 0 < len(want) <= n
    got = R.relabel_clean(label, lut)
    for k, pm in enumerate(want):
        assert np.array_equal(got == k + 1, O.clean_delicate_mask(pm))
    assert np.array_equal(R.same_label_neighbours(lut[label]) > 1, got > 0)


@pytest.mark.parametrize("seed", range(4))
def test_grow_equals_refine_masks_with_watershed(seed):
    H, W = ((33, 70), (40, 129), (64, 64), (21, 200))[seed]
    rgb = R.random_rgb(H, W, seed)
    planes = R.sketch_planes(rgb)
    n = 9
    label = R.random_labels(H, W, seed, list(range(1, n + 1)) * 2)
    want = O.refine_masks_with_watershed(O.pil_luma(rgb), _label_masks(label, n))
    g = R.grow(label, planes)
    for l in range(1, n + 1):
        assert np.array_equal(g["grown"] == l, want[l - 1]), l
    assert not (g["grown"] > n).any()
    # the list is what refine_masks_with_boxes walks: np.where of the stroke pixels no grown mask claims
    ys, xs = np.where(~(O.pil_luma(rgb) > 250) & ~np.any(want, axis=0))
    assert g["count"] == len(ys) and np.array_equal(g["yx"], np.stack([ys, xs], 1))
    for l in range(1, n + 1):
        bb = O.compute_mask_bbox(want[l - 1])
        assert g["bbox"][l].tolist() == ([W, H, -1, -1] if bb is None else [int(v) for v in bb])


def test_grow_case_equals_refine_masks_with_watershed():
    label, planes = R.grow_case()
    want = O.refine_masks_with_watershed(np.where(planes[2], 0, 255).astype(np.uint8), _label_masks(label, 254))
    g = R.grow(label, planes)
    for l in range(1, 255):
        assert np.array_equal(g["grown"] == l, want[l - 1]), l


@pytest.mark.parametrize("seed", range(4))
def test_finalize_equals_create_unlabeled_mask(seed):
    H, W = ((9, 70), (30, 129), (16, 64), (5, 65))[seed]
    rs = np.random.RandomState(seed)
    rgb = R.random_rgb(H, W, seed)
    if seed < 2:                                                  # wide strokes, so that the opening leaves something
        rgb[rs.rand(H, W) < 0.8] = 10
    planes = R.sketch_planes(rgb)
    label = R.random_labels(H, W, seed, [1, 2, 3])
    assign = np.array([[rs.randint(H), rs.randint(W), rs.randint(1, 4)] for _ in range(5)], np.int32)
    lab, extra, cnt = R.finalize(label, assign, planes)
    want_lab = label.copy()
    want_lab[assign[:, 0], assign[:, 1]] = assign[:, 2]           # (no pixel twice for these seeds, checked below)
    assert len({(int(a), int(b)) for a, b, _ in assign}) == len(assign) and np.array_equal(lab, want_lab)
    out = O.create_unlabeled_mask(O.png_gray(rgb), _label_masks(lab, 3))
    if cnt:
        assert len(out) == 4 and np.array_equal(out[3] > 0, extra) and cnt == extra.sum()
    else:
        assert len(out) == 3
    if seed < 2:
        assert cnt > 0


@pytest.mark.parametrize("seed", range(5))
def test_pair_tables_equal_compute_major_overlap_matrix(seed):
    from inklayer_amd import refine_stage as S
    rs = np.random.RandomState(seed)
    H, W, n = 41, 150, 6
    rgb = R.random_rgb(H, W, seed)
    planes = R.sketch_planes(rgb)
    masks = list(R.random_masks(n, H, W, 10 + seed))
    masks[2] = np.zeros((H, W), bool)
    masks[2][5:30, 10:100] = rs.rand(25, 90) < 0.8
    masks[4] = masks[2] & (rs.rand(H, W) < 0.9)                  # a pair that overlaps by far more than 60 %
    boxes = []
    for m in masks:
        bb = O.compute_mask_bbox(m) or [0, 0, 5, 5]
        boxes.append([int(bb[0]) - 2, int(bb[1]), int(bb[2]) + 3, int(bb[3]) + 1 + int(rs.randint(0, 3))])
    boxes[4] = boxes[2]
    rect = S.overlap_rects(np.asarray(boxes, dtype=int), H, W)
    dil, pair, per, area = R.pair_tables(masks, planes, rect)
    binary = O.sketch_to_01binary(rgb[..., ::-1]).astype(bool)
    want = O.compute_major_overlap_matrix([m & binary for m in masks], bboxes=boxes, dilate_px=1)
    got = np.zeros((n, n), bool)
    for i in range(n):
        for j in range(i + 1, n):
            inter, a = int(pair[i, j, 1]), (int(per[i, 1]), int(per[j, 1]))
            got[i, j] = got[j, i] = bool(inter and a[0] and a[1] and inter / float(min(a)) >= 0.6)
    assert np.array_equal(got, want) and want[2, 4] and not want.all()
    luma = O.pil_luma(rgb)
    assert area == np.sum(luma < 250)
    for i in range(n):
        assert per[i, 0] == masks[i].sum() and per[i, 2] == np.sum(np.logical_and(masks[i] > 0, luma < 250))
        assert np.array_equal(dil[i], O.sk_dilate(masks[i] & binary, R.CROSS))
        for j in range(n):
            assert pair[i, j, 0] == np.sum(np.logical_and(masks[i], masks[j]))
    assert np.array_equal(pair, pair.transpose(1, 0, 2))


@pytest.mark.parametrize("top", [255, 253, 0])
def test_sketch_planes_equal_the_oracles_thresholds(top):
    rgb = R.random_rgb(23, 131, 3, top)
    assert rgb.max() == top
    pl = R.sketch_planes(rgb)
    luma = O.pil_luma(rgb)
    assert np.array_equal(pl[0], O.sketch_to_01binary(rgb[..., ::-1]) > 0)
    assert np.array_equal(pl[1], luma < 250) and np.array_equal(pl[2], ~(luma > 250))
    assert np.array_equal(pl[3], O.png_gray(rgb) < 250)
    if top == 0:
        assert pl.all()


def test_query_dists_equal_the_distance_transform():
    from scipy import ndimage
    label, q, _ = R.query_case()
    d2 = R.query_dists(label, q[:40])
    for l in (1, 63, 64, 128, 250, 254):
        e = ndimage.distance_transform_edt(label != l)
        assert np.array_equal(d2[:, l], np.rint(e[q[:40, 0], q[:40, 1]] ** 2).astype(np.int64))
    assert (d2[:, R.QUERY_ABSENT] == R.INT_MAX).all() and (d2[:, 0] == R.INT_MAX).all() and (d2[:, 255] == R.INT_MAX).all()


# ---------------------------------------------------------------------------------------------------------------
# (b) the generated inputs do their work
# ---------------------------------------------------------------------------------------------------------------
def test_threshold_palette_straddles_every_threshold():
    pal = R.threshold_palette()
    luma, gray = O.pil_luma(pal[None])[0], O.png_gray(pal[None])[0]
    assert {249, 250, 251} <= set(luma.tolist()) and {249, 250} <= set(gray.tolist())
    assert (luma != gray).any()                                  # triples for which the two grays disagree
    assert {126, 127, 128} <= set(pal[:, 2].tolist())
    for top in (255, 253):
        rgb = R.random_rgb(7, 129, 1, top)
        pl = R.sketch_planes(rgb)
        assert (pl[1] != pl[2]).any() and pl[1].any() and not pl[2].all()
        assert pl[0][rgb[..., 2] == 126].all() and (rgb[..., 2] == 127).any() and (rgb[..., 2] == 128).any()
        assert pl[0][rgb[..., 2] == 127].all() == (top == 255) and not pl[0][rgb[..., 2] == 128].any()


def test_grow_case_holds_the_50_and_51_pixel_components_and_both_kinds_of_label():
    label, planes = R.grow_case()
    g = R.grow(label, planes)
    sizes = g["closed_sizes"].tolist()
    assert 50 in sizes and 51 in sizes
    present = [int(l) for l in np.unique(label) if l]
    assert present == [1, 3, 7, 200, 254]
    assert g["flags"][3] == 1 and g["flags"][7] == 0 and g["flags"].sum() >= 1
    d2 = R.query_dists(label, np.argwhere(g["unl"]).astype(np.int32))
    assert ((d2 > 4) & (d2 <= 9)).any(1).any(), "no unlabeled pixel with a label at distance^2 in (4, 9]"
    assert ((d2 <= 4).sum(1) >= 2).any(), "no unlabeled pixel with two labels in reach"
    far = (d2.min(1) > 4) & (d2.min(1) <= 9)                      # reached by disk(3) only
    ys, xs = np.argwhere(g["unl"])[far].T
    assert (g["grown"][ys, xs] == 3).any() and (g["grown"][ys, xs] == 0).any()      # flagged grows, unflagged does not
    assert ((label > 0) & (g["grown"] == 0)).any()               # a labelled pixel off the strokes loses its label
    assert g["count"] > 0 and g["bbox"][254].tolist() != [200, 48, -1, -1] and g["bbox"][2].tolist() == [200, 48, -1, -1]


def test_relabel_case_has_0_1_and_2_same_label_neighbours_inside_and_on_the_border():
    L, drop, merge = R.relabel_case()
    H, W = L.shape
    border = np.zeros(L.shape, bool)
    border[[0, -1], :] = border[:, [0, -1]] = True
    for lut in (np.arange(256, dtype=np.uint8), drop, merge):
        M = lut[L]
        cnt = R.same_label_neighbours(M)
        for where in (border, ~border):
            for c in (0, 1, 2):
                assert ((cnt == c) & (M > 0) & where).any(), (c, where[0, 0])
    assert L.max() == 254 and (drop[L] == 0)[L == 3].all() and len(np.unique(merge[L])) < len(np.unique(L))
    assert (R.relabel_clean(L, merge) != R.relabel_clean(L, np.arange(256, dtype=np.uint8))).any()
    assert np.array_equal(R.relabel_clean(L, drop) > 0, R.same_label_neighbours(drop[L]) > 1)


def test_pair_rects_cover_the_word_boundaries():
    H, W = R.PAIR_RECTS_HW
    masks, planes, rect = R.pair_rects_case()
    rects = {tuple(int(v) for v in rect[i, j]) for i in range(6) for j in range(i + 1, 6)}
    assert rects == set(R.PAIR_RECTS) and len(R.PAIR_RECTS) == 15
    area = lambda r: max(r[1] - r[0], 0) * max(r[3] - r[2], 0)
    words = lambda r: (r[3] - 1) // 64 - r[2] // 64 + 1
    assert any(area(r) == 0 for r in rects) and (0, H, 0, W) in rects and any(area(r) == 1 for r in rects)
    assert any(area(r) > 1 and words(r) == 1 and r[2] % 64 and r[3] % 64 for r in rects)
    assert any(words(r) == 3 for r in rects)
    assert {63, 64, 65, 128} <= {r[2] for r in rects} and {63, 64, 65, 128} <= {r[3] for r in rects}
    assert all(0 <= r[0] <= r[1] <= H and 0 <= r[2] <= r[3] <= W for r in rects)
    assert np.array_equal(rect, rect.transpose(1, 0, 2))


def test_query_case_has_candidates_in_every_word_an_absent_one_and_a_nearest_pixel_in_another_row():
    label, q, cands = R.query_case()
    present = set(np.unique(label).tolist())
    assert present == set(range(255)) - {R.QUERY_ABSENT}
    assert {l >> 6 for l in cands[0]} == {0, 1, 2, 3} and R.QUERY_ABSENT in cands[0] and cands[1] == []
    w = R.candidate_words(cands)
    assert all((w[:, k] != 0).any() for k in range(4)) and not w[1].any()
    assert w[2].tolist() == [(1 << 1) | (1 << 63), 1 | (1 << 63), 1 | (1 << 63), 1 | (1 << 62)]
    qy, qx = q[0]
    ys, xs = np.nonzero(label == 250)
    d = (ys - qy) ** 2 + (xs - qx) ** 2
    assert (ys == qy).any() and ys[np.argmin(d)] != qy and R.query_dists(label, q[:1])[0, 250] == 25
    assert len(q) == 300 and all(all(1 <= l <= 254 for l in c) for c in cands)


def test_overflow_cases_have_more_than_65536_unlabeled_stroke_pixels():
    rgb = R.dark_sketch()
    planes = R.sketch_planes(rgb)
    assert planes.all() and planes[2].sum() == 90000 > 65536
    one = np.zeros((300, 300), np.uint8)
    one[100:140, 100:160] = 1                                    # the one mask of the whole-stage case
    g = R.grow(one, planes)
    assert g["count"] > 65536 and g["count"] < 90000 - 2400


def test_edge_sizes_reach_the_second_row_scan_pass_and_the_second_word_loop():
    hs, ws = [h for h, _ in R.EDGE_SIZES], [w for _, w in R.EDGE_SIZES]
    assert any(1024 < h <= 2048 for h in hs) and any(h > 2048 for h in hs) and any((w + 63) // 64 > 64 for w in ws)
    assert {1, 63, 64, 65, 129} <= set(ws)
    for H, W in R.EDGE_SIZES:
        if H > 1024:                                              # stroke pixels before and after every carry
            rows = np.nonzero((R.random_planes(H, W, 1)[2] & (R.random_labels(H, W, 2, [1, 2]) == 0)).any(1))[0]
            assert rows.min() < 1024 and rows.max() >= 1024 * (H // 1024)


# ---------------------------------------------------------------------------------------------------------------
# (c) the reference tells the classic mistakes apart
# ---------------------------------------------------------------------------------------------------------------
def _differs(a, b):
    return a.shape != b.shape or bool((a != b).any())


def test_reference_discriminates_the_classic_mistakes():
    # the row scan without the carry between its passes of 1024 rows
    plane = R.random_planes(1030, 70, 1)[2]
    n, yx = R.pixel_list(plane)
    ys, xs = np.where(plane)
    assert n == len(ys) and np.array_equal(yx, np.stack([ys, xs], 1))
    n_bad, yx_bad = R.pixel_list(plane, wrong="no_carry")
    assert n_bad != n and _differs(yx_bad, yx)
    assert np.array_equal(R.pixel_list(plane, cap=100)[1], yx[:100]) and R.pixel_list(plane, cap=100)[0] == n
    # a clip rectangle with an inclusive right edge
    masks, planes, rect = R.pair_rects_case()
    good, bad = R.pair_tables(masks, planes, rect)[1], R.pair_tables(masks, planes, rect, wrong="inclusive_right")[1]
    assert _differs(good[..., 1], bad[..., 1]) and np.array_equal(good[..., 0], bad[..., 0])
    # growth: >= 50, disk(2) for every label, the smallest label wins
    label, planes = R.grow_case()
    g = R.grow(label, planes)
    for wrong in ("ge_50", "disk2_always", "smallest_wins"):
        assert _differs(R.grow(label, planes, wrong=wrong)["grown"], g["grown"]), wrong
    assert _differs(R.grow(label, planes, wrong="ge_50")["flags"], g["flags"])
    # cleaning: cnt < 1
    L, drop, merge = R.relabel_case()
    for lut in (drop, merge):
        assert _differs(R.relabel_clean(L, lut, wrong="cnt_lt_1"), R.relabel_clean(L, lut))
    # the 2 x 2 dilation anchored down / right
    planes = R.random_planes(7, 129, 3)
    lab = R.random_labels(7, 129, 4, [1, 2])
    none = np.zeros((0, 3), np.int32)
    assert R.finalize(lab, none, planes)[2] > 0
    assert _differs(R.finalize(lab, none, planes, wrong="anchor_down_right")[1], R.finalize(lab, none, planes)[1])
    # luma < 250 in the place of <= 250
    rgb = R.random_rgb(7, 129, 1)
    assert _differs(R.sketch_planes(rgb, wrong="luma_lt_250")[2], R.sketch_planes(rgb)[2])


def test_finalize_case_reaches_the_borders_and_crosses_the_word_boundary():
    label, planes = R.finalize_case()
    un = planes[3] & (label == 0)
    op = O.sk_dilate(O.sk_erode(un, R.SQUARE3), R.SQUARE3)
    _, extra, cnt = R.finalize(label, np.zeros((0, 3), np.int32), planes)
    assert op[0, 0] and op[0, 129] and op[11].any() and cnt == extra.sum() > op.sum()      # opened up to three borders
    assert op[:, 63].any() and not op[:, 64].any() and extra[:, 64].any()                # a bit moves into the next word
    assert un[5:7, 20:40].all() and not extra[4:9, 22:38].any()                          # the thin stroke is opened away
    assert extra[3:10, 80:85].any() and not extra[3:10, 86:90].any()                     # claimed pixels stay out
    assert extra[3, 0:4].all() and extra[0:4, 3].all() and not extra[4, 0:5].any() and not extra[0:5, 4].any()   # one down, one right


def test_composite_cases_let_high_ranks_keep_pixels():
    import test_refine_stage_ops_gpu as T
    for hw in ((1030, 70), (2, 4100)):
        masks, order = T._composite_case(hw, 254, 50 + 254)
        label, hist = R.composite(masks, order, hw)
        assert len(np.unique(label)) > 150 and label.max() > 240 and -1 in order
        assert (np.stack([masks[m] for m in order if m >= 0]).sum(0) > 1).any()             # overlaps are decided
