"""The case lists of tests/amg_cases.py have power: for each RLE, small-region and NMS list a planted variant of
tests/amg_ref.py gives a result that differs from the true one on at least one case, and the stats geometries are valid
argument sets that reach the paths they are named for.  No GPU: a reviewer can check the edge suite
(tests/test_amg_edges_gpu.py) from here."""
import numpy as np
import pytest
import torch

import amg_cases as C
import amg_ref as R


# ------------------------------------------------------------------------------------------------ stats geometries
def _bands(crop_hw, xy0, orig_hw):
    y0, ch = xy0[1], crop_hw[0]
    return y0 // 64, (y0 + ch - 1) // 64


def test_stats_geometries_are_valid_and_reach_the_paths():
    rows_two_trips = one_band_inside = starts_on_line = ends_on_line = 0
    heights, forms_x0, forms_x1 = set(), set(), set()
    for crop_hw, xy0, orig_hw in C.STATS_GEOMS:
        (ch, cw), (x0, y0) = crop_hw, xy0
        oh, ow = orig_hw or crop_hw
        in_h, in_w = C.stats_input_hw(crop_hw)
        assert ch > 0 and cw > 0 and x0 >= 0 and y0 >= 0 and x0 + cw <= ow and y0 + ch <= oh
        assert 0 < in_h <= 1024 and 0 < in_w <= 1024 and max(in_h, in_w) == 1024
        assert orig_hw is not None or (x0, y0) == (0, 0)
        heights.add(oh)
        b0, b1 = _bands(crop_hw, xy0, orig_hw)
        rows_two_trips += cw % 4 == 0 and cw > 1024
        one_band_inside += b0 == b1 and y0 % 64 != 0 and (y0 + ch) % 64 != 0 and orig_hw is not None
        starts_on_line += y0 % 64 == 0 and y0 > 0
        ends_on_line += (y0 + ch) % 64 == 0 and y0 + ch < oh
        if orig_hw is not None:
            if x0 == 0:
                forms_x0.add(cw % 4 == 0)
            if x0 + cw == ow:
                forms_x1.add(cw % 4 == 0)
    assert rows_two_trips >= 1 and one_band_inside >= 1 and starts_on_line >= 1 and ends_on_line >= 1
    assert {63, 64, 65} <= heights
    assert forms_x0 == {True, False} and forms_x1 == {True, False}
    widths = {g[0][1] for g in C.STATS_GEOMS}
    assert {1, 3, 4} <= widths and any(g[0][0] == 1 for g in C.STATS_GEOMS)
    # a crop with one row on each side of a band line, one exactly on an aligned band, one ending with the frame
    assert any(g[1][1] == 63 and g[0][0] == 2 for g in C.STATS_GEOMS)
    assert any(g[1][1] % 64 == 0 and g[0][0] == 64 and g[2] is not None for g in C.STATS_GEOMS)
    assert any(g[2] is not None and g[1][1] + g[0][0] == g[2][0] for g in C.STATS_GEOMS)


def test_stats_input_hw_is_the_oracles():
    from oracle import sam_ref
    for crop_hw, _, _ in C.STATS_GEOMS:
        assert C.stats_input_hw(crop_hw) == sam_ref.preprocess_shape(crop_hw[0], crop_hw[1], 1024)


def test_ramps_peak_at_their_corner():
    for (b, r) in C.RAMP_CORNERS:
        m = C.ramp(b, r)
        assert (m == m.max()).sum() == 1 and m[255 * b, 255 * r] == m.max()
        assert torch.equal(m, m.round())
    low = C.stats_low("ramps", 3)
    assert low.shape == (5, 256, 256) and C.stats_low("noise", 3).shape == (5, 256, 256)


def test_tie_thresholds_hit_logits_in_float32():
    lg = C.smooth_noise(4, 1, 40, 40)[0]
    thr, off, a, b = C.tie_thresholds(lg)
    assert (lg == np.float32(thr + off)).any() and (lg == np.float32(thr - off)).any() and a > b
    assert (lg == C.second_largest(lg)).sum() >= 1 and (lg > C.second_largest(lg)).sum() == 1


# ------------------------------------------------------------------------------------------------ planes
@pytest.mark.parametrize("shape", C.RSR_SHAPES + C.RLE_SHAPES[:3])
def test_planes_round_trip(shape):
    H, W = shape
    masks, _ = C.rle_masks(H, W)
    planes = C.pack_planes(masks)
    assert planes.shape == (len(masks), W, -(-H // 64)) and planes.dtype == torch.int64
    assert torch.equal(C.unpack_planes(planes, H), masks)


# ------------------------------------------------------------------------------------------------ RLE
def _rle_variant(masks, wrong):
    out = []
    for r, m in zip(R.mask_to_rle(masks.transpose(1, 2) if wrong == "row_major" else masks), masks):
        c = list(r["counts"])
        if wrong == "no_leading_zero" and c[0] == 0:
            c = c[1:]
        out.append(c)
    return out


def test_rle_cases_reach_their_regimes():
    words = sorted(W * -(-H // 64) for H, W in C.RLE_SHAPES)
    assert {255, 256, 257, 513} <= set(words) and words[0] == 1
    assert {(H - 1) & 63 for H, _ in C.RLE_SHAPES} >= {0, 62, 63}
    for H, W in C.RLE_SHAPES:
        masks, names = C.rle_masks(H, W)
        rles = R.mask_to_rle(masks)
        for name, m, r in zip(names, masks, rles):
            assert np.array_equal(R.rle_to_mask(r), m.numpy()), name
        alt0, alt1 = rles[names.index("alt0")]["counts"], rles[names.index("alt1")]["counts"]
        assert alt0 == [1] * (H * W) and alt1 == [0] + [1] * (H * W)          # every position a change
        if "one_run" in names:
            assert rles[names.index("one_run")]["counts"] == [3 * H, (W - 6) * H, 3 * H]
        sel = C.rle_select(len(masks))
        assert sel[0] == sel[1] and sel[1:] == sorted(sel[1:], reverse=True)


@pytest.mark.parametrize("wrong", ["no_leading_zero", "row_major"])
def test_rle_cases_catch(wrong):
    caught = []
    for H, W in C.RLE_SHAPES:
        masks, names = C.rle_masks(H, W)
        true = [r["counts"] for r in R.mask_to_rle(masks)]
        caught += [f"{H}x{W}:{n}" for n, t, v in zip(names, true, _rle_variant(masks, wrong)) if t != v]
    print(wrong, len(caught), caught[:6])
    assert caught


# ------------------------------------------------------------------------------------------------ small regions
def _rsr_variant(mask, area_thresh, mode, conn8=True, le=False, tie="first"):
    """amg_ref.remove_small_regions with its three rules as switches: connectivity, the compare with the area, and
    which of the equal largest islands stays (first / last in raster order of first pixels, or first in (x, y) order)."""
    from scipy import ndimage
    holes = mode == "holes"
    working = (holes ^ mask).astype(np.uint8)
    lab, n = ndimage.label(working, structure=np.ones((3, 3), dtype=np.int32) if conn8 else None)
    H, W = mask.shape
    yy, xx = np.mgrid[0:H, 0:W]
    key = (xx * H + yy) if tie == "xy" else (yy * W + xx)
    first = np.full(n + 1, key.size, dtype=np.int64)
    np.minimum.at(first, lab.ravel(), key.ravel())
    order = np.argsort(first[1:], kind="stable")
    remap = np.zeros(n + 1, dtype=np.int64)
    remap[order + 1] = np.arange(1, n + 1)
    regions = remap[lab]
    sizes = np.bincount(regions.ravel(), minlength=n + 1)[1:]
    small = [i + 1 for i, s in enumerate(sizes) if (s <= area_thresh if le else s < area_thresh)]
    if not small:
        return mask, False
    fill = [0] + small
    if not holes:
        fill = [i for i in range(n + 1) if i not in fill]
        if not fill:
            best = np.flatnonzero(sizes == sizes.max())
            fill = [int(best[-1] if tie == "last" else best[0]) + 1]
    return np.isin(regions, fill), True


def _rsr_all(fn):
    """{(shape, min_area, modes, name): (mask, changed)} over every case of every shape"""
    out = {}
    for H, W in C.RSR_SHAPES:
        for a, names, masks in C.rsr_cases(H, W):
            for modes in C.RSR_MODES:
                for name, m in zip(names, masks):
                    cur, ch = m.numpy(), False
                    for mode in modes:
                        cur, c = fn(cur, a, mode)
                        ch = ch or c
                    out[(H, W, a, modes, name)] = (cur, ch)
    return out


@pytest.fixture(scope="module")
def rsr_true():
    return _rsr_all(R.remove_small_regions)


def test_rsr_variant_base_is_the_reference(rsr_true):
    base = _rsr_all(_rsr_variant)
    assert base.keys() == rsr_true.keys() and len(base) > 1000
    for k, (m, c) in rsr_true.items():
        assert np.array_equal(base[k][0], m) and base[k][1] == c, k


def test_rsr_cases_reach_their_regimes():
    shapes = set(C.RSR_SHAPES)
    assert {(1, 1), (1, 70), (70, 1), (63, 5), (64, 5), (65, 5)} <= shapes
    for H, W in C.RSR_SHAPES:
        names = {n for _, ns, _ in C.rsr_cases(H, W) for n in ns}
        assert {"empty", "full", "one_pixel", "checker0", "checker1", "bern10", "bern50", "bern90"} <= names
        if H % 2 == 1 and H > 1:               # the run bound (H + 1) / 2 is met in column 0 of a checkerboard
            chk = dict(C.rsr_general(H, W))["checker0"].numpy()
            assert chk[:, 0].sum() == (H + 1) // 2
        if max(H, W) >= 20:
            assert {"islands_all", "island_3", "island_4", "island_5"} <= names
            areas = dict(C.rsr_areas(H, W))
            assert [int(areas[f"island_{n}"].sum()) for n in (3, 4, 5)] == [3, 4, 5] and C.RSR_A == 4
            if min(H, W) >= 3:
                for n in (3, 4, 5):
                    hole = areas[f"hole_{n}"].numpy()
                    assert (~hole).sum() - n == _outer_background(hole), (H, W, n)
        if H >= 65 and W >= 4:
            ct = dict(C.rsr_general(H, W))["corner_touch"].numpy()
            assert ct[63, 1] and ct[64, 2] and not ct[63, 2] and not ct[64, 1]
    names = {n for H, W in C.RSR_SHAPES for n, _ in C.rsr_ties(H, W)}
    assert names == {"same_row", "upper_right_first", "three_equal"}
    assert 0 in C.RSR_MIN_AREAS and 1 in C.RSR_MIN_AREAS


def _outer_background(mask):
    """area of the background component(s) other than the one enclosed hole = everything but the hole"""
    from scipy import ndimage
    lab, n = ndimage.label(~mask, structure=np.ones((3, 3), dtype=np.int32))
    sizes = np.bincount(lab.ravel())[1:]
    return int(sizes.sum() - sizes.min()) if n > 1 else 0


@pytest.mark.parametrize("wrong", [dict(conn8=False), dict(le=True), dict(tie="last"), dict(tie="xy")],
                         ids=["conn4", "le_min_area", "last_largest", "tie_by_xy"])
def test_rsr_cases_catch(rsr_true, wrong):
    got = _rsr_all(lambda m, a, mode: _rsr_variant(m, a, mode, **wrong))
    caught = [k for k, (m, c) in rsr_true.items() if not np.array_equal(got[k][0], m) or got[k][1] != c]
    print(wrong, len(caught), caught[:4])
    assert caught
    if "tie" in wrong:                             # the tie masks are what catches a wrong tie rule
        assert any(k[4] in ("same_row", "upper_right_first", "three_equal") for k in caught)
    if wrong == dict(conn8=False):
        assert any(k[4].startswith("corner_touch") for k in caught) and any(k[4] == "diagonal" for k in caught)
    if wrong == dict(le=True):
        assert any(k[4] in ("islands_all", "island_4") for k in caught) and any(k[4] in ("holes_all", "hole_4") for k in caught)


def test_tie_cases_keep_the_first_in_raster_order(rsr_true):
    for H, W in C.RSR_SHAPES:
        for name, m in C.rsr_ties(H, W):
            out, changed = rsr_true[(H, W, 10 ** 6, ("islands",), name)]
            assert changed and out.sum() == 2 and m.sum() > 4, (H, W, name)
            ys, xs = np.nonzero(out)
            if name == "same_row":
                assert xs.tolist() == [0, 1] and ys[0] == ys[1] == min(1, H - 1)
            elif name == "upper_right_first":
                assert xs.tolist() == [4, 4] and ys.tolist() == [0, 1]
            elif H >= 12:
                assert ys.tolist() == [3, 4] and xs[0] == xs[1] == min(W - 1, 2)
            else:
                assert xs.tolist() == [3, 4] and ys.tolist() == [0, 0]


# ------------------------------------------------------------------------------------------------ NMS
def _nms_variant(boxes, scores, thr, wrong):
    b0 = boxes.float().numpy()
    s = scores.float().numpy().astype(np.float64)
    n = len(b0)
    if wrong == "unstable":                       # ties to the HIGHER index
        order = np.lexsort((-np.arange(n), -s))
    else:
        order = np.argsort(-s, kind="stable")
    b = b0[order]
    area = (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
    removed = np.zeros(n, dtype=bool)
    keep = []
    with np.errstate(invalid="ignore", divide="ignore"):
        for i in range(n):
            if removed[i]:
                if wrong != "suppressed_suppress":
                    continue
            else:
                keep.append(order[i])
            w = np.maximum(np.float32(0), np.minimum(b[i, 2], b[i + 1:, 2]) - np.maximum(b[i, 0], b[i + 1:, 0]))
            h = np.maximum(np.float32(0), np.minimum(b[i, 3], b[i + 1:, 3]) - np.maximum(b[i, 1], b[i + 1:, 1]))
            inter = w * h
            iou = inter / (area[i] + area[i + 1:] - inter)
            removed[i + 1:] |= (iou >= np.float32(thr)) if wrong == "ge" else (iou > np.float32(thr))
    return torch.as_tensor(np.asarray(keep, dtype=np.int64))


@pytest.fixture(scope="module")
def nms_true():
    return {name: R.nms(b, s, thr) for name, b, s, thr in C.nms_cases()}


def test_nms_variant_base_is_the_reference(nms_true):
    for name, b, s, thr in C.nms_cases():
        assert torch.equal(_nms_variant(b, s, thr, None), nms_true[name]), name


def test_nms_cases_are_what_they_say(nms_true):
    cases = {name: (b, s, thr) for name, b, s, thr in C.nms_cases()}
    assert {len(cases[f"clusters_{n}_0.7"][0]) for n in (127, 128, 192, 193)} == {127, 128, 192, 193}
    for n in (127, 128, 192, 193):
        assert 5 < len(nms_true[f"clusters_{n}_0.3"]) < len(nms_true[f"clusters_{n}_0.7"]) < n
        kept = nms_true[f"equal_scores_{n}"]
        assert kept[0] == 0 and 5 < len(kept) < n and torch.equal(kept, kept.sort().values)
    assert len(nms_true["edges_thr0"]) == len(cases["edges_thr0"][0])           # shared edges: all kept
    assert len(nms_true["edges_equal_scores_thr0"]) == len(cases["edges_thr0"][0])
    assert 40 < len(nms_true["slivers_thr0"]) < len(cases["slivers_thr0"][0])
    for pos in C.CHAIN_POSITIONS:
        b, s, perm = C.chain_case(pos)
        order = np.argsort(-s.numpy().astype(np.float64), kind="stable")
        assert [int(perm[order[p]]) for p in pos] == list(pos) and torch.equal(b[order[list(pos)]], C.CHAIN)
        kept = nms_true[f"chain_{pos[0]}_{pos[1]}_{pos[2]}"].tolist()
        assert len(kept) == len(b) - 1 and order[pos[1]] not in kept and order[pos[2]] in kept and order[pos[0]] in kept
    assert (cases["negative"][0] < 0).any() and len(nms_true["negative"]) < 150
    inv = cases["inverted_0.5"][0]
    assert (inv[:, 2] < inv[:, 0]).sum() >= 40 and (inv[:, 3] < inv[:, 1]).sum() >= 15
    assert len({len(nms_true[f"inverted_{t}"]) for t in (0.5, 0.0, -0.5)}) == 3
    assert nms_true["iou_equals_thr"].tolist() == [0, 1, 2]


@pytest.mark.parametrize("wrong", ["ge", "unstable", "suppressed_suppress"])
def test_nms_cases_catch(nms_true, wrong):
    caught = [name for name, b, s, thr in C.nms_cases() if not torch.equal(_nms_variant(b, s, thr, wrong), nms_true[name])]
    print(wrong, caught)
    assert caught
    if wrong == "ge":
        assert {"edges_thr0", "iou_equals_thr"} <= set(caught)
    if wrong == "unstable":
        assert any(c.startswith("equal_scores") for c in caught)
    if wrong == "suppressed_suppress":
        assert all(f"chain_{p[0]}_{p[1]}_{p[2]}" in caught for p in C.CHAIN_POSITIONS)
