"""tests/mask_handoff_ref.py on the CPU: (a) its statement of the cleanup and of the sketch IoU counts equals
oracle/refine_ref.py (scipy's morphology, the reference's own committed outputs), (b) the inputs
tests/test_mask_handoff_ops_gpu.py feeds the kernels contain what they are meant to contain and stay, by the reference
alone, within the run bound that sizes the kernel's workspace, (c) on those inputs the reference tells every planted
mistake from the right answer."""
import glob
from pathlib import Path

import numpy as np
import pytest

import mask_handoff_ref as R
from oracle import refine_ref as O

GOLD = sorted(glob.glob(str(Path(__file__).resolve().parent / "golden" / "refine_*.npz")))


# ---------------------------------------------------------------------------------------------------------------
# (a) pinned to the oracle
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hw", R.CLOSE_SHAPES, ids=lambda hw: f"{hw[0]}x{hw[1]}")
def test_closing_equals_scipys_at_every_k_of_the_grid(hw):
    for k in R.CLOSE_KS:
        for kind in ("noise", "edge"):
            case = R.cleanup_case(f"close {kind} {hw[0]}x{hw[1]} k={k}")
            for m in case.masks:
                assert np.array_equal(R.close(m > 127, k), O.morph_close_rect(m > 127, k)), (kind, k)


def test_closing_equals_scipys_on_the_planted_cases():
    for name in R.SMALL_CLEANUP_CASES:
        if name.startswith("close") and not name.startswith(("close noise", "close edge")):
            case = R.cleanup_case(name)
            for m in case.masks:
                assert np.array_equal(R.close(m > 127, case.k), O.morph_close_rect(m > 127, case.k)), name


def test_cleanup_equals_clean_up_mask_on_the_grid():
    """The oracle has no parameters: the masks of every case, with the closing size and the thresholds it would use."""
    for name in R.SMALL_CLEANUP_CASES:
        for m in R.cleanup_case(name).masks:
            assert np.array_equal(R.cleanup(m, O.calculate_kernel_size(m.shape)), O.clean_up_mask(m)), name


@pytest.mark.parametrize("hw", [(200, 333), (333, 517)], ids=lambda hw: f"{hw[0]}x{hw[1]}")
def test_cleanup_equals_clean_up_mask_on_blobs(hw):
    """Closing sizes 5 and 9 with components on both sides of the area and of the aspect threshold."""
    from scipy import ndimage
    rs = np.random.RandomState(hw[1])
    for _ in range(3):
        f = ndimage.gaussian_filter(rs.standard_normal(hw), sigma=rs.uniform(2, 8))
        m = R._u8((f > np.quantile(f, rs.uniform(0.6, 0.95))) | (rs.rand(*hw) < 0.002))
        want = O.clean_up_mask(m)
        assert np.array_equal(R.cleanup(m, O.calculate_kernel_size(hw)), want)
        assert 0 < want.sum() < (R.cleanup(m, O.calculate_kernel_size(hw), -1) > 0).sum() * 255     # some dropped, some kept


@pytest.mark.parametrize("path", GOLD[:2], ids=lambda p: Path(p).stem)
def test_cleanup_reproduces_the_references_committed_outputs(path):
    g = np.load(path)
    h, w = (int(v) for v in g["hw"])
    unpack = lambda a: np.unpackbits(a, axis=-1)[..., :w].astype(bool)
    masks, cleaned = unpack(g["masks"]), unpack(g["masks_cleaned"])
    assert len(masks) >= 2 and (masks != cleaned).any()
    got = R.cleanup(R._u8(masks), O.calculate_kernel_size((h, w)))
    assert np.array_equal(got > 0, cleaned) and set(np.unique(got)) <= {0, 255}


def test_two_golden_sets_exist():
    assert len(GOLD) >= 2


def test_sketch_iou_counts_equal_the_oracles_sets():
    H, W, n = 37, 70, 4
    rgb, masks = R.count_sketch(H, W), R.count_masks(n, H, W)
    got = R.sketch_iou_counts(masks, rgb)
    S = O.sketch_pixels(rgb)
    assert np.array_equal(R.pil_luma(rgb), O.pil_luma(rgb)) and 0 < S.sum() < H * W
    for i in range(n):
        for j in range(n):
            a, b = np.logical_and(masks[i] > 0, S), np.logical_and(masks[j] > 0, S)
            assert got[i, j].tolist() == [int((a & b).sum()), int((a | b).sum())]


def test_pillow_agrees_on_the_palette():
    from PIL import Image
    pal = R.sketch_palette()
    assert np.array_equal(np.asarray(Image.fromarray(pal[None]).convert("L"))[0], R.pil_luma(pal))


# ---------------------------------------------------------------------------------------------------------------
# (b) the inputs do their work
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(R.CLEANUP_CASES))
def test_closed_images_stay_within_the_run_bound(name):
    """A condition, not a measurement: the GPU test asserts that the overflow flag stays 0, and that has to be true of
    the reference alone."""
    case = R.cleanup_case(name)
    W = case.masks.shape[2]
    assert W >= 8 and max(case.masks.shape[1:]) <= 16383
    for m in case.masks:
        assert R.max_runs_per_row(R.close(m > 127, case.k)) <= R.run_bound(W, case.k), name


def test_the_closest_approaches_to_the_run_bound():
    assert R.max_runs_per_row(R.stripes257()) == 129 and R.run_bound(257, 1) == 130
    wide = R.wide_masks() > 127
    assert R.max_runs_per_row(wide[0]) == 2081 and R.run_bound(4161, 1) == 2082
    long_rows = R.long_row_masks() > 127
    assert R.max_runs_per_row(R.close(long_rows[1], 3)) == 4096
    one_run = R.close(long_rows[2], 3)                          # the gap of r + 1 = 2 against the right border stays
    assert one_run[:, :16381].all() and not one_run[:, 16381:].any()


def test_grid_reaches_r_beyond_the_image_and_both_scan_widths():
    rs = [k // 2 for k in R.CLOSE_KS]
    assert {1, 2} <= set(rs)
    assert any(r >= H for r in rs for H, _ in R.CLOSE_SHAPES) and any(r >= W for r in rs for _, W in R.CLOSE_SHAPES)
    ws = [W for _, W in R.CLOSE_SHAPES]
    assert any(W <= 256 for W in ws) and any(256 < W <= 512 for W in ws)          # per = 1 and per = 2 of the row scan
    assert any(H > 128 for H, _ in R.CLOSE_SHAPES) and any(H == 128 for H, _ in R.CLOSE_SHAPES)
    edge = R.cleanup_case("close edge 40x65 k=3").masks
    assert not edge[0].any() and (edge[1] == 255).all() and set(np.unique(edge[2])) == set(R.MASK_BYTES.tolist())


@pytest.mark.parametrize("k", R.GAP_KS)
def test_gap_line_closes_as_stated(k):
    r = k // 2
    line, want = R.gap_line(k), R.gap_line_closed(k)
    assert np.array_equal(R.close(line[None].repeat(3, 0), k)[1], want)
    assert want[:r].all() and want[r + 3:r + 3 + 2 * r].all()                      # border gap r, interior gap 2 r: closed
    assert not want[3 * r + 6:5 * r + 7].any() and not want[-(r + 1):].any()       # interior 2 r + 1, border r + 1: open
    masks = R.gap_masks(k) > 127
    closed = np.stack([R.close(m, k) for m in masks])
    assert np.array_equal(closed[1], closed[0].T) and np.array_equal(closed[0][0], want)
    assert np.array_equal(closed[2], np.outer(want, want[::-1])) and (closed != masks).any()


def test_seam_pixels_and_corners():
    case = R.cleanup_case("close seam pixels k=5")
    m = case.masks > 127
    assert m.shape[1] == 129 and m[0, 127].sum() == 3 and m[1, 128].sum() == 3
    closed = np.stack([R.close(x, 5) for x in m])
    grown = m[0].copy()
    grown[128] = m[0, 127]                                      # one clear row (<= r) against the bottom border: closes
    assert np.array_equal(closed[0], grown) and np.array_equal(closed[1], m[1])     # on the border: closes to itself
    assert closed[2][123:129, 40].all() and not closed[2][123:128, 60].any()         # gap 2 r closes over the seam, 2 r + 1 not
    assert closed[2][127:129, 10:14].sum() > 2
    for x in R.cleanup_case("close corners 33x64 k=11").masks > 127:
        assert np.array_equal(R.close(x, 11), x)


def test_keep_blocks_meet_the_rule_at_its_boundaries():
    from scipy import ndimage
    m = R.keep_mask()
    assert ndimage.label(m, structure=np.ones((3, 3), bool))[1] == len(R.KEEP_BLOCKS)       # no two blocks touch
    assert m[0].any() and m[-1].any() and m[:, 0].any() and m[:, -1].any()
    assert R.keep_block("22x23-5").sum() == 501 and R.keep_block("22x23-6").sum() == 500 and R.keep_block("22x23").sum() == 506
    for b in ("22x23-5", "22x23-6"):
        ys, xs = np.nonzero(R.keep_block(b))
        assert ys.max() - ys.min() + 1 == 22 and xs.max() - xs.min() + 1 == 23
        assert ndimage.label(R.keep_block(b))[1] == 1

    def kept(params):
        out = R.cleanup(R._u8(m), 1, *R.KEEP_PARAMS[params]) > 0
        res = set()
        for b in R.KEEP_BLOCKS:
            blk = R.keep_block(b)
            assert out[blk].all() or not out[blk].any()
            if out[blk].any():
                res.add(b)
        assert not (out & ~m).any()
        return res

    assert kept("default") == {"22x23", "22x23-5", "10x12", "12x10", "1x2", "2x1"}
    assert kept("aspect_0") == {"22x23", "22x23-5"}
    assert kept("aspect_2") == {"22x23", "22x23-5"}
    assert kept("aspect_1.99999") == {"22x23", "22x23-5"}
    assert kept("area_0") == set(R.KEEP_BLOCKS) and kept("area_1e9") == {"10x12", "12x10", "1x2", "2x1"}


def test_labelling_cases_are_joined_where_they_say():
    from scipy import ndimage
    n8 = lambda b: ndimage.label(b, structure=np.ones((3, 3), bool))[1]
    n4 = lambda b: ndimage.label(b)[1]
    m, thr = R.staircase()
    assert n8(m) == 2 and n4(m) == 6 and m.sum() == 140 and thr == 69
    assert n8(m[:32]) == 2 and n8(m[:33]) == 2 and n4(m[31:33]) == 4 and n4(m[63:65]) == 4
    for H in (33, 65):
        m, thr = R.comb(H)
        assert n8(m) == 1 and n8(m[:-1]) == 21 and thr == m.sum() - 1 and (H - 1) % 32 == 0
    m, thr = R.checkerboard()
    assert m.shape == (66, 130) and n8(m) == 1 and n4(m) == m.sum() == thr + 1 and R.max_runs_per_row(m) == 65
    m = R.stripes257()
    assert n8(m) == 129 and m.shape[0] == 34
    for name, kept in (("label stripes257 whole", True), ("label stripes257 merged", False)):
        assert bool(R.cleanup_want(R.cleanup_case(name)).any()) == kept
    m, thr = R.spiral()
    assert n8(m) == 1 and thr == m.sum() - 1 and m.sum() > 900 and R.max_runs_per_row(m) >= 20
    assert not (m[:-1, :-1] & m[1:, 1:] & ~m[:-1, 1:] & ~m[1:, :-1]).any()        # one pixel wide, no diagonal contacts
    for name in R.SMALL_CLEANUP_CASES:
        if name.startswith("label") and name != "label stripes257 merged":
            case = R.cleanup_case(name)
            assert np.array_equal(R.cleanup_want(case), case.masks), name          # kept whole <=> merged correctly


def test_wide_and_tall_cases():
    wide = R.wide_masks() > 127
    assert wide.shape == (3, 6, 4161) and (4161 + 63) // 64 == 66
    assert wide[1, 1, 4095] and wide[1, 1, 4096] and not wide[1, 1, 4094] and wide[1, 4, 4032:].all()
    assert wide[1, 5, 4096] and not wide[1, 5, 4094] and wide[2, 3, 4094:4098].all()
    for name in ("wide 6x4161 k=1 all", "wide 6x4161 k=1 area 6"):
        want = R.cleanup_want(R.cleanup_case(name)) > 0
        assert want.any() and (name.endswith("all")) == bool(np.array_equal(want, wide))
    assert R.long_row_masks().shape == (3, 3, 16383) and R.tall_masks().shape == (3, 16383, 8)
    tall = R.cleanup_case("tall 16383x8 k=3")
    want = R.cleanup_want(tall) > 0
    assert want[2][:, 1].all() and 0 < want[0].sum() and (want[1] != R.close(tall.masks[1] > 127, 3)).any()


@pytest.mark.parametrize("hw", R.COUNT_SHAPES, ids=lambda hw: f"{hw[0]}x{hw[1]}")
def test_count_inputs_hold_the_threshold_colours_and_every_mask_byte(hw):
    H, W = hw
    luma = R.pil_luma(R.sketch_palette())
    assert luma[0] == 249 and luma[1] == 250 and {249, 250, 251, 255, 0} <= set(luma.tolist())
    assert R.pil_luma(np.array(R.TRUNCATION_COLOUR, np.uint8)) == 250
    assert R.pil_luma(np.array(R.TRUNCATION_COLOUR, np.uint8), truncated=True) == 249
    if H * W == 1:
        assert [int(R.pil_luma(R.count_sketch(1, 1, rot))[0, 0]) for rot in (0, 1)] == [249, 250]
    else:
        l = R.pil_luma(R.count_sketch(H, W))
        assert (l == 249).any() and (l == 250).any()
    if H * W >= 64:
        assert set(np.unique(R.count_masks(2, H, W))) == set(R.MASK_BYTES.tolist())
        assert (R.count_sketch(H, W) == np.array(R.TRUNCATION_COLOUR, np.uint8)).all(-1).any()
    assert R.count_masks(1, H, W)[0, -1, -1] != 0


def test_count_shapes_give_the_word_counts_they_are_there_for():
    assert [(H * W + 63) // 64 for H, W in R.COUNT_SHAPES] == [1, 1, 1, 2, 256, 256, 256, 257]
    assert 16385 % 64 == 1 and (127 * 129) % 64 != 0 and (5 * 13 + 63) // 64 % 4 != 0 and R.COUNT_NS == [1, 2, 5, 33]


def test_nms_case_drops_a_box_in_the_filter_and_has_decisions_to_make():
    rgb, masks, boxes, scores = R.nms_case()
    assert rgb.shape == R.NMS_HW + (3,) and len(masks) == 6
    kept = O.filter_full_or_empty_bbox(O.png_gray(rgb), boxes)
    assert kept.tolist() == [0, 1, 3, 4, 5, 6]                                   # filtered index != original from box 3 on
    cleaned = R.cleanup(masks, O.calculate_kernel_size(R.NMS_HW))
    res = [O.sketch_nms(rgb, boxes, scores, list(cleaned), t).tolist() for t in R.NMS_THRESHOLDS]
    assert all(0 < len(r) < 6 for r in res) and len({tuple(r) for r in res}) > 1, res
    shifted = [O.sketch_nms(rgb, boxes, scores, list(np.roll(cleaned, 1, axis=0)), t).tolist() for t in R.NMS_THRESHOLDS]
    assert shifted != res                                                        # which mask goes with which box matters


# ---------------------------------------------------------------------------------------------------------------
# (c) every planted mistake changes the result of a named case
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("wrong", R.MISTAKES_CLEANUP)
def test_cleanup_cases_catch_the_planted_mistake(wrong):
    caught = []
    for name in R.SMALL_CLEANUP_CASES:
        case = R.cleanup_case(name)
        if not np.array_equal(R.cleanup_want(case, wrong), R.cleanup_want(case)):
            caught.append(name)
    print(f"{wrong}: caught by {len(caught)} cases, first: {caught[:3]}")
    assert caught, wrong


@pytest.mark.parametrize("wrong", R.MISTAKES_COUNTS)
def test_count_cases_catch_the_planted_mistake(wrong):
    caught = []
    for H, W in R.COUNT_SHAPES:
        for n in (1, 2):
            for rot in ((0, 1) if H * W == 1 else (0,)):
                rgb, masks = R.count_sketch(H, W, rot), R.count_masks(n, H, W)
                if not np.array_equal(R.sketch_iou_counts(masks, rgb, wrong), R.sketch_iou_counts(masks, rgb)):
                    caught.append(f"{H}x{W} n={n} rot={rot}")
    print(f"{wrong}: caught by {len(caught)} cases, first: {caught[:3]}")
    assert caught, wrong
