"""The two entry points of csrc/refine.hip, ink_mask_cleanup and ink_mask_sketch_iou_counts, called as
ops.mask_cleanup / ops.mask_sketch_iou_counts and straight through the C ABI, against tests/mask_handoff_ref.py (pinned
to the oracle, and shown to tell the classic mistakes apart, by tests/test_mask_handoff_ref_cpu.py).  Every comparison
is exact: bytes and integer counts.  Every cleanup call also asserts that the workspace's overflow flag stayed 0.

What is covered where:
  closing alone (area_threshold = -1)   test_closing_grid (shapes x k x densities, empty / full masks, bytes 0 / 1 / 127 /
                                        128 / 255, r >= H, r >= W, W <= 256 and W > 256 of the row scan),
                                        test_closing_planted (the four gap widths in both axes, pixels at the 128-row
                                        seam of the column pass, corners)
  keep rule alone (k = 1)               test_keep_rule (blocks at the area and aspect boundaries, every parameter set)
  labelling (k = 1, aspect off)         test_labelling (diagonal joins over the row-block seams, joins by the last row,
                                        more than 64 runs per row, 129 runs against a bound of 130, a spiral)
  wide and tall                         test_wide_rows (66 words per row, 2081 runs per row), test_longest_row (W = 16383:
                                        64 KiB of dynamic LDS), test_tallest_image (H = 16383)
  C entry points                        test_cleanup_c_entry_*, test_counts_c_entry (poisoned scratch, guards, offsets)
  rejections                            test_cleanup_rejections
  sketch IoU counts                     test_sketch_iou_counts, test_counts_of_full_masks_are_the_stroke_count
  end to end                            test_sketch_nms_end_to_end
GPU box only."""
import ctypes as C

import numpy as np
import pytest
import torch

import mask_handoff_ref as R

pytestmark = pytest.mark.gpu

GUARD = 256                      # sentinel bytes on both sides of a guarded buffer
SENTINEL = 0xA5


def _up(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def run_cleanup(dev, case: R.Case):
    """ops.mask_cleanup on a case -> uint8 [n, H, W]; asserts the overflow flag."""
    from inklayer_amd import ops
    got = ops.mask_cleanup(_up(case.masks, dev), case.k, case.area_threshold, case.aspect_threshold)
    assert int(got._ink_overflow_flag.item()) == 0
    out = got.cpu().numpy()
    assert out.shape == case.masks.shape and set(np.unique(out)) <= {0, 255}
    return out


def check_case(dev, name):
    case = R.cleanup_case(name)
    got, want = run_cleanup(dev, case), R.cleanup_want(case)
    assert np.array_equal(got, want), (name, [int((g != w).sum()) for g, w in zip(got, want)])


# ---------------------------------------------------------------------------------------------------------------
# cleanup through the wrapper
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hw", R.CLOSE_SHAPES, ids=lambda hw: f"{hw[0]}x{hw[1]}")
def test_closing_grid(dev, hw):
    for k in R.CLOSE_KS:
        check_case(dev, f"close noise {hw[0]}x{hw[1]} k={k}")
        check_case(dev, f"close edge {hw[0]}x{hw[1]} k={k}")


@pytest.mark.parametrize("name", [n for n in R.SMALL_CLEANUP_CASES
                                  if n.startswith("close") and not n.startswith(("close noise", "close edge"))])
def test_closing_planted(dev, name):
    check_case(dev, name)


@pytest.mark.parametrize("name", [n for n in R.SMALL_CLEANUP_CASES if n.startswith("keep")])
def test_keep_rule(dev, name):
    check_case(dev, name)


@pytest.mark.parametrize("name", [n for n in R.SMALL_CLEANUP_CASES if n.startswith("label")])
def test_labelling(dev, name):
    check_case(dev, name)


@pytest.mark.parametrize("name", ["wide 6x4161 k=1 all", "wide 6x4161 k=1 area 6"])
def test_wide_rows(dev, name):
    check_case(dev, name)


def test_longest_row(dev):
    """W = 16383, the widest row the argument check accepts: the row pass asks for 65536 B of dynamic LDS next to its
    16 B of static LDS.  The launch is accepted on the MI355X (a workgroup may hold up to 160 KiB)."""
    check_case(dev, "wide 3x16383 k=3")


def test_tallest_image(dev):
    check_case(dev, "tall 16383x8 k=3")


# ---------------------------------------------------------------------------------------------------------------
# cleanup through the C entry point
# ---------------------------------------------------------------------------------------------------------------
class Guarded:
    """A byte buffer of `nbytes` inside a larger allocation: `offset` extra bytes in front (so that the view can start
    at any address), sentinels on both sides, the payload prefilled with `fill` or uploaded from `data`."""

    def __init__(self, dev, nbytes, fill=None, data=None, offset=0):
        self.n, self.lo = nbytes, GUARD + offset
        self.raw = torch.full((self.lo + nbytes + GUARD,), SENTINEL, device=dev, dtype=torch.uint8)
        if data is not None:
            self.raw[self.lo:self.lo + nbytes] = _up(np.ascontiguousarray(data).view(np.uint8).reshape(-1), dev)
        elif fill is not None:
            self.raw[self.lo:self.lo + nbytes] = fill
        self.ptr = self.raw.data_ptr() + self.lo

    def read(self, dtype=np.uint8):
        a = self.raw.cpu().numpy()
        assert (a[:self.lo] == SENTINEL).all() and (a[self.lo + self.n:] == SENTINEL).all(), "written outside the buffer"
        return a[self.lo:self.lo + self.n].copy().view(dtype)


def _lib():
    from inklayer_amd import _lib as m
    return m


def _stream():
    from inklayer_amd import ops
    return ops._stream()


def workspace_ints(n, H, W, k):
    need = C.c_int64(0)
    _lib().check(_lib().lib().ink_mask_cleanup_workspace_ints(n, H, W, k, C.byref(need)), "ink_mask_cleanup_workspace_ints")
    assert need.value == 1 + n * (H + 7 * H * R.run_bound(W, k))
    return need.value


def run_cleanup_c(dev, case: R.Case, mask_offset=13, out_offset=7, bufs=None):
    """ink_mask_cleanup with both scratch images and the workspace full of 0x7f, the masks and the output as views at odd
    addresses inside guarded buffers.  -> (rc, output bytes, the buffers)."""
    n, H, W = case.masks.shape
    if bufs is None:
        ws_k = case.k if case.k >= 1 and case.k % 2 else 1
        bufs = dict(masks=Guarded(dev, n * H * W, data=case.masks, offset=mask_offset),
                    ta=Guarded(dev, n * H * W, fill=0x7F), tb=Guarded(dev, n * H * W, fill=0x7F),
                    ws=Guarded(dev, 4 * workspace_ints(n, H, W, ws_k), fill=0x7F),
                    out=Guarded(dev, n * H * W, fill=0x7F, offset=out_offset))
    b = bufs
    assert b["ta"].ptr % 8 == 0 and b["ws"].ptr % 4 == 0
    rc = _lib().lib().ink_mask_cleanup(b["masks"].ptr, n, H, W, case.k, case.area_threshold, float(case.aspect_threshold),
                                       b["ta"].ptr, b["tb"].ptr, b["ws"].ptr, b["out"].ptr, _stream())
    torch.cuda.synchronize()
    for key in ("masks", "ta", "tb", "ws"):
        b[key].read()                                               # guards
    assert np.array_equal(b["masks"].read(), case.masks.reshape(-1))
    return rc, b["out"].read().reshape(n, H, W), b


C_ENTRY_CASES = ["close noise 40x65 k=5", "close edge 129x130 k=11", "close gaps k=5", "keep default", "label checkerboard",
                 "label stripes257 whole", "label comb H=65"]


@pytest.mark.parametrize("name", C_ENTRY_CASES)
def test_cleanup_c_entry_needs_no_zeroed_scratch_and_stays_inside_its_buffers(dev, name):
    case = R.cleanup_case(name)
    rc, out, bufs = run_cleanup_c(dev, case)
    assert rc == 0 and int(bufs["ws"].read(np.int32)[0]) == 0       # the overflow flag
    assert np.array_equal(out, run_cleanup(dev, case)) and np.array_equal(out, R.cleanup_want(case))
    rc2, out2, _ = run_cleanup_c(dev, case, bufs=bufs)              # the same call again, on the buffers as it left them
    assert rc2 == 0 and np.array_equal(out2, out) and int(bufs["ws"].read(np.int32)[0]) == 0


def test_cleanup_c_entry_each_mask_of_a_batch_equals_its_own_call(dev):
    H, W, k = 70, 131, 5
    rs = np.random.RandomState(5)
    masks = np.stack([R._u8(rs.rand(H, W) < d) for d in (0.01, 0.05, 0.2, 0.5, 0.8)])
    masks[3, 60:, 100:] = 0
    case = R.Case(masks, k, 40, 1.5)
    rc, out, _ = run_cleanup_c(dev, case)
    want = R.cleanup_want(case)
    assert rc == 0 and np.array_equal(out, want) and 0 < want.sum() < (R.cleanup(masks, k, -1) > 0).sum() * 255
    for i in range(5):
        rc, one, _ = run_cleanup_c(dev, R.Case(masks[i:i + 1], k, 40, 1.5), mask_offset=i, out_offset=5 - i)
        assert rc == 0 and np.array_equal(one[0], out[i]), i


BAD_ARGUMENTS = {"W=7": (8, 7, 3), "even k": (16, 16, 4), "k=0": (16, 16, 0), "H=16384": (16384, 8, 3),
                 "W=16384": (1, 16384, 3)}


@pytest.mark.parametrize("what", list(BAD_ARGUMENTS))
def test_cleanup_rejections(dev, what):
    H, W, k = BAD_ARGUMENTS[what]
    case = R.Case(np.full((1, H, W), 255, np.uint8), k, 500, 1.1)
    rc, out, bufs = run_cleanup_c(dev, case)
    assert rc == 1 and (out == 0x7F).all()                          # "bad argument"; the output keeps its prefill
    assert (bufs["ta"].read() == 0x7F).all() and (bufs["tb"].read() == 0x7F).all()      # refused before any launch


def test_cleanup_rejects_a_misaligned_scratch_image_and_the_wrapper_raises(dev):
    from inklayer_amd import ops
    case = R.Case(np.full((1, 16, 16), 255, np.uint8), 3, 500, 1.1)
    _, _, bufs = run_cleanup_c(dev, case)
    bufs["ta"] = Guarded(dev, 256, fill=0x7F, offset=4)
    assert bufs["ta"].ptr % 8 == 4
    b = bufs
    rc = _lib().lib().ink_mask_cleanup(b["masks"].ptr, 1, 16, 16, 3, 500, 1.1, b["ta"].ptr, b["tb"].ptr, b["ws"].ptr,
                                       b["out"].ptr, _stream())
    torch.cuda.synchronize()
    assert rc == 1 and (b["ta"].read() == 0x7F).all()
    for H, W, k in ((16, 16, 4), (16, 16, 0), (8, 7, 3), (16384, 8, 3), (1, 16384, 3)):
        with pytest.raises(_lib().InkLayerHipError, match="bad argument"):
            ops.mask_cleanup(torch.zeros((1, H, W), device=dev, dtype=torch.uint8), k)


# ---------------------------------------------------------------------------------------------------------------
# sketch IoU counts
# ---------------------------------------------------------------------------------------------------------------
def _check_table(counts, want):
    assert counts.dtype == np.int32 and np.array_equal(counts.astype(np.int64), want)
    assert np.array_equal(counts, counts.transpose(1, 0, 2))                            # symmetric
    d = np.arange(len(counts))
    assert np.array_equal(counts[d, d, 0], counts[d, d, 1])                             # |r & r| = |r | r|


@pytest.mark.parametrize("hw", R.COUNT_SHAPES, ids=lambda hw: f"{hw[0]}x{hw[1]}")
def test_sketch_iou_counts(dev, hw):
    from inklayer_amd import ops
    H, W = hw
    for rot in ((0, 1) if H * W == 1 else (0,)):
        rgb = R.count_sketch(H, W, rot)
        luma = R.pil_luma(rgb)
        assert H * W == 1 or ((luma == 249).any() and (luma == 250).any())
        for n in R.COUNT_NS:
            masks = R.count_masks(n, H, W)
            got = ops.mask_sketch_iou_counts(_up(masks, dev), _up(rgb, dev)).cpu().numpy()
            _check_table(got, R.sketch_iou_counts(masks, rgb))


@pytest.mark.parametrize("hw", R.COUNT_SHAPES, ids=lambda hw: f"{hw[0]}x{hw[1]}")
def test_counts_of_full_masks_are_the_stroke_count(dev, hw):
    """Every pair of full masks intersects and unites in exactly the stroke pixels: no bit behind the image counts."""
    from inklayer_amd import ops
    H, W = hw
    rgb = R.count_sketch(H, W)
    strokes = int((R.pil_luma(rgb) < 250).sum())
    assert strokes > 0
    for n, byte in ((1, 255), (5, 1)):
        masks = np.full((n, H, W), byte, np.uint8)
        got = ops.mask_sketch_iou_counts(_up(masks, dev), _up(rgb, dev)).cpu().numpy()
        assert (got == strokes).all(), (n, strokes)


@pytest.mark.parametrize("hw,n", [((5, 13), 5), ((127, 129), 2), ((1, 16385), 33), ((1, 1), 1)])
def test_counts_c_entry(dev, hw, n):
    """The bit workspace full of 0xff, the sketch and the masks one byte into their allocations, guards all round."""
    H, W = hw
    rgb, masks = R.count_sketch(H, W), R.count_masks(n, H, W)
    nwords = (H * W + 63) // 64
    b_rgb, b_masks = Guarded(dev, rgb.size, data=rgb, offset=1), Guarded(dev, masks.size, data=masks, offset=1)
    bits, counts = Guarded(dev, 8 * n * nwords, fill=0xFF), Guarded(dev, 4 * n * n * 2, fill=0xFF)
    assert b_rgb.ptr % 2 == 1 and b_masks.ptr % 2 == 1 and bits.ptr % 8 == 0
    want = R.sketch_iou_counts(masks, rgb)
    for _ in range(2):                                              # twice on the same buffers
        rc = _lib().lib().ink_mask_sketch_iou_counts(b_masks.ptr, b_rgb.ptr, n, H, W, bits.ptr, counts.ptr, _stream())
        torch.cuda.synchronize()
        assert rc == 0
        _check_table(counts.read(np.int32).reshape(n, n, 2), want)
        b_rgb.read(), b_masks.read()
        words = bits.read(np.uint64).reshape(n, nwords)
        tail = H * W - 64 * (nwords - 1)
        assert tail == 64 or not (words[:, -1] >> np.uint64(tail)).any()               # the tail bits are clear


# ---------------------------------------------------------------------------------------------------------------
# end to end
# ---------------------------------------------------------------------------------------------------------------
def test_sketch_nms_end_to_end(dev):
    from oracle import refine_ref as O
    from inklayer_amd import refine
    rgb, masks, boxes, scores = R.nms_case()
    cleaned = refine.clean_masks(_up(masks, dev))
    assert int(cleaned._ink_overflow_flag.item()) == 0
    want_masks = R.cleanup(masks, O.calculate_kernel_size(R.NMS_HW))
    assert np.array_equal(cleaned.cpu().numpy(), want_masks)
    for thr in R.NMS_THRESHOLDS:
        want = O.sketch_nms(rgb, boxes, scores, list(want_masks), thr)
        got = refine.sketch_nms(rgb, boxes, scores, cleaned, thr)
        assert np.array_equal(got, want), (thr, got, want)
