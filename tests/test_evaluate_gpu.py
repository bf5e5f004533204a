"""Evaluation kernels (csrc/evaluate.hip) on the GPU: exact equality with the independent numpy statement of
tests/evaluate_ref.py - label ranks, contingency table, label boxes, ground-truth picture - over the small grid whose
power tests/test_evaluate_cpu.py shows with planted mistakes, the label patterns that stress the wave aggregation, the
stroke bound, misaligned buffers, the committed sets at their real sizes, and the Evaluator end to end.  No tolerance:
every compared quantity is an integer, or float64 arithmetic on the host over such integers."""
import numpy as np
import pytest
import torch

import evaluate_ref as R
from inklayer_amd import _lib, evaluate as E, ops

GTVIS = np.load(R.GOLDEN / "gtvis_small.npz")


def _t(a, dev):
    return torch.from_numpy(np.array(a)).to(dev)                # a copy: the shared fixtures are read-only


def _table(dev, pred, labels, sketch=None, stroke_only=False, n_labels=None):
    """contingency on CUDA tensors -> numpy."""
    T, values = E.contingency(_t(pred, dev), _t(labels, dev), None if sketch is None else _t(sketch, dev), stroke_only,
                              n_labels=n_labels)
    assert torch.is_tensor(T) and T.is_cuda and T.dtype == torch.int32 and values.is_cuda
    return T.cpu().numpy(), values.cpu().numpy()


@pytest.mark.gpu
@pytest.mark.parametrize("n", R.MASK_COUNTS)
@pytest.mark.parametrize("shape", R.SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_small_grid_equals_reference(dev, shape, n):
    """Stack form, U in {1, 2, 256}, uint8 / uint16 / int32 labels: ranks, table (all pixels and stroke-only), boxes."""
    for U in R.VALUE_COUNTS:
        for dtype in R.DTYPES:
            masks, labels, sketch = R.small_case(shape, n, U, dtype)
            values, rank = R.ranks(labels)
            got_rank, got_values, info = ops.eval_label_ranks(_t(labels, dev))
            assert info.cpu().tolist() == [len(values), 0]
            assert np.array_equal(got_values.cpu().numpy()[:len(values)], values)
            assert np.array_equal(got_rank.cpu().numpy(), rank)
            for so in (False, True):
                T, v = _table(dev, masks, labels, sketch, so)
                want, _ = R.contingency(masks, labels, sketch, so)
                assert np.array_equal(v, values) and np.array_equal(T, want), (U, dtype, so)
            boxes, v = E.label_boxes(_t(labels, dev))
            assert np.array_equal(boxes.cpu().numpy(), R.boxes(labels)) and np.array_equal(v.cpu().numpy(), values)
            # the wrappers themselves, on the rank image of above
            U_ = len(values)
            assert np.array_equal(ops.eval_contingency(_t(masks, dev), got_rank, U_).cpu().numpy(), R.contingency(masks, labels)[0])
            assert np.array_equal(ops.eval_label_boxes(got_rank, U_).cpu().numpy(), R.boxes(labels))
            colors = np.array([(255, 255, 255)] + E.pastel_colors(U_ - 1), np.uint8)
            assert np.array_equal(ops.eval_paint_labels(got_rank, _t(colors, dev)).cpu().numpy(), R.picture(labels, colors))


@pytest.mark.gpu
@pytest.mark.parametrize("shape", R.SHAPES[1:], ids=lambda s: f"{s[0]}x{s[1]}")
def test_label_form_with_255_masks(dev, shape):
    H, W = shape
    rs = np.random.RandomState(H * W)
    labels = R.make_labels(rs, H, W, 256, np.uint16)
    pred = rs.randint(0, 256, size=(H, W)).astype(np.uint8)
    pred[0, 0], pred[H - 1, W - 1] = 255, 255
    for n in (255, 33, 3, 0):                              # labels above n count as no mask
        T, _ = _table(dev, pred, labels, n_labels=n)
        assert np.array_equal(T, R.contingency(pred, labels, n_labels=n)[0]), n
    T, _ = E.contingency(_t(pred, dev), _t(labels, dev))   # n = the largest label
    assert T.shape[0] == 256 and np.array_equal(T.cpu().numpy(), R.contingency(pred, labels, n_labels=255)[0])
    stack = np.stack([pred == l for l in range(1, 34)])    # the same table from the masks of these labels
    assert np.array_equal(_table(dev, stack, labels)[0], R.contingency(pred, labels, n_labels=33)[0])


@pytest.mark.gpu
@pytest.mark.parametrize("channels", [1, 3])
@pytest.mark.parametrize("shape", R.SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_stroke_only_straddles_the_bound(dev, shape, channels):
    H, W = shape
    rs = np.random.RandomState(31 * H + W + channels)
    sketch = R.make_sketch(rs, H, W, channels)
    g = R.gray(sketch)
    if H * W > 1:
        assert (g == 249).any() and (g == 250).any()
    labels = R.make_labels(rs, H, W, 9, np.uint8)
    for n in (1, 33):
        masks = R.make_masks(rs, n, H, W)
        T, _ = _table(dev, masks, labels, sketch, True)
        assert np.array_equal(T, R.contingency(masks, labels, sketch, True)[0])
        assert T[-1].sum() == (g < 250).sum()
    label_pred = rs.randint(0, 4, size=(H, W)).astype(np.uint8)
    T, _ = _table(dev, label_pred, labels, sketch, True, n_labels=3)
    assert np.array_equal(T, R.contingency(label_pred, labels, sketch, True, n_labels=3)[0])


@pytest.mark.gpu
def test_label_patterns(dev):
    """Per-pixel random labels over 256 values (the lanes of a wave rarely share a bin), a checkerboard (two bins
    alternating lane by lane) and one constant 1024 x 1024 image (a single bin of 1 048 576)."""
    rs = np.random.RandomState(5)
    H, W = 64, 129
    masks = R.make_masks(rs, 5, H, W)
    random = rs.randint(0, 256, size=(H, W)).astype(np.uint8)
    yy, xx = np.mgrid[0:H, 0:W]
    checker = np.where((yy + xx) % 2 == 0, 40000, 3).astype(np.int32)
    for labels in (random, checker):
        T, v = _table(dev, masks, labels)
        want, values = R.contingency(masks, labels)
        assert np.array_equal(T, want) and np.array_equal(v, values)
        assert np.array_equal(E.label_boxes(_t(labels, dev))[0].cpu().numpy(), R.boxes(labels))
    const = _t(np.full((1024, 1024), 7, np.uint16), dev)
    full = torch.ones((2, 1024, 1024), dtype=torch.uint8, device=dev)
    full[1, :, 512:] = 0
    T, v = E.contingency(full, const)
    assert v.cpu().tolist() == [7] and T.cpu().tolist() == [[1048576], [524288], [1048576]]
    assert E.label_boxes(const)[0].cpu().tolist() == [[0, 0, 1023, 1023]]


@pytest.mark.gpu
def test_error_flag_raises(dev):
    masks = torch.ones((1, 8, 16), dtype=torch.uint8, device=dev)
    for bad in (65536, -1, -2 ** 31):
        labels = torch.zeros((8, 16), dtype=torch.int32, device=dev)
        labels[7, 15] = bad                                # the last pixel
        with pytest.raises(ValueError, match="0 .. 65535"):
            E.contingency(masks, labels)
        with pytest.raises(ValueError, match="0 .. 65535"):
            E.label_picture(labels)
    labels = torch.arange(8 * 64, dtype=torch.int32, device=dev).reshape(8, 64)
    with pytest.raises(ValueError, match="at most 256"):
        E.contingency(torch.ones((1, 8, 64), dtype=torch.uint8, device=dev), labels)
    rank, values, info = ops.eval_label_ranks(labels)      # the rank kernel itself has no such limit
    assert info.cpu().tolist() == [512, 0] and np.array_equal(rank.cpu().numpy(), np.arange(512).reshape(8, 64))
    assert values.cpu().tolist() == list(range(256))


@pytest.mark.gpu
def test_misaligned_buffers(dev):
    """The sketch, the prediction label image and the ground-truth label image each start one byte into their
    allocation (views into larger buffers), straight through the C entry points."""
    rs = np.random.RandomState(3)
    H, W, n = 33, 64, 5
    sketch = R.make_sketch(rs, H, W, 3)
    labels = R.make_labels(rs, H, W, 17, np.uint8)
    labels32 = R.make_labels(rs, H, W, 17, np.int32)
    pred = rs.randint(0, n + 1, size=(H, W)).astype(np.uint8)
    masks = R.make_masks(rs, n, H, W)

    def off1(a):
        flat = torch.zeros(a.nbytes + 8, device=dev, dtype=torch.uint8)
        flat[1:1 + a.nbytes] = torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1)).to(dev)
        assert (flat.data_ptr() + 1) % 4 == 1
        return flat, flat.data_ptr() + 1

    L, st = _lib.lib(), ops._stream()
    keep = [off1(a) for a in (sketch, labels, labels32, pred, masks)]
    sk, lab, lab32, pl, mk = (k[1] for k in keep)
    for ptr, esize, src in ((lab, 1, labels), (lab32, 4, labels32)):
        values, want_rank = R.ranks(src)
        work = torch.empty(4096, device=dev, dtype=torch.int32)
        vals = torch.zeros(256, device=dev, dtype=torch.int32)
        info = torch.empty(2, device=dev, dtype=torch.int32)
        rank = torch.empty((H, W), device=dev, dtype=torch.uint16)
        assert L.ink_eval_label_ranks(ptr, esize, H, W, work.data_ptr(), vals.data_ptr(), 256, info.data_ptr(), rank.data_ptr(), st) == 0
        assert info.cpu().tolist() == [17, 0] and np.array_equal(vals.cpu().numpy()[:17], values)
        assert np.array_equal(rank.cpu().numpy(), want_rank)
        for p, count, by_label, ref_pred, kw in ((pl, n, 1, pred, dict(n_labels=n)), (mk, n, 0, masks, {})):
            T = torch.empty((n + 1, 17), device=dev, dtype=torch.int32)
            assert L.ink_eval_contingency(p, count, by_label, rank.data_ptr(), 17, sk, 3, 1, H, W, T.data_ptr(), st) == 0
            assert np.array_equal(T.cpu().numpy(), R.contingency(ref_pred, src, sketch, True, **kw)[0])
    # the picture into a buffer that starts one byte off: nothing is written outside it
    colors = _t(np.array([(255, 255, 255)] + E.pastel_colors(16), np.uint8), dev)
    out = torch.full((H * W * 3 + 8,), 7, device=dev, dtype=torch.uint8)
    assert L.ink_eval_paint_labels(rank.data_ptr(), colors.data_ptr(), 17, H, W, out.data_ptr() + 1, st) == 0
    got = out.cpu().numpy()
    assert got[0] == 7 and (got[1 + H * W * 3:] == 7).all()
    assert np.array_equal(got[1:1 + H * W * 3].reshape(H, W, 3), R.picture(labels32, colors.cpu().numpy()))


@pytest.mark.gpu
def test_ground_truth_picture(dev):
    for k in range(5):
        labels, want = GTVIS[f"labels_{k}"], GTVIS[f"picture_{k}"]
        got = E.label_picture(_t(labels, dev))                 # device in, device out (float64 labels included)
        assert torch.is_tensor(got) and got.is_cuda and np.array_equal(got.cpu().numpy(), want), k
        got = E.label_picture(labels)                          # host in: uploaded, host out
        assert isinstance(got, np.ndarray) and np.array_equal(got, want)
    for shape in R.SHAPES:                                     # odd sizes, 256 colours
        labels = R.make_labels(np.random.RandomState(shape[1]), *shape, 256, np.uint16)
        U = len(np.unique(labels))
        want = R.picture(labels, [(255, 255, 255)] + E.pastel_colors(U - 1))
        assert np.array_equal(E.label_picture(_t(labels, dev)).cpu().numpy(), want)


@pytest.mark.gpu
@pytest.mark.parametrize("name", R.SETS)
def test_committed_sets_at_their_real_sizes(dev, name):
    s = R.load_set(name)
    masks, label, sk = _t(s["masks"].view(np.uint8), dev), _t(s["label"], dev), _t(s["input"], dev)
    for so in (False, True):
        want, values = R.set_table(name, so)
        T, v = E.contingency(masks, label, sk, so)
        assert np.array_equal(T.cpu().numpy(), want) and np.array_equal(v.cpu().numpy(), values)
        T2, _ = E.contingency(masks, label, sk, so)            # determinism: the same call again
        assert torch.equal(T, T2)
    T, v = E.contingency(s["masks"], s["label"], s["input"], True)      # host in: uploaded, host out
    assert isinstance(T, np.ndarray) and np.array_equal(T, R.set_table(name, True)[0])
    n = int(s["label"].max())
    final, _ = E.contingency(label, label, n_labels=n)                  # the final label image against itself
    assert E.panoptic(final, v)["PQ"] == 1.0
    assert np.array_equal(E.label_boxes(label)[0].cpu().numpy(), R.boxes(s["label"]))


@pytest.mark.gpu
def test_evaluator_end_to_end_equals_host_path(dev):
    on_dev, on_host = E.Evaluator(), E.Evaluator()
    for name in R.SETS[:3]:
        s = R.load_set(name)
        T, v = E.contingency(_t(s["masks"].view(np.uint8), dev), _t(s["label"], dev), _t(s["input"], dev), True)
        on_dev.add(E.iou_matrix(T, v), s["scores"])
        Th, vh = E.contingency(s["masks"], s["label"], s["input"], True, use_gpu=False)
        on_host.add(E.iou_matrix(Th, vh), s["scores"])
        assert E.panoptic(T, v) == E.panoptic(Th, vh)
    assert on_dev.summary() == on_host.summary() and 0.0 < on_dev.summary()["AP"] <= 1.0
