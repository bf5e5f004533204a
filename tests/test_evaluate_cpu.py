"""Evaluation stage without a GPU: the ground-truth picture against the reference's own output, the metrics against hand
values, the numpy counting path against tests/evaluate_ref.py, the planted mistakes, tools/eval_dir.py on a temporary
tree, the loaders and the argument checks of the four C entry points."""
import json
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import evaluate_ref as R
from inklayer_amd import evaluate as E

ROOT = Path(__file__).resolve().parent.parent
GTVIS = np.load(ROOT / "tests" / "golden" / "gtvis_small.npz")


def _dropin():
    import importlib.util
    spec = importlib.util.spec_from_file_location("_read_GT_mat_file", ROOT / "InkScenes" / "read_GT_mat_file.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


# ----------------------------------------------------------------------------------------------------------------------
# the ground-truth picture
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", range(5))
def test_label_picture_equals_the_reference_picture(k, tmp_path):
    from PIL import Image
    labels, want = GTVIS[f"labels_{k}"], GTVIS[f"picture_{k}"]
    got = E.label_picture(labels, use_gpu=False)
    assert got.dtype == np.uint8 and np.array_equal(got, want), str(GTVIS["names"][k])
    assert np.array_equal(got, R.picture(labels, [(255, 255, 255)] + E.pastel_colors(len(np.unique(labels)) - 1)))
    mod = _dropin()                                                  # the drop-in on a file (no scipy needed for .npy)
    np.save(tmp_path / "gt.npy", labels)
    im = mod.visualize_label_matrix(str(tmp_path / "gt.npy"), "INSTANCE_GT", str(tmp_path / "vis.png"))
    assert np.array_equal(np.asarray(im), want)
    assert np.array_equal(np.asarray(Image.open(tmp_path / "vis.png").convert("RGB")), want)


def test_golden_matrices_are_the_five_of_the_issue():
    lab = [GTVIS[f"labels_{k}"] for k in range(5)]
    assert lab[0].shape == (40, 56) and lab[0].dtype == np.uint8 and set(np.unique(lab[0])) == {0, 1, 2, 5, 9}
    assert set(np.unique(lab[1])) == {3, 4, 7}
    assert lab[2].dtype == np.uint16 and lab[2].max() == 60000
    assert lab[3].dtype == np.float64
    assert not lab[4].any()
    first = GTVIS["picture_1"][lab[1] == 3]                          # the quirk: without 0 the smallest label is white
    assert (first == 255).all()


def test_dropin_names_and_cli(tmp_path):
    mod = _dropin()
    colors = np.load(ROOT / "tests" / "golden" / "vis_colors.npz")
    for n in (0, 1, 5, 64):
        assert np.array_equal(np.asarray(mod.generate_pastel_colors(n), np.int64).reshape(n, 3), colors[f"colors_{n}"])
    np.save(tmp_path / "gt.npy", GTVIS["labels_0"])
    r = subprocess.run([sys.executable, str(ROOT / "InkScenes" / "read_GT_mat_file.py"), "--mat_file", str(tmp_path / "gt.npy"),
                        "--output", str(tmp_path / "o.png")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    from PIL import Image
    assert np.array_equal(np.asarray(Image.open(tmp_path / "o.png").convert("RGB")), GTVIS["picture_0"])


# ----------------------------------------------------------------------------------------------------------------------
# metrics: hand cases
# ----------------------------------------------------------------------------------------------------------------------
def _summary(iou, scores):
    ev = E.Evaluator()
    ev.add(np.asarray(iou, np.float64), scores)
    return ev.summary()


def test_perfect_prediction():
    lab = np.zeros((12, 12), np.uint8)
    lab[1:5, 1:5], lab[6:11, 2:9], lab[0:3, 8:12] = 1, 2, 7
    T, values = E.contingency(lab, lab, use_gpu=False, n_labels=7)          # label form; masks 3 .. 6 are empty
    assert list(values) == [0, 1, 2, 7] and T.shape == (8, 4)
    iou = E.iou_matrix(T, values)
    assert np.array_equal(iou[[0, 1, 6]], np.eye(3)) and not iou[2:6].any()
    s = _summary(iou[[0, 1, 6]], [0.9, 0.8, 0.7])
    assert s["AP"] == 1.0 and s["AP50"] == 1.0 and s["AP75"] == 1.0 and s["AR"] == 1.0
    pq = E.panoptic(T, values)
    assert pq["PQ"] == 1.0 and pq["SQ"] == 1.0 and pq["RQ"] == 1.0 and pq["accuracy"] == 1.0 and pq["mean_best_iou"] == 1.0
    assert (pq["tp"], pq["fp"], pq["fn"]) == (3, 0, 0)                      # empty rows are no predictions


def test_false_positive_with_the_top_score():
    """One instance; a false positive scored above the true positive: recall reaches 1 at precision 1/2, the envelope is
    1/2 at all 101 recall points."""
    s = _summary([[0.0], [1.0]], [0.9, 0.8])
    assert s["AP"] == 0.5 and s["AP50"] == 0.5 and s["AR"] == 1.0
    # two instances, TP (0.9), FP (0.8), TP (0.7): precision envelope 1 up to recall 0.5 (51 points), 2/3 above (50)
    s = _summary([[1.0, 0.0], [0.0, 0.0], [0.0, 1.0]], [0.9, 0.8, 0.7])
    assert abs(s["AP"] - (51 + 50 * (2 / 3)) / 101) < 1e-12 and s["AR"] == 1.0


def test_duplicate_detection():
    """Two detections of one instance: the better scored one matches, the other is a false positive after it."""
    iou = [[0.8], [0.9]]
    assert list(E.match_coco(np.asarray(iou), [0.9, 0.5], 0.5)) == [0, -1]
    s = _summary(iou, [0.9, 0.5])
    assert s["AP50"] == 1.0 and s["AP75"] == 1.0          # the false positive comes after full recall
    # thresholds 0.50 .. 0.80 are met by the first detection (IoU 0.8): 7 of 10; at 0.85 and 0.90 the second one (0.9)
    # matches as a later true positive at precision 1/2; at 0.95 nothing matches
    assert abs(s["AP"] - (7 * 1.0 + 2 * 0.5 + 0.0) / 10) < 1e-12
    assert abs(s["AR"] - 0.9) < 1e-12
    # ties: the lowest instance index; scores equal: the lowest detection index goes first
    assert list(E.match_coco(np.asarray([[0.7, 0.7], [0.7, 0.7]]), [0.5, 0.5], 0.5)) == [0, 1]
    # a detection takes the best still-unmatched instance, not the best one
    assert list(E.match_coco(np.asarray([[0.9, 0.6], [0.8, 0.1]]), [0.9, 0.8], 0.5)) == [0, -1]
    assert list(E.match_coco(np.asarray([[0.9, 0.6], [0.8, 0.1]]), [0.8, 0.9], 0.5)) == [1, 0]


def test_no_predictions_and_no_instances():
    s = _summary(np.zeros((0, 3)), [])
    assert s["AP"] == 0.0 and s["AR"] == 0.0 and s["instances"] == 3 and s["detections"] == 0
    s = _summary(np.zeros((2, 0)), [0.5, 0.4])
    assert s["AP"] == -1.0 and s["AR"] == -1.0 and s["instances"] == 0            # COCO's "undefined"
    lab = np.zeros((6, 6), np.uint8)
    T, values = E.contingency(np.zeros((0, 6, 6), np.uint8), lab, use_gpu=False)
    assert T.shape == (1, 1) and T[0, 0] == 36 and E.iou_matrix(T, values).shape == (0, 0)
    pq = E.panoptic(T, values)
    assert pq["PQ"] == 0.0 and (pq["tp"], pq["fp"], pq["fn"]) == (0, 0, 0)
    lab[1:3, 1:3] = 4                                                              # one instance, still no prediction
    pq = E.panoptic(*E.contingency(np.zeros((0, 6, 6), np.uint8), lab, use_gpu=False))
    assert pq["PQ"] == 0.0 and pq["fn"] == 1 and pq["accuracy"] == 0.0
    ones = np.ones((1, 6, 6), np.uint8)                                            # one prediction, no instance
    pq = E.panoptic(*E.contingency(ones, np.zeros((6, 6), np.uint8), use_gpu=False))
    assert pq["PQ"] == 0.0 and pq["fp"] == 1


def test_iou_exactly_at_a_threshold():
    lab = np.zeros((4, 8), np.uint8)
    lab[0, 0:4] = 1                                       # instance of 4 pixels
    half = np.zeros((1, 4, 8), np.uint8)
    half[0, 0, 2:8] = 1                                   # 6 pixels, 2 shared: IoU 2 / 8
    T, values = E.contingency(half, lab, use_gpu=False)
    assert E.iou_matrix(T, values)[0, 0] == 0.25
    half[0, 0, 0:8] = 1                                   # 8 pixels, 4 shared: IoU 4 / 8, exactly the first threshold
    iou = E.iou_matrix(*E.contingency(half, lab, use_gpu=False))
    assert iou[0, 0] == 0.5
    assert list(E.match_coco(iou, [1.0], 0.5)) == [0] and list(E.match_coco(iou, [1.0], 0.55)) == [-1]
    s = _summary(iou, [1.0])
    assert s["AP50"] == 1.0 and s["AP75"] == 0.0 and abs(s["AP"] - 0.1) < 1e-12 and abs(s["AR"] - 0.1) < 1e-12
    assert E.panoptic(T, values)["tp"] == 0 and E.panoptic(*E.contingency(half, lab, use_gpu=False))["tp"] == 0   # > 0.5
    three = np.zeros((1, 4, 8), np.uint8)
    three[0, 0, 1:4] = 1                                  # 3 of 4: IoU 0.75, exactly the sixth threshold
    iou = E.iou_matrix(*E.contingency(three, lab, use_gpu=False))
    assert iou[0, 0] == 0.75 and _summary(iou, [1.0])["AP75"] == 1.0 and abs(_summary(iou, [1.0])["AP"] - 0.6) < 1e-12


def test_more_than_100_detections_per_image_are_cut_by_score():
    iou = np.zeros((101, 1))
    iou[100, 0] = 1.0
    scores = np.linspace(1.0, 0.5, 101)                   # the only true positive has the lowest score
    assert _summary(iou, scores)["AR"] == 0.0
    assert _summary(iou[1:], scores[1:])["AR"] == 1.0


def test_box_iou():
    a = [[0, 0, 2, 2], [0, 0, 1, 1], [5, 5, 5, 5]]
    b = [[1, 1, 3, 3], [0, 0, 2, 2]]
    got = E.box_iou(a, b)
    assert got.shape == (3, 2) and got.dtype == np.float64
    assert got[0, 0] == 1 / 7 and got[0, 1] == 1.0 and got[1, 0] == 0.0 and got[1, 1] == 0.25
    assert not got[2].any()                               # an empty box
    assert E.box_iou(np.zeros((0, 4)), b).shape == (0, 2)


def test_panoptic_by_hand():
    lab = np.zeros((4, 10), np.uint8)
    lab[0, :], lab[1, :], lab[2, 0:4] = 1, 2, 3
    pred = np.zeros((4, 10), np.uint8)
    pred[0, 0:8] = 1                                      # IoU 8 / 10 with instance 1
    pred[1, 0:5], pred[3, 0:5] = 2, 2                     # IoU 5 / 15 with instance 2: no match
    pq = E.panoptic(*E.contingency(pred, lab, use_gpu=False))
    assert (pq["tp"], pq["fp"], pq["fn"]) == (1, 1, 2)
    assert pq["SQ"] == 0.8 and pq["RQ"] == 1 / 2.5 and pq["PQ"] == 0.8 / 2.5
    assert pq["accuracy"] == 8 / 24 and abs(pq["mean_best_iou"] - (0.8 + 5 / 15 + 0.0) / 3) < 1e-12
    pooled = E.panoptic_pool([pq, pq])
    assert abs(pooled["PQ"] - pq["PQ"]) < 1e-12 and pooled["tp"] == 2


# ----------------------------------------------------------------------------------------------------------------------
# counting: the numpy path against the independent statement
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stroke_only", [False, True], ids=["all", "strokes"])
@pytest.mark.parametrize("name", R.SETS)
def test_numpy_path_equals_reference_on_the_committed_sets(name, stroke_only):
    s = R.load_set(name)
    want, values = R.set_table(name, stroke_only)
    T, v = E.contingency(s["masks"], s["label"], s["input"], stroke_only, use_gpu=False)
    assert np.array_equal(T, want) and np.array_equal(v, values)
    assert want[-1].sum() == ((R.gray(s["input"]) < 250).sum() if stroke_only else s["label"].size)


def test_numpy_path_on_the_small_grid():
    for shape, n, U, dtype in R.small_cases():
        masks, labels, sketch = R.small_case(shape, n, U, dtype)
        for so in (False, True):
            T, v = E.contingency(masks, labels, sketch, so, use_gpu=False)
            want, values = R.contingency(masks, labels, sketch, so)
            assert np.array_equal(T, want) and np.array_equal(v, values), (shape, n, U, dtype, so)
    masks, labels, sketch = R.small_case((33, 256), 255, 256, np.uint16)
    label_pred = np.random.RandomState(1).randint(0, 256, size=(33, 256)).astype(np.uint8)
    T, v = E.contingency(label_pred, labels, use_gpu=False, n_labels=255)
    assert np.array_equal(T, R.contingency(label_pred, labels, n_labels=255)[0])
    T3, _ = E.contingency(label_pred, labels, use_gpu=False, n_labels=3)            # labels above n count as 0
    assert np.array_equal(T3, R.contingency(label_pred, labels, n_labels=3)[0]) and np.array_equal(T3[-1], T[-1])
    boxes, values = E.label_boxes(labels, use_gpu=False)
    assert np.array_equal(boxes, R.boxes(labels)) and np.array_equal(values, R.ranks(labels)[0])


@pytest.mark.parametrize("mistake", R.MISTAKES)
def test_every_planted_mistake_shows_on_the_gpu_tests_inputs(mistake):
    """The small grid of tests/test_evaluate_gpu.py (all pixels and stroke-only): at least one of its tables changes under
    each planted mistake, otherwise equality on those inputs would not rule the mistake out."""
    changed = 0
    for shape, n, U, dtype in R.small_cases():
        if dtype != np.uint16:
            continue                                          # the masks and sketches do not depend on the dtype
        masks, labels, sketch = R.small_case(shape, n, U, dtype)
        for so in (False, True):
            good = R.contingency(masks, labels, sketch, so)[0]
            changed += not np.array_equal(good, R.contingency(masks, labels, sketch, so, mistake=mistake)[0])
    assert changed > 0, mistake


# ----------------------------------------------------------------------------------------------------------------------
# errors, loaders, tool
# ----------------------------------------------------------------------------------------------------------------------
def test_limits_are_named():
    lab = np.arange(300, dtype=np.uint16).reshape(10, 30)
    m = np.ones((1, 10, 30), np.uint8)
    with pytest.raises(ValueError, match="at most 256"):
        E.contingency(m, lab, use_gpu=False)
    for bad in (np.full((10, 30), 65536, np.int32), np.full((10, 30), -1, np.int32)):
        with pytest.raises(ValueError, match="0 .. 65535"):
            E.contingency(m, bad, use_gpu=False)
    with pytest.raises(ValueError, match="integral"):
        E.contingency(m, np.full((10, 30), 1.5), use_gpu=False)
    with pytest.raises(ValueError, match="differ in shape"):
        E.contingency(m, lab[:, :29], use_gpu=False)
    with pytest.raises(ValueError, match="sketch"):
        E.contingency(m, lab[:, :3].repeat(10, 1), np.zeros((10, 29, 3), np.uint8), True, use_gpu=False)
    with pytest.raises(ValueError, match="sketch"):
        E.contingency(m, np.zeros((10, 30), np.uint8), None, True, use_gpu=False)
    T, v = E.contingency(m, np.full((10, 30), 3.0), use_gpu=False)                  # integral floats are labels
    assert list(v) == [3] and T.tolist() == [[300], [300]]


def test_loaders(tmp_path):
    from PIL import Image
    rs = np.random.RandomState(0)
    lab16 = rs.randint(0, 60001, size=(9, 13)).astype(np.uint16)
    lab8 = rs.randint(0, 256, size=(9, 13)).astype(np.uint8)
    np.save(tmp_path / "a.npy", lab16)
    assert np.array_equal(E.load_labels(tmp_path / "a.npy"), lab16)
    Image.fromarray(lab8).save(tmp_path / "b.png")
    Image.fromarray(lab16).save(tmp_path / "c.png")
    assert np.array_equal(E.load_labels(tmp_path / "b.png"), lab8)
    assert np.array_equal(E.load_labels(str(tmp_path / "c.png")), lab16)
    Image.fromarray(np.zeros((4, 4, 3), np.uint8)).save(tmp_path / "rgb.png")
    with pytest.raises(ValueError, match="single-channel"):
        E.load_labels(tmp_path / "rgb.png")
    d = tmp_path / "masks_final"
    d.mkdir()
    a, b = np.zeros((9, 13), bool), np.zeros((9, 13), bool)
    a[0:4, 0:6], b[2:8, 4:10] = True, True                           # overlapping: the later file wins
    Image.fromarray(a).save(d / "mask_0.png")
    Image.fromarray((b * 255).astype(np.uint8)).save(d / "mask_10.png")
    (d / "notes.txt").write_text("x")
    got = E.load_labels(d)
    want = np.zeros((9, 13), np.uint8)
    want[a], want[b] = 1, 11
    assert np.array_equal(got, want)
    with pytest.raises(ValueError):
        E.load_labels(tmp_path / "a.txt")


def test_mat_loader_round_trip(tmp_path):
    sio = pytest.importorskip("scipy.io")
    inst, cls = GTVIS["labels_2"], GTVIS["labels_0"]
    sio.savemat(tmp_path / "gt.mat", {"INSTANCE_GT": inst, "CLASS_GT": cls})
    assert np.array_equal(E.load_labels(tmp_path / "gt.mat"), inst)
    assert np.array_equal(E.load_labels(tmp_path / "gt.mat", key="CLASS_GT"), cls)
    with pytest.raises(KeyError, match="NOPE"):
        E.load_labels(tmp_path / "gt.mat", key="NOPE")
    im = _dropin().visualize_label_matrix(str(tmp_path / "gt.mat"), "CLASS_GT", str(tmp_path / "v.png"))
    assert np.array_equal(np.asarray(im), GTVIS["picture_0"])


def test_missing_scipy_is_reported(tmp_path, monkeypatch):
    (tmp_path / "gt.mat").write_bytes(b"")
    monkeypatch.setitem(sys.modules, "scipy.io", None)
    with pytest.raises(ImportError, match="needs scipy"):
        E.load_labels(tmp_path / "gt.mat")


def _write_tree(root, name):
    """<root>/<name>/ as run_dir.py leaves it, from a committed set."""
    from PIL import Image
    s = R.load_set(name)
    d = root / name
    (d / "masks").mkdir(parents=True)
    (d / "masks_final").mkdir()
    Image.fromarray(s["input"]).save(d / "input.png")
    for i, m in enumerate(s["masks"]):
        Image.fromarray(m).save(d / "masks" / f"mask_{i}.png")
    for i, m in zip(s["final_indices"], s["final"]):
        Image.fromarray(m).save(d / "masks_final" / f"mask_{i}.png")
    (d / "bboxes.json").write_text(json.dumps({"bboxes": s["bboxes"].tolist(), "scores": s["scores"].tolist()}))
    (d / "bboxes_final.json").write_text(json.dumps({"bboxes": s["final_bboxes"].tolist(), "scores": s["final_scores"].tolist(),
                                                     "kept_indices": s["final_kept"].tolist()}))


def test_eval_dir_on_a_tree_against_itself(tmp_path):
    names = ["fscoco_animals", "office_sketch"]
    for name in names:
        _write_tree(tmp_path / "out", name)
    (tmp_path / "out" / "stray.txt").write_text("not a sketch")
    r = subprocess.run([sys.executable, str(ROOT / "tools" / "eval_dir.py"), "--pred", str(tmp_path / "out"), "--gt",
                        str(tmp_path / "out"), "--cpu", "--json", str(tmp_path / "r.json")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    lines = [json.loads(l) for l in r.stdout.strip().splitlines()]
    assert [l["name"] for l in lines[:-1]] == names and lines[-1]["summary"] is True and lines[-1]["sketches"] == 2
    for l in lines:
        assert l["panoptic"]["PQ"] == 1.0 and l["panoptic"]["accuracy"] == 1.0
        assert l["masks_final"]["AP"] == 1.0 and l["masks_final"]["AR"] == 1.0
        assert 0.0 <= l["masks"]["AP"] <= 1.0 and 0.0 < l["boxes"]["AP50"] <= 1.0
    assert json.loads((tmp_path / "r.json").read_text())["summary"] == lines[-1]
    # the segmentor's masks of the first set, by the library: the tool's figure is the Evaluator's
    s = R.load_set(names[0])
    T, values = R.set_table(names[0], False)
    ev = E.Evaluator()
    ev.add(E.iou_matrix(T, values), s["scores"])
    assert lines[0]["masks"] == ev.summary()


def test_bad_arguments_are_rejected_without_launch():
    """The four entry points check their arguments before any HIP call (fake non-null pointers; no GPU needed)."""
    from inklayer_amd import _lib
    L = _lib.lib()
    p = 16
    good = dict(lab=p, es=1, H=8, W=8, ws=p, vals=p, cap=256, info=p, rank=p)
    ranks = lambda **kw: L.ink_eval_label_ranks(*{**good, **kw}.values(), None)
    for k in ("lab", "ws", "vals", "info", "rank"):
        assert ranks(**{k: None}) == 1, k
    assert ranks(es=0) == 1 and ranks(es=3) == 1 and ranks(es=8) == 1
    assert ranks(H=0) == 1 and ranks(W=0) == 1 and ranks(H=-1) == 1 and ranks(W=-8) == 1
    assert ranks(H=65536, W=32768) == 1 and ranks(cap=0) == 1                       # H W = 2^31
    good = dict(pred=p, n=2, by_label=0, rank=p, U=3, sk=p, ch=3, so=1, H=8, W=8, T=p)
    cont = lambda **kw: L.ink_eval_contingency(*{**good, **kw}.values(), None)
    assert cont(rank=None) == 1 and cont(T=None) == 1 and cont(sk=None) == 1 and cont(pred=None) == 1
    assert cont(pred=None, n=0, by_label=1) == 1                                    # only an empty stack may be null
    assert cont(U=0) == 1 and cont(U=257) == 1 and cont(U=-1) == 1
    assert cont(n=-1) == 1 and cont(n=256, by_label=1) == 1 and cont(n=-1, by_label=1) == 1
    assert cont(H=0) == 1 and cont(W=0) == 1 and cont(H=-2) == 1 and cont(H=65536, W=32768) == 1
    assert cont(ch=2) == 1 and cont(ch=0) == 1 and cont(ch=4) == 1
    good = dict(rank=p, U=3, H=8, W=8, boxes=p)
    box = lambda **kw: L.ink_eval_label_boxes(*{**good, **kw}.values(), None)
    assert box(rank=None) == 1 and box(boxes=None) == 1 and box(U=0) == 1 and box(U=257) == 1
    assert box(H=0) == 1 and box(W=0) == 1 and box(W=-1) == 1
    good = dict(rank=p, col=p, U=3, H=8, W=8, out=p)
    paint = lambda **kw: L.ink_eval_paint_labels(*{**good, **kw}.values(), None)
    assert paint(rank=None) == 1 and paint(col=None) == 1 and paint(out=None) == 1
    assert paint(U=0) == 1 and paint(U=257) == 1 and paint(H=0) == 1 and paint(W=0) == 1 and paint(H=-1) == 1
