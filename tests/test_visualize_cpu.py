"""Visualisation stage without a GPU: the colours, the tables and the numpy path of inklayer_amd/visualize.py against the
reference's own committed pictures and against tests/vis_ref.py, the box drawings of the shim against the reference's
bboxes.png / bboxes_final.png, the shim's import surface, and the runner writing segmented_sketch.png through it."""
import inspect
import textwrap
from pathlib import Path

import numpy as np
import pytest
from PIL import Image

import vis_cases
import vis_ref
from inklayer_amd import visualize

ROOT = Path(__file__).resolve().parent.parent


def test_pastel_colors_equal_the_recorded_reference_colours():
    z = np.load(vis_cases.GOLDEN / "vis_colors.npz")
    assert sorted(z["ns"].tolist()) == list(range(65)) + [255]
    for n in z["ns"].tolist():
        got = visualize.pastel_colors(n)
        assert len(got) == n and all(isinstance(c, tuple) and all(isinstance(v, int) for v in c) for c in got)
        assert np.array_equal(np.asarray(got, np.int64).reshape(n, 3), z[f"colors_{n}"]), n


@pytest.mark.parametrize("name", vis_cases.SETS)
def test_host_path_reproduces_the_reference_pictures(name):
    s = vis_cases.load_set(name)
    for masks, picture in ((s["masks"], "segmented_sketch"), (s["masks_final"], "segmented_sketch_final")):
        got = visualize.colour_sketch(s["input"], list(masks), use_gpu=False)
        assert got.dtype == np.uint8 and got.shape == s[picture].shape
        assert int((got != s[picture]).any(-1).sum()) == 0, (name, picture)
    # the label form of the same masks
    label = visualize.label_image(list(s["masks_final"]), s["input"].shape[:2])
    got = visualize.colour_sketch(s["input"], label, n_labels=len(s["masks_final"]), use_gpu=False)
    assert np.array_equal(got, s["segmented_sketch_final"])


@pytest.mark.parametrize("case", vis_cases.synthetic_cases(), ids=lambda c: c[0])
def test_host_path_equals_the_literal_restatement(case):
    _, sketch, masks, kw = case
    colors = kw.get("colors", visualize.pastel_colors(len(masks)))
    want = vis_ref.color_sketch_by_masks(sketch, masks, colors, kw.get("enhance_factor", 1.5), kw.get("min_opacity", 0.2))
    got = visualize.colour_sketch(sketch, masks, use_gpu=False, **kw)
    assert np.array_equal(got, want)
    if case[0] == "no stroke pixel at all":
        assert (got == 255).all()
    if case[0] == "n = 0":
        assert (got[..., 0] == got[..., 1]).all() and (got < 255).any()      # black strokes only


def test_the_two_branches_differ_where_they_should():
    """The 229 / 230 pair of the synthetic cases really lands on different branches (the test above would pass a table
    whose variants were swapped on both sides only if vis_ref were wrong in the same way; this pins the direction)."""
    cases = {c[0]: c for c in vis_cases.synthetic_cases()}
    faint, dark = cases["faint, darkest pixel 230"], cases["faint but for one pixel at 229"]
    a = visualize.colour_sketch(faint[1], faint[2], use_gpu=False)
    b = visualize.colour_sketch(dark[1], dark[2], use_gpu=False)
    assert (a[:-1] != b[:-1]).any()                     # one pixel in the last row changes the opacity of all strokes
    t = visualize.colour_tables([(10, 20, 30)])
    assert t.shape == (2, 2, 256, 3) and (t[:, :, 250:] == 255).all() and (t[0, :, :250] != t[1, :, :250]).any()


def _font_preconditions():
    import PIL
    from PIL import ImageFont
    if int(PIL.__version__.split(".")[0]) != 12:
        return f"Pillow {PIL.__version__}: the stored label pixels are those of Pillow 12's default font"
    try:
        ImageFont.truetype("arial.ttf", 16)
        return "arial.ttf is installed: draw_boxes would not fall back to the default font"
    except Exception:
        pass
    if not isinstance(ImageFont.load_default(), ImageFont.FreeTypeFont):
        return "ImageFont.load_default() is not a FreeType font (Pillow built without FreeType)"
    return None


def _pixel_boxes(s):
    """The integer pixel boxes the reference's runner drew (bboxes.json holds them divided by the image size)."""
    H, W = s["input"].shape[:2]
    return [[int(v) for v in np.rint(b * [W, H, W, H])] for b in s["bboxes"]]


def _label_area(s, boxes, normalised, tab):
    """bool [H, W]: where the text of the drawing may land (tab: draw_boxes' filled label rectangle above the box;
    otherwise the phrase's bounding box at the corner, generously)."""
    H, W = s["input"].shape[:2]
    area = np.zeros((H, W), bool)
    for b in boxes:
        x1, y1 = (b[0] * W, b[1] * H) if normalised else (b[0], b[1])
        if tab:
            y0, yy, x0, xx = y1 - 20, y1, x1, x1 + len("0.00") * 16 + 4
        else:
            y0, yy, x0, xx = y1, y1 + 16, x1, x1 + 90
        area[max(0, int(np.floor(y0))): max(0, int(np.ceil(yy)) + 1), max(0, int(np.floor(x0))): max(0, int(np.ceil(xx)) + 1)] = True
    return area


@pytest.mark.parametrize("name", vis_cases.SETS)
def test_box_drawings_equal_the_reference_files(name):
    from InkLayer.utils.visualization import draw_boxes, draw_norm_bbox_on_image
    s = vis_cases.load_set(name)
    pil = Image.fromarray(s["input"])
    final = np.asarray(draw_boxes(pil, s["final_bboxes"].tolist(), s["final_scores"].tolist()))
    boxes = _pixel_boxes(s)
    first = np.asarray(draw_norm_bbox_on_image(pil, boxes, ["object [SEP]"] * len(boxes)))
    # the rectangles (everything outside the label areas) do not depend on the font: always exact
    off_final = ~_label_area(s, s["final_bboxes"], True, tab=True)
    off_first = ~_label_area(s, boxes, False, tab=False)
    assert np.array_equal(final[off_final], s["bboxes_final_png"][off_final])
    assert np.array_equal(first[off_first], s["bboxes_png"][off_first])
    assert (final != s["input"]).any() and (first != s["input"]).any()
    why = _font_preconditions()
    if why:
        pytest.skip(why)
    assert int((final != s["bboxes_final_png"]).any(-1).sum()) == 0
    assert int((first != s["bboxes_png"]).any(-1).sum()) == 0


def test_draw_functions_follow_the_reference_rules(tmp_path):
    from InkLayer.utils.visualization import draw_boxes, draw_norm_bbox_on_image, generate_pastel_colors
    im = Image.new("RGB", (100, 80), (255, 255, 255))
    a = np.asarray(draw_norm_bbox_on_image(im, [[0.1, 0.25, 0.5, 0.75], [60, 10, 90, 70]]))     # normalised and pixel boxes
    b = np.asarray(draw_norm_bbox_on_image(im, [[10, 20, 50, 60], [60, 10, 90, 70]]))
    assert np.array_equal(a, b)
    c0, c1 = generate_pastel_colors(2)
    assert tuple(a[20, 30]) == c0 and tuple(a[24, 30]) == c0 and tuple(a[25, 30]) == (255, 255, 255)   # 5 px wide
    assert tuple(a[10, 75]) == c1
    out = tmp_path / "boxes.png"
    d = draw_boxes(im, [[0.1, 0.5, 0.5, 0.9]], scores=None, output_path=str(out))        # no scores: no label tab
    assert np.array_equal(np.asarray(Image.open(out)), np.asarray(d))
    d = np.asarray(d)
    assert tuple(d[40, 30]) == generate_pastel_colors(1)[0] and tuple(d[42, 30]) != (255, 255, 255) \
        and tuple(d[43, 30]) == (255, 255, 255)                                          # 3 px wide
    assert (d[:40] == 255).all()
    e = np.asarray(draw_boxes(str(out), [[0.1, 0.5, 0.5, 0.9]], scores=[0.5], show_scores=False))
    assert np.array_equal(e, d)
    f = np.asarray(draw_boxes(im, [[0.1, 0.5, 0.5, 0.9]], scores=[0.5]))
    tab = generate_pastel_colors(1)[0]                                                   # 20 px high, 4 * 16 + 4 wide
    assert tuple(f[21, 77]) == tab and tuple(f[21, 78]) == tab and tuple(f[21, 79]) == (255, 255, 255)
    assert (f[:20] == 255).all() and (f[21:39, 11:77] != np.asarray(tab)).any()          # text on the tab


def test_shim_exports_the_reference_surface():
    import InkLayer.utils.visualization as V
    want = {
        "generate_pastel_colors": [("n_colors", inspect.Parameter.empty)],
        "color_sketch_by_masks": [("sketch_image_pil", inspect.Parameter.empty), ("seg_masks", inspect.Parameter.empty),
                                  ("colors", None), ("enhance_factor", 1.5), ("min_opacity", 0.2)],
        "get_background_idxs": [("sketch", inspect.Parameter.empty), ("seg_masks", inspect.Parameter.empty)],
        "draw_norm_bbox_on_image": [("image_pil", inspect.Parameter.empty), ("bboxes", inspect.Parameter.empty),
                                    ("pred_phrases", None), ("color", (255, 0, 0)), ("thickness", 5)],
        "draw_boxes": [("image", inspect.Parameter.empty), ("boxes", inspect.Parameter.empty), ("scores", None),
                       ("labels", None), ("line_width", 3), ("font_size", 16), ("show_scores", True), ("output_path", None)],
    }
    for name, params in want.items():
        got = [(p.name, p.default) for p in inspect.signature(getattr(V, name)).parameters.values()]
        assert got == params, name
    from InkLayer.utils.visualization import color_sketch_by_masks, draw_norm_bbox_on_image, generate_pastel_colors, draw_boxes  # noqa: F401


def test_shim_colour_function_takes_pil_and_array_masks():
    from InkLayer.utils.visualization import color_sketch_by_masks, get_background_idxs
    _, sketch, masks, _ = next(c for c in vis_cases.synthetic_cases() if c[0] == "overlapping masks")
    want = vis_ref.color_sketch_by_masks(sketch, masks, visualize.pastel_colors(len(masks)))
    pil = Image.fromarray(sketch)
    forms = [[Image.fromarray(m) for m in masks],                                   # mode "1", as the reference's runner
             [Image.fromarray(m.astype(np.uint8) * 255) for m in masks],           # mode "L"
             [m.astype(np.uint8) for m in masks], masks]
    assert forms[0][0].mode == "1" and forms[1][0].mode == "L"
    for f in forms:
        got = color_sketch_by_masks(pil, f)
        assert isinstance(got, Image.Image) and got.mode == "RGB" and np.array_equal(np.asarray(got), want)
    gray = Image.fromarray(sketch).convert("L")                                    # single-channel sketch
    assert np.array_equal(np.asarray(color_sketch_by_masks(gray, masks)),
                          vis_ref.color_sketch_by_masks(np.asarray(gray), masks, visualize.pastel_colors(len(masks))))
    bg = get_background_idxs(np.asarray(gray), masks)
    assert bg.dtype == bool and np.array_equal(bg, ~np.any(masks, axis=0))
    with pytest.raises(IndexError):
        color_sketch_by_masks(pil, masks, colors=[(1, 2, 3)])


# The stand-ins of tests/test_config5_cpu.py for the GPU plugins (copied: a test module does not import another), with
# a detector that answers three boxes.
FAKES = textwrap.dedent('''
    import numpy as np, torch
    from PIL import Image
    import InkLayer.runner as R
    import InkLayer.refinement.mask_cleaner as MC
    import InkLayer.refinement.bbox_filter as BF
    import InkLayer.refinement.refiner as RF
    from inklayer_amd import refine_stage
    from oracle import refine4_ref

    BOXES = [[0.1, 0.2, 0.5, 0.6], [0.3333, 0.25, 0.9, 0.8], [0.05, 0.05, 0.6, 0.45]]

    def fake_sam(image_pil, boxes_filt):
        W, H = image_pil.size
        ms = []
        for b in boxes_filt.tolist():
            m = np.zeros((H, W), dtype=bool)
            m[int(b[1]):int(b[3]), int(b[0]):int(b[2])] = True
            ms.append(m)
        return ms

    def install():
        R.run_ft_dino_on_sketch = lambda sketch_path: {"bboxes": BOXES, "scores": [0.9, 0.4, 0.35], "labels": ["object"] * 3}
        R.run_SAM = fake_sam
        MC.clean_masks_on_device = lambda masks: np.stack([np.asarray(m, dtype=np.uint8) * 255 for m in masks])
        BF.process_json_with_sketch_NMS = lambda sp, md, d, iou_threshold=0.2, cleaned_masks=None, sketch_rgb=None: {
            "bboxes": d["bboxes"][:2], "scores": d["scores"][:2], "kept_indices": [0, 1], "threshold": iou_threshold}
        RF.get_depth_map_device = lambda path, sketch_rgb=None: torch.from_numpy(np.tile(
            np.linspace(0, 3, Image.open(path).size[0], dtype=np.float32), (Image.open(path).size[1], 1)))
        RF._stack_on_gpu = lambda masks, shape: torch.from_numpy(np.stack([(np.asarray(m) > 0) for m in masks]).astype(np.uint8))

        def fake_stage(masks, boxes, rgb, depth, **kw):
            ms = [m.numpy() * 255 for m in masks]
            dis, sboxes, info = refine4_ref.parse_masks_to_disjoint_masks(ms, boxes, rgb, depth.numpy())
            fin = refine4_ref.improve_sam_masks(rgb, dis, sboxes)
            lab = lambda lst: sum(((np.asarray(m) > 0).astype(np.uint8) * (i + 1) for i, m in enumerate(lst)),
                                  np.zeros(rgb.shape[:2], np.uint8))
            extra = np.asarray(fin[-1]) > 0 if len(fin) > len(dis) else None
            return refine_stage.RefineResult([], [], sboxes, lab(dis), len(dis), info, lab(fin[:len(dis)]), extra)
        refine_stage.refine_masks = fake_stage
''')


@pytest.fixture
def restore_plugins():
    import InkLayer.runner as R
    import InkLayer.refinement.mask_cleaner as MC
    import InkLayer.refinement.bbox_filter as BF
    import InkLayer.refinement.refiner as RF
    from inklayer_amd import refine_stage
    saved = [(m, k, getattr(m, k)) for m, k in ((MC, "clean_masks_on_device"), (BF, "process_json_with_sketch_NMS"),
                                                (RF, "get_depth_map_device"), (RF, "_stack_on_gpu"),
                                                (refine_stage, "refine_masks"), (R, "run_ft_dino_on_sketch"), (R, "run_SAM"))]
    yield
    for m, k, v in saved:
        setattr(m, k, v)


def test_runner_writes_the_reference_visualisations(tmp_path, restore_plugins):
    ns = {}
    exec(FAKES, ns)
    ns["install"]()
    import InkLayer.runner as R
    from InkLayer.utils.processing import process_dino_output
    from InkLayer.utils.visualization import color_sketch_by_masks, draw_boxes, draw_norm_bbox_on_image
    assert not hasattr(R, "colour_by_masks") and not hasattr(R, "_draw_boxes")
    w, h = 80, 60
    a = np.full((h, w, 3), 255, np.uint8)
    a[h // 3: h // 3 + 3, 5: w - 5] = 0
    a[5: h - 5, w // 2: w // 2 + 2] = 90
    a[40:44, 3:70] = (200, 120, 240)                                   # a coloured, lighter stroke
    src = tmp_path / "sk.v1.png"
    Image.fromarray(a).save(src)
    out = Path(R.run_inklayer_pipeline(str(src), str(tmp_path / "out")))
    pil = Image.open(out / "input.png").convert("RGB")
    assert np.array_equal(np.asarray(pil), a)
    # segmented_sketch.png = color_sketch_by_masks(input, the masks the segmentor returned) (runner.py:49-52, 61)
    boxes_tensor, _ = process_dino_output({"bboxes": ns["BOXES"], "scores": [0.9, 0.4, 0.35], "labels": ["object"] * 3}, pil)
    masks = ns["fake_sam"](pil, boxes_tensor)
    got = np.asarray(Image.open(out / "segmented_sketch.png"))
    assert np.array_equal(got, np.asarray(color_sketch_by_masks(pil, [Image.fromarray(m) for m in masks])))
    assert np.array_equal(got, vis_ref.color_sketch_by_masks(a, masks, visualize.pastel_colors(3)))
    assert (got != a).any()
    # segmented_sketch_final.png = the same of masks_final/ (refiner.py:360-362)
    finals = [np.asarray(Image.open(out / "masks_final" / f"mask_{i}.png")) > 0
              for i in range(len(list((out / "masks_final").iterdir())))]
    got = np.asarray(Image.open(out / "segmented_sketch_final.png"))
    assert np.array_equal(got, vis_ref.color_sketch_by_masks(a, finals, visualize.pastel_colors(len(finals))))
    # bboxes.png / bboxes_final.png through the shim's drawing functions
    boxes_int = [[int(v) for v in b] for b in boxes_tensor.tolist()]
    assert np.array_equal(np.asarray(Image.open(out / "bboxes.png")),
                          np.asarray(draw_norm_bbox_on_image(pil, boxes_int, ["object"] * 3)))
    import json
    kept = json.loads((out / "bboxes_final.json").read_text())
    assert np.array_equal(np.asarray(Image.open(out / "bboxes_final.png")),
                          np.asarray(draw_boxes(pil, kept["bboxes"], kept["scores"])))
