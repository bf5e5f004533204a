"""Layer assembly on the GPU (csrc/layers.hip, inklayer_amd/layers.py, InkLayer/inpainting) against the numpy / scipy
restatement tests/layers_ref.py: every kernel bit for bit at 70 x 130 and 130 x 70 (two plane words per row with a
ragged tail / one ragged word; more rows than one 32-row component band; a chamfer tile edge inside the image), then
the whole stage on two of the reference's own output sets, every written PNG pixel for pixel."""
import os

import numpy as np
import pytest
import torch

import layers_cases as K
import layers_ref as R
from test_layers_ref_cpu import load_set

pytestmark = pytest.mark.gpu


def _eq(got, want):
    got = got.cpu() if torch.is_tensor(got) else torch.from_numpy(np.ascontiguousarray(got))
    want = want.cpu() if torch.is_tensor(want) else torch.from_numpy(np.ascontiguousarray(want))
    return got.dtype == want.dtype and torch.equal(got, want)


def _planes(bits, dev):
    from inklayer_amd import layers
    bits = np.asarray(bits, bool)
    return layers.pack_planes(bits if bits.ndim == 3 else bits[None], dev)


def _bits(planes, W):
    from inklayer_amd import layers
    return layers.unpack_planes(planes, W)


@pytest.mark.parametrize("shape", K.SHAPES)
def test_histogram_otsu_and_threshold(dev, shape):
    from inklayer_amd import ops
    H, W = shape
    two = np.full(shape, 255, np.uint8)
    two[10:20, 10:40] = 0
    ramp = (np.arange(H * W).reshape(shape) * 7 % 251).astype(np.uint8)
    ramp[::3] //= 2
    gray = np.stack([two, ramp, K.closed_sketch(shape)])
    for invert in (True, False):
        planes, hist, thresh = ops.layers_otsu_planes(torch.from_numpy(gray).to(dev), invert=invert)
        torch.cuda.synchronize()
        for k in range(3):
            v = 255 - gray[k] if invert else gray[k]
            h = R.histogram(v)
            assert _eq(hist[k], h.astype(np.int32))
            t = R.otsu_from_hist(h)
            assert int(thresh[k]) == t
            assert _eq(_bits(planes, W)[k], v > t)
    assert int(thresh[1]) not in (0, 255)


@pytest.mark.parametrize("shape", K.SHAPES)
def test_ellipse_dilation_at_the_image_edge(dev, shape):
    from inklayer_amd import ops
    H, W = shape
    a = np.zeros(shape, bool)
    a[0, 0] = a[H - 1, W - 1] = a[0, W - 1] = a[H // 2, 63] = a[H // 2 + 9, 64] = a[H - 1, 5] = a[33, 0] = True
    p = _planes(a, dev)
    for k, its in ((5, (1, 2, 10)), (3, (1, 5))):
        for it in its:
            assert _eq(_bits(ops.layers_dilate(p, W, k, it), W)[0], R.dilate(a, k, it)), (k, it)
    one = R.dilate(np.pad(np.ones((1, 1), bool), 3), 5, 1)
    assert one.sum() == 17 and not one[1, 1] and one[1, 3] and one[2, 1]          # rows of half width 0, 2, 2, 2, 0


@pytest.mark.parametrize("shape", K.SHAPES)
def test_border_band(dev, shape):
    from inklayer_amd import ops
    H, W = shape
    pts = [(2, 40), (3, 40), (H - 3, 9), (H - 4, 9), (30, 2), (30, 3), (31, W - 3), (31, W - 4), (H // 2, W // 2)]
    stack = np.zeros((len(pts),) + shape, bool)
    for k, (y, x) in enumerate(pts):
        stack[k, y, x] = True
    for band in (2, 3):
        flags = ops.layers_border_band(_planes(stack, dev), W, band).cpu().numpy()
        assert flags.tolist() == [int(R.touches_band(s, band)) for s in stack], band
    assert ops.layers_border_band(_planes(stack, dev), W, 3).cpu().tolist() == [1, 0, 1, 0, 1, 0, 1, 0, 0]


@pytest.mark.parametrize("shape", K.SHAPES)
def test_flood_from_the_corner_is_four_connected(dev, shape):
    from scipy import ndimage
    from inklayer_amd import ops
    H, W = shape
    a = K.diagonal_gap(shape)
    sil, hdr = ops.layers_components(_planes(a, dev), W, "flood")
    lab4, _ = ndimage.label(~a, structure=R.CROSS)
    lab8, _ = ndimage.label(~a, structure=R.ONES3)
    want4, want8 = ~(lab4 == lab4[0, 0]), ~(lab8 == lab8[0, 0])
    assert int(hdr[0]) == 0 and _eq(_bits(sil, W)[0], want4)
    assert not np.array_equal(want4, want8)
    b = a.copy()
    b[0, 0] = True                                        # a set seed pixel: nothing is flooded
    assert _bits(ops.layers_components(_planes(b, dev), W, "flood")[0], W)[0].all()


@pytest.mark.parametrize("shape", K.SHAPES)
def test_hole_filling_with_islands(dev, shape):
    from inklayer_amd import layers, ops
    H, W = shape
    a = K.holes_image(shape)
    stack = np.stack([a, K.two_components(shape), np.zeros(shape, bool), np.ones(shape, bool)])
    p = _planes(stack, dev)
    got, hdr = ops.layers_components(p, W, "fill_all")
    assert int(hdr[0]) == 0
    for k in range(4):
        assert _eq(_bits(got, W)[k], R.fill_enclosed_regions(stack[k])), k
    got, hdr = ops.layers_components(p, W, "fill_rule")
    h = hdr.cpu().numpy()
    assert h[0] == 0 and h[1] == 1 and h[2] == 0 and h[7] == 92        # D: undecided, twice 46 of the area 62 it surrounds
    assert int((_bits(got, W)[0] & ~a).sum()) == 42 + (34 * 24 - 22 * 15) + 16
    fixed = layers._resolve_undecided(p, got, W, h)
    for k in range(4):
        assert _eq(_bits(fixed, W)[k], R.fill_holes_not_touching_border(stack[k])), k


@pytest.mark.parametrize("shape", K.SHAPES)
def test_largest_component_by_contour_area(dev, shape):
    from inklayer_amd import ops
    H, W = shape
    stack = np.stack([K.two_components(shape), K.equal_components(shape), K.blob(shape)])
    got, hdr = ops.layers_components(_planes(stack, dev), W, "largest")
    assert int(hdr[0]) == 0
    for k in range(3):
        assert _eq(_bits(got, W)[k], R.largest_component(stack[k])), k


@pytest.mark.parametrize("shape", K.SHAPES)
def test_chamfer_distance_across_tiles(dev, shape):
    from inklayer_amd import ops
    H, W = shape
    masks = np.stack([K.blob(shape), R.largest_component(R.dilate(K.closed_sketch(shape) < 128, 3, 5))])
    strokes = np.stack([K.blob_strokes(shape), K.closed_sketch(shape) < 128])
    want = np.stack([R.chamfer_fixed(m) for m in masks])
    assert want.max() > 16 * 65536                                     # more than the 8 moves one launch can see
    mp, sp = _planes(masks, dev), _planes(strokes, dev)
    for margin in (0, 1, 40):
        dist, mn, shrink, thr = ops.layers_chamfer(mp, sp, W, margin, full=True)
        assert _eq(dist, want)
        for k in range(2):
            m = int(want[k][strokes[k]].min())
            s = max(0, int(np.floor(R.dist_float(want[k])[strokes[k]].min())) - margin)
            assert int(mn[k]) == m and int(shrink[k]) == s
            assert _eq(_bits(thr, W)[k], R.dist_float(want[k]) >= np.float32(s) if s > 0 else masks[k]), (k, margin)
    dist, mn, shrink, thr2 = ops.layers_chamfer(mp, sp, W, 1, full=False)       # stops early: exact below the bound only
    d = dist.cpu().numpy()
    for k in range(2):
        below = want[k] < int(mn[k]) + 65536
        assert int(mn[k]) == int(want[k][strokes[k]].min()) and np.array_equal(d[k][below], want[k][below])
        assert (d[k] >= want[k]).all()
    ref1 = ops.layers_chamfer(mp, sp, W, 1, full=True)[3]
    assert _eq(thr2, ref1)


@pytest.mark.parametrize("shape", K.SHAPES)
def test_get_mask_both_branches(dev, shape):
    from inklayer_amd import layers
    H, W = shape
    gray = np.stack([K.closed_sketch(shape), K.open_sketch(shape), 255 - K.overlap_masks(shape)[0]])
    g = torch.from_numpy(gray).to(dev)
    for params in ({}, dict(safety_margin=10), layers.OVERLAP_PARAMS, dict(kernel_size=5, dilate_iter=2, border_band=3)):
        planes, branch, shrink = layers.background_masks(g, params)
        got = _bits(planes, W)
        for k in range(3):
            m, b, s = R.get_mask(gray[k], **params)
            assert (branch[k], shrink[k]) == (b, s), (k, params)
            assert _eq(got[k], m), (k, params)
    _, branch, shrink = layers.background_masks(g, {})
    assert branch[:2] == ["closed-silhouette", "open-curve"] and shrink[0] == 4
    assert layers.background_masks(g, dict(safety_margin=10))[2][0] == 0
    bright = layers.background_masks(torch.from_numpy(K.overlap_masks(shape)[:1]).to(dev), {}, strokes_bright=True)
    assert _eq(_bits(bright[0], W)[0], R.get_mask(gray[2])[0])


@pytest.mark.parametrize("shape", K.SHAPES)
def test_assembly_composite_and_rgba(dev, shape):
    from inklayer_amd import layers, ops
    H, W = shape
    masks, rgb = K.overlap_masks(shape), K.coloured_sketch(shape)
    md = torch.from_numpy(masks).to(dev)
    bbox, overlap = ops.layers_mask_tables(md)
    assert bbox.cpu().tolist() == [R.mask_to_bbox(m) for m in masks]
    assert [np.nonzero(r)[0].tolist() for r in overlap.cpu().numpy()] == [R.overlap_list(masks, i) for i in range(4)] \
        == [[], [], [], [0]]
    got = layers.assemble_layers(rgb, md)
    fake = np.random.default_rng(1).integers(0, 256, rgb.shape, dtype=np.uint8)
    for i, l in enumerate(got):
        want = R.assemble(rgb, masks, i)
        assert _eq(l.sketch_layer, want["sketch_layer"]) and l.overlaps == want["overlaps"]
        assert (l.edit_mask is None) == (want["edit_mask"] is None)
        if i == 0:
            assert l.debug_vis is None
        elif want["edit_mask"] is None:
            assert _eq(l.debug_vis.cpu().numpy() > 0, want["debug_vis"])
        else:
            assert _eq(l.edit_mask.cpu().numpy() > 0, want["edit_mask"]) and _eq(l.debug_vis, want["debug_vis"])
            fin = R.composite(fake, want["sketch_layer"], want["original_sketch_mask"])
            assert _eq(layers.composite(fake, l.sketch_layer), fin)
            assert _eq(ops.layers_composite(torch.from_numpy(fake).to(dev), l.sketch_layer.contiguous()), fin)
    assert tuple(got[3].sketch_layer[15, 18].tolist()) == (90, 30, 200)
    # tables and planes handed over directly
    bgp, _, _ = layers.background_masks(md[:1], layers.OVERLAP_PARAMS, strokes_bright=True)
    bg = torch.zeros((4,) + tuple(bgp.shape[1:]), device=dev, dtype=torch.int64)
    bg[0] = bgp[0]
    sk, ed, dbg = ops.layers_assemble(torch.from_numpy(rgb).to(dev), md, bg, bbox, overlap)
    assert _eq(ed[3].cpu().numpy() > 0, R.assemble(rgb, masks, 3)["edit_mask"]) and not ed[:3].any()
    # RGBA layers
    files = np.stack([rgb, np.repeat(K.closed_sketch(shape)[..., None], 3, 2), np.repeat(K.open_sketch(shape)[..., None], 3, 2)])
    fd = torch.from_numpy(files).to(dev)
    gray = ops.layers_gray(fd)
    assert _eq(gray, np.stack([R.png_gray(f) for f in files]))
    rgba, branch, shrink = layers.rgba_layers(fd)
    for k in range(3):
        assert _eq(rgba[k], R.rgba_layer(files[k])), k
    bgk, _, _ = layers.background_masks(gray, {})
    assert _eq(ops.layers_rgba(gray, bgk), rgba)


# ---- the whole stage on the reference's own output sets --------------------------------------------------------------------
def _png(path):
    from PIL import Image
    return Image.open(path)


@pytest.mark.parametrize("name", ["fscoco_animals", "Clipasso_brushpen_0249"])
def test_whole_stage_reproduces_the_reference_files(dev, name, tmp_path):
    from PIL import Image
    import InkLayer.inpainting as reg
    from InkLayer.inpainting.fill_object_bg_mask import create_rgba_with_background_mask_on_dir
    from InkLayer.inpainting.inpaint_ControlNet import run_inpainting_on_sketch_dir
    from InkLayer.utils.io import flush
    S = load_set(name)
    d = tmp_path / name
    (d / "masks_final").mkdir(parents=True)
    Image.fromarray(S["input"]).save(d / "input.png")
    for i, m in enumerate(S["masks"]):
        Image.fromarray(m).save(d / "masks_final" / f"mask_{i}.png")
    calls = []

    def stored(input_image, mask_image):
        mask = np.asarray(mask_image) > 0
        hits = [i for i in S["index"] if np.array_equal(mask, S["edit"][i])]
        assert len(hits) >= 1 and mask_image.mode == "L" and input_image.mode == "RGB"
        i = [h for h in hits if h not in calls][0]
        assert np.array_equal(np.asarray(input_image), S["sketch"][i])
        calls.append(i)
        return Image.fromarray(S["inpainted"][S["index"].index(i)])

    old = reg.get_inpaint_func()
    reg.set_inpaint_func(stored)
    try:
        out = run_inpainting_on_sketch_dir(str(d))
        flush()
        rgba_dir = create_rgba_with_background_mask_on_dir(out, out.replace("layers", "layers_rgba"))
        flush()
    finally:
        reg.set_inpaint_func(old)
    assert calls == [i for i in range(S["n"]) if S["need"][i]]
    assert sorted(os.listdir(rgba_dir)) == sorted(os.listdir(out)) == sorted(f"layer_{i}.png" for i in range(S["n"]))
    for i in range(S["n"]):
        proc = d / "complete_layers_process" / f"mask_{i}"
        assert np.array_equal(np.asarray(_png(proc / "sketch_layer.png").convert("RGB")), S["sketch"][i]), i
        layer = np.asarray(_png(d / "complete_layers" / f"layer_{i}.png").convert("RGB"))
        if S["need"][i]:
            k = S["index"].index(i)
            assert np.array_equal(np.asarray(_png(proc / "edit_mask.png").convert("L")) > 0, S["edit"][i]), i
            assert _png(proc / "edit_mask.png").mode == "L"
            assert np.array_equal(np.asarray(_png(proc / "inpainted_image.png").convert("RGB")), S["inpainted"][k]), i
            assert np.array_equal(np.asarray(_png(proc / "final_composited.png").convert("RGB")), S["final"][k]), i
            assert np.array_equal(layer, S["final"][k]), i
            assert (proc / "debug_vis.png").exists()
        else:
            assert not (proc / "edit_mask.png").exists() and np.array_equal(layer, S["sketch"][i]), i
            assert (proc / "debug_vis.png").exists() == (i > 0)
        im = _png(d / "complete_layers_rgba" / f"layer_{i}.png")
        assert im.mode == "RGBA"
        r = np.asarray(im)
        assert np.array_equal(r[..., 3] > 0, S["alpha"][i]) and set(np.unique(r[..., 3]).tolist()) <= {0, 255}, i
        for c in range(3):
            assert np.array_equal(r[..., c], S["rgb"][i]), (i, c)


def test_runner_writes_the_layer_directories(dev, tmp_path, monkeypatch):
    """finish_sketch(inpaint=True) with a registered function: the three directories come out of the masks the
    refinement stage just made, and agree with the restatement run on the masks_final/ files it wrote."""
    from PIL import Image
    monkeypatch.setenv("INKLAYER_RANDOM_WEIGHTS", "1")
    import InkLayer.inpainting as reg
    import InkLayer.runner as RUN
    from PIL import ImageDraw
    H = W = 256
    # Two outlined right triangles that are opposite halves of overlapping boxes: the masks are made disjoint in depth
    # order, so a later mask keeps no pixel inside an earlier MASK - but each triangle has strokes inside the other's
    # BOX and outside its mask, so whichever comes first, the other one overlaps its box and needs inpainting.
    boxes = [(30, 40, 200, 180), (120, 100, 230, 220)]
    tris = [[(30, 40), (30, 180), (200, 180)], [(120, 100), (230, 100), (230, 220)]]
    sketch = Image.new("RGB", (W, H), (255, 255, 255))
    masks = []
    for tri in tris:
        ImageDraw.Draw(sketch).line(tri + tri[:1], fill=(0, 0, 0), width=3)
        m = Image.new("L", (W, H), 0)
        ImageDraw.Draw(m).polygon(tri, fill=255, outline=255)
        ImageDraw.Draw(m).line(tri + tri[:1], fill=255, width=5)
        masks.append(np.asarray(m) > 0)
    rgb = np.array(sketch)
    out_dir = tmp_path / "sk"
    out_dir.mkdir()
    pil = Image.fromarray(rgb)
    pil.save(out_dir / "input.png")
    seen = []

    def white(input_image, mask_image):
        seen.append(np.asarray(mask_image).copy())
        return Image.new("RGB", input_image.size, (250, 250, 250))

    old = reg.get_inpaint_func()
    reg.set_inpaint_func(white)
    try:
        RUN.finish_sketch(str(out_dir), pil, {"scores": [0.9, 0.8]}, torch.tensor(boxes, dtype=torch.float32), masks,
                          inpaint=True)
    finally:
        reg.set_inpaint_func(old)
    n = len(list((out_dir / "masks_final").glob("mask_*.png")))
    assert n >= 2 and len(seen) >= 1
    final = np.stack([np.asarray(Image.open(out_dir / "masks_final" / f"mask_{i}.png").convert("L")) for i in range(n)])
    k = 0
    for i in range(n):
        want = R.assemble(rgb, final, i, {})
        proc = out_dir / "complete_layers_process" / f"mask_{i}"
        assert np.array_equal(np.asarray(Image.open(proc / "sketch_layer.png")), want["sketch_layer"]), i
        layer = want["sketch_layer"]
        if want["edit_mask"] is not None:
            assert np.array_equal(seen[k] > 0, want["edit_mask"]), i
            assert np.array_equal(np.asarray(Image.open(proc / "edit_mask.png")) > 0, want["edit_mask"]), i
            layer = R.composite(np.full_like(rgb, 250), want["sketch_layer"], want["original_sketch_mask"])
            assert np.array_equal(np.asarray(Image.open(proc / "final_composited.png")), layer), i
            k += 1
        else:
            assert not (proc / "edit_mask.png").exists()
        assert np.array_equal(np.asarray(Image.open(out_dir / "complete_layers" / f"layer_{i}.png")), layer), i
        assert np.array_equal(np.asarray(Image.open(out_dir / "complete_layers_rgba" / f"layer_{i}.png")), R.rgba_layer(layer)), i
    assert k == len(seen)
    # without a function the tree and the message stay as before
    out2 = tmp_path / "sk2"
    out2.mkdir()
    pil.save(out2 / "input.png")
    RUN.finish_sketch(str(out2), pil, {"scores": [0.9, 0.8]}, torch.tensor(boxes, dtype=torch.float32), masks, inpaint=True)
    assert not (out2 / "complete_layers").exists() and (out2 / "masks_final").is_dir()
