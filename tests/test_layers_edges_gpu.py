"""Layer assembly at its geometry edges (csrc/layers.hip, the component machinery of csrc/bitplane.h, inklayer_amd/layers.py)
against the numpy / scipy restatement tests/layers_ref.py, bit for bit: no tolerance anywhere.  The shapes and planes come
from tests/layers_cases.py, and tests/test_layers_cases_cpu.py shows on the CPU which branch each of them reaches (a
wave's second seam, more than 64 runs in a row, the second 64-word chunk, rows without tail bits, the hole rule's
thresholds, the record cap, ties between components, chamfer tiles of every kind)."""
import functools

import numpy as np
import pytest
import torch

import layers_cases as K
import layers_ref as R

pytestmark = pytest.mark.gpu

BIG = [s for s in K.EDGE_SHAPES if min(s) >= 64]


def _eq(got, want):
    got = got.cpu() if torch.is_tensor(got) else torch.from_numpy(np.ascontiguousarray(got))
    want = want.cpu() if torch.is_tensor(want) else torch.from_numpy(np.ascontiguousarray(want))
    return got.dtype == want.dtype and torch.equal(got, want)


def _planes(bits, dev):
    from inklayer_amd import layers
    bits = np.asarray(bits, bool)
    return layers.pack_planes(bits if bits.ndim == 3 else bits[None], dev)


def _bits(planes, W):
    """The planes as bool [n, H, W]; the tail bits of every row's last word must be 0."""
    a = np.unpackbits(planes.cpu().numpy().view(np.uint8), axis=-1, bitorder="little")
    assert not a[..., W:].any(), "tail bits set"
    return a[..., :W].astype(bool)


def _chunks(planes, k=4):
    return [np.stack(planes[i:i + k]) for i in range(0, len(planes), k)]


@pytest.mark.parametrize("shape", K.EDGE_SHAPES)
def test_otsu_planes(dev, shape):
    from inklayer_amd import ops
    H, W = shape
    rng = np.random.default_rng(5)
    two = np.where(K.noise(shape, 0.3, 6), 40, 200).astype(np.uint8)
    ramp = (np.arange(H * W).reshape(shape) % 256).astype(np.uint8)
    gray = np.stack([rng.integers(0, 256, shape, dtype=np.uint8), np.full(shape, 77, np.uint8), two, ramp])
    for invert in (True, False):
        planes, hist, thresh = ops.layers_otsu_planes(torch.from_numpy(gray).to(dev), invert=invert)
        got = _bits(planes, W)
        for k in range(4):
            v = 255 - gray[k] if invert else gray[k]
            h = R.histogram(v)
            assert _eq(hist[k], h.astype(np.int32)), (k, invert)
            assert int(thresh[k]) == R.otsu_from_hist(h), (k, invert)
            assert _eq(got[k], v > R.otsu_from_hist(h)), (k, invert)
        assert int(thresh[1]) == 0 and got[1].all()                     # a constant image


@pytest.mark.parametrize("shape", K.EDGE_SHAPES)
def test_dilation(dev, shape):
    from inklayer_amd import ops
    H, W = shape
    stack = np.stack(K.dilate_planes(shape))
    p = _planes(stack, dev)
    for k in (3, 5):
        for it in (1, 2, 7, 8):                                          # both parities of the tmp / out ping-pong
            got = _bits(ops.layers_dilate(p, W, k, it), W)
            for i, a in enumerate(stack):
                assert _eq(got[i], R.dilate(a, k, it)), (k, it, i)


@pytest.mark.parametrize("shape", K.EDGE_SHAPES)
def test_border_band(dev, shape):
    from inklayer_amd import ops
    H, W = shape
    for band in (1, 2, 3, min(H, W) // 2 + 1):
        stack = np.concatenate([K.band_planes(shape, band), np.stack([K.noise(shape, 0.01, 70)])])
        flags = ops.layers_border_band(_planes(stack, dev), W, band).cpu().tolist()
        assert flags == [int(R.touches_band(s, band)) for s in stack], band


@pytest.mark.parametrize("shape", K.EDGE_SHAPES)
def test_flood_from_the_corner(dev, shape):
    from inklayer_amd import ops
    H, W = shape
    for stack in _chunks(K.flood_planes(shape)):
        sil, hdr = ops.layers_components(_planes(stack, dev), W, "flood")
        assert int(hdr[0]) == 0
        got = _bits(sil, W)
        for k, a in enumerate(stack):
            assert _eq(got[k], K.corner_flood_complement(a)), k


@pytest.mark.parametrize("shape", K.EDGE_SHAPES)
def test_fill_all_holes(dev, shape):
    from inklayer_amd import ops
    H, W = shape
    for stack in _chunks(K.fill_all_planes(shape)):
        out, hdr = ops.layers_components(_planes(stack, dev), W, "fill_all")
        assert int(hdr[0]) == 0
        got = _bits(out, W)
        for k, a in enumerate(stack):
            assert _eq(got[k], R.fill_enclosed_regions(a)), k


def _check_records(h, stack):
    """The header's undecided holes are the ones the restated rule leaves undecided, with their boxes and own areas."""
    want = {(k,) + t["first"]: t for k, a in enumerate(stack) for t in K.hole_table(a) if t["undecided"]}
    assert int(h[1]) == len(want)
    recs = h[2:2 + 8 * min(int(h[1]), 64)].reshape(-1, 8)
    assert sorted((int(r[0]), int(r[6]), int(r[7])) for r in recs) == sorted(want)
    for r in recs:
        t = want[(int(r[0]), int(r[6]), int(r[7]))]
        assert tuple(int(v) for v in r[1:5]) == t["box"] and int(r[5]) == t["own2"]


@pytest.mark.parametrize("shape", K.EDGE_SHAPES)
def test_fill_rule_with_undecided_holes(dev, shape):
    from inklayer_amd import layers, ops
    H, W = shape
    for c, stack in enumerate(K.fill_rule_calls(shape)):
        p = _planes(stack, dev)
        out, hdr = ops.layers_components(p, W, "fill_rule")
        h = hdr.cpu().numpy()
        assert h[0] == 0
        _bits(out, W)
        _check_records(h, stack)
        got = _bits(layers._resolve_undecided(p, out, W, h), W)
        for k, a in enumerate(stack):
            assert _eq(got[k], R.fill_holes_not_touching_border(a)), (c, k)


def test_undecided_cap_is_per_call(dev):
    from inklayer_amd import layers, ops
    from inklayer_amd._lib import InkLayerHipError
    H, W = K.RING_GRID_SHAPE

    def run(stack):
        p = _planes(stack, dev)
        out, hdr = ops.layers_components(p, W, "fill_rule")
        h = hdr.cpu().numpy()
        assert h[0] == 0
        return p, out, h
    full = K.ring_grid(64)
    p, out, h = run(full[None])
    _check_records(h, full[None])
    assert h[1] == 64 and _eq(_bits(layers._resolve_undecided(p, out, W, h), W)[0], R.fill_holes_not_touching_border(full))
    p, out, h = run(K.ring_grid(65)[None])
    assert h[1] == 65
    with pytest.raises(InkLayerHipError):
        layers._resolve_undecided(p, out, W, h)
    forty = K.ring_grid(40)
    p, out, h = run(np.stack([forty, forty]))
    assert h[1] == 80
    with pytest.raises(InkLayerHipError):
        layers._resolve_undecided(p, out, W, h)
    want = R.fill_holes_not_touching_border(forty)
    for _ in range(2):
        p, out, h = run(forty[None])
        _check_records(h, forty[None])
        assert h[1] == 40 and _eq(_bits(layers._resolve_undecided(p, out, W, h), W)[0], want)


@pytest.mark.parametrize("shape", K.EDGE_SHAPES)
def test_largest_component(dev, shape):
    from inklayer_amd import ops
    H, W = shape
    for stack in _chunks(K.largest_planes(shape)):
        out, hdr = ops.layers_components(_planes(stack, dev), W, "largest")
        assert int(hdr[0]) == 0
        got = _bits(out, W)
        for k, a in enumerate(stack):
            assert _eq(got[k], R.largest_component(a) if a.any() else a), k


@functools.lru_cache(maxsize=None)
def _chamfer_case(shape):
    masks = np.stack([m for _, m in K.chamfer_masks(shape)])
    return masks, np.stack([R.chamfer_fixed(m) for m in masks])


def _chamfer_expect(want, mask, strokes, margin):
    """(min or None without strokes, shrink_by, thresholded plane) of one plane by the restatement."""
    if not strokes.any():
        return None, 0, mask
    f = R.dist_float(want)
    s = max(0, int(np.floor(f[strokes].min())) - margin)
    return int(want[strokes].min()), s, (f >= np.float32(s)) if s > 0 else mask


@pytest.mark.parametrize("kind", ["subset", "empty", "on_zero"])
@pytest.mark.parametrize("shape", K.EDGE_SHAPES)
def test_chamfer_full(dev, shape, kind):
    from inklayer_amd import ops
    H, W = shape
    masks, want = _chamfer_case(shape)
    strokes = K.chamfer_strokes(masks, kind)
    mp, sp = _planes(masks, dev), _planes(strokes, dev)
    for margin in (0, 1, 40):
        dist, mn, shrink, thr = ops.layers_chamfer(mp, sp, W, margin, full=True)
        assert _eq(dist, want)
        got = _bits(thr, W)
        for k in range(len(masks)):
            m, s, plane = _chamfer_expect(want[k], masks[k], strokes[k], margin)
            assert m is None or int(mn[k]) == m, (k, margin)
            assert int(shrink[k]) == s and _eq(got[k], plane), (k, margin)
            if kind == "on_zero" and not masks[k].all():
                assert int(mn[k]) == 0 and int(shrink[k]) == 0


@pytest.mark.parametrize("kind", ["subset", "empty", "on_zero"])
@pytest.mark.parametrize("shape", K.EDGE_SHAPES)
def test_chamfer_early_exit(dev, shape, kind):
    from inklayer_amd import ops
    H, W = shape
    masks, want = _chamfer_case(shape)
    strokes = K.chamfer_strokes(masks, kind)
    mp, sp = _planes(masks, dev), _planes(strokes, dev)
    for margin in (0, 1, 40):
        _, mn1, shrink1, thr1 = ops.layers_chamfer(mp, sp, W, margin, full=True)
        dist, mn, shrink, thr = ops.layers_chamfer(mp, sp, W, margin, full=False)
        assert _eq(mn, mn1) and _eq(shrink, shrink1) and _eq(thr, thr1), margin
        _bits(thr, W)
        d = dist.cpu().numpy()
        for k in range(len(masks)):
            below = want[k].astype(np.int64) < int(mn[k]) + 65536
            assert np.array_equal(d[k][below], want[k][below]) and (d[k] >= want[k]).all(), (k, margin)


def _ref_bbox(m):
    H, W = m.shape
    return R.mask_to_bbox(m) if (m > 127).any() else [W, H, -1, -1]


@pytest.mark.parametrize("n", [1, 40])
@pytest.mark.parametrize("shape", K.EDGE_SHAPES)
def test_mask_tables(dev, shape, n):
    from inklayer_amd import ops
    masks = K.object_masks(shape, n, n)
    bbox, overlap = ops.layers_mask_tables(torch.from_numpy(masks).to(dev))
    boxes = [_ref_bbox(m) for m in masks]
    assert bbox.cpu().tolist() == boxes
    want = [[j for j in range(i) if R.mask_within_bbox(masks[i] > 0, boxes[j]).any()] for i in range(n)]
    assert [np.nonzero(r)[0].tolist() for r in overlap.cpu().numpy()] == want
    if n == 40:
        assert boxes[3] == [shape[1], shape[0], -1, -1] and not overlap[:, 3].any() and not overlap[3].any()
        assert all(0 not in want[i] for i in (6, 7))


@pytest.mark.parametrize("shape", BIG)
def test_assembly_composite_and_rgba(dev, shape):
    from inklayer_amd import layers, ops
    H, W = shape
    masks, rgb = K.layer_masks(shape)
    md, rd = torch.from_numpy(masks).to(dev), torch.from_numpy(rgb).to(dev)
    fake = np.random.default_rng(1).integers(0, 256, rgb.shape, dtype=np.uint8)
    cache = {}
    want = [R.assemble(rgb, masks, i, cache) for i in range(6)]
    got = layers.assemble_layers(rgb, md)
    edits = 0
    for i, (l, w) in enumerate(zip(got, want)):
        assert _eq(l.sketch_layer, w["sketch_layer"]) and l.overlaps == w["overlaps"], i
        assert (l.edit_mask is None) == (w["edit_mask"] is None), i
        if i == 0:
            assert l.debug_vis is None
        elif w["edit_mask"] is None:
            assert _eq(l.debug_vis.cpu().numpy() > 0, w["debug_vis"]), i
        else:
            edits += 1
            assert _eq(l.edit_mask.cpu().numpy() > 0, w["edit_mask"]) and _eq(l.debug_vis, w["debug_vis"]), i
            fin = R.composite(fake, w["sketch_layer"], w["original_sketch_mask"])
            assert _eq(layers.composite(fake, l.sketch_layer), fin), i
            assert _eq(ops.layers_composite(torch.from_numpy(fake).to(dev), l.sketch_layer.contiguous()), fin), i
    assert edits >= 1
    # the kernel on tables and planes handed over directly
    bbox, overlap = ops.layers_mask_tables(md)
    bg = torch.zeros((6, H, (W + 63) // 64), device=dev, dtype=torch.int64)
    for j, b in cache.items():
        bg[j] = _planes(b, dev)[0]
    sk, ed, dbg = ops.layers_assemble(rd, md, bg, bbox, overlap)
    for i, w in enumerate(want):
        assert _eq(sk[i], w["sketch_layer"]), i
        assert _eq(ed[i].cpu().numpy() > 0, w["edit_mask"] if w["edit_mask"] is not None else np.zeros(shape, bool)), i
    # grey conversion and RGBA layers
    files = np.stack([rgb] + [np.repeat(K.grey_of(p)[..., None], 3, 2) for p in K.sketch_planes(shape)[1:]])
    fd = torch.from_numpy(files).to(dev)
    gray = ops.layers_gray(fd)
    assert _eq(gray, np.stack([R.png_gray(f) for f in files]))
    rgba, branch, shrink = layers.rgba_layers(fd)
    for k in range(len(files)):
        assert _eq(rgba[k], R.rgba_layer(files[k])), k
    bgk, _, _ = layers.background_masks(gray, {})
    assert _eq(ops.layers_rgba(gray, bgk), rgba)


@pytest.mark.parametrize("shape", K.EDGE_SHAPES)
def test_background_masks(dev, shape):
    from inklayer_amd import layers
    H, W = shape
    gray = np.stack([K.grey_of(p) for p in K.sketch_planes(shape)])
    g = torch.from_numpy(gray).to(dev)
    seen = set()
    for params in K.BG_PARAM_SETS:
        planes, branch, shrink = layers.background_masks(g, params)
        got = _bits(planes, W)
        for k in range(len(gray)):
            m, b, s = R.get_mask(gray[k], **params)
            assert (branch[k], shrink[k]) == (b, s), (k, params)
            assert _eq(got[k], m), (k, params)
        seen |= set(branch)
    assert seen == ({"open-curve", "closed-silhouette"} if shape in BIG else {"open-curve"})
