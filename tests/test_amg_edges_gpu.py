"""The kernels of csrc/amg.hip at their edges, on the case lists of tests/amg_cases.py against tests/amg_ref.py (and, for
the stats op's floats, ops.sam_postprocess): the stats kernel's column loop, band arithmetic, box bookkeeping and strict
compares, the RLE kernel's chunks and carries, remove_small_regions on small planes and box NMS around its 64-box words.
Everything here is integer logic on floats that are bit for bit those of ops.sam_postprocess: every comparison is
exact.  tests/test_amg_edges_ref_cpu.py shows without a GPU that the lists tell plausible mistakes apart."""
import numpy as np
import pytest
import torch

import amg_cases as C
import amg_ref as R
from test_amg_gpu import _check_rle, ref_table

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------------------------------ 1. stats op
def _postprocess(low, geom):
    from inklayer_amd import ops
    crop_hw = geom[0]
    return ops.sam_postprocess(low, 1024, C.stats_input_hw(crop_hw), crop_hw, 0.0, want_logits=True)[1].cpu()


def _stats(low, geom, thr, off, **kw):
    from inklayer_amd import ops
    crop_hw, xy0, orig_hw = geom
    return ops.sam_amg_stats(low, 1024, C.stats_input_hw(crop_hw), crop_hw, thr, off, xy0, orig_hw, want_logits=True, **kw)


def _check_stats(low, want, geom, thr, off, index=None):
    """test_stats_op_exact's method: the floats of sam_postprocess, the table and the planes of amg_ref on them, no bit
    in rows >= orig_h (unpack_planes asserts it).  want: sam_postprocess's logits of `low` on the host."""
    (ch, cw), (x0, y0), orig_hw = geom
    oh, ow = orig_hw or (ch, cw)
    table, planes, lg = _stats(low, geom, thr, off, index=index)
    src = want if index is None else want[index.cpu().long()]
    assert torch.equal(lg.cpu(), src), "the stats kernel's floats are not those of ink_sam_postprocess"
    ref, masks = ref_table(src, thr, off)
    assert torch.equal(table.cpu().long(), ref), (table.cpu().tolist(), ref.tolist())
    assert torch.equal(C.unpack_planes(planes, oh), R.uncrop_masks(masks, [x0, y0, x0 + cw, y0 + ch], oh, ow))
    return ref, table, planes, lg


def _check_ties(low, want, geom, k):
    """thresholds read from mask k's logits: thr = its second-largest value with offset 0 (one pixel equals thr and only
    the maximum is above it), then thr +- offset on two logits that occur.  Returns the table row of the first."""
    thr = C.second_largest(want[k])
    assert (want[k] == np.float32(thr)).any() or want[k].numel() == 1, "no logit equals thr: the case tests no tie"
    ref, *_ = _check_stats(low, want, geom, thr, 0.0)
    assert ref[k, 0] == ref[k, 1] == ref[k, 2] == (want[k] > thr).sum()
    thr2, off2, a, b = C.tie_thresholds(want[k])
    assert (want[k] == np.float32(thr2 + off2)).any() and (want[k] == np.float32(thr2 - off2)).any()
    assert np.float32(thr2 + off2) == np.float32(a) and np.float32(thr2 - off2) == np.float32(b)
    ref2, *_ = _check_stats(low, want, geom, thr2, off2)
    assert ref2[k, 0] == (want[k] > np.float32(a)).sum() and ref2[k, 1] == (want[k] > np.float32(b)).sum()
    return ref[k]


@torch.no_grad()
@pytest.mark.parametrize("content", ["noise", "ramps"])
@pytest.mark.parametrize("g", range(len(C.STATS_GEOMS)), ids=lambda g: "%dx%d@%d,%d" % (C.STATS_GEOMS[g][0] + C.STATS_GEOMS[g][1]))
def test_stats_edges_exact(dev, g, content):
    geom = C.STATS_GEOMS[g]
    ch, cw = geom[0]
    low = C.stats_low(content, 300 + g).to(dev)
    want = _postprocess(low, geom)
    if content == "noise":
        ref, *_ = _check_stats(low, want, geom, 0.0, 1.0)
        print(ref.tolist())
        assert ref[2].tolist() == [0] * 8 and ref[3].tolist() == [ch * cw] * 3 + [0, 0, cw - 1, ch - 1, 0]
        if ch * cw >= 400:                     # the noise does what it is for: both stability thresholds cut
            assert all(0 < ref[k, 0] < ref[k, 2] < ref[k, 1] < ch * cw for k in (0, 1, 4))
        _check_stats(low, want, geom, 0.3, 0.7)
        _check_ties(low, want, geom, 0)
        # every compare a tie: all counts 0, the box [0, 0, 0, 0], the plane empty
        zero = torch.zeros(4, 256, 256, device=dev)
        assert not _postprocess(zero, geom).any()
        table, planes, lg = _stats(zero, geom, 0.0, 0.0)
        assert not table.any() and not planes.any() and not lg.any()
        return
    _check_stats(low, want, geom, -20.5, 6.25)
    for k, (bottom, right) in enumerate(C.RAMP_CORNERS):
        cy, cx = (ch - 1) * bottom, (cw - 1) * right
        assert want[k, cy, cx] == want[k].max(), "the ramp's maximum is not at its corner"
        row = _check_ties(low, want, geom, k)
        if ch * cw == 1:
            assert row.tolist() == [0] * 8                               # the one logit is thr itself
        elif C.stats_corner_is_shared(geom[0]):
            assert 1 <= row[2] <= 4
        else:
            assert row.tolist() == [1, 1, 1, cx, cy, cx, cy, 0], "one pixel, at the corner"
    _check_ties(low, want, geom, 4)


INDEX_GEOMS = [1, 10, 13, 16]      # rows form in a frame, one-pixel form full frame (planes beyond count unwritten), two crops


@torch.no_grad()
@pytest.mark.parametrize("g", INDEX_GEOMS)
def test_stats_index_and_count(dev, g):
    geom = C.STATS_GEOMS[g]
    low = C.stats_low("noise", 400 + g).to(dev)
    want = _postprocess(low, geom)
    n = len(low)
    for idx in ([2, 0, 2, 4, 1, 2], [4, 3, 2, 1, 0]):                    # a repeated entry; a permutation
        index = torch.tensor(idx, dtype=torch.int32, device=dev)
        _, table, planes, lg = _check_stats(low, want, geom, 0.0, 1.0, index=index)
        m = len(idx)
        for c in (0, 1, m):
            cnt = torch.tensor([c], dtype=torch.int32, device=dev)
            t2, p2, l2 = _stats(low, geom, 0.0, 1.0, index=index, count=cnt)
            assert torch.equal(t2[:c], table[:c]) and not t2[c:].any()
            assert torch.equal(p2[:c], planes[:c]) and torch.equal(l2[:c], lg[:c])
    _, table, planes, _ = _check_stats(low, want, geom, 0.0, 1.0)
    for c in (0, 1, n):
        t2, p2, _ = _stats(low, geom, 0.0, 1.0, count=torch.tensor([c], dtype=torch.int32, device=dev))
        assert torch.equal(t2[:c], table[:c]) and not t2[c:].any() and torch.equal(p2[:c], planes[:c])


# ------------------------------------------------------------------------------------------------ 2. RLE op
@torch.no_grad()
@pytest.mark.parametrize("shape", C.RLE_SHAPES, ids=lambda s: "%dx%d" % s)
def test_rle_edges_exact(dev, shape):
    H, W = shape
    masks, _ = C.rle_masks(H, W)
    planes = C.pack_planes(masks, dev)
    _check_rle(masks, planes, H, W)
    _check_rle(masks, planes, H, W, torch.tensor(C.rle_select(len(masks)), dtype=torch.int32, device=dev))


# ------------------------------------------------------------------------------------------------ 3. small regions
@torch.no_grad()
@pytest.mark.parametrize("shape", C.RSR_SHAPES, ids=lambda s: "%dx%d" % s)
def test_small_regions_edges_exact(dev, shape):
    from inklayer_amd import ops
    H, W = shape
    n_changed = 0
    for min_area, names, masks in C.rsr_cases(H, W):
        planes = C.pack_planes(masks, dev)
        for modes in C.RSR_MODES:
            out, changed = ops.remove_small_regions(planes, H, W, min_area, modes=modes)
            got = C.unpack_planes(out, H)
            for i, name in enumerate(names):
                m, ch = masks[i].numpy(), False
                for mode in modes:
                    m, c = R.remove_small_regions(m, min_area, mode)
                    ch = ch or c
                assert np.array_equal(got[i].numpy(), m), (min_area, modes, name)
                assert bool(changed[i]) == ch, (min_area, modes, name)
                n_changed += ch
            out1, changed1 = ops.remove_small_regions(planes, H, W, min_area, max_workspace_bytes=1, modes=modes)
            assert torch.equal(out1, out) and torch.equal(changed1, changed)
    assert n_changed > 0


@torch.no_grad()
@pytest.mark.parametrize("shape", C.RSR_SHAPES, ids=lambda s: "%dx%d" % s)
def test_pack_col_planes_edges(dev, shape):
    from inklayer_amd import ops
    H, W = shape
    masks = torch.stack([m for _, m in C.rsr_general(H, W)])
    want = C.pack_planes(masks, dev)
    assert torch.equal(ops.pack_col_planes(masks.to(dev)), want)
    for v in (1, 2, 128, 255):
        assert torch.equal(ops.pack_col_planes((masks.to(torch.uint8) * v).to(dev)), want), v
    rs = np.random.RandomState(H + W)
    mixed = torch.from_numpy(rs.choice(np.array([1, 2, 128, 255], dtype=np.uint8), size=tuple(masks.shape)))
    assert torch.equal(ops.pack_col_planes((mixed * masks.to(torch.uint8)).to(dev)), want)


# ------------------------------------------------------------------------------------------------ 4. NMS
@torch.no_grad()
def test_nms_edges_exact(dev):
    from inklayer_amd import ops
    for name, boxes, scores, thr in C.nms_cases():
        got = ops.box_nms(boxes.to(dev), scores.to(dev), thr)
        want = R.nms(boxes, scores, thr)
        assert got.dtype == torch.int64 and torch.equal(got.cpu(), want), name
