"""Every device entry point of csrc/refine_stage.hip on its own against tests/refine_stage_ref.py (pinned to the oracle
by tests/test_refine_stage_ref_cpu.py): exact equality, launch by launch.

Every output and workspace buffer is filled with 0x5A bytes before a call (nothing is zeroed for the kernels), carries a
guard behind its end that must stay 0x5A, and every entry point is also run twice on the SAME buffers, a larger input
and then a smaller one, with the second result checked.  Sizes: refine_stage_ref.EDGE_SIZES (one and two carries of the
row scan, 65 words per row, widths around a word).  GPU box only."""
import ctypes as C

import numpy as np
import pytest
import torch

import refine_stage_ref as R

pytestmark = pytest.mark.gpu

GUARD = 64                       # elements behind every output buffer
SIZES = pytest.mark.parametrize("hw", R.EDGE_SIZES, ids=lambda hw: f"{hw[0]}x{hw[1]}")
BIG, SMALL = (7, 129), (3, 63)   # the pair of sizes of the runs that reuse their buffers


def _lib():
    from inklayer_amd import _lib as m
    return m


def _st():
    from inklayer_amd import ops
    return ops._stream()


def _up(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _planes(b, dev):
    """bool [..., H, W] -> packed int64 planes on the device."""
    return _up(R.pack(b).view(np.int64), dev)


class Bufs:
    """Poisoned output buffers by name.  get(): a flat tensor of at least `numel` elements plus the guard - the one made
    by an earlier call where it is large enough (left as that call left it), else a new one full of 0x5A."""

    def __init__(self, dev):
        self.dev, self.t, self.cap = dev, {}, {}

    def get(self, key, numel, dtype):
        if key not in self.t or self.cap[key] < numel:
            t = torch.empty(numel + GUARD, device=self.dev, dtype=dtype)
            t.view(torch.uint8).fill_(0x5A)
            self.t[key], self.cap[key] = t, numel
        return self.t[key]

    def read(self, key, numel, shape=None):
        a = self.t[key].cpu().numpy()
        assert (a[self.cap[key]:].view(np.uint8) == 0x5A).all(), f"{key}: written behind its end"
        a = a[:numel]
        return a if shape is None else a.reshape(shape)


def _check(rc, what):
    _lib().check(rc, what)
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------
# one runner per entry point: uploads, poisons, calls, reads back unpacked
# ---------------------------------------------------------------------------------------------------------------
def run_sketch_planes(dev, rgb, bufs=None):
    b = bufs or Bufs(dev)
    H, W = rgb.shape[:2]
    Wp = (W + 63) // 64
    out, mx = b.get("planes", 4 * H * Wp, torch.int64), b.get("max", 1, torch.int32)
    src = _up(rgb, dev)                                          # (inputs stay referenced until the call has run)
    _check(_lib().lib().ink_refine_sketch_planes(src.data_ptr(), H, W, out.data_ptr(), mx.data_ptr(), _st()),
           "ink_refine_sketch_planes")
    words = b.read("planes", 4 * H * Wp, (4, H, Wp))
    assert R.tail_is_clear(words, W)
    return R.unpack(words, W)


def run_bitplane_pack(dev, img, thresh, bufs=None):
    b = bufs or Bufs(dev)
    n, H, W = img.shape
    Wp = (W + 63) // 64
    out = b.get("planes", n * H * Wp, torch.int64)
    src = _up(img, dev)
    _check(_lib().lib().ink_bitplane_pack(src.data_ptr(), n, H, W, thresh, out.data_ptr(), _st()), "ink_bitplane_pack")
    words = b.read("planes", n * H * Wp, (n, H, Wp))
    assert R.tail_is_clear(words, W)
    return R.unpack(words, W)


def run_depth_samples(dev, masks, depth, pts, bufs=None):
    b = bufs or Bufs(dev)
    n, (H, W), P = len(masks), depth.shape, len(pts)
    vals, inside = b.get("vals", P, torch.float32), b.get("inside", n * P, torch.uint8)
    pl = _planes(masks, dev) if n else None
    dp, pt = _up(depth, dev), _up(pts.astype(np.int32), dev)
    _check(_lib().lib().ink_refine_depth_samples(pl.data_ptr() if n else None, n, dp.data_ptr(),
                                                 pt.data_ptr(), P, H, W, vals.data_ptr(),
                                                 inside.data_ptr() if n else None, _st()), "ink_refine_depth_samples")
    return b.read("vals", P), b.read("inside", n * P, (n, P))


def run_pair_tables(dev, masks, planes4, rect, bufs=None):
    b = bufs or Bufs(dev)
    n, (H, W) = len(masks), planes4.shape[1:]
    Wp = (W + 63) // 64
    dil, pair = b.get("dil", n * H * Wp, torch.int64), b.get("pair", n * n * 2, torch.int32)
    per, area = b.get("per", n * 3, torch.int32), b.get("area", 1, torch.int32)
    pl, rc = (_planes(masks, dev), _up(np.asarray(rect, np.int32), dev)) if n else (None, None)
    p = lambda t: t.data_ptr() if n else None
    sk = _planes(planes4, dev)
    _check(_lib().lib().ink_refine_pair_tables(p(pl), sk.data_ptr(), n, H, W, p(rc), p(dil), p(pair), p(per),
                                               area.data_ptr(), _st()), "ink_refine_pair_tables")
    words = b.read("dil", n * H * Wp, (n, H, Wp))
    assert R.tail_is_clear(words, W)
    return R.unpack(words, W), b.read("pair", n * n * 2, (n, n, 2)), b.read("per", n * 3, (n, 3)), int(b.read("area", 1)[0])


def run_composite(dev, masks, order, shape, bufs=None):
    b = bufs or Bufs(dev)
    (H, W), nr = shape, len(order)
    label, hist = b.get("label", H * W, torch.uint8), b.get("hist", 256, torch.int32)
    pl, od = (_planes(masks, dev), _up(np.asarray(order, np.int32), dev)) if nr else (None, None)
    _check(_lib().lib().ink_refine_composite(pl.data_ptr() if nr else None, od.data_ptr() if nr else None, nr, H, W,
                                             label.data_ptr(), hist.data_ptr(), _st()), "ink_refine_composite")
    return b.read("label", H * W, (H, W)), b.read("hist", 256)


def run_relabel_clean(dev, label, lut, bufs=None):
    b = bufs or Bufs(dev)
    H, W = label.shape
    out = b.get("out", H * W, torch.uint8)
    src, lt = _up(label, dev), _up(lut, dev)
    _check(_lib().lib().ink_refine_relabel_clean(src.data_ptr(), lt.data_ptr(), H, W, out.data_ptr(), _st()),
           "ink_refine_relabel_clean")
    return b.read("out", H * W, (H, W))


def run_grow(dev, label, planes4, cap, bufs=None):
    b = bufs or Bufs(dev)
    H, W = label.shape
    pw, ci = C.c_int64(0), C.c_int64(0)
    _lib().check(_lib().lib().ink_refine_grow_workspace(H, W, C.byref(pw), C.byref(ci)), "ink_refine_grow_workspace")
    assert pw.value == 4 * H * ((W + 63) // 64) and ci.value >= 1 + H + 1
    pws, ccw = b.get("pws", pw.value, torch.int64), b.get("ccw", ci.value, torch.int32)
    flags, bbox = b.get("flags", 256, torch.int32), b.get("bbox", 1024, torch.int32)
    grown, cnt = b.get("grown", H * W, torch.uint8), b.get("cnt", 1, torch.int32)
    unl = b.get("unl", 2 * cap, torch.int32)                    # in a fresh Bufs: exactly cap pairs, then the guard
    src, sk = _up(label, dev), _planes(planes4, dev)
    _check(_lib().lib().ink_refine_grow(src.data_ptr(), sk.data_ptr(), H, W, pws.data_ptr(),
                                        ccw.data_ptr(), flags.data_ptr(), grown.data_ptr(), bbox.data_ptr(), unl.data_ptr(),
                                        cap, cnt.data_ptr(), _st()), "ink_refine_grow")
    count = int(b.read("cnt", 1)[0])
    b.read("pws", pw.value)
    return {"grown": b.read("grown", H * W, (H, W)), "flags": b.read("flags", 256), "bbox": b.read("bbox", 1024, (256, 4)),
            "overflow": int(b.read("ccw", ci.value)[0]), "count": count,
            "yx": b.read("unl", 2 * min(cap, max(count, 0)), (-1, 2))}


def run_query_dists(dev, label, q, cands, bufs=None):
    b = bufs or Bufs(dev)
    (H, W), Q = label.shape, len(q)
    d2 = b.get("d2", Q * 256, torch.int32)
    src, qd, cd = _up(label, dev), _up(q.astype(np.int32), dev), _up(R.candidate_words(cands).view(np.int64), dev)
    _check(_lib().lib().ink_refine_query_dists(src.data_ptr(), qd.data_ptr(),
                                               cd.data_ptr(), Q, H, W,
                                               d2.data_ptr(), _st()), "ink_refine_query_dists")
    return b.read("d2", Q * 256, (Q, 256))


def run_finalize(dev, label, assign, planes4, bufs=None):
    b = bufs or Bufs(dev)
    (H, W), A = label.shape, len(assign)
    Wp = (W + 63) // 64
    lab = _up(label, dev)                                        # a fresh copy: the call writes into it
    ws, extra, cnt = b.get("ws", 3 * H * Wp, torch.int64), b.get("extra", H * Wp, torch.int64), b.get("cnt", 1, torch.int32)
    asg = _up(np.asarray(assign, np.int32).reshape(-1, 3), dev) if A else None
    sk = _planes(planes4, dev)
    _check(_lib().lib().ink_refine_finalize(lab.data_ptr(), asg.data_ptr() if A else None, A, sk.data_ptr(), H, W,
                                            ws.data_ptr(), extra.data_ptr(), cnt.data_ptr(), _st()), "ink_refine_finalize")
    words = b.read("extra", H * Wp, (H, Wp))
    b.read("ws", 3 * H * Wp)
    assert R.tail_is_clear(words, W)
    return lab.cpu().numpy(), R.unpack(words, W), int(b.read("cnt", 1)[0])


# ---------------------------------------------------------------------------------------------------------------
# comparisons
# ---------------------------------------------------------------------------------------------------------------
def _eq(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = got != want
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} differ, first at {np.argwhere(bad)[0].tolist()}: " \
                          f"got {got[bad][0]!r}, want {want[bad][0]!r}"


def _check_pair_tables(dev, masks, planes, rect, bufs=None, tag=""):
    dil, pair, per, area = run_pair_tables(dev, masks, planes, rect, bufs)
    wdil, wpair, wper, warea = R.pair_tables(masks, planes, rect)
    assert area == warea, (tag, area, warea)
    _eq(dil, wdil, f"{tag} dilated planes")
    _eq(pair, wpair, f"{tag} pair")
    _eq(per, wper, f"{tag} per")
    _eq(pair, pair.transpose(1, 0, 2), f"{tag} pair symmetry")


def _check_grow(dev, label, planes, bufs=None, tag=""):
    want = R.grow(label, planes)
    got = run_grow(dev, label, planes, max(want["count"], 1), bufs)
    _eq(got["grown"], want["grown"], f"{tag} grown")
    _eq(got["flags"][1:], want["flags"][1:], f"{tag} flags")
    _eq(got["bbox"], want["bbox"], f"{tag} bbox")
    assert got["overflow"] == 0 and got["count"] == want["count"], (tag, got["overflow"], got["count"], want["count"])
    _eq(got["yx"], want["yx"], f"{tag} pixel list")
    return want


def _check_query(dev, label, q, cands, bufs=None, tag=""):
    got = run_query_dists(dev, label, q, cands, bufs)
    want = R.query_dists(label, q)
    for k, ls in enumerate(cands):
        _eq(got[k, ls], want[k, ls], f"{tag} query {k} {ls}")


def _check_finalize(dev, label, assign, planes, bufs=None, tag=""):
    lab, extra, cnt = run_finalize(dev, label, assign, planes, bufs)
    wlab, wextra, wcnt = R.finalize(label, assign, planes)
    _eq(lab, wlab, f"{tag} label")
    _eq(extra, wextra, f"{tag} extra")
    assert cnt == wcnt == int(extra.sum()), (tag, cnt, wcnt)
    return wcnt


def _assignments(label, A, seed):
    """A assignments (y, x, label) at distinct pixels."""
    rs = np.random.RandomState(seed)
    H, W = label.shape
    flat = rs.permutation(H * W)[:A]
    return np.stack([flat // W, flat % W, rs.randint(0, 255, len(flat))], 1).astype(np.int32)


LABELS = [1, 2, 3, 19, 20, 21, 40, 63, 64, 65, 127, 128, 129, 200, 253, 254]


# ---------------------------------------------------------------------------------------------------------------
# ink_refine_sketch_planes, ink_bitplane_pack
# ---------------------------------------------------------------------------------------------------------------
@SIZES
def test_sketch_planes(dev, hw):
    for seed, top in ((1, 255), (2, 253), (3, 0)):                # maximum 255, an odd maximum, an all-zero image
        rgb = R.random_rgb(*hw, seed, top)
        assert rgb.max() == top
        _eq(run_sketch_planes(dev, rgb), R.sketch_planes(rgb), f"{hw} top {top}")


def test_sketch_planes_on_reused_buffers(dev):
    b = Bufs(dev)
    for hw, top in ((BIG, 255), (SMALL, 251)):
        rgb = R.random_rgb(*hw, 4, top)
        _eq(run_sketch_planes(dev, rgb, b), R.sketch_planes(rgb), f"{hw}")


@SIZES
def test_bitplane_pack(dev, hw):
    img = np.array([0, 1, 127, 128, 255], np.uint8)[np.random.RandomState(5).randint(0, 5, (3,) + hw)]
    for thresh in (0, 127):
        _eq(run_bitplane_pack(dev, img, thresh), R.bitplane_pack(img, thresh), f"{hw} thresh {thresh}")


def test_bitplane_pack_on_reused_buffers(dev):
    b = Bufs(dev)
    for hw in (BIG, SMALL):
        img = np.array([0, 1, 127, 128, 255], np.uint8)[np.random.RandomState(6).randint(0, 5, (3,) + hw)]
        _eq(run_bitplane_pack(dev, img, 127, b), R.bitplane_pack(img, 127), f"{hw}")


# ---------------------------------------------------------------------------------------------------------------
# ink_refine_depth_samples
# ---------------------------------------------------------------------------------------------------------------
def _depth_case(hw, P, n, seed):
    H, W = hw
    rs = np.random.RandomState(seed)
    depth = rs.randint(-2 ** 31, 2 ** 31, hw, dtype=np.int64).astype(np.int32).view(np.float32)    # every bit pattern
    pts = np.stack([rs.randint(0, H, P), rs.randint(0, W, P)], 1)
    fixed = np.array([(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1), (H // 2, min(63, W - 1)), (H // 2, min(64, W - 1))])
    pts[:min(P, len(fixed))] = fixed[:min(P, len(fixed))]         # the corners, x = 63 / 64
    return rs.rand(n, H, W) < 0.5, depth, pts


def _check_depth(dev, masks, depth, pts, bufs=None, tag=""):
    vals, inside = run_depth_samples(dev, masks, depth, pts, bufs)
    wvals, winside = R.depth_samples(masks, depth, pts)
    _eq(vals.view(np.int32), wvals.view(np.int32), f"{tag} vals (bitwise)")
    _eq(inside, winside.astype(np.uint8), f"{tag} inside")


@SIZES
def test_depth_samples(dev, hw):
    for P in (1, 257):
        for n in (0, 3):
            _check_depth(dev, *_depth_case(hw, P, n, P + n), tag=f"{hw} P {P} n {n}")


def test_depth_samples_on_reused_buffers(dev):
    b = Bufs(dev)
    _check_depth(dev, *_depth_case(BIG, 257, 3, 1), b, "big")
    _check_depth(dev, *_depth_case(SMALL, 40, 2, 2), b, "small")


# ---------------------------------------------------------------------------------------------------------------
# ink_refine_pair_tables
# ---------------------------------------------------------------------------------------------------------------
@SIZES
def test_pair_tables(dev, hw):
    planes = R.random_planes(*hw, 3)
    for n in (0, 1, 2, 5, 20):
        _check_pair_tables(dev, R.random_masks(n, *hw, 30 + n), planes, R.random_rects(n, *hw, 40 + n), tag=f"{hw} n {n}")


def test_pair_tables_clip_rectangles_at_the_word_boundaries(dev):
    _check_pair_tables(dev, *R.pair_rects_case(), tag="rects")


def test_pair_tables_on_reused_buffers(dev):
    b = Bufs(dev)
    _check_pair_tables(dev, R.random_masks(5, *BIG, 1), R.random_planes(*BIG, 2), R.random_rects(5, *BIG, 3), b, "big")
    _check_pair_tables(dev, R.random_masks(2, *SMALL, 4), R.random_planes(*SMALL, 5), R.random_rects(2, *SMALL, 6), b, "small")
    _check_pair_tables(dev, np.zeros((0,) + SMALL, bool), R.random_planes(*SMALL, 7), None, b, "small, no masks")


# ---------------------------------------------------------------------------------------------------------------
# ink_refine_composite, ink_refine_relabel_clean
# ---------------------------------------------------------------------------------------------------------------
def _composite_case(hw, nr, seed):
    rs = np.random.RandomState(seed)
    masks = R.small_masks(max(nr, 1), *hw, seed)
    if nr >= 3:
        masks[0] |= rs.rand(*hw) < 0.2                             # overlaps: the earlier rank decides
        masks[1] |= rs.rand(*hw) < 0.2
        masks[-1] |= rs.rand(*hw) < 0.5
    order = rs.permutation(nr).tolist()
    for r in range(2, nr, 7):
        order[r] = -1
    return masks, order


def _check_composite(dev, masks, order, hw, bufs=None, tag=""):
    label, hist = run_composite(dev, masks, order, hw, bufs)
    wlabel, whist = R.composite(masks, order, hw)
    _eq(label, wlabel, f"{tag} label")
    _eq(hist[1:], whist[1:], f"{tag} hist")
    _eq(hist[1:], np.bincount(label.ravel(), minlength=256)[1:], f"{tag} hist against the label image")
    return wlabel


@SIZES
def test_composite(dev, hw):
    for nr in (0, 1, 3, 254):
        wlabel = _check_composite(dev, *_composite_case(hw, nr, 50 + nr), hw, tag=f"{hw} ranks {nr}")
        if nr == 254 and hw[0] * hw[1] > 8000:
            assert len(np.unique(wlabel)) > 150 and wlabel.max() > 240       # the high ranks keep pixels


def test_composite_on_reused_buffers(dev):
    b = Bufs(dev)
    _check_composite(dev, *_composite_case(BIG, 254, 1), BIG, b, "big")
    _check_composite(dev, *_composite_case(SMALL, 3, 2), SMALL, b, "small")
    _check_composite(dev, *_composite_case(SMALL, 0, 3), SMALL, b, "small, no ranks")


def _random_lut(seed):
    rs = np.random.RandomState(seed)
    lut = rs.randint(1, 255, 256).astype(np.uint8)                 # many labels share a target
    lut[rs.rand(256) < 0.2] = 0
    lut[0] = 0
    lut[254] = 254
    return lut


@SIZES
def test_relabel_clean(dev, hw):
    label = R.random_labels(*hw, 60, LABELS * 4)
    for lut in (np.arange(256, dtype=np.uint8), _random_lut(61)):
        _eq(run_relabel_clean(dev, label, lut), R.relabel_clean(label, lut), f"{hw}")


def test_relabel_clean_isolated_pixels_pairs_and_lines(dev):
    label, drop, merge = R.relabel_case()
    b = Bufs(dev)
    big = R.random_labels(*BIG, 62, LABELS * 4)
    _eq(run_relabel_clean(dev, big, _random_lut(63), b), R.relabel_clean(big, _random_lut(63)), "big")
    for name, lut in (("identity", np.arange(256, dtype=np.uint8)), ("drop", drop), ("merge", merge)):
        _eq(run_relabel_clean(dev, label, lut, b), R.relabel_clean(label, lut), name)      # on the big run's buffer


# ---------------------------------------------------------------------------------------------------------------
# ink_refine_grow
# ---------------------------------------------------------------------------------------------------------------
@SIZES
def test_grow(dev, hw):
    label, planes = R.random_labels(*hw, 70, LABELS * 3), R.random_planes(*hw, 71)
    want = _check_grow(dev, label, planes, tag=f"{hw}")
    if hw[0] > 1024:
        assert want["yx"][0, 0] < 1024 and want["yx"][-1, 0] >= 1024 * (hw[0] // 1024)      # pixels on both sides of every carry


def test_grow_thresholds_radii_and_label_priority(dev):
    want = _check_grow(dev, *R.grow_case(), tag="grow case")
    assert want["flags"][3] == 1 and want["flags"][7] == 0


def test_grow_reports_the_full_count_when_the_list_does_not_fit(dev):
    for label, planes in (R.grow_case(), (R.random_labels(1030, 70, 72, LABELS), R.random_planes(1030, 70, 73))):
        want = R.grow(label, planes)
        for cap in (1, want["count"] // 2, want["count"] - 1):
            got = run_grow(dev, label, planes, cap)                 # (the guard behind the cap pairs is checked on read)
            assert got["count"] == want["count"] > cap and got["overflow"] == 0
            _eq(got["yx"], want["yx"][:cap], f"first {cap} pairs")
            _eq(got["grown"], want["grown"], "grown")


def test_grow_on_reused_buffers(dev):
    b = Bufs(dev)
    _check_grow(dev, R.random_labels(*BIG, 74, LABELS * 3), R.random_planes(*BIG, 75), b, "big")
    _check_grow(dev, R.random_labels(*SMALL, 76, [1, 2, 200]), R.random_planes(*SMALL, 77), b, "small")
    _check_grow(dev, np.zeros(SMALL, np.uint8), np.zeros((4,) + SMALL, bool), b, "small, empty")


# ---------------------------------------------------------------------------------------------------------------
# ink_refine_query_dists
# ---------------------------------------------------------------------------------------------------------------
def test_query_dists_over_254_labels(dev):
    label, q, cands = R.query_case()
    _check_query(dev, label, q, cands, tag="Q 300")
    _check_query(dev, label, q[:1], cands[:1], tag="Q 1")
    got = run_query_dists(dev, label, q[1:2], cands[1:2])           # an empty candidate set returns
    assert got.shape == (1, 256)
    assert run_query_dists(dev, label, q[:1], cands[:1])[0, R.QUERY_ABSENT] == R.INT_MAX


@SIZES
def test_query_dists(dev, hw):
    H, W = hw
    rs = np.random.RandomState(80)
    label = R.random_labels(H, W, 81, LABELS)
    q = np.stack([rs.randint(0, H, 12), rs.randint(0, W, 12)], 1)
    q[0], q[1] = (0, 0), (H - 1, W - 1)
    cands = [sorted(set(rs.choice(LABELS + [100], rs.randint(1, 6)).tolist())) for _ in range(12)]
    _check_query(dev, label, q, cands, tag=f"{hw}")


def test_query_dists_on_reused_buffers(dev):
    b = Bufs(dev)
    label, q, cands = R.query_case()
    _check_query(dev, label, q, cands, b, "big")
    small = R.random_labels(*SMALL, 82, [1, 200])
    _check_query(dev, small, np.array([[1, 5], [2, 62]]), [[1, 200, 254], [200]], b, "small")


# ---------------------------------------------------------------------------------------------------------------
# ink_refine_finalize
# ---------------------------------------------------------------------------------------------------------------
@SIZES
def test_finalize(dev, hw):
    label, planes = R.random_labels(*hw, 90, LABELS), R.random_planes(*hw, 91)
    for A in (0, 1, 257):
        _check_finalize(dev, label, _assignments(label, min(A, hw[0] * hw[1]), 92 + A), planes, tag=f"{hw} A {A}")


def test_finalize_opening_at_the_border_and_dilation_across_the_word_boundary(dev):
    label, planes = R.finalize_case()
    for A in (0, 1, 257):
        cnt = _check_finalize(dev, label, _assignments(label, A, 95), planes, tag=f"finalize case A {A}")
        assert cnt > 0 or A == 257


def test_finalize_on_reused_buffers(dev):
    b = Bufs(dev)
    big, small = R.random_labels(*BIG, 96, LABELS), R.random_labels(*SMALL, 97, [1, 2])
    assert _check_finalize(dev, big, _assignments(big, 257, 1), R.random_planes(*BIG, 98), b, "big") > 0
    _check_finalize(dev, small, _assignments(small, 1, 2), R.random_planes(*SMALL, 99), b, "small")
    _check_finalize(dev, small, _assignments(small, 0, 3), np.zeros((4,) + SMALL, bool), b, "small, empty")
