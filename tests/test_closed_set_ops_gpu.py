"""ops.class_scores and ops.select_boxes (csrc/closed_set.hip), each launch on its own, and the selection between them
(ops.topk_rowmax over the flattened (query, class) scores) against tests/closed_set_ref.py in float64.  GPU box only.

Tolerance of the scores: the reference's OWN float32 arithmetic (torch on the CPU: sigmoid, then the matmul with the
positive map) is compared with float64 on the same inputs; the kernel is allowed four times that maximum error, and
never less than 2^-22.  The factor covers the device's exp and a summation order that differs from torch's but is fixed.
Measured on an MI355X and the CPU beside it: the float32 statement is within 1.02e-7 of float64 on these shapes (the
largest), and so is the kernel (1.02e-7; 9.5e-8 at (2, 900, 195, 66) against 9.2e-8)."""
import numpy as np
import pytest
import torch

import closed_set_ref as ref

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1, 1, 1), (3, 7, 5, 2), (2, 64, 24, 7), (1, 900, 4, 1), (2, 900, 195, 66), (2, 900, 256, 86)]
FLOOR = 2.0 ** -22


def span_map(rs, C, T):
    """A positive map [C, T] as create_positive_map_from_span makes them: class c marks 1 to 3 consecutive tokens, one
    token (the "." of the caption) between two classes, token 0 ([CLS]) free where there is room; rows 1 / (n + 1e-6)."""
    n = rs.randint(1, 4, size=C)
    start = 1 if C + (C - 1) + 1 <= T else 0
    while n.sum() + (C - 1) + start > T:
        n[rs.choice(np.nonzero(n > 1)[0])] -= 1
    pm, t = torch.zeros(C, T), start
    for c in range(C):
        pm[c, t:t + n[c]] = 1.0
        t += n[c] + 1
    return pm / (pm.sum(-1)[:, None] + 1e-6)


def make_case(B, nq, T, C, seed=0):
    rs = np.random.RandomState(seed + 1000 * B + nq + 7 * T + 13 * C)
    logits = torch.from_numpy((-3.0 + 2.0 * rs.standard_normal((B, nq, T))).astype(np.float32))
    return logits, span_map(rs, C, T)


def tolerance(logits, pm, what=""):
    f64 = ref.class_scores_f64(logits, pm)
    own = (ref.class_scores_f32(logits, pm).double() - f64).abs().max().item()
    tol = max(4.0 * own, FLOOR)
    print(f"{what}: the reference's f32 arithmetic is within {own:.3e} of float64 -> bound {tol:.3e}")
    return f64, tol


_cases = {}


def case(shape):
    """(logits, map, float64 scores, bound) of a shape: computed once, shared, left unchanged."""
    if shape not in _cases:
        logits, pm = make_case(*shape)
        _cases[shape] = (logits, pm) + tolerance(logits, pm, f"{shape}")
    return _cases[shape]


@torch.no_grad()
@pytest.mark.parametrize("shape", SHAPES)
def test_class_scores_against_float64(dev, shape):
    from inklayer_amd import ops
    logits, pm, f64, tol = case(shape)
    got = ops.class_scores(logits.to(dev), pm.to(dev))
    assert got.dtype == torch.float32 and tuple(got.shape) == (shape[0], shape[1], shape[3])
    err = (got.cpu().double() - f64).abs().max().item()
    print(f"{shape}: kernel vs float64 max {err:.3e} (bound {tol:.3e})")
    assert not torch.isnan(got).any() and err <= tol
    # the per-image form with the same map for every image, and a wider row stride, are the same bits
    B, nq, T, C = shape
    wide = torch.full((B, nq, T + 3), 7.0, device=dev)
    wide[:, :, :T] = logits.to(dev)
    per = ops.class_scores(wide[:, :, :T], pm.to(dev).repeat(B, 1, 1).contiguous())
    assert torch.equal(per, got)


@torch.no_grad()
def test_class_scores_edges(dev):
    from inklayer_amd import ops
    B, nq, T, C = 2, 21, 24, 7
    logits, pm, f64, tol = case((2, 64, 24, 7))
    logits = logits[:, :nq].contiguous()
    base = ops.class_scores(logits.to(dev), pm.to(dev))
    # -inf pad columns, whatever the map holds there: exactly the unpadded result
    for pad in (1, 4, 232):
        lp = torch.full((B, nq, T + pad), float("-inf"))
        lp[:, :, :T] = logits
        pp = torch.cat([pm, torch.full((C, pad), 0.25)], dim=1).contiguous()
        got = ops.class_scores(lp.to(dev), pp.to(dev))
        assert torch.equal(got, base), pad
        pz = torch.cat([pm, torch.zeros(C, pad)], dim=1).contiguous()
        assert torch.equal(ops.class_scores(lp.to(dev), pz.to(dev)), base), pad
    # +inf contributes exactly the map's entry, -inf exactly 0
    one = torch.full((1, 3, T), float("-inf"))
    t1 = int(torch.nonzero(pm[2])[0])
    one[0, 0, t1] = float("inf")                   # query 0: only class 2's first token
    one[0, 1, :] = float("inf")                    # query 1: every token
    got = ops.class_scores(one.to(dev), pm.to(dev)).cpu()
    assert not torch.isnan(got).any()
    assert got[0, 0, 2].item() == pm[2, t1].item() and got[0, 0, :2].abs().sum().item() == 0.0
    assert torch.equal(got[0, 2], torch.zeros(C))                                   # all -inf: exactly 0
    assert (got[0, 1].double() - pm.double().sum(-1)).abs().max().item() <= FLOOR
    # logits of +-100
    big = torch.from_numpy(np.random.RandomState(5).choice([-100.0, 100.0], size=(2, 9, T)).astype(np.float32))
    got = ops.class_scores(big.to(dev), pm.to(dev)).cpu()
    w64, wtol = tolerance(big, pm, "+-100")
    assert not torch.isnan(got).any() and (got.double() - w64).abs().max().item() <= wtol
    # a zero map row scores exactly 0.0; classes past n_cls exactly -1.0, the others as without n_cls
    pz = pm.clone()
    pz[3] = 0.0
    got = ops.class_scores(logits.to(dev), pz.to(dev))
    assert torch.equal(got[:, :, 3], torch.zeros(B, nq, device=dev))
    assert torch.equal(got[:, :, :3], base[:, :, :3]) and torch.equal(got[:, :, 4:], base[:, :, 4:])
    n_cls = torch.tensor([7, 4], dtype=torch.int32, device=dev)
    got = ops.class_scores(logits.to(dev), pm.to(dev).repeat(B, 1, 1).contiguous(), n_cls)
    assert torch.equal(got[0], base[0]) and torch.equal(got[1, :, :4], base[1, :, :4])
    assert torch.equal(got[1, :, 4:], torch.full((nq, 3), -1.0, device=dev))
    # more classes than one output tile, and a class count that is no multiple of anything
    rs = np.random.RandomState(9)
    many = torch.from_numpy((rs.uniform(size=(131, T)) * (rs.uniform(size=(131, T)) < 0.2)).astype(np.float32))
    many = many / (many.sum(-1)[:, None] + 1e-6)
    lg = torch.from_numpy((-3 + 2 * rs.standard_normal((1, 11, T))).astype(np.float32))
    w64, wtol = tolerance(lg, many, "131 classes")
    got = ops.class_scores(lg.to(dev), many.to(dev)).cpu()
    assert (got.double() - w64).abs().max().item() <= wtol


@torch.no_grad()
def test_class_scores_batch_invariance(dev):
    """Image b of a batch of 3 with per-image maps and token counts == the same image run alone, bit for bit; two runs
    are bit-identical."""
    from inklayer_amd import ops
    rs = np.random.RandomState(21)
    nq, t_len, n_cls = 37, (195, 24, 256), (66, 7, 86)
    Tmax, Cmax = max(t_len), max(n_cls)
    logits = torch.full((3, nq, Tmax), float("-inf"))
    pm = torch.zeros(3, Cmax, Tmax)
    for b in range(3):
        logits[b, :, :t_len[b]] = torch.from_numpy((-3 + 2 * rs.standard_normal((nq, t_len[b]))).astype(np.float32))
        pm[b, :n_cls[b], :t_len[b]] = span_map(rs, n_cls[b], t_len[b])
    counts = torch.tensor(n_cls, dtype=torch.int32, device=dev)
    got = ops.class_scores(logits.to(dev), pm.to(dev), counts)
    again = ops.class_scores(logits.to(dev), pm.to(dev), counts)
    assert torch.equal(got, again) and not torch.isnan(got).any()
    for b in range(3):
        alone = ops.class_scores(logits[b:b + 1, :, :t_len[b]].contiguous().to(dev),
                                 pm[b, :n_cls[b], :t_len[b]].contiguous().to(dev))
        assert torch.equal(alone[0], got[b, :, :n_cls[b]]), b
        assert torch.equal(got[b, :, n_cls[b]:], torch.full((nq, Cmax - n_cls[b]), -1.0, device=dev))
        pair = ops.class_scores(logits[[b, 0]].contiguous().to(dev), pm[[b, 0]].contiguous().to(dev),
                                counts[[b, 0]].contiguous())
        assert torch.equal(pair[0], got[b]), b


@torch.no_grad()
@pytest.mark.parametrize("B,nq,Cmax,K", [(1, 1, 1, 1), (2, 900, 86, 300), (3, 64, 7, 40), (3, 7, 2, 14)])
def test_select_boxes_against_torch(dev, B, nq, Cmax, K):
    from inklayer_amd import ops
    rs = np.random.RandomState(B + nq + K)
    boxes = torch.from_numpy(rs.uniform(0.0, 1.0, size=(B, nq, 4)).astype(np.float32))
    idx = torch.from_numpy(rs.randint(0, nq * Cmax, size=(B, K)).astype(np.int32))
    idx[0, 0], idx[-1, -1] = 0, nq * Cmax - 1
    sizes = torch.tensor([[480.0, 640.0], [800.0, 1333.0], [751.0, 333.0]])[:B]              # (h, w)
    scale = torch.stack([sizes[:, 1], sizes[:, 0]], dim=1).contiguous()
    got_boxes, labels, query = ops.select_boxes(idx.to(dev), boxes.to(dev), scale.to(dev), Cmax)
    q = (idx // Cmax).long()
    want = torch.gather(ref.box_cxcywh_to_xyxy(boxes), 1, q.unsqueeze(-1).repeat(1, 1, 4))
    img_h, img_w = sizes.unbind(1)
    want = want * torch.stack([img_w, img_h, img_w, img_h], dim=1)[:, None, :]
    # exact: 0.5 * w is exact in binary, so no contraction can differ from the reference's two steps
    assert torch.equal(got_boxes.cpu(), want)
    assert torch.equal(labels.cpu(), idx % Cmax) and torch.equal(query.cpu(), idx // Cmax)
    assert labels.dtype == torch.int32 and query.dtype == torch.int32


@torch.no_grad()
@pytest.mark.parametrize("shape,num_select", [((2, 900, 256, 86), 300), ((3, 64, 24, 7), 40), ((3, 7, 5, 2), 300)])
def test_selection_end_to_end(dev, shape, num_select):
    from inklayer_amd import ops
    B, nq, T, C = shape
    logits, pm, f64, tol = case(shape)
    rs = np.random.RandomState(3)
    boxes = torch.from_numpy(rs.uniform(0.05, 0.95, size=(B, nq, 4)).astype(np.float32))
    sizes = torch.tensor([[480.0, 640.0], [800.0, 1333.0], [751.0, 333.0]])[:B]
    K = min(num_select, nq * C)
    prob = ops.class_scores(logits.to(dev), pm.to(dev))
    idx, val = ops.topk_rowmax(prob.view(B, nq * C, 1), K, want_values=True)
    scale = torch.stack([sizes[:, 1], sizes[:, 0]], dim=1).contiguous().to(dev)
    xyxy, labels, query = ops.select_boxes(idx, boxes.to(dev), scale, C)
    flat = prob.view(B, -1).cpu()
    # the indices are a stable descending sort of the kernel's own scores, exactly
    order = torch.sort(flat, dim=1, descending=True, stable=True)[1][:, :K]
    assert torch.equal(idx.cpu().long(), order) and torch.equal(val.cpu(), torch.gather(flat, 1, order))
    # against the float64 reference: the same (query, class) set, but for pairs within the scores' bound of the K-th
    want = ref.post_process(logits, boxes, pm, sizes, num_select)
    f64_flat = f64.view(B, -1)
    for b in range(B):
        got_set = set(idx[b].cpu().tolist())
        want_idx = (want[b]["query"] * C + want[b]["labels"]).tolist()
        assert len(want_idx) == K and len(got_set) == K
        kth = want[b]["scores"][-1].item()
        odd = got_set.symmetric_difference(want_idx)
        assert all(abs(f64_flat[b, i].item() - kth) <= tol for i in odd), (b, sorted(odd))
        assert len(odd) <= 0.02 * K, (b, len(odd))                # at most 2 % of K excused, both sides counted
        # scores, labels and boxes of the pairs both selected
        got_pos = {i: k for k, i in enumerate(idx[b].cpu().tolist())}
        both = [(got_pos[i], k) for k, i in enumerate(want_idx) if i in got_pos]
        gk, wk = torch.tensor([g for g, _ in both]), torch.tensor([w for _, w in both])
        assert (val[b].cpu()[gk].double() - want[b]["scores"][wk]).abs().max().item() <= tol
        assert torch.equal(labels[b].cpu()[gk].long(), want[b]["labels"][wk])
        assert torch.equal(query[b].cpu()[gk].long(), want[b]["query"][wk])
        assert (xyxy[b].cpu()[gk].double() - want[b]["boxes"][wk]).abs().max().item() <= 1333 * 2.0 ** -22
