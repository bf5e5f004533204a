"""SAM point / box / mask prompts and multimask output on the GPU: SamEngine.decode_prompts and SamPredictor against
the float64 restatement (tests/sam_prompt_ref.py, pinned to the reference by tests/test_sam_prompts_cpu.py), with the
bounds of test_sam_gpu.py::test_decoder_matches_oracle; plus the invariants of the new kernels (box prompts through the
general entry, mask 0 of the multimask path, the 9..16-query attention) and their op-level checks.
ViT-H decoder dimensions, a 4-block encoder."""
import math

import numpy as np
import pytest
import torch

import sam_prompt_ref as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng_sd(dev):
    from oracle import sam_ref
    from inklayer_amd import sam
    oc = sam_ref.SamConfig(depth=4, global_attn_indexes=(1, 3))
    sd = sam_ref.seeded_state_dict(sam_ref.sam_param_shapes(oc), 11)
    eng = sam.SamEngine(sd, sam.SamConfig(depth=4, global_attn_indexes=(1, 3)), dev, max_batch=1)
    return eng, oc, R.to64(sd)


@pytest.fixture(scope="module")
def embs():
    rs = np.random.RandomState(5)
    return torch.from_numpy(rs.standard_normal((2, 4096, 256)).astype(np.float32))


def _rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).abs().max() / b.abs().max()).item(), ((a - b).norm() / b.norm()).item()


def _ref(oc, sd64, embs, img, pts, lab, box, mask):
    emb = torch.stack([embs[i].t().reshape(256, 64, 64) for i in img]).double()
    sparse = R.embed_sparse(sd64, oc, pts, lab, box)
    return R.decode_all(sd64, oc, emb, sparse, mask.double() if mask is not None else None)


def _check(oc, low, iou, ref_low, ref_iou, input_hw=(1024, 768), orig_hw=(1500, 1125)):
    """The bounds of test_decoder_matches_oracle: low-res logits max-rel < 1e-4 and l2-rel < 2e-5, IoU predictions
    max-rel < 1e-4, final masks IoU >= 0.999 per instance with every flipped pixel within 1 % of the logit scale."""
    from oracle import sam_ref
    from inklayer_amd import ops
    mx, l2 = _rel(low, ref_low)
    print(f"low-res max-rel {mx:.2e} l2-rel {l2:.2e}  iou max-rel {_rel(iou, ref_iou)[0]:.2e}")
    assert mx < 1e-4 and l2 < 2e-5
    assert _rel(iou, ref_iou)[0] < 1e-4
    n, M = low.shape[:2]
    low_dev = low.reshape(n * M, 256, 256).contiguous().to("cuda")           # the op takes device tensors only
    got = ops.sam_postprocess(low_dev, 1024, input_hw, orig_hw, 0.0).cpu().bool()
    ref_logits = sam_ref.postprocess_masks(oc, ref_low.reshape(n * M, 1, 256, 256).float(), input_hw, orig_hw)[:, 0]
    ref_m = ref_logits > 0
    inter = (got & ref_m).flatten(1).sum(1).double()
    union = (got | ref_m).flatten(1).sum(1).double().clamp_min(1)
    assert (inter / union).min().item() >= 0.999
    flipped = got != ref_m
    if flipped.any():
        assert ref_logits[flipped].abs().max().item() < 1e-2 * ref_logits.std().item()


def _points(rs, P, N, box_too=False):
    pts = torch.from_numpy(rs.uniform(0, 1000, (P, N, 2)).astype(np.float32))
    lab = torch.from_numpy(rs.choice([-1, 0, 1], size=(P, N)).astype(np.int32))
    lab[:, 0] = 1
    return pts, lab


BOXES = torch.tensor([[10.0, 20.0, 500.0, 400.0], [300.5, 100.25, 900.0, 1000.0], [640.0, 320.0, 700.0, 380.0]])


@torch.no_grad()
@pytest.mark.parametrize("N", [1, 3, 10])
@pytest.mark.parametrize("multimask", [False, True])
def test_points_match_restatement(dev, eng_sd, embs, N, multimask):
    """1, 3 and 10 points (NT = 7, 9, 16) with labels -1 / 0 / 1, two prompts on two images, multimask on and off."""
    eng, oc, sd64 = eng_sd
    rs = np.random.RandomState(N)
    pts, lab = _points(rs, 2, N)
    img = [1, 0]
    low, iou = eng.decode_prompts(embs.to(dev), img, pts, lab, multimask_output=multimask)
    M = 3 if multimask else 1
    assert low.shape == (2, M, 256, 256) and iou.shape == (2, M)
    ref_low, ref_iou = _ref(oc, sd64, embs, img, pts, lab, None, None)
    sl = slice(1, 4) if multimask else slice(0, 1)
    _check(oc, low, iou, ref_low[:, sl], ref_iou[:, sl])


@torch.no_grad()
@pytest.mark.parametrize("multimask", [False, True])
def test_box_plus_points_match_restatement(dev, eng_sd, embs, multimask):
    eng, oc, sd64 = eng_sd
    pts, lab = _points(np.random.RandomState(7), 3, 4)
    img = [0, 0, 1]
    low, iou = eng.decode_prompts(embs.to(dev), img, pts, lab, BOXES, multimask_output=multimask)
    ref_low, ref_iou = _ref(oc, sd64, embs, img, pts, lab, BOXES, None)
    sl = slice(1, 4) if multimask else slice(0, 1)
    _check(oc, low, iou, ref_low[:, sl], ref_iou[:, sl])


@torch.no_grad()
@pytest.mark.parametrize("multimask", [False, True])
def test_box_plus_mask_input_match_restatement(dev, eng_sd, embs, multimask):
    """The mask input is the low-res logits of a previous call (the refinement loop of SamPredictor)."""
    eng, oc, sd64 = eng_sd
    img = [0, 1, 0]
    prev, prev_iou = eng.decode_prompts(embs.to(dev), img, None, None, BOXES, multimask_output=True)
    best = prev_iou.argmax(1).cpu()
    mask = torch.stack([prev[i, best[i]] for i in range(3)])[:, None].contiguous()
    low, iou = eng.decode_prompts(embs.to(dev), img, None, None, BOXES, mask, multimask_output=multimask)
    ref_low, ref_iou = _ref(oc, sd64, embs, img, None, None, BOXES, mask.cpu())
    sl = slice(1, 4) if multimask else slice(0, 1)
    _check(oc, low, iou, ref_low[:, sl], ref_iou[:, sl])
    # the mask prompt is not a no-op
    plain, _ = eng.decode_prompts(embs.to(dev), img, None, None, BOXES, multimask_output=multimask)
    assert not torch.equal(plain, low)


@torch.no_grad()
def test_box_prompts_general_entry_is_bitwise_decode_low_res(dev, eng_sd, embs):
    """decode_low_res is decode_prompts with boxes alone; both must give the bits of the box path as it was before the
    general entry existed: the output tokens copied in front of sam_pe_encode(add=corner embeddings) of host-normalised
    corners, through the same decoder."""
    from inklayer_amd import ops
    eng, oc, sd64 = eng_sd
    w, n = eng.w, BOXES.shape[0]
    img = [0, 1, 1]
    coords = ((BOXES + 0.5).reshape(-1, 2) / 1024.0).to(dev)
    tokens = torch.empty((n, 7, 256), device=dev)
    tokens[:, :5] = w["out_tok"]
    tokens[:, 5:] = ops.sam_pe_encode(coords, w["gauss"], add=w["pt_emb"][2:4]).view(n, 2, 256)
    o_low, o_iou = eng._decode_tokens_split(embs.to(dev), tokens, img)
    a_low, a_iou = eng.decode_low_res(embs.to(dev), BOXES, img)
    assert torch.equal(a_low, o_low[:, 0]) and torch.equal(a_iou, o_iou)
    b_low, b_iou = eng.decode_prompts(embs.to(dev), img, None, None, BOXES)
    assert torch.equal(b_low, o_low) and torch.equal(b_iou, o_iou)
    b_low, b_iou = eng.decode_prompts(embs.to(dev), img, None, None, BOXES.to(dev))   # prompts already on the device
    assert torch.equal(b_low, o_low) and torch.equal(b_iou, o_iou)
    a_low, a_iou = eng.decode_low_res(embs.to(dev), BOXES.to(dev), img)
    assert torch.equal(a_low, o_low[:, 0]) and torch.equal(a_iou, o_iou)


@torch.no_grad()
def test_multimask_mask0_is_bitwise_single_mask(dev, eng_sd, embs):
    eng, oc, sd64 = eng_sd
    pts, lab = _points(np.random.RandomState(3), 2, 3)
    for args in ((pts, lab, None), (None, None, BOXES[:2]), (pts, lab, BOXES[:2])):
        one, iou1 = eng.decode_prompts(embs.to(dev), [0, 1], *args, masks=(0, 1))
        four, iou4 = eng.decode_prompts(embs.to(dev), [0, 1], *args, masks=(0, 4))
        three, iou3 = eng.decode_prompts(embs.to(dev), [0, 1], *args, multimask_output=True)
        assert torch.equal(four[:, :1], one) and torch.equal(iou4[:, :1], iou1)
        assert torch.equal(four[:, 1:], three) and torch.equal(iou4[:, 1:], iou3)


@torch.no_grad()
def test_token_limit_raises_before_launch(dev, eng_sd, embs):
    eng, oc, sd64 = eng_sd
    pts, lab = _points(np.random.RandomState(0), 1, 11)
    with pytest.raises(ValueError, match="limit of 16"):
        eng.decode_prompts(embs.to(dev), [0], pts, lab)
    with pytest.raises(ValueError, match="limit of 16"):
        eng.decode_prompts(embs.to(dev), [0], pts[:, :10], lab[:, :10], BOXES[:1])


@torch.no_grad()
def test_predictor_numpy_predict_on_sketch(dev, eng_sd):
    """SamPredictor.predict end to end on a synthetic sketch (original-image pixels in, numpy out), multimask by default,
    then a refinement call with the best low-res mask as mask_input; against the restatement on the same features."""
    from inklayer_amd import sam, synthetic
    eng, oc, sd64 = eng_sd
    img = synthetic.synthetic_sketch(4, 600, 800)
    pred = sam.SamPredictor(eng)
    pred.set_image(img)
    pc, pl = np.array([[200.0, 150.0], [520.0, 400.0]]), np.array([1, 0])
    masks, iou, low = pred.predict(point_coords=pc, point_labels=pl)
    assert masks.shape == (3, 600, 800) and masks.dtype == np.bool_
    assert iou.shape == (3,) and low.shape == (3, 256, 256) and low.dtype == np.float32
    feats = pred.features.cpu()[None]
    tc = torch.from_numpy(R.apply_coords(pc, (600, 800), 1024)).float()[None]
    ref_low, ref_iou = _ref(oc, sd64, feats, [0], tc, torch.from_numpy(pl)[None], None, None)
    _check(oc, torch.from_numpy(low)[None], torch.from_numpy(iou)[None], ref_low[:, 1:], ref_iou[:, 1:],
           pred.input_size, pred.original_size)
    # refinement: box + the best low-res mask, single mask; logits when asked
    k = int(iou.argmax())
    box = np.array([150.0, 100.0, 600.0, 500.0])
    m2, iou2, low2 = pred.predict(point_coords=pc, point_labels=pl, box=box, mask_input=low[k][None],
                                  multimask_output=False, return_logits=True)
    assert m2.shape == (1, 600, 800) and m2.dtype == np.float32 and iou2.shape == (1,)
    tb = torch.from_numpy(pred.transform.apply_boxes(box, (600, 800))).float()
    ref_low2, ref_iou2 = _ref(oc, sd64, feats, [0], tc, torch.from_numpy(pl)[None], tb,
                              torch.from_numpy(low[k])[None, None])
    _check(oc, torch.from_numpy(low2)[None], torch.from_numpy(iou2)[None], ref_low2[:, :1], ref_iou2[:, :1],
           pred.input_size, pred.original_size)
    # predict_torch: batched prompts in the input frame, the reference's return shapes
    tm, ti, tl = pred.predict_torch(tc.expand(2, -1, -1).to(dev), torch.from_numpy(pl)[None].expand(2, -1).to(dev),
                                    multimask_output=True)
    assert tm.shape == (2, 3, 600, 800) and tm.dtype == torch.bool and ti.shape == (2, 3) and tl.shape == (2, 3, 256, 256)
    assert torch.equal(tl[0], tl[1]) and np.array_equal(tl[0].cpu().numpy(), low)


# ------------------------------------------------------------------------------------------------ op level
@torch.no_grad()
def test_prompt_tokens_op(dev, eng_sd):
    from inklayer_amd import ops
    eng, oc, sd64 = eng_sd
    w = eng.w
    # box-only: the same bits as sam_pe_encode(add=corner embeddings) behind the copied output tokens (the box path before
    # this op)
    n = BOXES.shape[0]
    coords = ((BOXES + 0.5).reshape(-1, 2) / 1024.0).to(dev)
    old = torch.empty((n, 7, 256), device=dev)
    old[:, :5] = w["out_tok"]
    old[:, 5:] = ops.sam_pe_encode(coords, w["gauss"], add=w["pt_emb"][2:4]).view(n, 2, 256)
    new = ops.sam_prompt_tokens(w["gauss"], w["pt_emb"], w["not_a_point"], w["out_tok"], 1024.0, n, boxes=BOXES.to(dev))
    assert torch.equal(old, new)
    # points (+ pad), labels -1 / 0 / 1 / 2, against float64
    pts, lab = _points(np.random.RandomState(1), 2, 5)
    lab[1, 2] = 2
    for box, pad in ((None, True), (BOXES[:2], False)):
        tok = ops.sam_prompt_tokens(w["gauss"], w["pt_emb"], w["not_a_point"], w["out_tok"], 1024.0, 2,
                                    points=pts.to(dev), labels=lab.to(dev),
                                    boxes=box.to(dev) if box is not None else None, pad=pad)
        assert tok.shape == (2, 5 + 5 + (1 if pad else 2), 256)
        ref = R.embed_sparse(sd64, oc, pts, lab, box)
        assert torch.equal(tok[:, :5].cpu(), w["out_tok"].cpu().expand(2, -1, -1))
        # f32 sine / cosine of an argument rounded a few times: the error grows with the argument's size
        c = torch.cat([pts.double() + 0.5, torch.zeros(2, 1, 2, dtype=torch.float64)], 1) / 1024
        vmax = (2 * math.pi * (2 * c - 1) @ sd64["prompt_encoder.pe_layer.positional_encoding_gaussian_matrix"]).abs().max()
        assert (tok[:, 5:].cpu().double() - ref).abs().max().item() < 6e-8 * vmax.item() + 1e-6
        nap = sd64["prompt_encoder.not_a_point_embed.weight"].float()
        assert torch.equal(tok[:, 5:10].cpu()[lab == -1], nap.expand(int((lab == -1).sum()), -1))


@torch.no_grad()
def test_mask_embed_op(dev, eng_sd, embs):
    from inklayer_amd import ops
    eng, oc, sd64 = eng_sd
    rs = np.random.RandomState(2)
    mask = torch.from_numpy((rs.standard_normal((3, 1, 256, 256)) * 6).astype(np.float32))
    img = [1, 0, 1]
    rows = torch.tensor([i * 4096 for i in img], dtype=torch.int32, device=dev)
    keys, ks = ops.sam_mask_embed(mask.to(dev), embs.reshape(-1, 256).to(dev), rows, eng.w["mask_ds"], 1e-6, split=True)
    ref = (R.mask_downscaling(sd64, mask).permute(0, 2, 3, 1).reshape(3, 4096, 256)
           + torch.stack([embs[i] for i in img]).double()).reshape(-1, 256)
    assert _rel(keys, ref)[0] < 1e-5
    hi, lo, h64 = ks[:, :256].float(), ks[:, 256:512].float(), ks[:, 512:].float()
    assert torch.equal(hi, keys.half().float()) and torch.equal(h64, (hi / 64).half().float())
    assert ((hi + lo / 64) - keys).abs().max().item() <= 1e-3 * keys.abs().max().item() * 2 ** -11
    only = ops.sam_mask_embed(mask.to(dev), embs.reshape(-1, 256).to(dev), rows, eng.w["mask_ds"], 1e-6)
    assert torch.equal(only, keys)


@torch.no_grad()
def test_upscale_tail_masks_op(dev, eng_sd):
    from inklayer_amd import ops
    eng, oc, sd64 = eng_sd
    w, n, g = eng.w, 3, 64
    rs = np.random.RandomState(4)
    u0 = torch.from_numpy(rs.standard_normal((n * g * g, 512)).astype(np.float32)).to(dev)[:, 256:]
    hyper = torch.from_numpy(rs.standard_normal((n, 4, 32)).astype(np.float32)).to(dev)
    args = (u0, n, g, w["up1.w"], w["up1.b"], 1e-6, w["up3.blob"], w["up3.b"])
    four = ops.sam_upscale_tail(*args, hyper)
    three = ops.sam_upscale_tail(*args, hyper[:, 1:].contiguous())
    one = ops.sam_upscale_tail(*args, hyper[:, :1].contiguous())
    assert four.shape == (n, 4, 256, 256) and three.shape == (n, 3, 256, 256) and one.shape == (n, 1, 256, 256)
    assert torch.equal(four[:, :1], one) and torch.equal(four[:, 1:], three)
    for m in range(1, 4):        # mask m of the 4-mask launch = a single-mask launch with hyper vector m
        assert torch.equal(four[:, m:m + 1], ops.sam_upscale_tail(*args, hyper[:, m:m + 1].contiguous()))


@torch.no_grad()
@pytest.mark.parametrize("shared", [False, True])
def test_attn_fewq_wide_matches_narrow(dev, shared):
    """9..16 queries (4 per wave) against the <= 8-query kernel on the rows both serve, and against float64."""
    from inklayer_amd import ops
    rs = np.random.RandomState(6)
    n, H, hd, nk = 3, 8, 16, 4096
    E = H * hd
    q16 = torch.from_numpy(rs.standard_normal((n, 16, E)).astype(np.float32))
    nkv = 2 if shared else n
    k = torch.from_numpy(rs.standard_normal((nkv * nk, E)).astype(np.float32))
    v = torch.from_numpy(rs.standard_normal((nkv * nk, E)).astype(np.float32))
    kadd = torch.from_numpy(rs.standard_normal((nk, E)).astype(np.float32) * 0.5)
    kv_rows = torch.tensor([0, nk, 0], dtype=torch.int32, device=dev) if shared else None
    kw = dict(n_batch=n, n_heads=H, head_dim=hd, scale=0.25, n_k=nk, kv_batch_rows=kv_rows, k_add=kadd.to(dev))
    for nq in (9, 12, 16):
        wide = ops.attn_fewq(q16[:, :nq].reshape(-1, E).contiguous().to(dev), k.to(dev), v.to(dev), n_q=nq, **kw)
        narrow = ops.attn_fewq(q16[:, :8].reshape(-1, E).contiguous().to(dev), k.to(dev), v.to(dev), n_q=8, **kw)
        a, b = wide.view(n, nq, E)[:, :8].cpu(), narrow.view(n, 8, E).cpu()
        print(f"n_q={nq}: wide == narrow bitwise: {torch.equal(a, b)}")
        assert (a - b).abs().max().item() <= 1e-6 * b.abs().max().item()
        kk = (k.view(nkv, nk, E)[[0, 1, 0] if shared else slice(None)] + kadd).double()
        vv = v.view(nkv, nk, E)[[0, 1, 0] if shared else slice(None)].double()
        qq = q16[:, :nq].double()
        s = torch.einsum("bqhd,bkhd->bhqk", qq.view(n, nq, H, hd), kk.view(n, nk, H, hd)) * 0.25
        ref = torch.einsum("bhqk,bkhd->bqhd", s.softmax(-1), vv.view(n, nk, H, hd)).reshape(n, nq, E)
        assert _rel(wide.view(n, nq, E), ref)[0] < 1e-5


@torch.no_grad()
@pytest.mark.parametrize("nk", [8, 11, 16])
def test_attn_fewkeys16_many_tokens(dev, nk):
    """image -> token attention against 8..16 tokens (the specialised head_dim-16 f32 kernel) vs float64."""
    from inklayer_amd import ops
    rs = np.random.RandomState(nk)
    B, T, H, hd = 2, 4096, 8, 16
    E = H * hd
    q = torch.from_numpy(rs.standard_normal((T, E)).astype(np.float32))
    qadd = torch.from_numpy(rs.standard_normal((T, E)).astype(np.float32) * 0.5)
    k = torch.from_numpy(rs.standard_normal((B * nk, E)).astype(np.float32))
    v = torch.from_numpy(rs.standard_normal((B * nk, E)).astype(np.float32))
    rows = torch.zeros(B, dtype=torch.int32, device=dev)
    out = ops.attn_fewkeys(q.to(dev), k.to(dev), v.to(dev), B=B, n_heads=H, head_dim=hd, scale=0.25, n_q=T,
                           q_batch_rows=rows, q_add=qadd.to(dev))
    qq = (q + qadd).double().view(1, T, H, hd).expand(B, -1, -1, -1)
    s = torch.einsum("bqhd,bkhd->bhqk", qq, k.double().view(B, nk, H, hd)) * 0.25
    ref = torch.einsum("bhqk,bkhd->bqhd", s.softmax(-1), v.double().view(B, nk, H, hd)).reshape(B * T, E)
    assert _rel(out, ref)[0] < 1e-5
