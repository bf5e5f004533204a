"""HIP SAM path vs the CPU oracle (oracle/sam_ref.py, pinned to the reference by
tests/golden/sam_small.npz) on the same seeded weights and inputs.  GPU box only.

Tolerances: GEMM operands are f16 with f32 accumulation, so stage
outputs are compared at ~1e-2 of the tensor's max and masks by IoU (north-star: >= 0.999)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _cfgs(depth=4, glob=(1, 3)):
    from oracle import sam_ref
    from inklayer_amd import sam
    oc = sam_ref.SamConfig(depth=depth, global_attn_indexes=glob)
    ec = sam.SamConfig(depth=depth, global_attn_indexes=glob)
    return oc, ec


def _rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).abs().max() / b.abs().max()).item(), ((a - b).norm() / b.norm()).item()


@pytest.fixture(scope="module")
def small_vith(dev):
    from oracle import sam_ref
    from inklayer_amd import sam
    oc, ec = _cfgs()
    sd = sam_ref.seeded_state_dict(sam_ref.sam_param_shapes(oc), 11)
    eng = sam.SamEngine(sd, ec, dev, max_batch=2)
    return sd, oc, eng


def _sketch(seed, h=1024, w=1024):
    """synthetic sketch: white background, black strokes."""
    from PIL import Image, ImageDraw
    rs = np.random.RandomState(seed)
    im = Image.new("RGB", (w, h), (255, 255, 255))
    d = ImageDraw.Draw(im)
    for _ in range(40):
        x0, y0, x1, y1 = rs.randint(0, w), rs.randint(0, h), rs.randint(0, w), rs.randint(0, h)
        wd = int(rs.randint(2, 7))
        if rs.rand() < 0.5:
            d.line([(x0, y0), (x1, y1), (rs.randint(0, w), rs.randint(0, h))], fill=(0, 0, 0), width=wd)
        else:
            d.ellipse([min(x0, x1), min(y0, y1), max(x0, x1) + 1, max(y0, y1) + 1], outline=(0, 0, 0), width=wd)
    return np.asarray(im)


@torch.no_grad()
def test_encoder_stages_match_oracle(dev, small_vith):
    from oracle import sam_ref
    sd, oc, eng = small_vith
    rs = np.random.RandomState(3)
    img = rs.randint(0, 256, size=(1024, 768, 3)).astype(np.uint8)     # w < L: exercises the zero pad
    x = sam_ref.preprocess(oc, torch.from_numpy(img).permute(2, 0, 1))[None]
    dimg = torch.from_numpy(img).to(dev)
    for upto in (1, 2, 4):
        ref = sam_ref.image_encoder(sd, oc, x, upto=upto)[0].reshape(4096, -1)
        got = eng.encode([dimg], upto=upto)[0]
        mx, l2 = _rel(got, ref)
        print(f"blocks={upto}: max-rel {mx:.2e}  l2-rel {l2:.2e}")
        assert mx < 1e-2 and l2 < 3e-3
    ref = sam_ref.image_encoder(sd, oc, x)[0].permute(1, 2, 0).reshape(4096, -1)
    got = eng.encode([dimg])[0]
    mx, l2 = _rel(got, ref)
    print(f"embedding: max-rel {mx:.2e}  l2-rel {l2:.2e}")
    assert mx < 1e-2 and l2 < 3e-3


@torch.no_grad()
def test_encoder_batch2_equals_batch1(dev, small_vith):
    sd, oc, eng = small_vith
    a = torch.from_numpy(_sketch(0)).to(dev)
    b = torch.from_numpy(_sketch(1, 900, 1024)).to(dev)
    e2 = eng.encode([a, b]).clone()
    assert torch.equal(e2[0], eng.encode([a])[0])
    assert torch.equal(e2[1], eng.encode([b])[0])


@torch.no_grad()
def test_encoder_graph_replay_equals_eager(dev, small_vith):
    """The blocks + neck are replayed as one HIP graph from the second sighting of a batch size on: eager, capturing
    and replaying calls must agree bit for bit, also after another batch size evicted nothing / was captured too."""
    sd, oc, eng = small_vith
    a = torch.from_numpy(_sketch(0)).to(dev)
    b = torch.from_numpy(_sketch(1, 900, 1024)).to(dev)
    saved = eng.graph_blocks
    try:
        eng.graph_blocks = False
        ref_a, ref_ab = eng.encode([a]).clone(), eng.encode([a, b]).clone()
        eng.graph_blocks = True
        eng._enc_graphs = type(eng._enc_graphs)(eng.graph_cache_size)
        eng._enc_seen.clear()
        for _ in range(3):                                   # eager, capture, replay
            assert torch.equal(eng.encode([a]), ref_a)
            assert torch.equal(eng.encode([a, b]), ref_ab)
        assert len(eng._enc_graphs) == 2
    finally:
        eng.graph_blocks = saved


@torch.no_grad()
def test_decoder_matches_oracle(dev, small_vith):
    from oracle import sam_ref
    sd, oc, eng = small_vith
    rs = np.random.RandomState(5)
    emb = torch.from_numpy(rs.standard_normal((4096, 256)).astype(np.float32))
    boxes = torch.tensor([[10.0, 20.0, 500.0, 400.0], [300.5, 100.25, 900.0, 1000.0],
                          [0.0, 0.0, 1023.0, 767.0], [640.0, 320.0, 700.0, 380.0],
                          [50.0, 600.0, 400.0, 760.0]])
    input_hw, orig_hw = (1024, 768), (1500, 1125)
    ref_low, ref_iou = sam_ref.mask_decoder(sd, oc, emb.t().reshape(1, 256, 64, 64),
                                            sam_ref.dense_pe(sd, oc), sam_ref.embed_boxes(sd, oc, boxes))
    ref_logits = sam_ref.postprocess_masks(oc, ref_low, input_hw, orig_hw)
    masks, low, iou, logits = eng.decode(emb.to(dev), boxes, input_hw, orig_hw, want_logits=True)
    mx, l2 = _rel(low, ref_low[:, 0])
    print(f"low-res logits: max-rel {mx:.2e} l2-rel {l2:.2e}")
    assert mx < 1e-4 and l2 < 2e-5                      # split-f16 decoder: fp32-grade
    assert _rel(iou, ref_iou)[0] < 1e-4
    # postprocess kernel alone (same low-res input) must agree to f32 rounding
    from inklayer_amd import ops
    m2, lg2 = ops.sam_postprocess(ref_low[:, 0].contiguous().to(dev), 1024, input_hw, orig_hw, 0.0, True)
    assert (lg2.cpu() - ref_logits[:, 0]).abs().max().item() < 1e-5 * ref_logits.abs().max().item() + 1e-6
    ref_m = ref_logits[:, 0] > 0
    flips = (m2.cpu().bool() != ref_m)
    assert flips.float().mean().item() < 1e-5
    # end-to-end masks of the f16 path: IoU per instance
    got = masks.cpu().bool()
    inter = (got & ref_m).flatten(1).sum(1).double()
    union = (got | ref_m).flatten(1).sum(1).double()
    print("decoder mask IoU:", (inter / union).tolist())
    # Random weights give noise-like masks (|logit| ~ 0 on a large share of the pixels), the worst
    # case for a threshold at exactly 0.  North-star tolerance: IoU >= 0.999 per instance; with the decoder on
    # split-f16 operands the low-res logits agree to ~1e-6 and the masks are identical up to a handful of pixels.
    # In addition EVERY flipped pixel must be explained by the stated fp tolerance, i.e. its fp32 reference logit lies
    # within 1 % of the logit scale of the threshold.
    assert (inter / union).min().item() >= 0.999
    flipped = got != ref_m
    tol = 1e-2 * ref_logits[:, 0].std().item()
    assert ref_logits[:, 0][flipped].abs().max().item() < tol
    decisive = ref_logits[:, 0].abs() >= tol
    assert torch.equal(got[decisive], ref_m[decisive])        # IoU == 1 on all decisive pixels


@torch.no_grad()
def test_run_sam_plugin_matches_oracle(dev, small_vith):
    """InkLayer.segmentor.sam.run_SAM surface: PIL image + pixel boxes -> list of HxW bool."""
    from PIL import Image
    from oracle import sam_ref
    from inklayer_amd import sam
    sd, oc, eng = small_vith
    img = _sketch(2, 750, 750)                      # data/bunny_cook_sketch.png is 750x750
    boxes = torch.tensor([[30.0, 40.0, 400.0, 420.0], [200.0, 100.0, 700.0, 640.0], [5.0, 500.0, 300.0, 745.0]])
    ref_logits, _, _ = sam_ref.run_sam(sd, oc, img, boxes, return_logits=True)
    ref = [m[0].numpy() for m in (ref_logits > 0.0)]
    got = sam.run_SAM(Image.fromarray(img), boxes, engine=eng)
    assert len(got) == 3 and got[0].shape == (750, 750) and got[0].dtype == np.bool_
    ious = [float((g & r).sum() / max(1, (g | r).sum())) for g, r in zip(got, ref)]
    print("run_SAM IoU:", ious)
    assert min(ious) >= 0.999                                 # north-star tolerance
    tol = 1e-2 * ref_logits.std().item()                      # flips only where |fp32 logit| < 1 % of its scale
    for g, r, lg in zip(got, ref, ref_logits[:, 0].numpy()):
        assert np.abs(lg[g != r]).max(initial=0.0) < tol
    assert sam.run_SAM(Image.fromarray(img), torch.zeros((0, 4)), engine=eng) == []


@torch.no_grad()
def test_pipeline_two_stream_overlap_equals_serial(dev, small_vith):
    """Detector + SAM encoder on two HIP streams must give bit-identical results to the serial order."""
    from inklayer_amd import gdino, pipeline, weights_init
    sd, oc, eng = small_vith
    gcfg = gdino.GDinoConfig(enc_layers=1, dec_layers=1, num_queries=100)
    det = gdino.GDinoEngine(weights_init.random_gdino_state_dict(gcfg, dev, 5), gcfg, dev,
                            encoded_text=weights_init.random_text_features(gcfg, dev))
    imgs = [_sketch(7, 600, 800), _sketch(8, 600, 800)]
    a = pipeline.InkLayerPipeline(det, eng, overlap=True).run_batch(imgs, top_n=5)
    b = pipeline.InkLayerPipeline(det, eng, overlap=False).run_batch(imgs, top_n=5)
    torch.cuda.synchronize()
    for ra, rb in zip(a, b):
        assert np.array_equal(ra.boxes_xyxy_norm, rb.boxes_xyxy_norm) and torch.equal(ra.masks, rb.masks)
        assert ra.masks.shape == (5, 600, 800) and ra.masks.dtype == torch.uint8
    # host-to-host entry (pinned sketches in, pinned u8 masks out), three batches in flight over the two slots
    pp = pipeline.InkLayerPipeline(det, eng, overlap=True)
    pinned = pp.pinned_like(imgs)
    t1 = pp.submit_host(pinned, top_n=5)
    t2 = pp.submit_host(pinned, top_n=5)
    r1 = pp.collect_host(t1)
    t3 = pp.submit_host(pinned, top_n=5)            # reuses slot 0 (collected above)
    for got in (r1, pp.collect_host(t2), pp.collect_host(t3)):
        for (xyxy, sc, pix, m), rb in zip(got, b):
            assert m.dtype == np.uint8 and m.shape == (5, 600, 800)
            assert np.array_equal(m, rb.masks.cpu().numpy()) and np.array_equal(xyxy, rb.boxes_xyxy_norm)


@torch.no_grad()
def test_pipeline_mixed_sizes_and_empty_detections(dev, small_vith):
    """A batch of differently sized sketches (detector runs per size group) and the zero-box edge case."""
    from inklayer_amd import gdino, pipeline, weights_init
    sd, oc, eng = small_vith
    gcfg = gdino.GDinoConfig(enc_layers=1, dec_layers=1, num_queries=100)
    det = gdino.GDinoEngine(weights_init.random_gdino_state_dict(gcfg, dev, 5), gcfg, dev,
                            encoded_text=weights_init.random_text_features(gcfg, dev))
    pipe = pipeline.InkLayerPipeline(det, eng)
    imgs = [_sketch(1, 512, 512), _sketch(2, 600, 800)]
    both = pipe.run_batch(imgs, top_n=3)
    solo = [pipe.run_batch([im], top_n=3)[0] for im in imgs]
    torch.cuda.synchronize()
    for r, s_, im in zip(both, solo, imgs):
        assert r.masks.shape == (3,) + im.shape[:2]
        assert np.allclose(r.boxes_xyxy_norm, s_.boxes_xyxy_norm, atol=1e-5) and torch.equal(r.masks, s_.masks)
    # threshold so high that nothing is detected -> empty results, no kernel is launched for the decoder
    det.cfg.box_threshold = 2.0
    res = pipe.run_batch(imgs)
    assert all(r.masks.shape[0] == 0 and r.boxes_xyxy_norm.shape == (0, 4) for r in res)
    # ... and through the host-to-host entry (nothing to download), mixed sizes included
    got = pipe.collect_host(pipe.submit_host(pipe.pinned_like(imgs)))
    assert [g[3].shape for g in got] == [(0, 512, 512), (0, 600, 800)] and all(g[0].shape == (0, 4) for g in got)
    det.cfg.box_threshold = 0.2
    got = pipe.collect_host(pipe.submit_host(pipe.pinned_like(imgs), top_n=3))
    for g, s_ in zip(got, solo):
        assert np.array_equal(g[3], s_.masks.cpu().numpy()) and g[3].dtype == np.uint8


@torch.no_grad()
@pytest.mark.parametrize("input_hw,orig_hw", [((1024, 1024), (1024, 1024)), ((768, 1024), (1200, 1600)), ((1024, 683), (768, 512))])
def test_postprocess_packed_path_matches_oracle(dev, small_vith, input_hw, orig_hw):
    """Output widths that are multiples of 4 take the 4-pixels-per-thread kernel (one packed store per lane): same
    arithmetic as the one-pixel kernel, checked against the oracle's two F.interpolate calls + threshold."""
    from oracle import sam_ref
    from inklayer_amd import ops
    sd, oc, eng = small_vith
    rs = np.random.RandomState(21)
    low = torch.from_numpy(rs.standard_normal((3, 1, 256, 256)).astype(np.float32))
    ref_logits = sam_ref.postprocess_masks(oc, low, input_hw, orig_hw)[:, 0]
    m, lg = ops.sam_postprocess(low[:, 0].contiguous().to(dev), 1024, input_hw, orig_hw, 0.0, True)
    assert tuple(m.shape) == (3,) + tuple(orig_hw)
    assert (lg.cpu() - ref_logits).abs().max().item() < 1e-5 * ref_logits.abs().max().item() + 1e-6
    assert (m.cpu().bool() != (ref_logits > 0)).float().mean().item() < 1e-5
    m2 = ops.sam_postprocess(low[:, 0].contiguous().to(dev), 1024, input_hw, orig_hw, 0.0, False)
    assert torch.equal(m2, m)


@torch.no_grad()
def test_engine_leaves_the_state_dict_untouched_and_bias_correction_helps(dev):
    """The load-time bias correction (SamEngine._calibrate_bias_correction) writes NEW bias tensors - the caller's state
    dict (which may share storage with the engine's f32 parameters) is not modified - and it lowers the error of the
    block stack on a sketch (depth 4 here; full depth: tests/test_full_depth_gpu.py)."""
    from oracle import sam_ref
    from inklayer_amd import sam, synthetic, weights_init
    oc, ec = _cfgs()
    sd = weights_init.random_sam_state_dict(ec, dev, 7)                 # device tensors: the engine may alias them
    before = {k: v.clone() for k, v in sd.items()}
    eng = sam.SamEngine(sd, ec, dev)
    assert all(torch.equal(v, before[k]) for k, v in sd.items())
    plain = sam.SamEngine(sd, ec, dev, bias_correction=False)
    img = synthetic.synthetic_sketch(4)
    x = sam_ref.preprocess(oc, torch.from_numpy(img.copy()).permute(2, 0, 1))[None]
    ref = sam_ref.image_encoder({k: v.cpu() for k, v in sd.items()}, oc, x, upto=4)[0].reshape(4096, -1)
    dimg = torch.from_numpy(img.copy()).to(dev)
    e_corr = _rel(eng.encode([dimg], upto=4)[0], ref)[1]
    e_plain = _rel(plain.encode([dimg], upto=4)[0], ref)[1]
    print(f"4 blocks on a sketch: l2-rel {e_plain:.2e} plain f16 weights, {e_corr:.2e} with the bias correction")
    assert e_corr < 0.85 * e_plain


@torch.no_grad()
@pytest.mark.parametrize("M", [1, 3, 4])
@pytest.mark.parametrize("n,g", [(3, 16), (2, 64), (5, 4)])
def test_upscale_tail_kernel_equals_the_three_kernel_form(dev, n, g, M):
    """ops.sam_upscale_tail (csrc/upscale_tail.hip) = LayerNorm2d + GELU + ConvTranspose2d(k2 s2) + GELU + hyper-network
    product (mask_decoder.py:54-60, 138-145) for M mask tokens per box: every mask against float64, mask 0 also against
    the three-kernel form the kernel replaces (layernorm_rows(split) + split GEMM + sam_mask_logits).  (5, 4) is 10 tiles:
    a partial last workgroup, and the box index changes inside a tile."""
    from inklayer_amd import ops
    gen = torch.Generator().manual_seed(100 * n + g)
    T = g * g
    u0 = torch.randn(n * T * 4, 64, generator=gen) * 1.7 + 0.2
    w3 = torch.randn(128, 64, generator=gen) / 8                      # rows (s2, c)
    b3 = (torch.randn(32, generator=gen) * 0.3).repeat(4)
    lg, lb = 1 + 0.2 * torch.randn(64, generator=gen), 0.2 * torch.randn(64, generator=gen)
    hyper = torch.randn(n, M, 32, generator=gen)
    gelu = torch.nn.functional.gelu
    a = gelu(torch.nn.functional.layer_norm(u0.double(), (64,), lg.double(), lb.double(), 1e-6))
    up = gelu(a @ w3.double().t() + b3.double()).view(n, 1, g, g, 2, 2, 2, 2, 32)    # [b, m, y, x, s1y, s1x, s2y, s2x, c]
    val = (up * hyper.double().view(n, M, 1, 1, 1, 1, 1, 1, 32)).sum(-1)
    want = val.permute(0, 1, 2, 4, 6, 3, 5, 7).reshape(n, M, 4 * g, 4 * g)           # Y = 4y + 2 s1y + s2y, X alike
    d = lambda t: t.to(dev).contiguous()
    ws = ops.split_weight(d(w3))
    low = ops.sam_upscale_tail(d(u0), n, g, d(lg), d(lb), 1e-6, ops.sam_upscale_pack(ws), d(b3), d(hyper))
    assert low.shape == (n, M, 4 * g, 4 * g)
    errs = [((low[:, m].double().cpu() - want[:, m]).abs().max() / want[:, m].abs().max()).item() for m in range(M)]
    u1 = ops.layernorm_rows(d(u0), d(lg), d(lb), 1e-6, act="gelu", split=True)
    u2 = ops.gemm(u1, ws, d(b3), act="gelu")
    three = ops.sam_mask_logits(u2, d(hyper[:, 0]), n, g)
    err3 = ((low[:, 0] - three).abs().max() / three.abs().max()).item()
    print(f"n={n} g={g} M={M}: fused tail vs float64 max-rel {max(errs):.2e}, vs the three-kernel form {err3:.2e}")
    assert max(errs) < 5e-6 and err3 < 5e-6


@torch.no_grad()
@pytest.mark.parametrize("shared", [False, True])
def test_proj_layernorm_kernel_equals_the_three_kernel_form(dev, shared):
    """ops.proj256_ln (csrc/proj_ln.hip) = LayerNorm(res + a W^T + b) with the projection on split-f16 operands, f32 and
    split outputs (transformer.py:175-182 on the per-box image tokens) against float64 and against add_split + GEMM +
    layernorm_rows; `shared`: the residual is a per-image tensor gathered per box."""
    from inklayer_amd import ops
    gen = torch.Generator().manual_seed(7 + int(shared))
    n, T = 3, 200                                     # 600 rows: a ragged last tile
    R = n * T
    a = torch.randn(R, 128, generator=gen) * 0.8
    w = torch.randn(256, 128, generator=gen) / 11
    b = torch.randn(256, generator=gen) * 0.2
    lg, lb = 1 + 0.1 * torch.randn(256, generator=gen), 0.1 * torch.randn(256, generator=gen)
    if shared:
        keys = torch.randn(2 * T, 256, generator=gen)                       # two images, boxes 0, 1 -> image 0, box 2 -> image 1
        rows = torch.tensor([0, 0, T], dtype=torch.int32)
        res = torch.cat([keys[0:T], keys[0:T], keys[T:2 * T]], 0)
    else:
        keys, rows, res = torch.randn(R, 256, generator=gen), None, None
        res = keys
    want = torch.nn.functional.layer_norm(res.double() + a.double() @ w.double().t() + b.double(), (256,), lg.double(),
                                          lb.double(), 1e-5)
    d = lambda t: t.to(dev).contiguous()
    ws = ops.split_weight(d(w))
    of, osp = ops.proj256_ln(d(a), ops.proj256_ln_pack(ws), d(b), d(keys), d(lg), d(lb), 1e-5,
                             res_batch_rows=d(rows) if shared else None, rows_per_batch=T if shared else 0)
    err = ((of.double().cpu() - want).abs().max() / want.abs().max()).item()
    hi, lo = osp[:, :256].float(), osp[:, 256:512].float() / 64.0
    rec = ((hi + lo).double().cpu() - want).abs().max().item()
    assert torch.equal(osp[:, 512:], (osp[:, :256].float() / 64.0).half())
    y = ops.gemm(ops.add_split_f16(d(a)), ws, d(b), residual=d(res))
    three = ops.layernorm_rows(y, d(lg), d(lb), 1e-5, out_dtype=torch.float32)
    e3 = ((of - three).abs().max() / three.abs().max()).item()
    print(f"shared={shared}: fused vs float64 max-rel {err:.2e}, split reconstruction max abs {rec:.2e}, vs three kernels {e3:.2e}")
    assert err < 3e-6 and e3 < 3e-6 and rec < 2e-5
    only_split = ops.proj256_ln(d(a), ops.proj256_ln_pack(ws), d(b), d(keys), d(lg), d(lb), 1e-5,
                                res_batch_rows=d(rows) if shared else None, rows_per_batch=T if shared else 0, want_f32=False)
    assert only_split[0] is None and torch.equal(only_split[1], osp)
