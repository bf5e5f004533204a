"""The depth engine beyond single-image ViT-B: the ViT-S and ViT-L encoders (one block and the DPT head against float64,
held as tests/test_depth_ops_gpu.py holds ViT-B, at 9 x 11 patches and B = 2; then the full models end to end through
infer_images against oracle/depth_ref.py, with the tolerance measured against the oracle's own f16-operand emulation),
ViT-B batched inference over two image sizes in one call, and the plugin's `encoder` switch.  Seeded weights from
depth_ref.seeded_state_dict; the oracle for ViT-S / ViT-L is pinned to the reference's modules by
tests/golden/depth_models_small.npz (tests/test_depth_models_cpu.py).  GPU box only."""
from dataclasses import replace

import numpy as np
import pytest
import torch

from test_depth_models_cpu import oracle_config
from test_depth_ops_gpu import HEAD_STAGES, MEAN, STD, block_refs, check_yardstick, head_refs

pytestmark = pytest.mark.gpu

PH, PW = 9, 11                      # a 160 x 200 sketch at input_size 126 -> 126 x 154 -> 9 x 11 patches
SKETCH = (160, 200)
CPU = torch.device("cpu")


def _l2(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).norm() / b.norm()).item()


def _rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).abs().max() / b.abs().max()).item(), ((a - b).norm() / b.norm()).item()


def _sketch_bgr(seed, hw=SKETCH):
    from inklayer_amd import synthetic
    return np.ascontiguousarray(synthetic.synthetic_sketch(seed, hw[0], hw[1])[..., ::-1])


# ---------------------------------------------------------------------------------------------------------------
# one encoder block and the DPT head per model
# ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=["vits", "vitl"])
def engine1(request, dev):
    """A depth-1 engine (one block, the whole DPT head) of the model on seeded weights, and the oracle's view of them
    (attn.proj doubled as in tests/test_depth_ops_gpu.py::engine1, for the dropped-LayerScale mistake at the median)."""
    from oracle import depth_ref
    from inklayer_amd import depth
    name = request.param
    cfg = oracle_config(name, depth=1, layer_idx=(0,))
    sd = depth_ref.seeded_state_dict(cfg, 17)
    for leaf in ("weight", "bias"):
        sd[f"pretrained.blocks.0.attn.proj.{leaf}"] = sd[f"pretrained.blocks.0.attn.proj.{leaf}"] * 2
    return name, sd, cfg, depth.DepthEngine(sd, replace(depth.config_for(name), depth=1, layer_idx=(0,)), dev)


@torch.no_grad()
def test_block_matches_float64(dev, engine1):
    """DepthEngine.encode at depth 1 for ViT-S / ViT-L at 9 x 11 patches (the interpolated position embedding), B = 2:
    each batch entry against block_refs of its own patches under check_yardstick (at every error quantile at most 2x
    the float64 block under f16_operands plus 2^-12 max |update|); the dropped LayerScale and the omitted q scale miss
    it >= 100x; entry 1 is not entry 0; the batch equals the single-image runs bit for bit."""
    from inklayer_amd import ops
    name, sd, cfg, eng = engine1
    T, D = PH * PW, cfg.embed_dim
    nh, nw = 14 * PH, 14 * PW
    pts = [ops.depth_patchify(torch.from_numpy(_sketch_bgr(seed)).to(dev), nh, nw, 14, eng.KP, MEAN, STD, chan_reverse=True)
           for seed in (4, 5)]
    both = eng.encode(pts, PH, PW)
    assert len(both) == 1 and tuple(both[0].shape) == (2 * T, D) and both[0].dtype == torch.float16
    for b in range(2):
        rec = (pts[b][:, :588].double() + pts[b][:, eng.KP:eng.KP + 588].double() / 64).cpu()
        ref, emul, wrongs, upd = block_refs(sd, cfg, rec, nh, nw, CPU)
        check_yardstick(f"{name} block {PH}x{PW} entry {b}", both[0][b * T:(b + 1) * T].double().cpu(), ref, emul, upd, wrongs)
        assert torch.equal(both[0][b * T:(b + 1) * T], eng.encode([pts[b]], PH, PW)[0])
    assert not torch.equal(both[0][:T], both[0][T:])


def head_wrong_from(stage):
    """Quantile from which the head's named mistakes have to miss the bound: 0.9 as for ViT-B, but 0.999 on the depth map
    - with these seeded weights more than 90 % of ViT-S's ReLU'd map is 0 whatever the head does."""
    return 0.999 if stage == "out" else 0.9


def head_features(cfg, seed):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(PH * PW, cfg.embed_dim, generator=g).half() for _ in range(4)]


@torch.no_grad()
def test_dpt_head_matches_float64(dev, engine1):
    """DepthEngine.head_batch for ViT-S (48 channels held as 64 on level 0) / ViT-L at 9 x 11 patches, B = 2, on random
    f16 features: every stage of each batch entry (layer_rn 1..4, path_4..path_1, the depth map) against
    depth_ref.dpt_head in float64 on that entry's features, under check_yardstick with STAGE_ABS * max |stage|."""
    name, sd, cfg, eng = engine1
    T, Fe = PH * PW, cfg.features
    feats = [head_features(cfg, 500), head_features(cfg, 501)]
    st = {}
    d = eng.head_batch([torch.cat([feats[0][i], feats[1][i]]).to(dev) for i in range(4)], 2, PH, PW, st)
    assert tuple(d.shape) == (2, 14 * PH, 14 * PW)
    assert tuple(st["rn"][0].shape) == (2 * 16 * T, Fe) and tuple(st["path"][0].shape) == (2 * 64 * T, Fe)
    for b in range(2):
        got = {"out": d[b].reshape(-1).double().cpu()}
        for i in range(4):
            for key, t in ((f"rn{i}", st["rn"][i]), (f"path{i}", st["path"][i])):
                n = t.shape[0] // 2
                got[key] = t[b * n:(b + 1) * n].double().cpu()
        ref, emul, wrongs = head_refs(sd, cfg, feats[b], PH, PW, CPU, mistakes=(b == 0))
        for stage in HEAD_STAGES:
            assert got[stage].shape == ref[stage].shape, stage
            ws = [] if stage.startswith("rn") else [(n, w[stage]) for n, w in wrongs.items()]
            check_yardstick(f"{name} head entry {b} {stage}", got[stage], ref[stage], emul[stage],
                            ref[stage].abs().max().item(), ws, wrong_from=head_wrong_from(stage))
    one = eng.head([f.to(dev) for f in feats[1]], PH, PW)
    assert torch.equal(one, d[1]) and not torch.equal(d[0], d[1])


# ---------------------------------------------------------------------------------------------------------------
# end to end, full depth
# ---------------------------------------------------------------------------------------------------------------
def oracle_stages(sd, cfg, bgr):
    """depth_ref.infer_image with its stages kept: the four taps [T, D], the network's map and the resized map."""
    from oracle import depth_ref
    x, (h, w) = depth_ref.image2tensor(bgr, cfg)
    st = {}
    net = depth_ref.forward(sd, cfg, x, stages=st)
    out = torch.nn.functional.interpolate(net[:, None], (h, w), mode="bilinear", align_corners=True)[0, 0]
    return {**{f"tap{i}": st["feats"][i][0][0] for i in range(4)}, "net": net[0], "depth": out}


E2E_STAGES = ["tap0", "tap1", "tap2", "tap3", "net", "depth"]


@torch.no_grad()
@pytest.mark.parametrize("name,seed", [("vits", 41), ("vitl", 43)])
def test_full_model_matches_oracle(dev, name, seed):
    """Two different 160 x 200 sketches through infer_images at input_size 126 (9 x 11 patches, the position-embedding
    interpolation, head levels 36x44 / 18x22 / 9x11 / 5x6) against depth_ref.infer_image.  Bound per batch entry and
    stage (four taps, the network's map, the resized map): the l2-relative error against the fp32 oracle is at most 2x
    that of the oracle itself under depth_ref.f16_operands() on the same input (the project's yardstick factor: the
    emulation does not round q, k, v and P inside the attention; the engine's split-f16 patch embedding errs the other
    way).  Entry 1 held against entry 0's oracle has to miss that bound (batch mix-up)."""
    from oracle import depth_ref
    from inklayer_amd import depth
    cfg = oracle_config(name, input_size=126)
    sd = depth_ref.seeded_state_dict(cfg, seed)
    eng = depth.DepthEngine(sd, replace(depth.config_for(name), input_size=126), dev)
    bgrs = [_sketch_bgr(s) for s in (4, 5)]
    groups = []
    got = eng.infer_images(bgrs, stages=groups)
    assert len(got) == 2 and len(groups) == 1 and groups[0]["indices"] == [0, 1]
    g = groups[0]
    T, D = PH * PW, cfg.embed_dim
    assert tuple(g["feats"][0].shape) == (2 * T, D) and tuple(g["depth_net"].shape) == (2, 14 * PH, 14 * PW)
    refs = []
    for b, bgr in enumerate(bgrs):
        assert tuple(got[b].shape) == SKETCH and got[b].dtype == torch.float32 and torch.isfinite(got[b]).all()
        mine = {**{f"tap{i}": g["feats"][i][b * T:(b + 1) * T] for i in range(4)}, "net": g["depth_net"][b], "depth": got[b]}
        ref = oracle_stages(sd, cfg, bgr)
        with depth_ref.f16_operands():
            emul = oracle_stages(sd, cfg, bgr)
        refs.append(ref)
        assert ref["net"].max().item() > 0.05, "dead depth map"
        for stage in E2E_STAGES:
            e_hip, e_emul = _l2(mine[stage], ref[stage]), _l2(emul[stage], ref[stage])
            print(f"  {name} entry {b} {stage}: l2-rel HIP {e_hip:.3e}  f16-operand oracle {e_emul:.3e}  ratio {e_hip / e_emul:.3f}")
            assert e_hip <= 2 * e_emul, (name, b, stage, e_hip, e_emul)
            if b == 1:
                swapped = _l2(mine[stage], refs[0][stage])
                assert swapped > 2 * e_emul, ("entry 1 passes against entry 0's oracle", name, stage, swapped, e_emul)
    single = eng.infer_image(bgrs[1])
    assert torch.equal(single, got[1])


# ---------------------------------------------------------------------------------------------------------------
# ViT-B: several sizes in one call
# ---------------------------------------------------------------------------------------------------------------
@torch.no_grad()
def test_vitb_infer_images_mixed_sizes(dev):
    """infer_images([266x266, 252x322, 266x266]) on ViT-B (input_size 266: 19 x 19 and 19 x 24 patches): two size groups,
    results in input order, each image within the bounds of tests/test_depth_gpu.py::test_depth_pipeline_matches_oracle
    against depth_ref; the two 266 x 266 images are different and each equals its single-image run bit for bit."""
    from oracle import depth_ref
    from inklayer_amd import depth
    cfg = depth_ref.DepthConfig(input_size=266)
    sd = depth_ref.seeded_state_dict(cfg, 31)
    eng = depth.DepthEngine(sd, depth.DepthConfig(input_size=266), dev)
    sizes = [(266, 266), (252, 322), (266, 266)]
    bgrs = [_sketch_bgr(10 + i, hw) for i, hw in enumerate(sizes)]
    groups = []
    got = eng.infer_images(bgrs, stages=groups)
    assert [g["indices"] for g in groups] == [[0, 2], [1]] and [g["size"] for g in groups] == [(266, 266), (252, 322)]
    for gi, g in enumerate(groups):
        B = len(g["indices"])
        for j, i in enumerate(g["indices"]):
            assert tuple(got[i].shape) == sizes[i]
            x, _ = depth_ref.image2tensor(bgrs[i], cfg)
            st = {}
            ref_net = depth_ref.forward(sd, cfg, x, stages=st)[0]
            ref = depth_ref.infer_image(sd, cfg, bgrs[i])
            T = (x.shape[-2] // 14) * (x.shape[-1] // 14)
            for k in range(4):
                mx, l2 = _rel(g["feats"][k][j * T:(j + 1) * T].float(), st["feats"][k][0][0])
                assert l2 < 3e-3, (i, k, l2)
                n = g["path"][k].shape[0] // B
                mx, l2 = _rel(g["path"][k][j * n:(j + 1) * n], st["path"][k][0].permute(1, 2, 0).reshape(-1, 128))
                assert l2 < 5e-3, (i, k, l2)
            net = g["depth_net"][j] if B > 1 else g["depth_net"]
            mx, l2 = _rel(net, ref_net)
            print(f"  image {i} {sizes[i]}: network depth max-rel {mx:.2e} l2-rel {l2:.2e}")
            assert mx < 1.5e-2 and l2 < 8e-3
            mx, l2 = _rel(got[i], torch.from_numpy(ref))
            assert mx < 1e-2 and l2 < 5e-3
            assert torch.equal(got[i], eng.infer_image(bgrs[i]))
    assert not torch.equal(got[0], got[2])


# ---------------------------------------------------------------------------------------------------------------
# the plugin's encoder switch
# ---------------------------------------------------------------------------------------------------------------
@torch.no_grad()
def test_plugin_encoder_switch(dev, monkeypatch, tmp_path):
    from PIL import Image
    from InkLayer.refinement import depth_sort
    from inklayer_amd import synthetic
    monkeypatch.setenv("INKLAYER_RANDOM_WEIGHTS", "1")
    monkeypatch.setattr(depth_sort, "_engine", None)
    monkeypatch.setattr(depth_sort, "_engine_encoder", None)
    monkeypatch.setattr(depth_sort, "encoder", "vits")
    path = tmp_path / "sketch.png"
    Image.fromarray(synthetic.synthetic_sketch(2, 150, 210)).save(path)
    d = depth_sort.get_depth_map_device(str(path))
    assert tuple(d.shape) == (150, 210) and d.dtype == torch.float32 and d.is_cuda and torch.isfinite(d).all()
    small = depth_sort._engine
    assert small.cfg.encoder == "vits" and small.cfg.embed_dim == 384 and small.ocp[0] == 64
    assert depth_sort._get_engine() is small
    depth_sort.encoder = "vitb"
    d2 = depth_sort.get_depth_map(str(path))
    base = depth_sort._engine
    assert base is not small and base.cfg.encoder == "vitb" and base.cfg.embed_dim == 768
    assert d2.shape == (150, 210) and d2.dtype == np.float32 and np.isfinite(d2).all()
