"""CPU side of the Depth-Anything-V2 model registry (ViT-S / ViT-B / ViT-L), the ViT-S channel padding, the batched
engine's interface and the direct 3x3 convolution's reference:
  * inklayer_amd.depth.DEPTH_CONFIGS against the reference's tables, config_for / config_from_state_dict, the plugin's
    `encoder` switch refusing "vitg" and unknown names before anything touches a GPU;
  * depth.pack_head_level: the packed-and-padded projects.0 -> resize_layers.0 -> layer1_rn chain equals the unpadded
    chain bit for bit;
  * oracle/depth_ref.py for ViT-S and ViT-L against tests/golden/depth_models_small.npz (the reference's own modules,
    tests/golden/make_depth_models_golden.py);
  * tests/conv3x3_ref.py: its two statements of the convolution agree, its bound is depth_ops_ref.gemm_tol, and every
    named mistake lands >= 100x outside it on the data tests/test_conv3x3_gpu.py runs;
  * ink_conv3x3_f16's argument checks (nothing is launched: there is no GPU here)."""
from pathlib import Path

import numpy as np
import pytest
import torch

import conv3x3_ref as R
import depth_ops_ref as DR

GOLD = Path(__file__).resolve().parent / "golden" / "depth_models_small.npz"

# the reference's tables, as literals:
#   features / out_channels: depth_model_configs, InkLayer/refinement/depth_sort.py:20-27
#   embed_dim / blocks / heads: vit_small, vit_base, vit_large, DA/dinov2.py:339-379
#   layer_idx: DepthAnythingV2.intermediate_layer_idx, DA/dpt.py:164-169
#   patch 14, image 518, interpolate_offset 0.1: DINOv2(), DA/dinov2.py:406-415
REFERENCE = {
    "vits": dict(embed_dim=384, depth=12, num_heads=6, layer_idx=(2, 5, 8, 11), features=64,
                 out_channels=(48, 96, 192, 384)),
    "vitb": dict(embed_dim=768, depth=12, num_heads=12, layer_idx=(2, 5, 8, 11), features=128,
                 out_channels=(96, 192, 384, 768)),
    "vitl": dict(embed_dim=1024, depth=24, num_heads=16, layer_idx=(4, 11, 17, 23), features=256,
                 out_channels=(256, 512, 1024, 1024)),
}
GOLDEN_SEEDS = {"vits": 41, "vitl": 43}


def oracle_config(name, **kw):
    from oracle import depth_ref
    return depth_ref.DepthConfig(**{**REFERENCE[name], **kw})


# ---------------------------------------------------------------------------------------------------------------
# registry
# ---------------------------------------------------------------------------------------------------------------
def test_registry_equals_reference_tables():
    from inklayer_amd import depth
    assert sorted(depth.DEPTH_CONFIGS) == sorted(REFERENCE)
    for name, want in REFERENCE.items():
        cfg = depth.config_for(name)
        assert cfg.encoder == name
        for k, v in want.items():
            assert getattr(cfg, k) == v, (name, k)
        assert (cfg.patch_size, cfg.img_size, cfg.interpolate_offset, cfg.mlp_ratio) == (14, 518, 0.1, 4)
        assert cfg.embed_dim // cfg.num_heads == 64                # the flash-attention instance the engine uses
        assert cfg is not depth.DEPTH_CONFIGS[name]                # a copy: callers may change input_size
    assert depth.config_for("vitb") == depth.DepthConfig()


def test_plugin_exposes_reference_model_table():
    from InkLayer.refinement import depth_sort
    want = {n: {"encoder": n, "features": r["features"], "out_channels": list(r["out_channels"])}
            for n, r in REFERENCE.items()}
    want["vitg"] = {"encoder": "vitg", "features": 384, "out_channels": [1536, 1536, 1536, 1536]}   # depth_sort.py:28-32
    assert depth_sort.depth_model_configs == want
    assert depth_sort.encoder == "vitb"                            # depth_sort.py:34


def test_config_from_state_dict_round_trips_and_rejects():
    from inklayer_amd import depth
    from oracle import depth_ref
    for name in REFERENCE:
        shapes = depth_ref.depth_param_shapes(oracle_config(name))
        assert depth.config_from_state_dict(shapes) == depth.config_for(name)
        tensors = {k: torch.empty(v, device="meta") for k, v in shapes.items()}
        assert depth.config_from_state_dict(tensors) == depth.config_for(name)
    vitb = depth_ref.depth_param_shapes(oracle_config("vitb"))
    vits = depth_ref.depth_param_shapes(oracle_config("vits"))
    for key in ("depth_head.scratch.layer1_rn.weight", "depth_head.projects.2.weight", "pretrained.cls_token"):
        mixed = dict(vitb)
        mixed[key] = vits[key]
        with pytest.raises(ValueError):
            depth.config_from_state_dict(mixed)
    short = {k: v for k, v in vitb.items() if not k.startswith("pretrained.blocks.11.")}
    with pytest.raises(ValueError):
        depth.config_from_state_dict(short)
    with pytest.raises(ValueError):
        depth.config_from_state_dict({"some.other.model": (1,)})


def test_vitg_and_unknown_names_are_refused():
    from inklayer_amd import depth
    with pytest.raises(NotImplementedError, match="SwiGLU"):
        depth.config_for("vitg")
    with pytest.raises(ValueError):
        depth.config_for("vith")
    with pytest.raises(NotImplementedError):
        depth.build_depth("/nonexistent/depth_anything_v2_vitg.pth", "vitg")
    with pytest.raises(ValueError):
        depth.build_depth("/nonexistent/depth_anything_v2_vitb.pth", "resnet")


def test_plugin_refuses_bad_encoder_before_any_gpu_work(monkeypatch):
    """Both branches of the plugin (checkpoint, INKLAYER_RANDOM_WEIGHTS=1): the name is checked before a checkpoint is
    looked for, a file is read or an engine is built (there is no GPU here: anything later would fail differently)."""
    from InkLayer.refinement import depth_sort
    monkeypatch.setattr(depth_sort, "_engine", None)
    monkeypatch.setattr(depth_sort, "_engine_encoder", None)
    for env in ("0", "1"):
        monkeypatch.setenv("INKLAYER_RANDOM_WEIGHTS", env)
        monkeypatch.setattr(depth_sort, "encoder", "vitg")
        with pytest.raises(NotImplementedError, match="SwiGLU"):
            depth_sort.get_depth_map_device("/nonexistent/sketch.png")
        with pytest.raises(NotImplementedError):
            depth_sort.get_depth_map("/nonexistent/sketch.png")
        monkeypatch.setattr(depth_sort, "encoder", "vitx")
        with pytest.raises(ValueError, match="vitx"):
            depth_sort.get_depth_map_device("/nonexistent/sketch.png")
    assert depth_sort._engine is None


def test_engine_interface():
    import inspect
    from inklayer_amd import depth, ops
    assert list(inspect.signature(depth.DepthEngine.infer_image).parameters) == ["self", "raw_bgr", "stages"]
    assert list(inspect.signature(depth.DepthEngine.head).parameters) == ["self", "feats16", "ph", "pw", "stages"]
    assert list(inspect.signature(depth.DepthEngine.infer_images).parameters)[:2] == ["self", "images"]
    sig = inspect.signature(ops.conv3x3)
    assert list(sig.parameters) == ["x16", "B", "H", "W", "w", "bias", "stride", "relu_in", "act", "residual", "out",
                                    "out_dtype"]
    assert sig.parameters["stride"].kind is inspect.Parameter.KEYWORD_ONLY and sig.parameters["out_dtype"].default == R.F32


# ---------------------------------------------------------------------------------------------------------------
# ViT-S channel padding
# ---------------------------------------------------------------------------------------------------------------
def test_vits_channel_padding_is_exact():
    """projects.0 -> resize_layers.0 -> layer1_rn of ViT-S (48 channels, held as 64) in float64: the engine's packed and
    zero-padded matrices (GEMM, GEMM + pixel shuffle, tap matrix + GEMM) against F.conv2d / F.conv_transpose2d /
    F.conv2d on the unpadded weights, bit for bit.  All numbers lie on a dyadic grid (inputs and intermediate maps
    multiples of 2^-6, weights of 2^-10) so that every float64 sum is exact and the summation order of either side
    cannot matter: what is compared is which terms are summed."""
    import torch.nn.functional as F
    from inklayer_amd import depth
    cfg = depth.config_for("vits")
    D, c, Fe = cfg.embed_dim, cfg.out_channels[0], cfg.features
    cp = depth.pad_channels(c)
    assert (c, cp) == (48, 64) and [depth.pad_channels(x) for x in (96, 192, 384, 256, 1024)] == [96, 192, 384, 256, 1024]
    ph, pw = 3, 4
    g = torch.Generator().manual_seed(5)
    grid = lambda t, s: (t * s).round().clamp(-8 * s + 1, 8 * s - 1) / s          # noqa: E731
    rnd = lambda *shape, sc=1.0: torch.randn(*shape, generator=g, dtype=torch.float64) * sc   # noqa: E731
    x = grid(rnd(ph * pw, D), 64)
    proj_w, proj_b = grid(rnd(c, D, 1, 1, sc=0.1), 1024), grid(rnd(c, sc=0.1), 1024)
    up_w, up_b = grid(rnd(c, c, 4, 4, sc=0.2), 1024), grid(rnd(c, sc=0.1), 1024)
    rn_w = grid(rnd(Fe, c, 3, 3, sc=0.1), 1024)
    q = lambda t: (t * 64).round() / 64                                             # noqa: E731
    # the reference's chain (DA/dpt.py:122-135), unpadded
    a = q(F.conv2d(x.t().reshape(1, D, ph, pw), proj_w, proj_b))
    a = q(F.conv_transpose2d(a, up_w, up_b, stride=4))
    want = F.conv2d(a, rn_w, None, padding=1)[0].permute(1, 2, 0).reshape(16 * ph * pw, Fe)
    # the engine's chain on the packed matrices
    pk = depth.pack_head_level(proj_w, proj_b, up_w, up_b, rn_w)
    assert tuple(pk["proj.w"].shape) == (cp, D) and tuple(pk["up.w"].shape) == (16 * cp, cp)
    assert tuple(pk["rn.w"].shape) == (Fe, 9 * cp) and tuple(pk["up.b"].shape) == (16 * cp,)
    t = q(x @ pk["proj.w"].t() + pk["proj.b"])
    assert (t[:, c:] == 0).all() and (t[:, :c] != 0).any()
    t = q(t @ pk["up.w"].t() + pk["up.b"])
    t = t.view(1, ph, pw, 4, 4, cp).permute(0, 1, 3, 2, 4, 5).reshape(16 * ph * pw, cp)
    assert (t[:, c:] == 0).all()
    case = R.Case(1, 4 * ph, 4 * pw, cp, Fe, 1, False, False, None, False, False)
    got = R.taps(t, case).reshape(-1, 9 * cp) @ pk["rn.w"].t()
    assert torch.equal(got, want) and want.abs().max() > 1
    # levels without padding are packed unchanged
    w3 = rnd(Fe, 96, 3, 3)
    pk1 = depth.pack_head_level(rnd(96, D, 1, 1), rnd(96), None, None, w3)
    assert "up.w" not in pk1 and torch.equal(pk1["rn.w"], w3.permute(0, 2, 3, 1).reshape(Fe, -1))


# ---------------------------------------------------------------------------------------------------------------
# the oracle for ViT-S and ViT-L against the reference's own modules
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["vits", "vitl"])
def test_oracle_matches_reference_golden(name):
    from oracle import depth_ref
    g = np.load(GOLD)
    assert int(g[f"{name}_seed"]) == GOLDEN_SEEDS[name]
    cfg = oracle_config(name)
    sd = depth_ref.seeded_state_dict(cfg, GOLDEN_SEEDS[name])
    x = torch.from_numpy(g["x"].astype(np.float32))
    assert tuple(x.shape) == (2, 3, 126, 154)
    st = {}
    d = depth_ref.forward(sd, cfg, x, stages=st)
    want = g[f"{name}_depth"]
    assert want.shape == (2, 126, 154) and want.max() > 0.1        # not a dead (all-ReLU'd) map
    assert np.abs(d.numpy() - want).max() < 2e-5 * max(1.0, np.abs(want).max())
    assert np.abs(want[0] - want[1]).max() > 0.1                   # two different images
    for i, (pt, cls) in enumerate(st["feats"]):
        assert np.abs(pt[:, ::7, ::16].numpy() - g[f"{name}_feat{i}"]).max() < 2e-4
        assert np.abs(cls.numpy() - g[f"{name}_cls{i}"]).max() < 2e-4


# ---------------------------------------------------------------------------------------------------------------
# the direct 3x3 convolution: reference, bound, mistakes, argument checks
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(R.CASES))
def test_conv3x3_bound_tells_mistakes_apart(name):
    c = R.CASES[name]
    d = R.conv_data(c, torch.Generator().manual_seed(900 + list(R.CASES).index(name)))
    ref, mag = R.conv_ref(c, d)
    assert tuple(ref.shape) == (R.rows(c), c.N)
    assert (ref - R.conv_ref_conv2d(c, d)).abs().max().item() <= 1e-12 * mag.max().item()
    tol = R.conv_tol(c, ref, mag)
    mistakes = R.conv_mistakes(c, d)
    assert len(mistakes) >= 2
    for what, wrong in mistakes:
        R.assert_discriminates(wrong, ref, tol, f"{name}: {what}")


def test_every_named_mistake_is_exercised():
    seen = set()
    for name, c in R.CASES.items():
        d = R.conv_data(c, torch.Generator().manual_seed(1))
        seen |= {what for what, _ in R.conv_mistakes(c, d)}
    assert seen == {"no zero padding (flat neighbours)", "batch stacked as one tall image", "ky / kx exchanged",
                    "input ReLU dropped", "input ReLU applied after the product", "last K-tile skipped",
                    "stride-2 centres on the odd pixels", "bias dropped", "residual dropped", "residual added twice"}
    shapes = {tuple(c[:6]) for c in R.CASES.values()}
    assert shapes == {(3, 1, 1, 32, 32, 1), (1, 2, 2, 64, 64, 1), (2, 5, 7, 32, 32, 1), (2, 9, 11, 96, 64, 1),
                      (2, 9, 11, 64, 64, 1), (2, 9, 11, 128, 128, 2), (1, 8, 10, 64, 32, 2), (2, 37, 37, 128, 128, 1),
                      (1, 19, 23, 256, 256, 1)}
    assert {R.bk(c) for c in R.CASES.values()} == {32, 64}


def test_conv3x3_bound_is_the_gemm_bound():
    """conv_tol is depth_ops_ref.gemm_tol at K = 9 C: on a 128 -> 128 channel case the two ResidualConvUnit forms are the
    GEMM forms 'rcu1' (ReLU, f16 out) and 'rcu2' (preloaded f32 residual, f32 out) of the im2col path."""
    assert DR.DEPTH_GEMMS["rcu1"].K == DR.DEPTH_GEMMS["rcu2"].K == 9 * 128
    c1 = R.CASES["many_tiles"]
    c2 = R.Case(1, 6, 5, 128, 128, 1, False, True, None, True, False)
    for c, form in ((c1, "rcu1"), (c2, "rcu2")):
        d = R.conv_data(c, torch.Generator().manual_seed(3))
        ref, mag = R.conv_ref(c, d)
        assert torch.equal(R.conv_tol(c, ref, mag), DR.gemm_tol(form, None, ref, None, mag))


def test_conv3x3_argument_checks_without_launch():
    """Fake non-null pointers: every one of these calls has to be refused (return 1) before any HIP call."""
    from inklayer_amd import _lib
    L = _lib.lib()
    args = dict(x=64, B=1, H=4, W=4, C=64, w=128, N=8, bias=None, stride=1, relu_in=0, act=0, res=None, out=256, f16=0)
    call = lambda **kw: L.ink_conv3x3_f16(*{**args, **kw}.values(), None)      # noqa: E731
    assert call(C=48) == 1 and call(C=16) == 1 and call(stride=3) == 1 and call(stride=0) == 1
    assert call(N=6) == 1 and call(N=0) == 1 and call(B=0) == 1 and call(H=0) == 1 and call(W=-1) == 1
    assert call(x=72) == 1 and call(w=136) == 1 and call(x=None) == 1 and call(w=None) == 1 and call(out=None) == 1
    assert call(act=1) == 1 and call(act=3) == 1 and call(relu_in=2) == 1 and call(f16=2) == 1
    assert call(B=8, H=20000, W=20000) == 1                        # B*OH*OW does not fit an int32
