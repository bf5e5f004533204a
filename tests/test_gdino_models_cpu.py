"""CPU half of the GroundingDINO Swin-B work (tests/test_swin_attn_gpu.py and tests/test_gdino_models_gpu.py run the
kernels): the model registry and reading a model off a checkpoint's shapes, the compact region ids and bias table
against the oracle's dense mask and relative_position_index, the argument contract of ink_swin_attn, the float64
yardstick of the kernel test, the plugin's config-file cross-check and model selection, and the oracle at Swin-B's true
depths against the reference's own backbone (tests/golden/gdino_swinb_small.npz)."""
import importlib
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import swin_attn_ref as R

GOLD = Path(__file__).parent / "golden" / "gdino_swinb_small.npz"
INK_ERR_ARG = 1
NAMES = ("swin_T_224_1k", "swin_B_224_22k", "swin_B_384_22k")


# ------------------------------------------------------------------------------------------------ registry, config
def test_registry_names_and_aliases():
    from inklayer_amd import gdino
    assert tuple(gdino.GDINO_CONFIGS) == NAMES
    assert gdino.config_for("swin_t") == gdino.GDinoConfig() == gdino.config_for("swin_T_224_1k")
    b = gdino.config_for("swin_b")
    assert b == gdino.config_for("swin_B_384_22k")
    assert (b.embed_dim, b.depths, b.num_heads, b.window_size) == (128, (2, 2, 18, 2), (4, 8, 16, 32), 12)
    b7 = gdino.config_for("swin_B_224_22k")
    assert (b7.embed_dim, b7.depths, b7.num_heads, b7.window_size) == (128, (2, 2, 18, 2), (4, 8, 16, 32), 7)
    assert gdino.config_for("swin_b") is not gdino.GDINO_CONFIGS["swin_B_384_22k"]      # a copy
    assert [gdino.model_name(gdino.config_for(n)) for n in NAMES] == list(NAMES)
    with pytest.raises(ValueError, match="unknown GroundingDINO model 'swin_L_384_22k'"):
        gdino.config_for("swin_L_384_22k")


@pytest.mark.parametrize("name", NAMES)
def test_config_from_state_dict_round_trips(name):
    """Shape tuples and meta tensors alike; a DataParallel prefix is stripped; the shapes of the config read back are
    the shapes it was read from."""
    from inklayer_amd import gdino, weights_init
    cfg = gdino.config_for(name)
    shapes = weights_init.gdino_param_shapes(cfg)
    assert gdino.config_from_state_dict(shapes) == cfg
    meta = {"module." + k: torch.empty(s, device="meta") for k, s in shapes.items()}
    got = gdino.config_from_state_dict(meta)
    assert got == cfg and weights_init.gdino_param_shapes(got) == shapes


def test_config_from_state_dict_reads_the_transformer():
    from inklayer_amd import gdino, weights_init
    cfg = gdino.GDinoConfig(embed_dim=128, depths=(2, 2, 2, 2), num_heads=(4, 8, 16, 32), window_size=12, enc_layers=2,
                            dec_layers=3, num_queries=300, dim_feedforward=1024)
    assert gdino.config_from_state_dict(weights_init.gdino_param_shapes(cfg)) == cfg


def _shapes(**kw):
    from inklayer_amd import gdino, weights_init
    return weights_init.gdino_param_shapes(gdino.GDinoConfig(**kw))


@pytest.mark.parametrize("what,kw,found", [
    ("head width 48", dict(embed_dim=144), r"head widths \[48\.0, 48\.0, 48\.0, 48\.0\]"),
    ("head width 64 in stage 3", dict(num_heads=(3, 6, 12, 12)), r"head widths \[32\.0, 32\.0, 32\.0, 64\.0\]"),
    ("window 8", dict(window_size=8), "window size 8"),
    ("window 14", dict(embed_dim=128, num_heads=(4, 8, 16, 32), window_size=14), "window size 14"),
    ("hidden_dim 384", dict(hidden_dim=384), "hidden_dim 384"),
    ("5 levels", dict(num_feature_levels=5), "num_feature_levels 5"),
    ("16 deformable heads", dict(nheads=16), r"sampling_offsets.weight has shape \(512, 256\)"),
])
def test_unserved_models_are_refused(what, kw, found):
    """ValueError naming what was found - from shapes alone, so before any device allocation (this runs without a GPU):
    head width != 32, a window size without a kernel, and the transformer shapes the constructor used to assert."""
    from inklayer_amd import gdino
    with pytest.raises(ValueError, match=found):
        gdino.config_from_state_dict(_shapes(**kw))


def test_engine_constructor_refuses_with_value_error():
    """GDinoEngine refuses an unserved config with the same ValueError, not a bare assertion (a CUDA device name, no
    GPU: the check comes before any allocation)."""
    from inklayer_amd import gdino
    with pytest.raises(ValueError, match="window size 8"):
        gdino.GDinoEngine({}, gdino.GDinoConfig(window_size=8), "cuda", encoded_text=torch.zeros(4, 256))
    with pytest.raises(ValueError, match="hidden_dim 128"):
        gdino.GDinoEngine({}, gdino.GDinoConfig(hidden_dim=128), "cuda", encoded_text=torch.zeros(4, 256))


def test_not_a_gdino_state_dict():
    from inklayer_amd import gdino
    with pytest.raises(ValueError, match="patch_embed.proj.weight is missing"):
        gdino.config_from_state_dict({"image_encoder.pos_embed": (1, 64, 64, 768)})
    sd = _shapes()
    sd["backbone.0.layers.2.blocks.3.attn.relative_position_bias_table"] = (529, 12)
    with pytest.raises(ValueError, match=r"inconsistent Swin backbone.*\(529, 12\)"):
        gdino.config_from_state_dict(sd)


# ------------------------------------------------------------------------------------------------ regions and bias
@pytest.mark.parametrize("hw", [(100, 148), (300, 412)])
def test_region_ids_reproduce_the_dense_mask(hw):
    """(region[w][:, None] != region[w][None, :]) * -100 == gdino_ref.swin_shift_mask(Hp, Wp, 12)[w] for every window of
    every stage.  At 100 x 148 the stage grids are 3x4, 2x2, 1x1 and 1x1 windows (stages 2 and 3: Hp == ws, a single
    window that is mostly padding).  The ws = 12 plan holds no dense mask."""
    from oracle import gdino_ref
    pl = R.plan(hw[0], hw[1], 2, 12)
    assert pl.shift_mask == [] and len(pl.region) == 4
    grids = []
    for i, (H, W) in enumerate(pl.stage_hw):
        Hp, Wp = -(-H // 12) * 12, -(-W // 12) * 12
        grids.append((Hp // 12, Wp // 12))
        reg = pl.region[i]
        assert reg.dtype == torch.uint8 and tuple(reg.shape) == (pl.nW[i], 144) and reg.is_contiguous() and int(reg.max()) <= 8
        dense = (reg[:, :, None] != reg[:, None, :]).float() * -100.0
        assert torch.equal(dense, gdino_ref.swin_shift_mask(Hp, Wp, 12))
    if hw == (100, 148):
        assert grids == [(3, 4), (2, 2), (1, 1), (1, 1)]
        assert int((pl.win_map[2][0][:144] < 0).sum()) > 72        # mostly padding


def test_swin_t_plan_is_unchanged():
    """window_size 7: the dense [nW, 49, 64] masks as before, no region ids."""
    from oracle import gdino_ref
    pl = R.plan(300, 412, 1, 7)
    assert pl.region == [] and len(pl.shift_mask) == 4
    H, W = pl.stage_hw[0]
    Hp, Wp = -(-H // 7) * 7, -(-W // 7) * 7
    assert tuple(pl.shift_mask[0].shape) == (pl.nW[0], 49, 64)
    assert torch.equal(pl.shift_mask[0][:, :, :49], gdino_ref.swin_shift_mask(Hp, Wp, 7) / R.SCALE)


@pytest.mark.parametrize("ws", [7, 12])
def test_bias_table_through_the_kernels_index_formula(ws):
    """table.T[h][(qy - ky + ws - 1) (2 ws - 1) + (qx - kx + ws - 1)] == table[relative_position_index][q, k, h]."""
    from oracle import gdino_ref
    from inklayer_amd import gdino
    nh, N = 4, ws * ws
    table = torch.randn((2 * ws - 1) ** 2, nh, generator=torch.Generator().manual_seed(ws))
    t = gdino.swin_bias_table(table, ws, nh)
    assert t.dtype == torch.float32 and tuple(t.shape) == (nh, (2 * ws - 1) ** 2) and t.is_contiguous()
    i = torch.arange(N)
    qy, qx, ky, kx = (i // ws)[:, None], (i % ws)[:, None], (i // ws)[None, :], (i % ws)[None, :]
    rel = (qy - ky + ws - 1) * (2 * ws - 1) + (qx - kx + ws - 1)
    assert torch.equal(rel, gdino_ref.swin_rel_index(ws))
    want = table[gdino_ref.swin_rel_index(ws).view(-1)].view(N, N, nh).permute(2, 0, 1)
    assert torch.equal(t[:, rel], want)


# ------------------------------------------------------------------------------------------------ argument contract
def _swin(**kw):
    """ink_swin_attn on a well-formed shifted ws = 12 call with fake, aligned, non-null pointers; arguments from kw."""
    from inklayer_amd import _lib
    a = dict(Q=4096, K=4096, V=4096, ldq=392, ldk=392, ldv=392, O=4096, ldo=128, n_windows=24, n_heads=4, ws=12,
             scale=32 ** -0.5, table=4096, region=4096, nW=12)
    assert set(kw) <= set(a)
    return _lib.lib().ink_swin_attn(*{**a, **kw}.values(), None)


def test_swin_attn_argument_contract():
    """Every refusal the header lists returns 1 before any launch (fake pointers: none of these calls may be accepted),
    and so does every window size the kernel does not serve."""
    from inklayer_amd import ops
    for name in ("Q", "K", "V", "O", "table"):
        assert _swin(**{name: None}) == INK_ERR_ARG, name
    for name in ("ldq", "ldk", "ldv", "ldo"):
        assert _swin(**{name: 132}) == INK_ERR_ARG, name                    # % 8 != 0
        assert _swin(**{name: 120}) == INK_ERR_ARG, name                    # below n_heads * 32
    for name in ("Q", "K", "V"):
        assert _swin(**{name: 4104}) == INK_ERR_ARG, name                   # 8-byte aligned only
    assert _swin(O=4100) == INK_ERR_ARG
    assert _swin(nW=0) == INK_ERR_ARG and _swin(nW=-1) == INK_ERR_ARG        # region with nW <= 0
    assert _swin(nW=5) == INK_ERR_ARG and _swin(region=None, nW=5) == INK_ERR_ARG      # n_windows % nW != 0
    assert _swin(n_windows=0) == INK_ERR_ARG and _swin(n_heads=0) == INK_ERR_ARG and _swin(scale=0.0) == INK_ERR_ARG
    assert ops.SWIN_ATTN_WINDOWS == (7, 12)
    for ws in range(-1, 40):
        if ws not in ops.SWIN_ATTN_WINDOWS:
            assert _swin(ws=ws) == INK_ERR_ARG, ws


def test_swin_attn_wrapper_refuses_before_native_code():
    from inklayer_amd import ops
    x = torch.zeros(144, 128, dtype=torch.float16)
    with pytest.raises(AssertionError, match="window sizes"):
        ops.swin_attn(x, x, x, n_windows=1, n_heads=4, ws=8, scale=0.1, bias_table=torch.zeros(4, 225))
    with pytest.raises(AssertionError):                                        # CPU tensors
        ops.swin_attn(x, x, x, n_windows=1, n_heads=4, ws=12, scale=0.1, bias_table=torch.zeros(4, 529))


# ------------------------------------------------------------------------------------------------ the yardstick
@pytest.mark.parametrize("ws,hw,stage", [(12, (100, 148), 2), (12, (100, 148), 0), (7, (100, 148), 1)])
def test_kernel_yardstick_discriminates(ws, hw, stage):
    """The float64 reference of tests/test_swin_attn_gpu.py rounded to f16 (the least any kernel does) is inside the
    bound, and each named mistake lands >= 100x outside it."""
    c = R.case(hw, stage, 1, ws)
    assert ((c.o.half().double() - c.o).abs() <= c.tol).all()
    assert set(c.wrongs) >= {"bias transposed to [h, k, q]", "bias of head h + 1", "mask omitted"}
    for what, wrong in c.wrongs.items():
        assert ((wrong - c.o).abs() / c.tol).max().item() >= 100, what


# ------------------------------------------------------------------------------------------------ plugin
@pytest.fixture
def plugin(monkeypatch, tmp_path):
    """InkLayer.detector.gdino with GDinoEngine replaced by a recorder and a shapes-only Swin-B/384 'checkpoint'."""
    from inklayer_amd import gdino, text_branch, weights_init
    mod = importlib.import_module("InkLayer.detector.gdino")
    built = []

    class Engine:
        def __init__(self, sd, cfg, device, encoded_text=None):
            built.append(cfg)
            self.cfg = cfg

    monkeypatch.setattr(gdino, "GDinoEngine", Engine)
    monkeypatch.setattr(text_branch, "encode_caption_from_checkpoint", lambda sd, ids: torch.zeros(4, 256))
    monkeypatch.setattr(weights_init, "random_gdino_state_dict", lambda cfg, device: {})
    monkeypatch.setattr(weights_init, "random_text_features", lambda cfg, device: torch.zeros(4, 256))
    monkeypatch.delenv("INKLAYER_RANDOM_WEIGHTS", raising=False)
    monkeypatch.delenv("INKLAYER_GDINO_MODEL", raising=False)
    shapes = weights_init.gdino_param_shapes(gdino.GDinoConfig(embed_dim=128, depths=(2, 2, 18, 2), num_heads=(4, 8, 16, 32),
                                                               window_size=12, enc_layers=1, dec_layers=1))
    sd = {k: torch.zeros(s, dtype=torch.float16) for k, s in shapes.items()
          if "mlp." not in k and "qkv" not in k and "attn.proj" not in k}        # what the config reader needs, small
    ckpt = tmp_path / "swinb.pth"
    torch.save({"model": {"module." + k: v for k, v in sd.items()}}, ckpt)
    return SimpleNamespace(mod=mod, built=built, ckpt=str(ckpt), tmp=tmp_path)


def test_plugin_reads_the_model_off_the_checkpoint(plugin):
    eng = plugin.mod.load_model(config_path=str(plugin.tmp / "absent.py"), checkpoint_path=plugin.ckpt)
    assert (eng.cfg.embed_dim, eng.cfg.depths, eng.cfg.window_size) == (128, (2, 2, 18, 2), 12)


def test_plugin_cross_checks_the_config_file_as_text(plugin):
    """The config file is parsed for its backbone line and never executed: the file below would raise if it were."""
    good = plugin.tmp / "GroundingDINO_SwinB_cfg.py"
    good.write_text('batch_size = 1\nmodelname = "groundingdino"\nbackbone = "swin_B_384_22k"\nraise SystemExit("executed")\n')
    assert plugin.mod.backbone_of_config(str(good)) == "swin_B_384_22k"
    assert plugin.mod.load_model(config_path=str(good), checkpoint_path=plugin.ckpt).cfg.window_size == 12
    bad = plugin.tmp / "GroundingDINO_SwinT_OGC.py"
    bad.write_text("backbone = 'swin_T_224_1k'\nraise SystemExit('executed')\n")
    n = len(plugin.built)
    with pytest.raises(ValueError, match="names backbone 'swin_T_224_1k', but .* holds swin_B_384_22k"):
        plugin.mod.load_model(config_path=str(bad), checkpoint_path=plugin.ckpt)
    assert len(plugin.built) == n                                   # refused before an engine was built
    nob = plugin.tmp / "no_backbone.py"
    nob.write_text("position_embedding = 'sine'\n")
    assert plugin.mod.backbone_of_config(str(nob)) is None
    assert plugin.mod.load_model(config_path=str(nob), checkpoint_path=plugin.ckpt).cfg.window_size == 12


def test_plugin_random_weights_model_names(plugin, monkeypatch):
    monkeypatch.setenv("INKLAYER_RANDOM_WEIGHTS", "1")
    assert plugin.mod.load_model().cfg.window_size == 7                       # default: swin_t
    monkeypatch.setenv("INKLAYER_GDINO_MODEL", "swin_b")
    cfg = plugin.mod.load_model().cfg
    assert (cfg.embed_dim, cfg.depths, cfg.window_size) == (128, (2, 2, 18, 2), 12)
    monkeypatch.setenv("INKLAYER_GDINO_MODEL", "swin_B_224_22k")
    assert plugin.mod.load_model().cfg.window_size == 7 and plugin.built[-1].embed_dim == 128
    n = len(plugin.built)
    monkeypatch.setenv("INKLAYER_GDINO_MODEL", "swin_l")
    with pytest.raises(ValueError, match="unknown GroundingDINO model 'swin_l'"):
        plugin.mod.load_model()
    assert len(plugin.built) == n


# ------------------------------------------------------------------------------------------------ oracle at true depths
@torch.no_grad()
def test_oracle_swin_b_matches_reference_golden():
    """oracle/gdino_ref.swin_forward with Swin-B/384's config at its true depths (2, 2, 18, 2) reproduces the feature
    maps of the reference's build_swin_transformer("swin_B_384_22k", 384, ...) on a seeded 100 x 148 image
    (tests/golden/make_gdino_swinb_golden.py), to the tolerance tests/test_oracle_gdino.py applies to feat1 / feat3."""
    from oracle import gdino_ref, sam_ref
    g = np.load(GOLD)
    cfg = gdino_ref.GDinoConfig(embed_dim=128, depths=(2, 2, 18, 2), num_heads=(4, 8, 16, 32), window_size=12)
    shapes = {k: s for k, s in gdino_ref.gdino_param_shapes(cfg).items() if k.startswith("backbone.0.")}
    sd = sam_ref.seeded_state_dict(shapes, int(g["seed"]))
    h, w = (int(v) for v in g["hw"])
    img = torch.from_numpy(np.random.RandomState(int(g["image_seed"])).standard_normal((1, 3, h, w)).astype(np.float32))
    feats = gdino_ref.swin_forward(sd, cfg, img)
    for f, name, step in zip(feats, ("feat1", "feat2", "feat3"), (8, 8, 16)):
        a, b = f[0, ::step].double().numpy(), g[name].astype(np.float64)
        assert a.shape == b.shape, (name, a.shape, b.shape)
        err = np.abs(a - b).max()
        assert err <= 2e-5 * max(1.0, np.abs(b).max()), (name, err)
