"""The SAM model registry (ViT-H / ViT-L / ViT-B) and the argument contract of the head_dim-64 rel-pos attention, on the
CPU: configurations are read off shape-only state dicts, and the C entry points refuse what they have no kernel for
before any launch."""
import ctypes
from dataclasses import replace

import pytest
import torch

from oracle import sam_ref

INK_ERR_ARG = 1
NAMES = ("vit_h", "vit_l", "vit_b")


def _oracle_cfg(cfg, **kw):
    """The oracle's configuration with the encoder fields of an engine configuration."""
    f = dict(embed_dim=cfg.embed_dim, depth=cfg.depth, num_heads=cfg.num_heads, global_attn_indexes=cfg.global_attn_indexes,
             window_size=cfg.window_size, img_size=cfg.img_size, patch_size=cfg.patch_size, mlp_ratio=cfg.mlp_ratio)
    f.update(kw)
    return sam_ref.SamConfig(**f)


def _meta_sd(ocfg):
    return {k: torch.empty(s, device="meta") for k, s in sam_ref.sam_param_shapes(ocfg).items()}


def test_registry_presets():
    from inklayer_amd import sam
    assert sorted(sam.SAM_CONFIGS) == sorted(NAMES)
    shape = lambda c: (c.embed_dim, c.depth, c.num_heads, c.global_attn_indexes, c.head_dim)  # noqa: E731
    assert shape(sam.config_for("vit_h")) == (1280, 32, 16, (7, 15, 23, 31), 80)
    assert shape(sam.config_for("vit_l")) == (1024, 24, 16, (5, 11, 17, 23), 64)
    assert shape(sam.config_for("vit_b")) == (768, 12, 12, (2, 5, 8, 11), 64)
    assert sam.config_for("default") == sam.config_for("vit_h") == sam.SamConfig()
    c = sam.config_for("vit_b")
    c.depth = 1                                         # a copy: the registry entry is untouched
    assert sam.config_for("vit_b").depth == 12
    with pytest.raises(ValueError, match="vit_x"):
        sam.config_for("vit_x")
    assert sorted(sam.sam_model_registry) == ["default", "vit_b", "vit_h", "vit_l"]
    assert sam.sam_model_registry["default"] is sam.build_sam_vit_h and sam.sam_model_registry["vit_h"] is sam.build_sam_vit_h
    assert sam.sam_model_registry["vit_l"] is sam.build_sam_vit_l and sam.sam_model_registry["vit_b"] is sam.build_sam_vit_b


@pytest.mark.parametrize("name", NAMES)
def test_config_from_meta_state_dict(name):
    """Shape-only (device="meta") state dicts of the three presets give back exactly the preset."""
    from inklayer_amd import sam
    want = sam.config_for(name)
    sd = _meta_sd(_oracle_cfg(want))
    assert sam.config_from_state_dict(sd) == want
    assert sam.config_from_state_dict({k: tuple(v.shape) for k, v in sd.items()}) == want     # shape tuples too
    assert sam.model_name(sam.config_from_state_dict(sd)) == name


def test_config_from_state_dict_reads_every_field():
    """A depth-4 model with global blocks (1, 3) and mlp_ratio 2 is none of the presets and is still read off exactly."""
    from inklayer_amd import sam
    want = replace(sam.config_for("vit_b"), depth=4, global_attn_indexes=(1, 3), mlp_ratio=2.0)
    got = sam.config_from_state_dict(_meta_sd(_oracle_cfg(want)))
    assert got == want and sam.model_name(got) is None


@pytest.mark.parametrize("what,kw,found", [
    ("head dim 48", dict(embed_dim=576, num_heads=12), "head dim 48"),
    ("grid 32", dict(img_size=512), "32 x 32 grid"),
    ("window 7", dict(window_size=7), r"window sizes \[7\]"),
])
def test_unserved_encoders_are_refused(what, kw, found):
    """Head dim 48, a 32 x 32 grid and 7 x 7 windows have no kernels: ValueError naming what the state dict holds."""
    from inklayer_amd import sam
    ocfg = _oracle_cfg(replace(sam.config_for("vit_b"), depth=4, global_attn_indexes=(1, 3)), **kw)
    with pytest.raises(ValueError, match=found):
        sam.config_from_state_dict(_meta_sd(ocfg))


def test_not_a_sam_state_dict():
    from inklayer_amd import sam
    with pytest.raises(ValueError, match="pos_embed is missing"):
        sam.config_from_state_dict({"pretrained.cls_token": (1, 1, 384)})


def test_model_type_mismatch_raises():
    """build_sam reads the model off the state dict; a model_type that names another one is refused (before any engine is
    built: this runs without a GPU), with depth.build_depth's wording."""
    from inklayer_amd import sam
    sd = _meta_sd(_oracle_cfg(sam.config_for("vit_b")))
    with pytest.raises(ValueError, match="holds a SAM vit_b model, not the 'vit_h' asked for"):
        sam.build_sam(state_dict=sd, model_type="vit_h")
    with pytest.raises(ValueError, match="holds a SAM vit_b model, not the 'default' asked for"):
        sam.build_sam(state_dict=sd, model_type="default")
    with pytest.raises(ValueError, match="unknown SAM model"):
        sam.build_sam(state_dict=sd, model_type="vit_g")


def _attn(l, **kw):
    """ink_flash_attn on a well-formed 64 x 64-grid global call with fake non-null pointers, fields overridden by kw."""
    from inklayer_amd import _lib
    p = _lib.InkAttn()
    p.Q = p.K = p.V = p.O = 16
    p.ldq = p.ldk = p.ldv = 3 * 192
    p.ldo = 192
    p.n_batch, p.n_heads, p.n_q, p.n_k, p.head_dim = 1, 3, 4096, 4096, 64
    p.scale, p.bias_mode, p.grid_w = 0.125, 1, 64
    p.rel_h = p.rel_w = 16
    for k, v in kw.items():
        setattr(p, k, v)
    return l.ink_flash_attn(ctypes.byref(p), None)


def test_head_dim_64_argument_contract():
    """Refused before any launch: f16 rel tables at head_dim 64 (a head_dim-80 feature), head_dim 48 with rel tables,
    and the shapes the global form cannot index (grid_w != 64, n_k no multiple of 64, n_k > 4096, missing tables);
    the window form without rel_aug, with a grid wider than 16, or tok_rows without pad rows; ink_relpos_bias at
    head_dim 48, and ink_relpos_bias64_f16 at head_dim 64."""
    from inklayer_amd import _lib
    l = _lib.lib()
    assert _attn(l, rel_f16=1) == INK_ERR_ARG
    assert _attn(l, head_dim=48) == INK_ERR_ARG and _attn(l, head_dim=48, bias_mode=2, rel_aug=16, grid_w=14) == INK_ERR_ARG
    assert _attn(l, grid_w=32) == INK_ERR_ARG and _attn(l, n_k=4000) == INK_ERR_ARG and _attn(l, n_k=8192) == INK_ERR_ARG
    assert _attn(l, rel_h=None) == INK_ERR_ARG and _attn(l, rel_w=None) == INK_ERR_ARG
    win = dict(bias_mode=2, n_q=196, n_k=196, grid_w=14, rel_aug=16)
    assert _attn(l, **{**win, "rel_aug": None}) == INK_ERR_ARG
    assert _attn(l, **{**win, "grid_w": 17, "n_q": 289, "n_k": 289}) == INK_ERR_ARG
    assert _attn(l, **{**win, "n_k": 200}) == INK_ERR_ARG                      # more keys than the 14 x 14 grid has
    assert _attn(l, **win, tok_rows=16) == INK_ERR_ARG                          # tok_rows without pad_k / pad_v
    assert _attn(l, **win, tok_rows=16, pad_k=16, pad_v=8) == INK_ERR_ARG      # pad rows must be 16-byte aligned
    rel = lambda hd, S, aug: l.ink_relpos_bias(16, 576, 16, 16, S, 1, 3, hd, 0.125, None,  # noqa: E731
                                               None if aug else 16, None if aug else 16, 16 if aug else None, None)
    assert rel(48, 14, True) == INK_ERR_ARG and rel(48, 64, False) == INK_ERR_ARG
    assert rel(64, 16, True) == INK_ERR_ARG                                     # windows: S = 14 only
    assert l.ink_relpos_bias64_f16(16, 576, 16, 16, 1, 3, 64, 0.125, 16, 16, None) == INK_ERR_ARG
