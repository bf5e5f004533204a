"""float64 parity of the detector's code between its layers, on a GDinoEngine with Swin depths (0, 0, 0, 0): backbone() is
then exactly the stem (swin_patchify, the GEMM against the zero-padded pe.w, LayerNorm), per stage the dual-output
s{i}.outnorm and the merge (layernorm_merge4 through pl.merge_map + the bias-free GEMM); neck() is input_proj (1x1 GEMMs
on the f16 copies, the 3x3 / stride 2 / pad 1 level from pl.lvl4_map + gather_rows, GroupNorm at a batch stride into the
flattened source).  References, fixtures and the yardstick are in tests/encoder_ends_ref.py: at every error quantile, the
maximum included, HIP <= 2 x the float64 reference under gdino_ref.f16_operands() (+ 2^-11 max|ref| for an f16 output);
the f32 output norm on given tokens, which involves no rounded product, <= 8 x its float32 evaluation.  Every level / stage
is held on its own, over the batch and per image.  tests/test_encoder_ends_ref_cpu.py shows on the CPU that the named
mistakes land >= 10x outside these bounds.  B = 2; 300 x 412 (grids 75x103, 38x52, 19x26, 10x13, level 4 5x7: three odd
merges, level-4 taps beyond the right edge), 160 x 224 (down to 5x7 and 3x4: taps beyond the bottom edge), 150 x 203
(ragged 4x4 patches on both sides).  GPU box only."""
import pytest
import torch

import encoder_ends_ref as R

pytestmark = pytest.mark.gpu

F16, F32 = torch.float16, torch.float32
B = R.DET_B
SIZES = pytest.mark.parametrize("hw", R.DET_SIZES, ids=lambda s: f"{s[0]}x{s[1]}")


@pytest.fixture(scope="module")
def eng(dev):
    from inklayer_amd import gdino
    cfg = gdino.GDinoConfig(depths=(0, 0, 0, 0), enc_layers=1, dec_layers=1, num_queries=100)
    return gdino.GDinoEngine(R.det_sd(), cfg, dev, encoded_text=R.det_text(), token_ids=R.DET_IDS)


def _images(dev, hw):
    return [torch.from_numpy(x).to(dev) for x in R.det_images(hw)]


def _groups():
    return [("", slice(None))] + [(f" image {b}", slice(b, b + 1)) for b in range(B)]


def _hold(got, ref, emul, what, f16_out=False):
    """got [B, N, C] against float64 ref / emulated-f16, over the batch and per image; -> the worst ratio."""
    got = got.double().cpu()
    return max(float(R.assert_within(got[b], ref[b], R.det_bound(ref[b], emul[b], f16_out), what + name).max())
               for name, b in _groups())


@torch.no_grad()
@SIZES
def test_backbone_seams_match_float64(dev, eng, hw):
    """backbone(imgs, pl): the f32 and the f16 output of every outnorm against swin_forward's maps, and the f16 output
    equal to the f32 one rounded to f16, bit for bit.  Measured on an MI355X, HIP error / bound: the f32 outputs 0.494 -
    0.507 at every quantile, stage, size and image (the HIP error is the emulated-f16 error: same operand roundings, f32
    accumulation; medians 2.6e-4 / 3.3e-4 / 3.7e-4 at stages 1 / 2 / 3 over the batch); the f16 outputs 0.09 - 0.15 at the median
    rising to 0.33 - 0.47 at the maximum (the absolute term of the output's own rounding dominates the bound below the tail)."""
    pl = eng.plan(hw[0], hw[1], B)
    assert [tuple(s) for s in pl.stage_hw] == R.stage_grids(hw)
    feats = eng.backbone(_images(dev, hw), pl)
    outs, _, emul = R.seam_refs(hw)
    assert sorted(feats) == [1, 2, 3]
    worst = 0.0
    for j, i in enumerate((1, 2, 3)):
        o32, o16 = feats[i]
        H, W = pl.stage_hw[i]
        C = 96 * 2 ** i
        assert o32.dtype == F32 and o16.dtype == F16 and tuple(o32.shape) == tuple(o16.shape) == (B * H * W, C)
        assert torch.equal(o16, o32.half()), f"stage {i}: the f16 output is not the f32 output rounded"
        ref, em = R.map_tokens(outs[j]), R.map_tokens(emul[j])
        worst = max(worst, _hold(o32.view(B, H * W, C), ref, em, f"{hw} outnorm {i} f32"),
                    _hold(o16.view(B, H * W, C), ref, em, f"{hw} outnorm {i} f16", f16_out=True))
    print(f"backbone seams {hw}: worst HIP / bound ratio {worst:.3f}")


@torch.no_grad()
@SIZES
def test_outnorm_alone_matches_float64(dev, eng, hw):
    """The dual-output layernorm_rows as backbone() calls it, on the reference's own pre-norm tokens (rounded to f32):
    no rounded product is involved, so the f32 output is held to 8 x the float32 evaluation of the same LayerNorm, and
    the f16 output is the f32 one rounded, bit for bit.  Measured on an MI355X, HIP error / bound: 0.10 - 0.154 over all
    quantiles, stages and sizes (HIP median 2.5e-8, the float32 evaluation's own error)."""
    from inklayer_amd import ops
    worst = 0.0
    for j, i in enumerate((1, 2, 3)):
        x32, ref, f32 = R.outnorm_refs(hw, j)
        x = x32.to(dev)
        o32 = torch.full_like(x, float("nan"))
        o16 = torch.full(x.shape, float("nan"), device=dev, dtype=F16)
        ops.layernorm_rows(x, eng.w[f"s{i}.outnorm.w"], eng.w[f"s{i}.outnorm.b"], 1e-5, out=o32, out2=o16)
        assert torch.equal(o16, o32.half())
        worst = max(worst, float(R.assert_within(o32, ref, R.f32_bound(ref, f32), f"{hw} outnorm {i} alone").max()))
    print(f"outnorm alone {hw}: worst HIP / bound ratio {worst:.3f}")


def _feats(dev, tok):
    """{stage: (f32 [B*H*W, C], the same rounded to f16)} on the GPU, as backbone() returns them."""
    out = {}
    for i, t in tok.items():
        f = t.reshape(-1, t.shape[-1]).to(dev).contiguous()
        out[i] = (f, f.half())
    return out


@torch.no_grad()
@SIZES
def test_input_proj_matches_float64(dev, eng, hw):
    """neck() on hand-made feature tokens (per-image scale and per-channel offsets; the f16 entry is the f32 one rounded)
    against the conv2d + group_norm lines of detector_forward: all four levels at their level_start offsets, over the
    batch and per image.  Image 0's features replaced: image 1's rows are bit-equal (the GroupNorm statistics are per
    image), image 0's are not.  Measured on an MI355X, HIP error / bound: 0.499 - 0.501 at every quantile, level, size and
    image (HIP median 1.8 - 2.1e-4 = the emulated-f16 error)."""
    pl = eng.plan(hw[0], hw[1], B)
    ref, emul = R.proj_refs(hw)
    assert [tuple(s) for s in pl.shapes] == R.level_shapes(hw) and pl.S == ref.shape[1]
    assert pl.level_start == [r.start for _, r in R.level_slices(hw)]
    src = eng.neck(_feats(dev, R.proj_tokens(hw)), pl, B)
    assert tuple(src.shape) == (B * pl.S, 256) and src.dtype == F32
    got = src.view(B, pl.S, 256)
    worst = max(_hold(got[:, rows], ref[:, rows], emul[:, rows], f"{hw} input_proj {name}")
                for name, rows in R.level_slices(hw))
    print(f"input_proj {hw}: worst HIP / bound ratio {worst:.3f}")
    other = {i: torch.cat([3 * t[:1] + 1, t[1:]]) for i, t in R.proj_tokens(hw, seed=1).items()}
    for i, t in R.proj_tokens(hw).items():
        other[i][1] = t[1]
    got2 = eng.neck(_feats(dev, other), pl, B).view(B, pl.S, 256)
    assert torch.equal(got2[1], got[1]), "image 1's rows depend on image 0's features"
    for _, rows in R.level_slices(hw):
        assert not torch.equal(got2[0, rows], got[0, rows])


@torch.no_grad()
def test_backbone_and_neck_match_float64(dev, eng):
    """backbone() followed by neck() on the 300 x 412 images against detector_forward(..., stages=...)["src"].  Measured on
    an MI355X, HIP error / bound: 0.48 - 0.53 over all quantiles, levels and images (HIP medians 3.3e-4 / 3.9e-4 / 4.3e-4 /
    4.0e-4 at levels 0 - 3)."""
    hw = (300, 412)
    pl = eng.plan(hw[0], hw[1], B)
    src = eng.neck(eng.backbone(_images(dev, hw), pl), pl, B).view(B, pl.S, 256)
    ref, emul = R.detector_src_refs(hw)
    worst = max(_hold(src[:, rows], ref[:, rows], emul[:, rows], f"{hw} src {name}") for name, rows in R.level_slices(hw))
    print(f"backbone + neck {hw}: worst HIP / bound ratio {worst:.3f}")
