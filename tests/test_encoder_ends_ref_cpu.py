"""CPU side of tests/test_encoder_ends_gpu.py and tests/test_detector_seams_gpu.py: the float64 restatements of
tests/encoder_ends_ref.py are pinned to oracle/sam_ref.py / oracle/gdino_ref.py, and every condition the GPU tests only
assume is asserted here on their own fixtures: each named mistake, evaluated in float64, lands >= 10x outside the case's
bound at every quantile where it should show (encoder_ends_ref.shows_at), and SAM's bound (8 x the float32 evaluation)
stays <= 1/16 of the error of the f16-operand evaluation, so a path fallen to f16 grade always fails."""
import pytest
import torch

import encoder_ends_ref as R
from oracle import gdino_ref as G
from oracle import sam_ref as S

F32, F64 = R.F32, R.F64


def _cap(ref, emul, bound, what):
    """SAM's cap: at every quantile the bound is <= 1/16 of the f16-operand error."""
    eq = R.quantiles((emul - ref).abs())
    print(f"  {what}: f16-operand error / bound at q{R.QUANTILES} = " + " ".join(f"{x:.0f}" for x in eq / bound))
    assert (R.SAM_CAP * bound <= eq).all(), (what, eq.tolist(), bound.tolist())


# ---------------------------------------------------------------------------------------------------------------
# SAM
# ---------------------------------------------------------------------------------------------------------------
@torch.no_grad()
def test_sam_restatements_match_oracle():
    """sam_pixels in f32 is sam_ref.preprocess bit for bit; sam_stem is image_encoder(upto=0) and sam_neck its neck, in
    float64, bit for bit, on two images (so a batch is covered)."""
    cfg, sd = R.sam_config(), R.sam_sd(F64)
    for i in (0, 1):
        img = R.sam_image(i)
        assert torch.equal(R.sam_pixels(img, cfg, F32), S.preprocess(cfg, torch.from_numpy(img).permute(2, 0, 1)))
    x = torch.stack([R.sam_pixels(R.sam_image(i), cfg, F64) for i in (0, 1)])
    stem = S.image_encoder(sd, cfg, x, upto=0)
    assert torch.equal(R.sam_stem(sd, cfg, x), stem)
    full = S.image_encoder(sd, cfg, x).permute(0, 2, 3, 1)
    assert (R.sam_neck(sd, stem) - full).abs().max().item() <= 1e-12
    for i in (0, 1):        # the per-image helpers the GPU test uses
        assert (R.sam_stem_refs(i)[0] - stem[i].reshape(4096, -1)).abs().max().item() <= 1e-12
        assert (R.sam_full_refs(i)[0] - full[i].reshape(4096, -1)).abs().max().item() <= 1e-12


@torch.no_grad()
@pytest.mark.parametrize("i", range(len(R.SAM_SIZES)))
def test_sam_stem_yardstick(i):
    """Image i of the stem cases (B = 1, 2, 8 use images 0 .. B-1): cap, and the mistakes RGB read as BGR, the pad
    normalised as (0 - mean) / std (images with a pad), pos_embed left off (images b >= 1)."""
    ref, f32 = R.sam_stem_refs(i)
    with S.f16_operands():
        emul = R.sam_stem_one(i, F64)
    bound = R.sam_bound(ref, f32)
    what = f"stem image {i} {R.SAM_SIZES[i]}"
    _cap(ref, emul, bound, what)
    R.assert_discriminates(R.sam_stem_one(i, F64, bgr=True), ref, bound, "RGB read as BGR", R.sam_pixel_share(i))
    if R.SAM_SIZES[i] != (1024, 1024):
        R.assert_discriminates(R.sam_stem_one(i, F64, pad_normalised=True), ref, bound, "pad pixels normalised",
                               R.sam_pad_share(i))
    if i >= 1:
        R.assert_discriminates(R.sam_stem_one(i, F64, no_pos=True), ref, bound, "pos_embed left off")


def test_stem_batches_reach_both_tile_families():
    """The patch-embedding GEMM (M = 4096 B, N = 1280, K' = 3 * 768) takes the 256x320 ping-pong tile (variant 45) at B = 8
    and the 128x128 family (variant 0) at B = 1 and 2: the GPU test's batch sizes cover both."""
    from inklayer_amd import _lib
    got = {B: int(_lib.lib().ink_gemm_query_variant(4096 * B, 1280, 2304)) for B in (1, 2, 5, 6, 8)}
    assert got == {1: 0, 2: 0, 5: 10, 6: 45, 8: 45}, got


def test_sam_stem_fixture_covers_both_pads():
    assert R.SAM_SIZES[0] == (1024, 768) and R.SAM_SIZES[1] == (683, 1024) and len(R.SAM_SIZES) == 8
    assert len({R.sam_image(i).tobytes() for i in range(8)}) == 8


@torch.no_grad()
@pytest.mark.parametrize("small", [False, True], ids=["a", "b"])
@pytest.mark.parametrize("i", range(8))
def test_sam_neck_yardstick(i, small):
    """Neck input (a) / (b) of image i: cap, neck.2 with ky / kx transposed, zero pad replaced by clamping (border tokens
    only: q0.99 and up); on (b) eps 1e-5 lands >= 10x outside the bound at the median and everywhere else, on (a) it
    stays inside (printed), which is why (b) exists."""
    x = R.neck_tokens(i, small)
    ref, f32 = R.sam_neck_refs(i, small)
    with S.f16_operands():
        emul = R.sam_neck_one(x, F64)
    bound = R.sam_bound(ref, f32)
    _cap(ref, emul, bound, f"neck image {i} input {'b' if small else 'a'}")
    R.assert_discriminates(R.sam_neck_one(x, F64, "neck.2 ky/kx transposed"), ref, bound, "ky/kx transposed")
    R.assert_discriminates(R.sam_neck_one(x, F64, "neck.2 border clamped"), ref, bound, "border clamped", R.NECK_BORDER_SHARE)
    wrong = R.sam_neck_one(x, F64, "eps 1e-5")
    if small:
        R.assert_discriminates(wrong, ref, bound, "eps 1e-5")
    else:
        f = R.quantiles((wrong - ref).abs()) / bound
        print("  eps 1e-5 on input (a): " + " ".join(f"{v:.2f}x" for v in f))
        assert f[0] < 1.0


@torch.no_grad()
@pytest.mark.parametrize("i", [0, 1])
def test_sam_stem_and_neck_yardstick(i):
    """encode() at B = 2 (images 0, 1): cap and every mistake of the stem and the neck through the composition."""
    ref, f32 = R.sam_full_refs(i)
    bound = R.sam_bound(ref, f32)
    with S.f16_operands():
        emul = R.sam_neck_one(R.sam_stem_one(i, F64), F64)
    _cap(ref, emul, bound, f"stem + neck image {i}")
    # the 3x3 convolution carries a stem mistake one token further: the shares of the stem are lower limits here
    for name, kw, share in (("RGB read as BGR", dict(bgr=True), R.sam_pixel_share(i)),
                            ("pad pixels normalised", dict(pad_normalised=True), R.sam_pad_share(i)),
                            ("pos_embed left off", dict(no_pos=True), 1.0)):
        if name != "pos_embed left off" or i >= 1:
            R.assert_discriminates(R.sam_neck_one(R.sam_stem_one(i, F64, **kw), F64), ref, bound, name, share)
    stem = R.sam_stem_one(i, F64)
    for m, share in zip(R.NECK_MISTAKES[:2], (1.0, R.NECK_BORDER_SHARE)):
        R.assert_discriminates(R.sam_neck_one(stem, F64, m), ref, bound, m, share)


# ---------------------------------------------------------------------------------------------------------------
# detector
# ---------------------------------------------------------------------------------------------------------------
@torch.no_grad()
def test_detector_restatements_match_oracle():
    """swin_seams is gdino_ref.swin_forward at zero depths and input_proj the conv2d + group_norm lines of
    detector_forward, in float64, bit for bit (160 x 224 and the ragged 150 x 203, B = 2); det_pixels in f32 is
    load_image's normalisation."""
    cfg, sd = R.det_config(), R.det_sd(F64)
    img = R.det_images((150, 203))
    x32 = torch.from_numpy(img[0]).permute(2, 0, 1).float() / 255.0
    want = (x32 - torch.tensor(R.PIXEL_MEAN).view(3, 1, 1)) / torch.tensor(R.PIXEL_STD).view(3, 1, 1)
    assert torch.equal(R.det_pixels(img, F32)[0], want)
    sm, pid = G.text_masks_and_position_ids(list(R.DET_IDS))
    for hw in ((160, 224), (150, 203)):
        x = R.det_pixels(R.det_images(hw), F64)
        outs, pre = R.swin_seams(sd, cfg, x)
        feats = G.swin_forward(sd, cfg, x)
        assert [tuple(o.shape[2:]) for o in outs] == R.stage_grids(hw)[1:]
        assert all(torch.equal(a, b) for a, b in zip(outs, feats))
        for j, i in enumerate(cfg.out_indices):
            assert torch.equal(G._ln(pre[j], sd, f"backbone.0.norm{i}"), R.map_tokens(outs[j]))
        st = {}
        G.detector_forward(sd, cfg, x, R.det_text().double(), sm, pid, stages=st)
        assert torch.equal(R.input_proj(sd, cfg, feats), st["src"])
        assert torch.equal(R.detector_src_refs(hw)[0], st["src"])
        assert st["src"].shape[1] == sum(a * b for a, b in R.level_shapes(hw))


def test_detector_sizes_exercise_what_they_should():
    assert R.stage_grids((300, 412)) == [(75, 103), (38, 52), (19, 26), (10, 13)] and R.level_shapes((300, 412))[-1] == (5, 7)
    assert R.stage_grids((160, 224))[-1] == (5, 7) and R.level_shapes((160, 224))[-1] == (3, 4)
    assert 150 % 4 and 203 % 4
    # level-4 taps 2 y + ky - 1: beyond the last row / column when the level-3 size is odd on that side
    assert 2 * (7 - 1) + 1 >= 13 and 2 * (5 - 1) + 1 < 10          # 300 x 412: on the right, not at the bottom
    assert 2 * (3 - 1) + 1 >= 5                                    # 160 x 224: at the bottom


def _groups(B):
    return [("all", slice(None))] + [(f"image {b}", slice(b, b + 1)) for b in range(B)]


@torch.no_grad()
@pytest.mark.parametrize("hw", R.DET_SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_backbone_seams_yardstick(hw):
    """Every output norm of the backbone case `hw`, per image: x1 / x2 swapped in the merge (every stage), odd-size merge
    padding by clamping (sizes with an odd merge), the ragged 4 x 4 patch pad normalised (150 x 203).  Held against the
    f16 output's bound, the wider of the two."""
    cfg, sd = R.det_config(), R.det_sd(F64)
    x = R.det_pixels(R.det_images(hw), F64)
    outs, _, emul = R.seam_refs(hw)
    grids = R.stage_grids(hw)
    mistakes = ["merge x1/x2 swapped"]
    if any(H % 2 or W % 2 for H, W in grids[:3]):
        mistakes.append("odd merge pad clamped")
    if hw[0] % 4 or hw[1] % 4:
        mistakes.append("ragged patch pad normalised")
    assert hw != (300, 412) or len(mistakes) == 2
    assert hw != (150, 203) or len(mistakes) == 3
    for m in mistakes:
        wrong = R.swin_seams(sd, cfg, x, m)[0]
        masks = R.reach(hw, m)
        for j, i in enumerate(cfg.out_indices):
            share = float(masks[i].double().mean())
            for name, b in _groups(R.DET_B):
                ref, em, wr = (R.map_tokens(t[j])[b] for t in (outs, emul, wrong))
                # the tokens outside the mask are untouched up to float64 rounding (a LayerNorm does not spread a change), nearly all inside
                # are changed (not the corner token of an odd x odd merge with x1 / x2 swapped: both are padding)
                same = ((wr - ref).abs() <= 1e-12).all(-1).all(0).view(masks[i].shape)
                assert same[~masks[i]].all() and (~same)[masks[i]].double().mean() > 0.99, (hw, m, i)
                R.assert_discriminates(wr, ref, R.det_bound(ref, em, f16_out=True), f"{hw} stage {i} {name}: {m}", share)


@torch.no_grad()
@pytest.mark.parametrize("hw", R.DET_SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_input_proj_yardstick(hw):
    """input_proj alone on the hand-made maps, per level and image: level 3 fed from level 2's projection, level-3 taps
    clamped, level-3 ky / kx transposed (level 3), GroupNorm statistics pooled over the batch (every level)."""
    cfg, sd = R.det_config(), R.det_sd(F64)
    maps = R.tokens_to_maps(R.proj_tokens(hw), hw, F64)
    ref, emul = R.proj_refs(hw)
    for m in R.PROJ_MISTAKES:
        wrong = R.input_proj(sd, cfg, maps, m)
        for l, (lname, rows) in enumerate(R.level_slices(hw)):
            for name, b in _groups(R.DET_B):
                r, e, w = ref[b, rows], emul[b, rows], wrong[b, rows]
                if m != "GroupNorm pooled over the batch" and l < 3:
                    assert torch.equal(w, r)
                    continue
                share = R.clamped_tap_share(hw) if m == "level-3 taps clamped" else 1.0
                R.assert_discriminates(w, r, R.det_bound(r, e), f"{hw} {lname} {name}: {m}", share)


@torch.no_grad()
def test_backbone_and_neck_yardstick():
    """backbone() then neck() on the 300 x 412 images against detector_forward's src, per level and image: every seam and
    input_proj mistake through the composition."""
    hw = (300, 412)
    cfg, sd = R.det_config(), R.det_sd(F64)
    x = R.det_pixels(R.det_images(hw), F64)
    ref, emul = R.detector_src_refs(hw)
    feats = R.seam_refs(hw)[0]
    wrongs = [(m, R.input_proj(sd, cfg, R.swin_seams(sd, cfg, x, m)[0])) for m in R.SEAM_MISTAKES[:2]]
    wrongs += [(m, R.input_proj(sd, cfg, feats, m)) for m in R.PROJ_MISTAKES]
    for m, wrong in wrongs:
        masks = R.reach(hw, m)[1:] if m in R.SEAM_MISTAKES else None
        for l, (lname, rows) in enumerate(R.level_slices(hw)):
            for name, b in _groups(R.DET_B):
                r, e, w = ref[b, rows], emul[b, rows], wrong[b, rows]
                if m in R.PROJ_MISTAKES[:3] and l < 3:
                    assert torch.equal(w, r)
                    continue
                share = (float(masks[l].double().mean()) if masks is not None else
                         R.clamped_tap_share(hw) if m == "level-3 taps clamped" else 1.0)
                R.assert_discriminates(w, r, R.det_bound(r, e), f"{hw} {lname} {name}: {m}", share)
