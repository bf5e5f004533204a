"""float64 parity of the SAM encoder's two ends as SamEngine composes them, on a depth-0 engine: the patch embedding
(sam_patchify(split=True) + one split-f16 GEMM for the batch with the tiled pos_rep residual) and the neck (add_split_f16,
1x1 GEMM, layernorm_rows(split=True), im2col3x3 on the 3E-wide split rows, the GEMM against the per-tap-split neck2.ws,
layernorm_rows).  References, fixtures and the yardstick are in tests/encoder_ends_ref.py: at every error quantile, the
maximum included, HIP <= 8 x the error of the same float64 restatement evaluated in float32 on the CPU (8 = 2^-21 / 2^-24,
the header's accuracy of a split product over f32's); every image is held against its own reference.
tests/test_encoder_ends_ref_cpu.py shows on the CPU that this bound sits >= 16x below f16-operand grade and that the named
mistakes (BGR, normalised pad, pos_embed left off, ky / kx transposed, clamped border, eps 1e-5) land >= 10x outside it.
GPU box only."""
import numpy as np
import pytest
import torch

import encoder_ends_ref as R

pytestmark = pytest.mark.gpu

T, D, E = 4096, 1280, 256
_ENGINES = {}


def _engine(dev, max_batch):
    """The depth-0 engine (seed 11, bias_correction off: the reference has the checkpoint's biases), one per max_batch."""
    from inklayer_amd import sam
    if max_batch not in _ENGINES:
        _ENGINES[max_batch] = sam.SamEngine(R.sam_sd(), sam.SamConfig(depth=0, global_attn_indexes=()), dev,
                                            max_batch=max_batch, bias_correction=False)
    return _ENGINES[max_batch]


def _images(dev, B):
    return [torch.from_numpy(R.sam_image(i)).to(dev) for i in range(B)]


def _hold(got, refs, what):
    """got [B, T, C] against per-image (float64, float32) references; returns the worst ratio per quantile."""
    worst = np.zeros(len(R.QUANTILES))
    for b, (ref, f32) in enumerate(refs):
        worst = np.maximum(worst, R.assert_within(got[b], ref, R.sam_bound(ref, f32), f"{what} image {b}"))
    print(f"{what}: worst HIP / bound per quantile " + " ".join(f"{x:.3f}" for x in worst))
    return worst


@torch.no_grad()
@pytest.mark.parametrize("B,max_batch", [(1, 1), (2, 2), (8, 8), (2, 8)], ids=["B1", "B2", "B8", "B2-of-8"])
def test_stem_matches_float64(dev, B, max_batch):
    """encode(imgs, upto=0) on images 0 .. B-1 of the fixture (1024 x 768: pad on the right; 683 x 1024: pad at the
    bottom, ending inside a patch row; six more sizes at B = 8).  B = 8 takes the 256x320 ping-pong GEMM (variant 45),
    B <= 2 the 128x128 family (variant 0); B = 2 on the max_batch = 8 engine reads the [:B*T] slices of buf_patches and
    pos_rep.  Every image within 8 x its own float32 evaluation, and bit-equal to the same image in another batch.
    Measured on an MI355X, HIP error / bound at q0.5 / 0.9 / 0.99 / 0.999 / 1.0, worst image: B = 1, B = 2 and B = 2 of 8
    0.098 / 0.106 / 0.114 / 0.114 / 0.129, B = 8 (variant 45) 0.125 / 0.108 / 0.114 / 0.114 / 0.133 - the split-f16 stem is
    0.8 - 1.1 x the float32 evaluation's own error (median 1.5e-7 on outputs of O(1)), under either tile family."""
    from inklayer_amd import _lib
    eng = _engine(dev, max_batch)
    assert eng.max_batch == max_batch and eng.buf_patches.shape[0] == max_batch * T and eng.pos_rep.shape[0] == max_batch * T
    variant = int(_lib.lib().ink_gemm_query_variant(B * T, D, 3 * 768))
    assert variant == (45 if B >= 6 else 0)
    got = eng.encode(_images(dev, B), upto=0).clone()
    assert tuple(got.shape) == (B, T, D)
    _hold(got, [R.sam_stem_refs(i) for i in range(B)], f"stem B={B} (max_batch {max_batch}, GEMM variant {variant})")
    if (B, max_batch) == (2, 8):              # the same rows from the B = 2 engine: tile family and slices change nothing
        assert torch.equal(got, _engine(dev, 2).encode(_images(dev, 2), upto=0))


@torch.no_grad()
@pytest.mark.parametrize("small", [False, True], ids=["a", "b"])
@pytest.mark.parametrize("B", [1, 2, 8])
def test_neck_matches_float64(dev, B, small):
    """_blocks(B, None) of the depth-0 engine is the neck alone: tokens written into eng.x[:B*T] as
    test_vith_block_matches_float64 does.  Input (a) is shaped like the residual stream (randn + 3 randn(D)); input (b) is
    (a) x 2^-7, where the first LayerNorm2d's variance (~1e-3) makes eps = 1e-5 instead of 1e-6 land >= 10x outside the
    bound at every quantile (on (a) it stays inside).  Engine max_batch = 8 for every B.
    Measured on an MI355X, HIP error / bound at q0.5 / 0.9 / 0.99 / 0.999 / 1.0, worst image: input (a) 0.092 / 0.089 /
    0.086 / 0.084 / 0.097, input (b) 0.092 / 0.089 / 0.086 / 0.084 / 0.092, the same at B = 1, 2 and 8 (HIP median 4.6e-7,
    0.7 x the float32 evaluation's 6.2e-7; the f16-operand evaluation is at 2.8e-4)."""
    eng = _engine(dev, 8)
    x = torch.stack([R.neck_tokens(i, small) for i in range(B)])
    eng.x[:B * T] = x.view(B * T, D).to(dev)
    if B < 8:
        eng.x[B * T:] = float("nan")                        # rows past the batch are not read
    got = eng._blocks(B, None)
    assert tuple(got.shape) == (B, T, E) and got.dtype == torch.float32
    _hold(got, [R.sam_neck_refs(i, small) for i in range(B)], f"neck B={B} input {'b' if small else 'a'}")


@torch.no_grad()
def test_stem_and_neck_match_float64(dev):
    """encode(imgs) at B = 2 against image_encoder(..., upto=None).  Measured on an MI355X, HIP error / bound at q0.5 / 0.9 /
    0.99 / 0.999 / 1.0: image 0 0.206 / 0.199 / 0.208 / 0.227 / 0.242, image 1 0.214 / 0.205 / 0.210 / 0.230 / 0.273 (HIP median
    5.2e-7, 1.7 x the float32 evaluation's)."""
    eng = _engine(dev, 8)
    got = eng.encode(_images(dev, 2)).clone()
    assert tuple(got.shape) == (2, T, E)
    _hold(got, [R.sam_full_refs(i) for i in range(2)], "stem + neck B=2")
