"""ops.swin_attn (csrc/attention_swin.hip: Swin window attention with the bias table and the region ids taken compact)
against float64 attention, as GDinoEngine._swin_block calls it for a Swin-B backbone.  Inputs, reference, bound and the
mistakes the bound must tell apart: tests/swin_attn_ref.py.  GPU box only."""
import pytest
import torch

import swin_attn_ref as R

pytestmark = pytest.mark.gpu

F16 = torch.float16
IMAGES = [(100, 148), (300, 412)]     # stage grids at ws = 12: 3x4, 2x2, 1x1, 1x1 and 7x9, 4x5, 2x3, 1x2 windows


def _assert_within(got, ref, tol, what):
    err = (got - ref).abs()
    bad = ~(err <= tol)                         # NaN-safe: a NaN output is out of bound
    if bad.any():
        i = int(bad.flatten().nonzero()[0])
        raise AssertionError(f"{what}: {int(bad.sum())} / {bad.numel()} elements out of bound; first at flat {i}: "
                             f"got {got.flatten()[i].item()!r}, ref {ref.flatten()[i].item()!r}, "
                             f"tol {tol.flatten()[i].item()!r}")


def _run(dev, c, ws):
    """The kernel on case c: q / k / v column slices of the packed buffer, output into a NaN-filled buffer whose 64
    following rows must stay NaN.  -> float64 [Bw, nh, N, 32]."""
    from inklayer_amd import ops
    C, rows = c.C, c.Bw * c.N
    bd = c.buf.to(dev)
    full = torch.full((rows + 64, C), R.NAN, dtype=F16, device=dev)
    got = ops.swin_attn(bd[:, :C], bd[:, C:2 * C], bd[:, 2 * C:3 * C], n_windows=c.Bw, n_heads=c.nh, ws=ws, scale=R.SCALE,
                        bias_table=c.table.t().contiguous().to(dev),
                        region=c.region.to(dev) if c.region is not None else None, nW=c.nW, out=full[:rows])
    assert got.data_ptr() == full.data_ptr()
    full = full.cpu()
    assert full[rows:].isnan().all(), "rows past n_windows * ws^2 were written"
    return full[:rows].double().view(c.Bw, c.N, c.nh, 32).permute(0, 2, 1, 3)


def _check_discriminates(c):
    for what, wrong in c.wrongs.items():
        m = ((wrong - c.o).abs() / c.tol).max().item()
        print(f"  {what}: {m:.0f}x the bound")
        assert m >= 100, f"the bound cannot tell the mistake '{what}' apart: max deviation {m:.1f}x the bound"


@torch.no_grad()
@pytest.mark.parametrize("shifted", [0, 1])
@pytest.mark.parametrize("stage", [0, 1, 2, 3])
@pytest.mark.parametrize("hw", IMAGES)
def test_swin_attn_ws12(dev, hw, stage, shifted):
    """swin_attn_kernel<12>, B = 2, the stage's head count (4, 8, 16, 32), shifted and unshifted, on the plans of a
    100 x 148 and a 300 x 412 image (stages 2 and 3 of the first are a single, mostly padded window).  Bound:
    swin_attn_ref.tol (derived there from the kernel's arithmetic: 144 keys in 160 slots, one-pass softmax, P rounded
    to f16 before P V)."""
    c = R.case(hw, stage, shifted, 12)
    _check_discriminates(c)
    got = _run(dev, c, 12)
    print(f"{hw} stage {stage} shifted {shifted}: worst error {((got - c.o).abs() / c.tol).max().item():.3f}x the bound")
    _assert_within(got, c.o, c.tol, f"swin_attn ws 12 {hw} stage {stage} shifted {shifted}")


@torch.no_grad()
@pytest.mark.parametrize("shifted", [0, 1])
def test_swin_attn_ws12_persistent_walk(dev, shifted):
    """B = 5 at stage 1 of the 300 x 412 plan: 100 windows x 8 heads = 800 units, more than the 2-per-CU grid of 512
    workgroups, so workgroups walk two units - a head change, and for some a window (and region) change, with the
    next unit's rows prefetched into registers."""
    c = R.case((300, 412), 1, shifted, 12, B=5)
    assert c.Bw * c.nh > 512
    got = _run(dev, c, 12)
    print(f"walk shifted {shifted}: worst error {((got - c.o).abs() / c.tol).max().item():.3f}x the bound")
    _assert_within(got, c.o, c.tol, f"swin_attn ws 12 persistent walk shifted {shifted}")


@torch.no_grad()
@pytest.mark.parametrize("shifted", [0, 1])
@pytest.mark.parametrize("stage", [0, 1, 2, 3])
@pytest.mark.parametrize("hw", IMAGES)
def test_swin_attn_ws7_and_flash_mode3(dev, hw, stage, shifted):
    """swin_attn_kernel<7> and ops.flash_attn bias_mode 3 on identical inputs (the same packed buffer; the table as the
    dense [nh, 49, 64] bias / the regions as the dense [nW, 49, 64] mask the Swin-T engine builds).  Each sits within
    its own bound of the float64 result; at ws = 7 the two bounds are the same expression (64 key slots, 49 keys:
    swin_attn_ref.tol equals test_detector_ops_gpu._swin_attn_tol term for term)."""
    from inklayer_amd import gdino, ops
    c = R.case(hw, stage, shifted, 7)
    _check_discriminates(c)
    got = _run(dev, c, 7)
    bd, C = c.buf.to(dev), c.C
    dense = gdino.swin_dense_bias(c.table, 7, c.nh, R.SCALE)
    mask = None
    if shifted:
        mask = torch.zeros((c.nW, 49, 64))
        mask[:, :, :49] = c.sm.float() / R.SCALE
    ref3 = ops.flash_attn(bd[:, :C], bd[:, C:2 * C], bd[:, 2 * C:3 * C], n_batch=c.Bw, n_heads=c.nh, head_dim=32,
                          scale=R.SCALE, n_q=49, n_k=49, dense_bias=dense.to(dev),
                          dense_mask=mask.to(dev) if shifted else None)
    got3 = ref3.cpu().double().view(c.Bw, 49, c.nh, 32).permute(0, 2, 1, 3)
    print(f"{hw} stage {stage} shifted {shifted}: swin_attn {((got - c.o).abs() / c.tol).max().item():.3f}x, "
          f"flash_attn mode 3 {((got3 - c.o).abs() / c.tol).max().item():.3f}x the bound")
    _assert_within(got, c.o, c.tol, f"swin_attn ws 7 {hw} stage {stage} shifted {shifted}")
    _assert_within(got3, c.o, c.tol, f"flash_attn mode 3 {hw} stage {stage} shifted {shifted}")
