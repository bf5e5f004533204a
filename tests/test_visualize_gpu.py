"""Visualisation kernels (csrc/visualize.hip) through their C entry points: exact equality with the numpy path of
inklayer_amd/visualize.py (which tests/test_visualize_cpu.py pins to the reference) at the sizes where the kernel takes
another path - one row, odd widths, a width below one vector, H W % 4 != 0 (byte loads of the mask planes and the tail),
misaligned base addresses - and with the reference's own pictures at their native sizes."""
import numpy as np
import pytest
import torch

import vis_cases
from inklayer_amd import _lib, ops, visualize

MIN_INIT = 0x7F7F7F7F
SHAPES = [(1, 130), (61, 67), (64, 64), (33, 257), (5, 3)]


def _host(sketch, masks, **kw):
    return visualize.colour_sketch(sketch, masks, use_gpu=False, **kw)


def _host_min(sketch):
    g = visualize.gray_host(sketch)
    return int(g[g < 250].min()) if (g < 250).any() else MIN_INIT


def _device(dev, sketch, second, n, by_label=False, min_buf=None):
    """Both kernels through ops.* -> (picture, minimum) on the host."""
    tables = torch.from_numpy(visualize.colour_tables(visualize.pastel_colors(n))).to(dev)
    sk = torch.from_numpy(np.ascontiguousarray(sketch)).to(dev)
    m = torch.from_numpy(np.ascontiguousarray(second).view(np.uint8)).to(dev)
    mn = ops.vis_gray_min(sk, out=min_buf)
    out = ops.vis_colour(sk, m, tables, mn, by_label=by_label)
    return out.cpu().numpy(), int(mn.item())


@pytest.mark.gpu
@pytest.mark.parametrize("n", [0, 1, 3, 40])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_stack_form_equals_host_path(dev, shape, n):
    H, W = shape
    rs = np.random.RandomState(1000 * H + W + n)
    sketch = vis_cases.rgb_of(vis_cases.strokes(rs, H, W))
    sketch[..., 1] = np.where(rs.rand(H, W) < 0.5, sketch[..., 1], rs.randint(0, 256, size=(H, W)))    # not only grey
    masks = vis_cases.random_masks(rs, n, H, W)
    masks_u8 = masks.astype(np.uint8) * rs.randint(1, 256, size=(n, 1, 1)).astype(np.uint8)             # any non-zero value
    got, mn = _device(dev, sketch, masks_u8, n)
    assert mn == _host_min(sketch)
    assert np.array_equal(got, _host(sketch, list(masks)))
    gray = np.ascontiguousarray(visualize.gray_host(sketch))                                            # single-channel form
    got1, mn1 = _device(dev, gray, masks_u8, n)
    assert mn1 == mn and np.array_equal(got1, _host(gray, list(masks)))


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(61, 67), (64, 64), (33, 257)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_label_form_equals_host_path(dev, shape):
    H, W = shape
    rs = np.random.RandomState(H + W)
    sketch = vis_cases.rgb_of(vis_cases.strokes(rs, H, W, density=0.6))
    for n in (255, 3, 0):
        label = rs.randint(0, n + 1, size=(H, W)).astype(np.uint8)
        if n == 255:
            label[0, 0], label[H - 1, W - 1] = 255, 255
            sketch[0, 0] = sketch[H - 1, W - 1] = 17
        got, _ = _device(dev, sketch, label, n, by_label=True)
        assert np.array_equal(got, _host(sketch, label, n_labels=n)), n
        if n == 3:                                                  # the same picture from the masks of these labels
            masks = np.stack([label == l for l in range(1, n + 1)])
            assert np.array_equal(got, _device(dev, sketch, masks, n)[0])
    label = np.full((H, W), 9, np.uint8)                            # labels above n count as "no mask"
    assert np.array_equal(_device(dev, sketch, label, 3, by_label=True)[0], _host(sketch, [], colors=[]))


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(33, 257), (64, 64)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_branch_flag_sees_the_last_pixel(dev, shape):
    """A faint image whose only grey-229 pixel is the last pixel of the last row takes the power-law branch, its twin
    with 230 there the raw * 3 branch: a reduction that drops its tail paints the first like the second."""
    H, W = shape
    rs = np.random.RandomState(5)
    faint = vis_cases.strokes(rs, H, W, lo=231, hi=250)
    masks = vis_cases.random_masks(rs, 3, H, W)
    pictures = []
    for last in (229, 230):
        g = faint.copy()
        g[H - 1, W - 1] = last
        for sketch in (vis_cases.rgb_of(g), g):
            got, mn = _device(dev, sketch, masks, 3)
            assert mn == last
            assert np.array_equal(got, _host(sketch, list(masks)))
        pictures.append(got)
    assert (pictures[0][:-1] != pictures[1][:-1]).any()


@pytest.mark.gpu
def test_image_without_strokes_and_reused_minimum(dev):
    rs = np.random.RandomState(11)
    H, W = 61, 67
    masks = vis_cases.random_masks(rs, 3, H, W)
    empty = vis_cases.rgb_of(rs.randint(250, 256, size=(H, W)).astype(np.uint8))
    buf = torch.zeros(1, device=dev, dtype=torch.int32)             # 0 would select the power law if it were not reset
    got, mn = _device(dev, empty, masks, 3, min_buf=buf)
    assert mn == MIN_INIT and (got == 255).all()
    # two different images back to back on one stream through the same minimum word
    dark = vis_cases.rgb_of(vis_cases.strokes(rs, H, W))
    faint = vis_cases.rgb_of(vis_cases.strokes(rs, H, W, lo=231, hi=250))
    tables = torch.from_numpy(visualize.colour_tables(visualize.pastel_colors(3))).to(dev)
    m = torch.from_numpy(masks.view(np.uint8)).to(dev)
    outs = []
    for sketch in (dark, faint, dark):
        sk = torch.from_numpy(sketch).to(dev)
        outs.append(ops.vis_colour(sk, m, tables, ops.vis_gray_min(sk, out=buf)))
    assert int(buf.item()) == _host_min(dark)
    for sketch, out in zip((dark, faint, dark), outs):
        assert np.array_equal(out.cpu().numpy(), _host(sketch, list(masks)))


@pytest.mark.gpu
def test_misaligned_pointers_take_the_byte_path(dev):
    """Every buffer one byte off a 4-byte boundary (views into larger allocations), straight through the C entry points."""
    rs = np.random.RandomState(3)
    H, W, n = 33, 64, 3                                             # H W % 4 == 0: only the base addresses are odd
    sketch = vis_cases.rgb_of(vis_cases.strokes(rs, H, W))
    masks = vis_cases.random_masks(rs, n, H, W)

    def off1(a):
        flat = torch.zeros(a.size + 8, device=dev, dtype=torch.uint8)
        flat[1:1 + a.size] = torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1)).to(dev)
        return flat, flat.data_ptr() + 1

    keep_s, sk = off1(sketch)
    keep_m, mk = off1(masks)
    tables = torch.from_numpy(visualize.colour_tables(visualize.pastel_colors(n))).to(dev)
    out = torch.full((H * W * 3 + 8,), 7, device=dev, dtype=torch.uint8)
    mn = torch.empty(1, device=dev, dtype=torch.int32)
    L, st = _lib.lib(), ops._stream()
    assert sk % 4 == 1 and mk % 4 == 1 and (out.data_ptr() + 1) % 4 == 1
    assert L.ink_vis_gray_min(sk, 3, H, W, mn.data_ptr(), st) == 0
    assert L.ink_vis_colour(sk, 3, mk, n, 0, tables.data_ptr(), mn.data_ptr(), H, W, out.data_ptr() + 1, st) == 0
    got = out.cpu().numpy()
    assert got[0] == 7 and (got[1 + H * W * 3:] == 7).all()         # nothing written outside the picture
    assert np.array_equal(got[1:1 + H * W * 3].reshape(H, W, 3), _host(sketch, list(masks)))
    assert int(mn.item()) == _host_min(sketch)


@pytest.mark.gpu
@pytest.mark.parametrize("name", vis_cases.SETS)
def test_kernels_reproduce_the_reference_pictures(dev, name):
    s = vis_cases.load_set(name)
    sk = torch.from_numpy(s["input"].copy()).to(dev)
    for stage, picture in (("masks", "segmented_sketch"), ("masks_final", "segmented_sketch_final")):
        masks = s[stage]
        n = len(masks)
        m = torch.from_numpy(masks.view(np.uint8).copy()).to(dev)
        got = visualize.colour_sketch(sk, m)                        # device in, device out
        assert torch.is_tensor(got) and got.is_cuda
        assert int((got.cpu().numpy() != s[picture]).any(-1).sum()) == 0, (name, picture, "stack")
        label = torch.from_numpy(visualize.label_image(list(masks), masks.shape[1:])).to(dev)
        got = visualize.colour_sketch(sk, label, n_labels=n)
        assert int((got.cpu().numpy() != s[picture]).any(-1).sum()) == 0, (name, picture, "label")
    got = visualize.colour_sketch(s["input"], list(s["masks"]))     # host in: uploaded, host out
    assert isinstance(got, np.ndarray) and np.array_equal(got, s["segmented_sketch"])


def test_bad_arguments_are_rejected_without_launch():
    """Argument validation happens before any HIP call (fake non-null pointers; no GPU needed)."""
    L = _lib.lib()
    p = 16
    good = dict(sk=p, ch=3, H=8, W=8, mn=p)
    gmin = lambda **kw: L.ink_vis_gray_min(*{**good, **kw}.values(), None)
    assert gmin(sk=None) == 1 and gmin(mn=None) == 1
    assert gmin(H=0) == 1 and gmin(W=0) == 1 and gmin(H=-3) == 1 and gmin(W=-1) == 1
    assert gmin(ch=2) == 1 and gmin(ch=0) == 1 and gmin(ch=4) == 1
    good = dict(sk=p, ch=3, m=p, n=2, by_label=0, tab=p, mn=p, H=8, W=8, out=p)
    col = lambda **kw: L.ink_vis_colour(*{**good, **kw}.values(), None)
    assert col(sk=None) == 1 and col(tab=None) == 1 and col(mn=None) == 1 and col(out=None) == 1
    assert col(m=None) == 1 and col(m=None, n=0, by_label=1) == 1   # only an empty stack may be null
    assert col(H=0) == 1 and col(W=0) == 1 and col(H=-1) == 1 and col(W=-8) == 1
    assert col(n=-1) == 1 and col(n=-1, by_label=1) == 1 and col(n=256, by_label=1) == 1
    assert col(ch=2) == 1
