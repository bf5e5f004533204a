"""CPU-side checks of the device-table MSDA forward / backward (ABI 5): both C entry points reject bad arguments
without launching anything, and the ops wrappers reject what the reference rejects before any launch.  No GPU."""
import ctypes

import pytest
import torch

FWD_ARGS = dict(dtype=0, B=2, S=30, M=2, C=32, Q=5, L=2, P=4, step=64)


def _fwd(l, ptr=16, **kw):
    a = {**FWD_ARGS, **kw}
    return l.ink_ms_deform_attn_forward_dev(ptr, ptr, ptr, ptr, ptr, a["dtype"], a["B"], a["S"], a["M"], a["C"],
                                            a["Q"], a["L"], a["P"], a["step"], ptr, None)


def _bwd(l, ptr=16, **kw):
    a = {**FWD_ARGS, **kw}
    return l.ink_ms_deform_attn_backward_dev(ptr, ptr, ptr, ptr, ptr, ptr, a["dtype"], a["B"], a["S"], a["M"], a["C"],
                                             a["Q"], a["L"], a["P"], a["step"], ptr, ptr, ptr, None)


@pytest.mark.parametrize("call", [_fwd, _bwd], ids=["forward_dev", "backward_dev"])
def test_device_table_entry_points_reject_bad_arguments_without_launch(call):
    # every case returns 1 before any HIP call (the pointers are never dereferenced on the host)
    from inklayer_amd import _lib
    l = _lib.lib()
    assert call(l, ptr=None) == 1                       # null pointers
    for bad in (dict(C=0), dict(C=-3), dict(L=0), dict(L=-1), dict(dtype=2), dict(dtype=-1),
                dict(B=3, step=2), dict(step=0), dict(B=0), dict(S=0), dict(M=0), dict(Q=0), dict(P=0),
                dict(B=2 ** 16, Q=2 ** 14, M=8)):      # more lanes than an int indexes
        assert call(l, **bad) == 1, bad


def test_backward_rejects_each_null_pointer():
    from inklayer_amd import _lib
    l = _lib.lib()
    a = FWD_ARGS
    for i in range(9):
        ptrs = [16] * 9
        ptrs[i] = None
        assert l.ink_ms_deform_attn_backward_dev(*ptrs[:6], a["dtype"], a["B"], a["S"], a["M"], a["C"], a["Q"],
                                                 a["L"], a["P"], a["step"], *ptrs[6:], None) == 1, i


def test_abi_version_is_10():
    from inklayer_amd import _lib
    assert _lib.lib().ink_abi_version() == 10
    assert "ink_ms_deform_attn_forward_dev" in _lib.SIGNATURES and "ink_ms_deform_attn_backward_dev" in _lib.SIGNATURES


def _inputs(dtype=torch.float32, shapes_dtype=torch.int64):
    shapes = torch.tensor([[4, 5], [2, 5]], dtype=shapes_dtype)
    starts = torch.tensor([0, 20], dtype=shapes_dtype)
    v = torch.zeros(2, 30, 2, 8, dtype=dtype)
    loc = torch.zeros(2, 5, 2, 2, 4, 2, dtype=dtype)
    aw = torch.zeros(2, 5, 2, 2, 4, dtype=dtype)
    return v, shapes, starts, loc, aw


def test_ops_reject_cpu_float_tensors():
    from inklayer_amd import ops
    v, ss, ls, loc, aw = _inputs()
    with pytest.raises(ValueError, match="GPU tensors"):
        ops.ms_deform_attn_forward(v, ss, ls, loc, aw, 64)
    with pytest.raises(ValueError, match="GPU tensors"):
        ops.ms_deform_attn_backward(v, ss, ls, loc, aw, torch.zeros(2, 5, 16), 64)
    with pytest.raises(ValueError, match="GPU tensors"):
        ops.ms_deform_attn(v, ss, ls, loc, aw)


def test_ops_reject_int32_shape_tables():
    from inklayer_amd import ops
    v, ss, ls, loc, aw = _inputs(shapes_dtype=torch.int32)
    with pytest.raises(ValueError, match="int64"):
        ops.ms_deform_attn_forward(v, ss, ls, loc, aw, 64)
    with pytest.raises(ValueError, match="int64"):
        ops.ms_deform_attn_backward(v, ss, ls, loc, aw, torch.zeros(2, 5, 16), 64)


def test_ops_reject_mixed_float_dtypes():
    from inklayer_amd import ops
    v, ss, ls, loc, aw = _inputs()
    with pytest.raises(ValueError, match="one dtype"):
        ops.ms_deform_attn_forward(v, ss, ls, loc.double(), aw, 64)
    with pytest.raises(ValueError, match="one dtype"):
        ops.ms_deform_attn_backward(v, ss, ls, loc, aw, torch.zeros(2, 5, 16, dtype=torch.float64), 64)
    with pytest.raises(ValueError, match="float32 or float64"):
        ops.ms_deform_attn_forward(v.half(), ss, ls, loc.half(), aw.half(), 64)
