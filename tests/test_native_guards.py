"""Host-side argument guards of the HIP kernel bindings: out-of-range shapes must
raise before anything is launched (checked on CPU: the binding throws before any
HIP call, so null pointers are never dereferenced)."""
import pytest

from xgserve.ops._native import kernels


@pytest.mark.parametrize("E,k", [(65, 2), (0, 1), (8, 0), (8, 17), (4, 5), (128, 8)])
def test_moe_topk_softmax_rejects_out_of_range(E, k):
    with pytest.raises(ValueError):
        kernels().moe_topk_softmax(0, 1, 4, E, k, 1, 0, 0, 0)


# The norm kernels hold a row in registers, at most 256 threads x 8 chunks x 8 columns:
# a wider row would be truncated without a fault, a narrower one has no chunk at all.
_NORM_CALLS = {
    "rmsnorm": lambda k, T, H: k.rmsnorm(0, 0, 0, T, H, 1e-5, H, H, 0),
    "fused_add_rmsnorm": lambda k, T, H: k.fused_add_rmsnorm(0, 0, 0, 0, T, H, 1e-5, 0),
    "layernorm": lambda k, T, H: k.layernorm(0, 0, 0, 0, T, H, 1e-5, 0),
    "add_partials_rmsnorm": lambda k, T, H: k.add_partials_rmsnorm(0, 2, T, 0, 0, 0, H, 1e-5, 0),
}


@pytest.mark.parametrize("H", [0, 4, 16392, 28672])
@pytest.mark.parametrize("op", sorted(_NORM_CALLS))
def test_norm_rejects_row_width_out_of_range(op, H):
    with pytest.raises(ValueError):
        _NORM_CALLS[op](kernels(), 1, H)
    with pytest.raises(ValueError):
        _NORM_CALLS[op](kernels(), 0, H)


@pytest.mark.parametrize("H", [8, 16384])
@pytest.mark.parametrize("op", sorted(_NORM_CALLS))
def test_norm_accepts_row_width_limits(op, H):
    assert (kernels().norm_min_h(), kernels().norm_max_h()) == (8, 16384)
    _NORM_CALLS[op](kernels(), 0, H)  # T = 0: the guard passes and nothing is launched


def test_moe_align_rejects_out_of_range():
    with pytest.raises(ValueError):
        kernels().moe_align(0, 4, 2, 300, 0, 64, 0, 0, 0, 0)
