"""The small row kernels against float64: norm.hip (rmsnorm, fused_add_rmsnorm, layernorm,
row_sumsq, embed_gather), activation.hip (silu_and_mul in both layouts, gelu_tanh), the
pooling kernels of sampling.hip (segment_sum, mean_l2norm_rows) and the routing and layout
part of moe.hip (moe_topk_softmax, moe_route, moe_route_norm, moe_align).

Every (threads, VPT) instantiation of the norms, eps larger than the variance, a mean far
from zero, the second trip of the grid-stride loops, routing weights compared expert by
expert, moe_align against its documented contract. The inputs, the float64 references and
the bounds are in tests/_row_ref.py; tests/test_row_refs_cpu.py holds the package's fp32
CPU paths to the same bounds on the same inputs. Outputs are NaN-filled before the call and
buffers are longer or wider than needed, with the slack compared bit for bit afterwards.
"""
import pytest
import torch

import _row_ref as R
from xgserve import ops
from xgserve.ops import _native
from xgserve.ops._native import stream_ptr
from xgserve.ops.linear import PendingSum

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(autouse=True, scope="module")
def _native_loaded():
    _native.kernels()  # fail loudly: the HIP library must be the one that runs
    torch.manual_seed(0)


# ---------------------------------------------------------------- norms
@pytest.mark.parametrize("regime", R.RMS_REGIMES)
@pytest.mark.parametrize("H", R.NORM_H)
def test_rmsnorm(H, regime):
    R.run_rmsnorm(DEV, 3, H, regime)


@pytest.mark.parametrize("T", [1, 70])
def test_rmsnorm_rows(T):
    R.run_rmsnorm(DEV, T, 4096, "unit")


@pytest.mark.parametrize("H,regime", [(8, "unit"), (1536, "small_eps1e-5"), (4104, "spike"), (16384, "unit")])
def test_rmsnorm_strided_x_and_out(H, regime):
    R.run_rmsnorm_strided(DEV, 3, H, regime)


@pytest.mark.parametrize("regime", R.RMS_REGIMES)
@pytest.mark.parametrize("H", R.NORM_H_REDUCED)
def test_fused_add_rmsnorm(H, regime):
    R.run_fused_add_rmsnorm(DEV, 3, H, regime)


@pytest.mark.parametrize("T", [1, 70])
def test_fused_add_rmsnorm_rows(T):
    R.run_fused_add_rmsnorm(DEV, T, 4096, "unit")


@pytest.mark.parametrize("regime", R.LN_REGIMES)
@pytest.mark.parametrize("H", R.NORM_H_REDUCED)
def test_layernorm(H, regime):
    R.run_layernorm(DEV, 3, H, regime)


@pytest.mark.parametrize("H", [128, 520, 2048, 4096, 8192])
def test_layernorm_far_mean_other_widths(H):
    R.run_layernorm(DEV, 3, H, "shifted")


@pytest.mark.parametrize("T", [1, 70])
def test_layernorm_rows(T):
    R.run_layernorm(DEV, T, 768, "shifted")


@pytest.mark.parametrize("eps", [1e-5, 1e-6])
def test_add_partials_rmsnorm_eps_above_variance(eps):
    """The split-K consumer of the same statistic: rows of variance 1e-6 (eps ten times / once that)."""
    part, res0, w = R.partials_inputs()
    S, T, H = part.shape
    res, ybuf = res0.clone().to(DEV), torch.full((T + 1, H), R.NAN, dtype=torch.bfloat16, device=DEV)
    y, r = ops.fused_add_rmsnorm(PendingSum(part.to(DEV), S), res, w.to(DEV), eps, out=ybuf[:T])
    assert r.data_ptr() == res.data_ptr() and y.data_ptr() == ybuf.data_ptr()
    assert torch.equal(R.bits(ybuf[T:]), R.bits(R._nan(1, H)))
    R.check_add_partials_rmsnorm(part, res0, w, eps, res.cpu(), ybuf[:T].cpu())


@pytest.mark.parametrize("T", [1, 5])
@pytest.mark.parametrize("H", [8, 2048, 4096, 28672])
def test_row_sumsq(H, T):
    R.run_row_sumsq(DEV, T, H)


# ---------------------------------------------------------------- activations
@pytest.mark.parametrize("interleave16", [False, True])
@pytest.mark.parametrize("T,F", R.SILU_SHAPES)
def test_silu_and_mul(T, F, interleave16):
    if interleave16 and F % 16:
        with pytest.raises(ValueError):  # the binding refuses the layout
            ops.silu_and_mul(R.silu_inputs(T, F).to(DEV), interleave16=True)
        return
    if T == 300:  # the grid-stride loop must run a second time
        assert T * (F // 8) > R.GRID_THREADS
    R.run_silu(DEV, R.silu_inputs(T, F), interleave16, f"silu_and_mul {T}x{F} interleave16={interleave16}")


@pytest.mark.parametrize("interleave16", [False, True])
def test_silu_and_mul_planted_gates(interleave16):
    R.run_silu(DEV, R.silu_planted_inputs(interleave16), interleave16, "silu_and_mul planted gates")


@pytest.mark.parametrize("T,N", R.GELU_SHAPES)
def test_gelu_tanh(T, N):
    if T == 1400:  # the grid-stride loop must run a second time
        assert T * N // 8 > R.GRID_THREADS
    R.run_gelu(DEV, R.gelu_inputs(T, N))


# ---------------------------------------------------------------- embedding and pooling
@pytest.mark.parametrize("H", R.EMBED_H)
def test_embed_gather(H):
    R.run_embed_gather(DEV, H)


@pytest.mark.parametrize("with_rows", [False, True])
@pytest.mark.parametrize("H", R.SEG_H)
def test_segment_sum_accumulates(H, with_rows):
    R.run_segment_sum(DEV, H, with_rows)


@pytest.mark.parametrize("H", R.L2N_H)
def test_mean_l2norm_rows(H):
    R.run_mean_l2norm(DEV, H)


# ---------------------------------------------------------------- MoE routing
@pytest.mark.parametrize("T", R.TOPK_T)
@pytest.mark.parametrize("E,k", R.TOPK_EK)
def test_moe_topk_softmax(E, k, T):
    R.run_topk_softmax(DEV, T, E, k)


@pytest.mark.parametrize("E,k", R.TOPK_EK)
def test_moe_topk_softmax_all_equal_logits(E, k):
    R.run_topk_softmax_ties(DEV, E, k)


@pytest.mark.parametrize("T,E,k,H", R.ROUTE_CASES)
def test_moe_route(T, E, k, H):
    R.run_moe_route(DEV, T, E, k, H)


@pytest.mark.parametrize("T,E,k,H", R.ROUTE_NORM_CASES)
def test_moe_route_norm(T, E, k, H):
    R.run_moe_route_norm(DEV, T, E, k, H)


@pytest.mark.parametrize("eps", [1e-5, 1e-6])
@pytest.mark.parametrize("H", [4096, 16392])
def test_moe_route_norm_eps_above_variance(H, eps):
    R.run_moe_route_norm(DEV, 3, 8, 2, H, scale=1e-3, eps=eps)


# ---------------------------------------------------------------- MoE layout
_ALIGN = R.align_cases()
SENTINEL = 0x5A5A5A5A


@pytest.mark.parametrize("name", sorted(_ALIGN))
def test_moe_align_contract(name):
    """The kernel on sentinel-filled buffers longer than needed: the whole capacity is
    written (-1 padding included) and nothing past it; then the wrapper, which sizes the
    buffers itself. BLOCK_M = 64 is the one value xgserve/ops/moe.py passes."""
    ids, E, eoff = _ALIGN[name]
    T, k = ids.shape
    bm = R.BLOCK_M
    assert bm == ops.moe.BLOCK_M
    cap = R.align_cap(T * k, E, bm)
    d_ids = ids.to(DEV)
    rows, offs, dest = (torch.full((n + 64,), SENTINEL, dtype=torch.int32, device=DEV) for n in (cap, E + 1, T * k))
    _native.kernels().moe_align(d_ids.data_ptr(), T, k, E, eoff, bm, rows.data_ptr(), offs.data_ptr(),
                                dest.data_ptr(), stream_ptr())
    for buf, n in ((rows, cap), (offs, E + 1), (dest, T * k)):
        assert bool((buf[n:] == SENTINEL).all()), "written past the end"
    R.check_align(ids, E, eoff, bm, rows[:cap], offs[:E + 1], dest[:T * k])
    R.check_align(ids, E, eoff, bm, *ops.moe_align(d_ids, E, eoff))
