"""The bounds and inputs of tests/test_row_kernels_gpu.py, checked without a GPU: the
package's own fp32 CPU paths (rmsnorm_ref, layernorm_ref, silu_and_mul_ref, gelu_tanh_ref and
the CPU branches of the other ops) run on the same inputs and must meet every bound against
the float64 references of tests/_row_ref.py. A bound that a correct fp32 implementation
cannot meet is wrong; the near-tie caps of the router cases must hold for the committed
seeds; the moe_align contract checker must accept a plain implementation and refuse broken
layouts. `pytest -s` prints the largest share of each bound that the fp32 paths use.
"""
import pytest
import torch

import _row_ref as R
from xgserve import ops

DEV = "cpu"
WORST = {}


def note(res):
    for name, v in res.items():
        WORST[name] = max(WORST.get(name, 0.0), v)


# ---------------------------------------------------------------- the helpers themselves
def test_round_bf16_rounds_once():
    x = torch.tensor([1.0, -1.0, 0.0, 1.00390625, 1.01171875, 1.0 + 2.0 ** -8 + 2.0 ** -40, -(1.0 + 2.0 ** -8 + 2.0 ** -40),
                      3.0e38, 1e-30, 2000.0078125], dtype=torch.float64)
    want = torch.tensor([1.0, -1.0, 0.0, 1.0, 1.015625, 1.0078125, -1.0078125, 3.0e38, 1e-30, 2000.0]).bfloat16()
    assert torch.equal(R.bits(R.round_bf16(x)), R.bits(want))
    # 1 + 2^-8 + 2^-40 is above the tie, but a cast through fp32 first rounds it onto the tie and then to even
    assert float(x[5:6].float().bfloat16()) == 1.0
    r = torch.randn(4096, generator=R.gen("round")).double()
    assert torch.equal(R.bits(R.round_bf16(r.float().double())), R.bits(r.float().bfloat16()))


def test_check_refuses_what_is_out_of_bound():
    want = torch.tensor([1.0, 100.0], dtype=torch.float64)
    assert R.check(torch.tensor([1.0 + 2.0 ** -8, 100.0]), want, **R.ULP) == pytest.approx(0.5, rel=1e-2)
    with pytest.raises(AssertionError):
        R.check(torch.tensor([1.0, 101.0]), want, **R.ULP)
    with pytest.raises(AssertionError):
        R.dense(torch.ones(1, 2), torch.tensor([[3, 3]]), 8)
    with pytest.raises(AssertionError):
        R.dense(torch.ones(1, 2), torch.tensor([[3, 8]]), 8)


# ---------------------------------------------------------------- norms
@pytest.mark.parametrize("regime", R.RMS_REGIMES)
@pytest.mark.parametrize("H", R.NORM_H)
def test_rmsnorm(H, regime):
    note(R.run_rmsnorm(DEV, 3, H, regime))


def test_rmsnorm_rows_and_strides():
    for T in (1, 70):
        note(R.run_rmsnorm(DEV, T, 4096, "unit"))
    for H, regime in [(8, "unit"), (1536, "small_eps1e-5"), (4104, "spike"), (16384, "unit")]:
        note(R.run_rmsnorm_strided(DEV, 3, H, regime))


@pytest.mark.parametrize("regime", R.RMS_REGIMES)
@pytest.mark.parametrize("H", R.NORM_H_REDUCED)
def test_fused_add_rmsnorm(H, regime):
    note(R.run_fused_add_rmsnorm(DEV, 3, H, regime))
    if H == 8 and regime == "unit":
        for T in (1, 70):
            note(R.run_fused_add_rmsnorm(DEV, T, 4096, "unit"))


@pytest.mark.parametrize("regime", R.LN_REGIMES)
@pytest.mark.parametrize("H", R.NORM_H_REDUCED)
def test_layernorm(H, regime):
    note(R.run_layernorm(DEV, 3, H, regime))


def test_layernorm_far_mean():
    for H in (128, 520, 2048, 4096, 8192):
        note(R.run_layernorm(DEV, 3, H, "shifted"))
    for T in (1, 70):
        note(R.run_layernorm(DEV, T, 768, "shifted"))


def test_eps_regime_tells_a_wrong_eps():
    """What the small-scale regime is for: without eps the output is off by about a factor
    of 3, with the other eps by tens of percent."""
    c = R.norm_inputs(3, 4096, "small_eps1e-5")
    want = R.rmsnorm64(c["x"], c["w"], 1e-5)
    no_eps, other = R.rmsnorm64(c["x"], c["w"], 0.0), R.rmsnorm64(c["x"], c["w"], 1e-6)
    assert 3.0 < float((no_eps / want).abs().median()) < 3.7
    assert 2.0 < float((other / want).abs().median()) < 2.7
    s = R.norm_inputs(3, 4096, "shifted")
    assert float(s["x"].float().mean()) > 15.9


@pytest.mark.parametrize("eps", [1e-5, 1e-6])
def test_add_partials_rmsnorm_eps_above_variance(eps):
    part, res0, w = R.partials_inputs()
    acc = res0.float()
    for s in range(part.shape[0]):  # slab order, fp32, one rounding at the end
        acc = acc + part[s]
    res = acc.bfloat16()
    note(R.check_add_partials_rmsnorm(part, res0, w, eps, res, ops.rmsnorm_ref(res, w, eps)))


@pytest.mark.parametrize("T", [1, 5])
@pytest.mark.parametrize("H", [8, 2048, 4096, 28672])
def test_row_sumsq(H, T):
    note(R.run_row_sumsq(DEV, T, H))


# ---------------------------------------------------------------- activations
@pytest.mark.parametrize("interleave16", [False, True])
@pytest.mark.parametrize("T,F", R.SILU_SHAPES)
def test_silu_and_mul(T, F, interleave16):
    if interleave16 and F % 16:
        return
    note(R.run_silu(DEV, R.silu_inputs(T, F), interleave16, f"silu_and_mul {T}x{F} interleave16={interleave16}"))


def test_silu_and_mul_planted_gates():
    x = R.silu_planted_inputs(False)
    assert torch.equal(x[0, :len(R.SILU_PLANTED)].float(), torch.tensor(R.SILU_PLANTED).bfloat16().float())
    assert bool((x[0, 16:] == 1).all())
    for il in (False, True):
        note(R.run_silu(DEV, R.silu_planted_inputs(il), il, "silu_and_mul planted gates"))


@pytest.mark.parametrize("T,N", R.GELU_SHAPES)
def test_gelu_tanh(T, N):
    x = R.gelu_inputs(T, N)
    assert x.view(-1)[:2].tolist() == [100.0, -100.0]
    note(R.run_gelu(DEV, x))


def test_grid_stride_cases_reach_the_second_trip():
    T, F = R.SILU_SHAPES[-1]
    assert T * (F // 8) > R.GRID_THREADS and T * 2 * F * 2 < 20e6
    T, N = R.GELU_SHAPES[-1]
    assert T * N // 8 > R.GRID_THREADS and T * N * 2 < 20e6


# ---------------------------------------------------------------- embedding and pooling
@pytest.mark.parametrize("H", R.EMBED_H)
def test_embed_gather(H):
    note(R.run_embed_gather(DEV, H))


@pytest.mark.parametrize("with_rows", [False, True])
@pytest.mark.parametrize("H", R.SEG_H)
def test_segment_sum(H, with_rows):
    note(R.run_segment_sum(DEV, H, with_rows))


def test_segment_sum_bound_is_scaled_to_the_segment():
    hidden, cu, out0 = R.segment_inputs(4096)
    atol = R.segment_sum_atol(hidden, cu, out0)
    assert 1e-4 < atol < 2e-3, atol  # 301 additions of partial sums up to a few tens
    # the same bound for sequential fp32 addition, the order of the kernel
    seq = out0.clone()
    for s in range(len(R.SEG_LENS)):
        acc = torch.zeros(hidden.shape[1])
        for t in range(int(cu[s]), int(cu[s + 1])):
            acc = acc + hidden[t].float()
        seq[s] += acc
    note({"SEG": R.check(seq, R.segment_sum64(hidden, cu, out0), atol=atol, rtol=1e-5)})


@pytest.mark.parametrize("H", R.L2N_H)
def test_mean_l2norm_rows(H):
    note(R.run_mean_l2norm(DEV, H))


# ---------------------------------------------------------------- MoE routing
@pytest.mark.parametrize("T", R.TOPK_T)
@pytest.mark.parametrize("E,k", R.TOPK_EK)
def test_moe_topk_softmax(E, k, T):
    lg = R.topk_logits(T, E)
    assert all(lg[t].unique().numel() == E for t in range(0, T, 37)), "rows must be free of ties"
    assert torch.equal(lg.bfloat16().float(), lg)
    note(R.run_topk_softmax(DEV, T, E, k))


@pytest.mark.parametrize("E,k", R.TOPK_EK)
def test_moe_topk_softmax_all_equal_logits(E, k):
    note(R.run_topk_softmax_ties(DEV, E, k))


def test_dense_compare_tells_swapped_weights():
    """Weights paired with the wrong experts pass two independent sorts, not the expert -> weight map."""
    lg = R.topk_logits(5, 8)
    w, ids = ops.moe_topk_softmax(lg, 2, True)
    want = R.topk_softmax64(lg, 2, True)
    R.check(R.dense(w, ids, 8), want, **R.ROUTE)
    with pytest.raises(AssertionError):
        R.check(R.dense(w.flip(-1), ids, 8), want, **R.ROUTE)


@pytest.mark.parametrize("T,E,k,H", R.ROUTE_CASES)
def test_moe_route(T, E, k, H):
    h, router, _ = R.route_inputs(T, E, k, H)
    tie = R.near_tie_rows(h.double() @ router.double().t(), k)
    assert int(tie.sum()) <= R.ROUTE_TIE_CAP * T  # the float64 reference alone, for the committed seed
    note(R.run_moe_route(DEV, T, E, k, H))


@pytest.mark.parametrize("T,E,k,H", R.ROUTE_NORM_CASES)
def test_moe_route_norm(T, E, k, H):
    note(R.run_moe_route_norm(DEV, T, E, k, H))


@pytest.mark.parametrize("eps", [1e-5, 1e-6])
@pytest.mark.parametrize("H", [4096, 16392])
def test_moe_route_norm_eps_above_variance(H, eps):
    note(R.run_moe_route_norm(DEV, 3, 8, 2, H, scale=1e-3, eps=eps))


# ---------------------------------------------------------------- MoE layout
_ALIGN = R.align_cases()


@pytest.mark.parametrize("name", sorted(_ALIGN))
def test_align_contract_checker(name):
    ids, E, eoff = _ALIGN[name]
    rows, offs, dest = R.align_ref(ids, E, eoff, R.BLOCK_M)
    R.check_align(ids, E, eoff, R.BLOCK_M, rows, offs, dest)
    local = (dest >= 0).nonzero()[:, 0]
    broken = []
    if local.numel() >= 2:  # two pairs on one row
        d = dest.clone()
        d[local[1]] = d[local[0]]
        broken.append((rows, offs, d))
    r = rows.clone()  # a row that names the wrong token
    r[dest[local[0]]] += 1
    broken.append((r, offs, dest))
    r = rows.clone()  # padding that is not -1
    r[-1] = 0
    broken.append((r, offs, dest))
    o = offs.clone()  # a segment that is not padded to block_m
    o[-1] -= 1
    broken.append((rows, o, dest))
    if bool((dest < 0).any()):  # a foreign pair that was placed
        d = dest.clone()
        d[(dest < 0).nonzero()[0, 0]] = 0
        broken.append((rows, offs, d))
    for b in broken:
        with pytest.raises(AssertionError):
            R.check_align(ids, E, eoff, R.BLOCK_M, *b)


def test_align_cases_cover_the_edges():
    c = _ALIGN
    assert c["575x2_E8"][0].numel() > 1024 and c["625x8_E64"][0].numel() == 5000 and c["100x6_E256"][1] == 256
    ids, E, eoff = c["exact_block"]
    cnt = torch.bincount(ids.reshape(-1).long(), minlength=E)
    assert cnt.tolist() == [0, 64, 128, 0]
    assert c["shard_4of8"][1:] == (4, 4) and bool((c["negative_ids"][0] < 0).any())
    assert c["one_expert"][0].unique().numel() == 1


def test_zz_report_worst_share_of_each_bound():
    """Not a check of its own: prints what the fp32 paths used of each bound (pytest -s)."""
    for name in sorted(WORST):
        print(f"fp32 CPU path, largest share of bound {name}: {WORST[name]:.3g}")
    assert all(v <= 1.0 for v in WORST.values())
