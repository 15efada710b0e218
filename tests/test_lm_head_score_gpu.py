"""lm_head_score.hip through ops.score_rows against float64 log_softmax. Operands are small integers, so every logit
is exact in fp32 and the bound covers the exp / sum / log rounding of epilogue and merge:
|d lp| <= (BN + n_tiles + 8) 2^-24 (1 + |lp|) + |z_t - max| 2^-23, for best_lp with z_t = max."""
import pytest
import torch

from xgserve import ops
from xgserve.ops._native import kernels
from xgserve.ops.score import score_tile

DEV = "cuda:0"
BM, BN = 128, 256  # the kernel's tile (asserted against the library below)


def check(h, w, V, targets, tag):
    """Runs score_rows and holds all three outputs to the bound; returns the worst share used."""
    z = h.double() @ w.double().t()
    assert torch.equal(z.float().double(), z), "the test's logits are not exact in fp32"
    ref = torch.log_softmax(z, dim=-1)
    zmax = z.max(dim=-1).values
    want_id = torch.where(z == zmax[:, None], torch.arange(V), V).min(dim=-1).values  # the lowest index of a tie
    K = h.shape[1]  # device copies with padded row strides: NaN in the padding and in w's rows past V
    hd = torch.full((len(h), K + 8), float("nan"), dtype=torch.bfloat16, device=DEV)
    wd = torch.full((V + 8, K + 8), float("nan"), dtype=torch.bfloat16, device=DEV)
    hd[:, :K], wd[:V, :K] = h.bfloat16(), w.bfloat16()
    lp, best_id, best_lp = (t.cpu() for t in ops.score_rows(hd[:, :K], wd[:, :K], V, targets.to(DEV)))
    assert torch.equal(best_id.long(), want_id), f"{tag}: best_id"
    has = targets >= 0
    want_lp = torch.where(has, ref.gather(1, targets.clamp(min=0).long()[:, None])[:, 0], torch.zeros(len(h)).double())
    z_t = torch.where(has, z.gather(1, targets.clamp(min=0).long()[:, None])[:, 0], zmax)
    unit = (BN + -(-V // BN) + 8) * 2.0 ** -24
    share = 0.0
    for got, want, gap in ((lp, want_lp, (z_t - zmax).abs()), (best_lp, ref.max(dim=-1).values, torch.zeros(len(h)))):
        assert bool(torch.isfinite(got).all()), f"{tag}: inf or NaN"
        lim = unit * (1 + want.abs()) + gap * 2.0 ** -23
        share = max(share, float(((got.double() - want).abs() / lim).max()))
    assert bool((lp[~has] == 0).all()), f"{tag}: a row without a target has lp != 0"
    assert share <= 1.0, f"{tag}: {share:.3f} of the bound"
    return share


@pytest.mark.gpu
@pytest.mark.parametrize("K", (64, 192))
@pytest.mark.parametrize("V", (BN - 1, BN + 3, 2 * BN + 1))
@pytest.mark.parametrize("M", (1, BM - 1, BM + 1))
def test_score_rows_exact_logits(M, V, K):
    assert score_tile() == (BM, BN)
    g = torch.Generator().manual_seed(1000 * M + 10 * V + K)
    h = torch.randint(-2, 3, (M, K), generator=g).float()
    w = torch.randint(-2, 3, (V, K), generator=g).float()
    # column 0, column V - 1, the first column of the last (partial) tile, no target
    kinds = torch.tensor([0, V - 1, (V - 1) // BN * BN, -1], dtype=torch.int32)
    share = max(check(h, w, V, kinds[(torch.arange(M) + rot) % 4], f"M {M} V {V} K {K} rot {rot}") for rot in range(4))
    print(f"lm_head_score M {M} V {V} K {K}: {share:.3f} of the bound")


@pytest.mark.gpu
def test_tie_across_tiles_takes_lower_index():
    M, V, K = 3, 2 * BN + 1, 64
    g = torch.Generator().manual_seed(7)
    h, w = torch.zeros(M, K), torch.randint(-3, 4, (V, K), generator=g).float()
    h[:, 0] = 1                      # z[m, v] = w[v, 0]
    w[[5, BN + 7, 2 * BN], 0] = 9    # the row maximum in all three tiles
    check(h, w, V, torch.tensor([BN + 7, 5, -1], dtype=torch.int32), "tie")


@pytest.mark.gpu
def test_large_logits_are_max_subtracted_across_tiles():
    M, V, K = 2, 2 * BN + 1, 64
    g = torch.Generator().manual_seed(11)
    c = torch.randint(-10, 10, (V,), generator=g).float() / 4   # z = 128 c: -320 .. 288 in steps of 32
    c[BN + 1] = 2.5                                              # 320, in the middle tile only
    h, w = torch.full((M, K), 2.0), c[:, None].expand(V, K).clone()
    h[1] = -2.0                                                  # the mirrored row: its maximum is 320 as well
    check(h, w, V, torch.tensor([0, V - 1], dtype=torch.int32), "large")


@pytest.mark.parametrize("K", (32, 100))
def test_bad_k_raises_before_any_launch(K):
    with pytest.raises(ValueError):
        kernels().lm_head_score(0, K, 1, K, 0, K, 10, 0, 0, 0, 0, 0, 0)


def test_no_rows_no_launch():
    k = kernels()
    assert k.lm_head_score(0, 64, 0, 64, 0, 64, 10, 0, 0, 0, 0, 0, 0) is None
    assert k.lm_head_score_ws_floats(0, 10) == 0 and k.lm_head_score_ws_floats(BM + 1, 2 * BN + 1) == (BM + 1) * 10
