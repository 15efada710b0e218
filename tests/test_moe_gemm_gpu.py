"""The grouped (MoE) gemm_m64g kernels called directly, at every instantiation.

fused_moe's planner reaches only a few (cfg, nw, S, row body) combinations; here every
cfg 0-6 x nw x mode runs on a small layout that reaches the 16-, 32-, 64- and 128-row
bodies, an empty expert, capacity padding, both x forms (gathered / already padded),
both row-occupancy forms (sorted rows / all 64 rows) and every ring-tail residue of
the K-chunk loop. Outputs start as NaN: real rows are compared with a float64 CPU
reference (tolerances of tests/test_skinny_gpu.py for the same modes of the dense
kernel) and, with K rotation off, bit for bit with the dense gemm_m64g on the same
rows; tiles without a real row must keep the NaN.
"""
import pytest
import torch

from xgserve import tune
from xgserve.ops import _native
from xgserve.ops._native import stream_ptr
from xgserve.ops.linear import M64G_CFGS, MODE_BF16, MODE_PARTIAL, MODE_SILU

pytestmark = pytest.mark.gpu
DEV = "cuda"
N = 256
E = 5
PAD_TILES = 2  # capacity padding past the last segment: never written
# max_rows -> real rows per expert
LAYOUTS = {16: (5, 0, 16, 1, 9), 64: (5, 0, 20, 40, 150), 300: (5, 0, 20, 40, 150)}
KS = ((128, 1), (384, 1), (512, 1), (640, 1), (512, 2), (768, 2))  # (K, S)
MODES = {"partial": MODE_PARTIAL, "bf16": MODE_BF16, "silu": MODE_SILU}


def rel_err(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-6))


class Layout:
    """Block-64 padded expert-sorted layout of `real` rows per expert, built by hand."""

    def __init__(self, real, gen):
        self.real = real
        self.T = sum(real)
        offs, rows, src = [0], [], torch.randperm(self.T, generator=gen).tolist()
        self.tiles = []  # (first padded row, real rows, expert) of every tile that holds real rows
        for e, n in enumerate(real):
            seg = -(-n // 64) * 64
            rows += src[:n] + [-1] * (seg - n)
            src = src[n:]
            self.tiles += [(offs[-1] + 64 * t, min(64, n - 64 * t), e) for t in range(seg // 64)]
            offs.append(offs[-1] + seg)
        self.P = offs[-1] + 64 * PAD_TILES
        rows += [-1] * (64 * PAD_TILES)
        self.rows_cpu = torch.tensor(rows, dtype=torch.int32)
        self.rows = self.rows_cpu.to(DEV)
        self.offs = torch.tensor(offs, dtype=torch.int32, device=DEV)
        self.end = offs[-1]
        self.real_idx = (self.rows_cpu >= 0).nonzero()[:, 0].to(DEV)
        self.expert_of = torch.zeros(self.P, dtype=torch.long)
        for e in range(E):
            self.expert_of[offs[e]:offs[e + 1]] = e


class Case:
    """Inputs of one (layout, K) and their float64 reference, made once per module."""

    def __init__(self, lay, K, gen):
        self.lay, self.K = lay, K
        x = torch.randn(lay.T, K, generator=gen).bfloat16()
        w = (torch.randn(E, N, K, generator=gen) * 0.05).bfloat16()
        xp = torch.randn(lay.P, K, generator=gen).bfloat16()  # pad rows: finite, never compared
        real = lay.rows_cpu >= 0
        xp[real] = x[lay.rows_cpu[real].long()]
        # y[p] = x_pad[p] . W[expert of p]^T, float64 from the bf16 inputs (real rows only are used)
        y = torch.zeros(lay.P, N, dtype=torch.float64)
        for e in range(E):
            seg = lay.expert_of == e
            y[seg] = xp[seg].double() @ w[e].double().t()
        g, u = y.view(lay.P, N // 32, 2, 16)[:, :, 0], y.view(lay.P, N // 32, 2, 16)[:, :, 1]
        self.ref = y[real].to(DEV)
        self.ref_silu = (torch.nn.functional.silu(g) * u).reshape(lay.P, N // 2)[real].to(DEV)
        self.x, self.w, self.xp = x.to(DEV), w.to(DEV), xp.to(DEV)


@pytest.fixture(scope="module")
def cases():
    k = _native.kernels()
    k.set_k_rotation(0)  # dense and grouped walk the K chunks in the same order
    gen = torch.Generator().manual_seed(0)
    lays = {real: Layout(real, gen) for real in set(LAYOUTS.values())}
    made = {}

    def get(max_rows, K):
        key = (LAYOUTS[max_rows], K)
        if key not in made:
            made[key] = Case(lays[key[0]], K, gen)
        return made[key]

    yield get
    k.set_k_rotation(tune.get_int("krot", 1))


def grouped(c, cfg, nw, mode, S, max_rows, gather, use_valid):
    """One moe_gemm_m64g_rows launch into NaN-filled buffers -> the written tensor [P, cols]."""
    lay = c.lay
    part = torch.full((S, lay.P, N), float("nan"), device=DEV)
    out = torch.full((lay.P, N // 2 if mode == MODE_SILU else N), float("nan"), device=DEV, dtype=torch.bfloat16)
    _native.kernels().moe_gemm_m64g_rows(
        (c.x if gather else c.xp).data_ptr(), lay.rows.data_ptr() if gather else 0, lay.offs.data_ptr(), E, c.K,
        c.w.data_ptr(), N, lay.P, part.data_ptr() if mode == MODE_PARTIAL else 0,
        0 if mode == MODE_PARTIAL else out.data_ptr(), S, mode, nw, cfg, max_rows, stream_ptr(),
        lay.rows.data_ptr() if use_valid else 0, 0)
    return part if mode == MODE_PARTIAL else out


def dense_rows(c, cfg, nw, mode, S):
    """The dense gemm_m64g on every tile's real rows and its expert's weight -> [real rows, cols]
    in padded-row order (S slabs first for partials)."""
    k = _native.kernels()
    got = []
    for p0, n, e in c.lay.tiles:
        part = torch.empty(S, n, N, device=DEV)
        out = torch.empty(n, N // 2 if mode == MODE_SILU else N, device=DEV, dtype=torch.bfloat16)
        k.gemm_m64g(c.xp[p0:p0 + n].data_ptr(), n, c.K, c.w[e].data_ptr(), N, part.data_ptr(), out.data_ptr(), S,
                    mode, nw, cfg, stream_ptr())
        got.append(part if mode == MODE_PARTIAL else out)
    return torch.cat(got, dim=-2)


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("nw", [1, 2])
@pytest.mark.parametrize("cfg", list(range(7)))
def test_moe_gemm_rows_every_instantiation(cases, cfg, nw, mode):
    md = MODES[mode]
    kc = M64G_CFGS[cfg][1]
    for max_rows in LAYOUTS:
        if max_rows == 300 and kc != 64:
            continue  # the 128-row kernels exist for the KC 64 configurations only
        for K, S in KS:
            c = cases(max_rows, K)
            if (md == MODE_SILU and (nw != 2 or S != 1)):
                with pytest.raises(ValueError):
                    grouped(c, cfg, nw, md, S, max_rows, True, True)
                continue
            if md == MODE_BF16 and S != 1:
                continue  # bf16 rows of a split K are not a mode (the dense kernel refuses them)
            dense = dense_rows(c, cfg, nw, md, S)
            ref = c.ref_silu if md == MODE_SILU else c.ref
            for gather in (True, False):
                for use_valid in (True, False):
                    tag = (max_rows, K, S, gather, use_valid)
                    got = grouped(c, cfg, nw, md, S, max_rows, gather, use_valid)
                    real = got.index_select(-2, c.lay.real_idx)
                    if md == MODE_PARTIAL:
                        err = rel_err(real.sum(0), ref)
                        print(tag, "partial rel_err", err)
                        assert err < 1e-5, tag
                    else:
                        err = rel_err(real, ref)
                        print(tag, mode, "rel_err", err)
                        assert err < 1e-2, tag
                    assert torch.equal(real, dense), tag  # same chunk order, same MFMA sequence
                    assert bool(torch.isnan(got[..., c.lay.end:, :]).all()), tag


def test_moe_gemm_rows_refuses_bad_operands(cases):
    c = cases(64, 512)
    with pytest.raises(ValueError):
        grouped(c, 7, 1, MODE_PARTIAL, 1, 64, True, True)   # cfg 7 has no grouped form
    with pytest.raises(ValueError):
        grouped(c, 0, 3, MODE_PARTIAL, 1, 64, True, True)   # nw
    with pytest.raises(ValueError):
        grouped(c, 0, 1, MODE_PARTIAL, 3, 64, True, True)   # K % (S * KC)


@pytest.mark.parametrize("nw", [1, 2])
@pytest.mark.parametrize("cfg", list(range(7)))
def test_moe_gemm_resid_in_launch_combine(cfg, nw):
    """GG_MOE_RESID: the w2 launch adds the weighted (token, choice) rows into the bf16
    residual and writes the per-column-tile statistics of the rounded residual."""
    k = _native.kernels()
    T, kk, K = 8, 2, 512
    cols = 16 * nw * M64G_CFGS[cfg][0]
    assert N // cols <= 64
    gen = torch.Generator().manual_seed(1 + cfg)
    ids = torch.stack([torch.randperm(E, generator=gen)[:kk] for _ in range(T)])  # [T, k], distinct per token
    wts = torch.rand(T, kk, generator=gen) + 0.25
    count = [int((ids == e).sum()) for e in range(E)]
    offs = [0]
    for n in count:
        offs.append(offs[-1] + -(-n // 64) * 64)
    P = offs[-1] + 64 * PAD_TILES
    rows = torch.full((P,), -1, dtype=torch.int32)
    dest = torch.empty(T * kk, dtype=torch.int32)
    fill = list(offs[:E])
    for i, e in enumerate(ids.reshape(-1).tolist()):
        dest[i], rows[fill[e]] = fill[e], i // kk
        fill[e] += 1
    act = torch.randn(P, K, generator=gen).bfloat16()   # x already in the padded layout
    w = (torch.randn(E, N, K, generator=gen) * 0.05).bfloat16()
    resid0 = torch.randn(T, N, generator=gen).bfloat16()
    expert_of = torch.zeros(P, dtype=torch.long)
    for e in range(E):
        expert_of[offs[e]:offs[e + 1]] = e
    y = torch.zeros(P, N, dtype=torch.float64)
    for e in range(E):
        y[expert_of == e] = act[expert_of == e].double() @ w[e].double().t()
    terms = wts.double().reshape(-1, 1) * y[dest.long()]                    # [T * k, N]
    exact = resid0.double() + terms.view(T, kk, N).sum(1)
    act_d, w_d, rows_d, dest_d = act.to(DEV), w.to(DEV), rows.to(DEV), dest.to(DEV)
    offs_d = torch.tensor(offs, dtype=torch.int32, device=DEV)
    wts_d = wts.reshape(-1).contiguous().to(DEV)
    for S in (1, 2):
        part = torch.full((S, P, N), float("nan"), device=DEV)
        resid = resid0.to(DEV)
        ss = torch.full((N // cols, T), float("nan"), device=DEV)
        counters = torch.zeros(N // cols, dtype=torch.int32, device=DEV)
        k.moe_gemm_m64g_resid(act_d.data_ptr(), 0, offs_d.data_ptr(), E, K, w_d.data_ptr(), N, P, part.data_ptr(), S,
                              nw, cfg, T * kk, stream_ptr(), rows_d.data_ptr(), dest_d.data_ptr(), wts_d.data_ptr(),
                              resid.data_ptr(), ss.data_ptr(), counters.data_ptr(), T, kk, T * kk)
        got = resid.cpu().double()
        err = rel_err(got, exact)
        print((cfg, nw, S), "resid rel_err", err)
        assert err < 1e-2, S
        # one bf16 rounding of the fp32 sum: 2^-9 relative (2^-8 where the fp32 sum's own
        # error, <= 1e-5 of the largest term, moves it across a rounding boundary)
        tol = exact.abs() * 2.0 ** -8 + 1e-5 * terms.abs().max()
        assert bool(((got - exact).abs() <= tol).all()), S
        # statistics: the ROUNDED residual's sum of squares per column tile; an fp32 sum
        # of <= 128 squares is within 128 * 2^-24 < 1e-5 of the exact one
        want = got.view(T, N // cols, cols).pow(2).sum(-1).t()
        torch.testing.assert_close(ss.cpu().double(), want, rtol=1e-5, atol=0)
        assert int(counters.abs().sum()) == 0, S   # every ticket winner re-arms its word
        # the partial rows behind it are the grouped kernel's; capacity tiles stay untouched
        assert rel_err(part.sum(0)[dest_d.long()], y[dest.long()].to(DEV)) < 1e-5, S
        assert bool(torch.isnan(part[:, offs[-1]:]).all()), S
