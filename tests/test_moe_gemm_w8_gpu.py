"""moe_gemm_w8 (csrc/kernels/moe_gemm_w8.hip), the grouped GEMM on fp8 / int8 / int4 expert
codes, called directly at every format x configuration x epilogue, and through fused_moe.

The layouts of tests/test_moe_gemm_gpu.py: real rows per expert that reach the 16-, 32- and
64-row bodies, an empty expert, an expert of three row tiles (temporal weight loads) and two
capacity tiles past the last segment; both x forms and both `valid` forms; K and S giving 1,
2 and 0 / 1 / 2 mod 3 chunks. Outputs start as NaN. Real rows are compared with float64 on
the CPU (x times dequantize_weight of the row's expert) and, with K rotation off, with the
dense gemm_w8 on the same rows and that expert's codes: bit for bit for fp8 / int8 (same
chunk order, MFMA sequence and scale multiply), within twice its error for int4 (the fold
here is explicit fmaf). Tiles without a real row must keep the NaN."""
import pytest
import torch

from xgserve import tune
from xgserve.ops import _native, fused_moe, moe_forward_ref
from xgserve.ops._native import stream_ptr
from xgserve.ops.linear import (MODE_PARTIAL, MODE_SILU, WQ_FP8, WQ_INT4, WQ_INT8, dequantize_weight,
                                quantize_expert_stack)
from xgserve.ops.moe import MOE_W8_GEOM

pytestmark = pytest.mark.gpu
DEV = "cuda"
N, E, PAD_TILES = 256, 5, 2
LAYOUTS = {16: (5, 0, 16, 1, 9), 64: (5, 0, 20, 40, 150)}  # max_rows -> real rows per expert
KS = ((1, 1), (3, 1), (4, 1), (5, 1), (4, 2), (6, 2))          # (K / KC, S)
FMTS = {"fp8": WQ_FP8, "int8": WQ_INT8, "int4": WQ_INT4}
MODES = {"partial": MODE_PARTIAL, "silu": MODE_SILU}
BOUND = {WQ_FP8: 1e-5, WQ_INT8: 1e-5, WQ_INT4: 2e-3}          # summed partials; SiLU rows: 1e-2


def rel_err(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-6))


class Layout:
    """Block-64 padded expert-sorted layout of `real` rows per expert, built by hand."""

    def __init__(self, real, gen):
        self.T = sum(real)
        offs, rows, src, self.tiles = [0], [], torch.randperm(self.T, generator=gen).tolist(), []
        for e, n in enumerate(real):
            seg = -(-n // 64) * 64
            rows += src[:n] + [-1] * (seg - n)
            src = src[n:]
            self.tiles += [(offs[-1] + 64 * t, min(64, n - 64 * t), e) for t in range(seg // 64)]  # (row, real, expert)
            offs.append(offs[-1] + seg)
        self.end, self.P = offs[-1], offs[-1] + 64 * PAD_TILES
        self.rows_cpu = torch.tensor(rows + [-1] * (64 * PAD_TILES), dtype=torch.int32)
        self.rows, self.offs = self.rows_cpu.to(DEV), torch.tensor(offs, dtype=torch.int32, device=DEV)
        self.real_idx = (self.rows_cpu >= 0).nonzero()[:, 0].to(DEV)
        self.expert_of = torch.repeat_interleave(torch.arange(E), torch.tensor(offs).diff())


class Case:
    """Inputs of one (layout, K, format) and their float64 reference, made once per module."""

    def __init__(self, lay, K, fmt, gen):
        self.lay, self.K, self.fmt = lay, K, fmt
        x = torch.randn(lay.T, K, generator=gen).bfloat16()
        q, sc = quantize_expert_stack(torch.randn(E, N, K, generator=gen) * 0.05, fmt)
        xp = torch.randn(lay.P, K, generator=gen).bfloat16()  # pad rows: finite, never compared
        real = lay.rows_cpu >= 0
        xp[real] = x[lay.rows_cpu[real].long()]
        y = torch.zeros(lay.P, N, dtype=torch.float64)
        for e in range(E):
            seg = torch.zeros(lay.P, dtype=torch.bool)
            seg[:lay.end] = lay.expert_of == e
            y[seg] = xp[seg].double() @ dequantize_weight(q[e], sc[e], fmt).double().t()
        g, u = y.view(lay.P, N // 32, 2, 16)[:, :, 0], y.view(lay.P, N // 32, 2, 16)[:, :, 1]
        self.ref = y[real].to(DEV)
        self.ref_silu = (torch.nn.functional.silu(g) * u).reshape(lay.P, N // 2)[real].to(DEV)
        self.x, self.xp, self.q, self.sc = x.to(DEV), xp.to(DEV), q.to(DEV), sc.to(DEV)


@pytest.fixture(scope="module")
def cases():
    k = _native.kernels()
    k.set_k_rotation(0)  # dense and grouped walk the K chunks in the same order
    gen = torch.Generator().manual_seed(0)
    lays = {real: Layout(real, gen) for real in LAYOUTS.values()}
    made = {}

    def get(max_rows, K, fmt):
        key = (LAYOUTS[max_rows], K, fmt)
        if key not in made:
            made[key] = Case(lays[key[0]], K, fmt, gen)
        return made[key]

    yield get
    k.set_k_rotation(tune.get_int("krot", 1))


def grouped(c, cfg, mode, S, max_rows, gather=True, use_valid=True, fmt=None):
    """One moe_gemm_w8 launch into NaN-filled buffers -> the written tensor [(S,) P, cols]."""
    lay = c.lay
    part = torch.full((S, lay.P, N), float("nan"), device=DEV)
    out = torch.full((lay.P, N // 2), float("nan"), device=DEV, dtype=torch.bfloat16)
    _native.kernels().moe_gemm_w8(
        (c.x if gather else c.xp).data_ptr(), lay.rows.data_ptr() if gather else 0, lay.offs.data_ptr(), E,
        c.K, c.q.data_ptr(), c.sc.data_ptr(), N, lay.P, part.data_ptr() if mode == MODE_PARTIAL else 0,
        0 if mode == MODE_PARTIAL else out.data_ptr(), S, mode, cfg, c.fmt if fmt is None else fmt, max_rows,
        stream_ptr(), lay.rows.data_ptr() if use_valid else 0, 0)
    return part if mode == MODE_PARTIAL else out


def dense_rows(c, cfg, mode, S):
    """The dense gemm_w8 on every tile's real rows and its expert's codes, in padded-row order."""
    got = []
    for p0, n, e in c.lay.tiles:
        part = torch.empty(S, n, N, device=DEV)
        out = torch.empty(n, N // 2, device=DEV, dtype=torch.bfloat16)
        _native.kernels().gemm_w8(c.xp[p0:p0 + n].data_ptr(), n, c.K, c.q[e].data_ptr(), c.sc[e].data_ptr(), N,
                                  part.data_ptr(), out.data_ptr(), S, mode, cfg, stream_ptr(), c.fmt)
        got.append(part if mode == MODE_PARTIAL else out)
    return torch.cat(got, dim=-2)


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("cfg", list(MOE_W8_GEOM))
@pytest.mark.parametrize("kind", list(FMTS))
def test_moe_gemm_w8_every_instantiation(cases, kind, cfg, mode):
    fmt, md, (nw, _, kc) = FMTS[kind], MODES[mode], MOE_W8_GEOM[cfg]
    for max_rows in LAYOUTS:
        if max_rows > 16 and kc != 128:
            continue  # the KC 256 configurations have the 16-row body only
        for nk, S in KS:
            c = cases(max_rows, nk * kc, fmt)
            if md == MODE_SILU and (nw != 2 or S != 1):
                with pytest.raises(ValueError):
                    grouped(c, cfg, md, S, max_rows)
                continue
            dense, ref = dense_rows(c, cfg, md, S), c.ref_silu if md == MODE_SILU else c.ref
            dense = dense.sum(0) if md == MODE_PARTIAL and fmt == WQ_INT4 else dense
            for gather in (True, False):
                for use_valid in (True, False):
                    tag = (max_rows, nk * kc, S, gather, use_valid)
                    got = grouped(c, cfg, md, S, max_rows, gather, use_valid)
                    real = got.index_select(-2, c.lay.real_idx)
                    val = real.sum(0) if md == MODE_PARTIAL else real
                    err = rel_err(val, ref)
                    print(tag, kind, mode, "rel_err", err)
                    assert err < (BOUND[fmt] if md == MODE_PARTIAL else 1e-2), tag
                    if fmt == WQ_INT4:
                        derr = rel_err(dense, ref)
                        print(tag, "dense gemm_w8 rel_err", derr)
                        assert err <= 2 * derr, tag
                    else:
                        assert torch.equal(real, dense), tag
                    assert bool(torch.isnan(got[..., c.lay.end:, :]).all()), tag


def test_moe_gemm_w8_refuses_bad_operands(cases):
    c = cases(64, 512, WQ_FP8)
    for bad in (dict(cfg=5), dict(cfg=0, fmt=3), dict(cfg=0, S=3), dict(cfg=0, mode=MODE_SILU, S=2),
                dict(cfg=3)):                                   # the last: KC 256 at max_rows 64
        kw = dict(dict(mode=MODE_PARTIAL, S=1, max_rows=64), **bad)
        with pytest.raises(ValueError):
            grouped(c, **kw)
    # int4 scales that do not fit: 33 groups x 128 columns > WQ_SC_FLOATS (real operands of that shape)
    big = Case(c.lay, 33 * 128, WQ_INT4, torch.Generator().manual_seed(1))
    with pytest.raises(ValueError):
        grouped(big, 0, MODE_PARTIAL, 1, 64)
    assert bool(torch.isfinite(grouped(big, 1, MODE_PARTIAL, 1, 64)[0, :c.lay.end][c.lay.rows[:c.lay.end] >= 0]).all())


@pytest.mark.parametrize("T", [1, 8, 64])
@pytest.mark.parametrize("kind", list(FMTS))
def test_fused_moe_on_codes_matches_the_reference(kind, T):
    """fused_moe(wq=...) against moe_forward_ref on the dequantized weights, routing given
    (no ties): both round the activation to bf16, the output is one bf16 rounding of an fp32 sum."""
    fmt, H, F, Ex, k = FMTS[kind], 512, 512, 8, 2
    gen = torch.Generator().manual_seed(3)
    x = torch.randn(T, H, generator=gen).bfloat16().to(DEV)
    w13, w2 = torch.randn(Ex, 2 * F, H, generator=gen) * 0.05, torch.randn(Ex, H, F, generator=gen) * 0.05
    ids = torch.stack([torch.randperm(Ex, generator=gen)[:k] for _ in range(T)]).to(torch.int32).to(DEV)
    wts = (torch.rand(T, k, generator=gen) + 0.25).to(DEV)
    (q13, s13), (q2, s2) = quantize_expert_stack(w13.to(DEV), fmt), quantize_expert_stack(w2.to(DEV), fmt)
    d13 = torch.stack([dequantize_weight(q13[e], s13[e], fmt) for e in range(Ex)])
    d2 = torch.stack([dequantize_weight(q2[e], s2[e], fmt) for e in range(Ex)])
    got = fused_moe(x, d13.bfloat16(), d2.bfloat16(), wts, ids, wq=(q13, s13, q2, s2, fmt))
    err = rel_err(got, moe_forward_ref(x, d13, d2, wts, ids))
    print(kind, T, "fused_moe rel_err", err)
    assert err < 2e-2
