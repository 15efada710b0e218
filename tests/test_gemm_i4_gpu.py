"""gemm_i4 (csrc/kernels/gemm_i4.hip) and quant_rows_int8_i4 against float64 on the helpers of _gemm_ref:
one-hot rows at every k, exact full-range integer grids, the quantizer bit for bit, a derived bound, refusals."""
import math

import pytest
import torch

import _gemm_ref as G
from _row_ref import gen
from xgserve.ops import _native, linear as L
from xgserve.ops._native import stream_ptr

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
P, B, SI, KT = G.MODE_PARTIAL, G.MODE_BF16, G.MODE_SILU, L.F8_KT


def product(va, sx, vq, gs):   # float64 [M, N] of code values va [M, K], vq [N, K], row and group scales
    return (va.double() * sx.double()[:, None]) @ (vq.double() * G.scale_matrix(gs, G.INT4, va.shape[1])).t()


def on_device(va, sx, vq, gs):   # as the kernel reads them, the leading rows of allocations with poisoned tails
    return (G.with_tail(L.i4_order(G.encode(va, G.INT8)), DEV, 0x7F), G.with_tail(sx[:, None].float(), DEV),
            G.with_tail(G.pack_int4(vq), DEV, 0xFF), G.with_tail(gs, DEV))


def launch(a, sx, q, gs, S, mode, cfg):
    (M, K), N, k = a.shape, q.shape[0], _native.kernels()
    shape = (S, M, N) if mode == P else (M, N // 2 if mode == SI else N)
    flat, res = G.guarded(shape, torch.float32 if mode == P else torch.bfloat16, DEV)
    part, out = (res.data_ptr(), 0) if mode == P else (0, res.data_ptr())
    k.gemm_i4(a.data_ptr(), sx.data_ptr(), M, K, q.data_ptr(), gs.data_ptr(), N, part, out, S, mode, cfg, stream_ptr())
    assert G.guards_intact(flat, math.prod(shape)), "wrote outside its output"
    return res


@pytest.mark.parametrize("kind,S", (("order", 1), ("pairs", 2)))
@pytest.mark.parametrize("cfg", sorted(L.I4_CFGS))
def test_one_hot(cfg, kind, S):
    """order: row m of A is one-hot at k = m, so out[m, n] = q[n, m] gs[m // 128, n] sx[m]: permutation, nibble
    order, sign, factor 16, the scale's group and column. pairs: row m holds code m - 128 (all 256) at one k on
    either side of a K-tile or split boundary. The 256 columns hold all 16 weight codes at every k."""
    K, g, rows = (256, gen("i4-order"), torch.arange(256)) if kind == "order" else (3 * KT, gen("i4-pairs"), torch.arange(256))
    hot = rows if kind == "order" else torch.tensor([0, KT - 1, KT, 2 * KT - 1, 2 * KT, K - 1])[rows % 6]
    va = torch.zeros(256, K, dtype=torch.int64)
    va[rows, hot] = 1 if kind == "order" else rows - 128
    vq = (5 * torch.arange(K)[None, :] + rows[:, None]) % 16 - 8
    sx, gs = G.pow2_scales(g, G.INT8, 256, K, 7), G.pow2_scales(g, G.INT4, 256, K, 5)
    y = product(va, sx, vq, gs)
    assert torch.equal(y.float().double(), y) and float(y.min()) < 0 < float(y.max())
    G.check_partial(launch(*on_device(va, sx, vq, gs), S, P, cfg), y.float().to(DEV), f"{kind} cfg {cfg}")


@pytest.mark.parametrize("mode", (P, B, SI), ids=lambda m: G.MODE_NAMES[m])
@pytest.mark.parametrize("cfg", sorted(L.I4_CFGS))
def test_exact(cfg, mode):
    """a in -127..127, q in -8..7, group scales 2^0..2^-2, row scales 2^0..2^-6: a running sum stays below 2^20 in
    units of 2^-2 times a row's power of two: exact. K: one tile, fewer tiles than the ring, uneven splits."""
    bm, ns = L.I4_CFGS[cfg]
    for M, N, K in ((1, 256, KT), (bm - 1, 512, 3 * KT), (bm + 1, 256, KT * (ns + 2))):
        g = gen("i4-grid", M, N, K, mode)
        va, vq = G._ints(g, (M, K), -127, 127), G._ints(g, (N, K), -8, 7)
        sx, gs = G.pow2_scales(g, G.INT8, M, K, 7), G.pow2_scales(g, G.INT4, N, K, 3)
        y = product(va, sx, vq, gs)
        if mode == SI:   # the SiLU tolerance rule of test_gemm_f8_gpu: |y| <= SILU_MAX, SILU_RTOL of the reference
            ex = max(0, math.ceil(math.log2(max(float(y.abs().max()), 1.0) / G.SILU_MAX)))
            sx, y = sx * 2.0 ** -ex, y * 2.0 ** -ex
        assert torch.equal(y.float().double(), y) and (mode != B or G.bf16_rounding_stats(y)[0] >= 0.25)
        want, ops = G.Want(G.Problem("quant", torch.zeros(M, K), y), mode, DEV), on_device(va, sx, vq, gs)
        for S in ((1, 2, 3) if mode == P else (1,)):
            if S <= K // KT:
                want.check(launch(*ops, S, mode, cfg), f"cfg {cfg} M {M} N {N} K {K} S {S}")


@pytest.mark.parametrize("K", (16, 144, 28672))
def test_quant_rows_bit_identical(K):
    g = gen("i4-quant", K)
    x = (torch.randn(3, K, generator=g) * 2.0 ** torch.randint(-8, 4, (3, K), generator=g)).bfloat16()
    x[0] = ((torch.arange(K) % 16).double() + 0.5).mul(0.125).bfloat16()   # exact .5 ties at scale 2^-3 ...
    x[0, -1] = 127 * 0.125                                                 # ... which this maximum sets
    x[1] = 0                                                               # the scale floor
    x[2] = -x[2].abs() - 1                                                 # the row's maximum is negative
    nat, want_s = L.quantize_rows_int8(x)
    assert float(want_s[0]) == 0.125 and nat[0, :4].view(torch.int8).tolist() == [0, 2, 2, 4]   # half to even
    got_q, got_s = L.quant_rows_int8_i4(x.to(DEV))
    assert torch.equal(got_q.cpu(), L.i4_order(nat)) and torch.equal(G.ibits(got_s.cpu()), G.ibits(want_s))


def test_real_valued():
    """A group's integer sum and its float are exact (|16 sum| < 2^22). Each of the K / 128 folds, the row scale and
    each further slab round once: K / 128 + S <= K / 128 + 3 roundings of 2^-24 of values bounded by |A| |W|, + 1 for second order."""
    M, N, K = 300, 768, 1024
    g = gen("i4-real", M, N, K)
    x = torch.randn(M, K, generator=g).bfloat16()
    q, gs = L.quantize_int4((torch.randn(N, K, generator=g) * 0.02).bfloat16())
    a, sx = L.quantize_rows_int8(x)
    av, wv = a.view(torch.int8).double() * sx.double()[:, None], L.dequantize_int4(q, gs).double()
    p = G.Problem("real", x, av @ wv.t(), q=q, scale=gs, fmt=G.INT4, bound=(K // KT + 4) * 2.0 ** -24 * (av.abs() @ wv.abs().t()))
    for mode in (P, B, SI):
        got = L.i4_linear(x.to(DEV), q.to(DEV), gs.to(DEV), mode, plan=(3, 1) if mode == P else None)
        print("share of the bound", G.MODE_NAMES[mode], G.Want(p, mode, DEV).check(got.part if mode == P else got, G.MODE_NAMES[mode]))


def test_refusals():
    (M, N, K), k = (64, 256, 3 * KT), _native.kernels()
    a = torch.zeros(M, K, dtype=torch.uint8, device=DEV)
    q = torch.zeros(N + 64, K // 2, dtype=torch.uint8, device=DEV)
    sx, gs = torch.ones(M, device=DEV), torch.ones(K // KT, N, device=DEV)
    res = torch.empty(4, M, N + 64, device=DEV)
    ptrs = [a.data_ptr(), sx.data_ptr(), q.data_ptr(), gs.data_ptr(), res.data_ptr()]
    # K % 128, N % 256, more splits than K tiles, bf16 at split 2; then a, w, gs and part off 16 B
    cases = [(K - 64, N, 1, P, ptrs), (K, N + 64, 1, P, ptrs), (K, N, 4, P, ptrs), (K, N, 2, B, ptrs)]
    cases += [(K, N, 1, P, [v + 4 * (j == i) for j, v in enumerate(ptrs)]) for i in (0, 2, 3, 4)]
    for kk, n, S, mode, p in cases:
        assert k.i4_supports(M, kk, n, S, mode, 0) == L._i4_valid(M, n, kk, mode, S, 0) == (p is not ptrs)
        with pytest.raises(ValueError):
            k.gemm_i4(p[0], p[1], M, kk, p[2], p[3], n, p[4], p[4], S, mode, 0, stream_ptr())
    out = torch.empty(M, N // 2, dtype=torch.bfloat16, device=DEV)
    for kw in (dict(gs=gs[1:]), dict(mode=B, out=out)):   # a wrong scale count, an out of the wrong shape
        with pytest.raises(ValueError):
            L.i4_linear_codes(**{**dict(a=a, sx=sx, q=q[:N], gs=gs, mode=P), **kw})
