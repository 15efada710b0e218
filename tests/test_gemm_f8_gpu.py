"""gemm_f8 and quant_rows_fp8 (csrc/kernels/gemm_f8.hip) against float64, on the helpers of _gemm_ref:
exact answers on E4M3 grids with power-of-two row and channel scales at every cfg x mode, one-hot
probes of every code on both sides, the row quantizer bit for bit against quantize_rows_fp8, one
real-valued problem at the fp32 worst-case bound, and every refused shape."""
import math

import pytest
import torch

import _gemm_ref as G
from _row_ref import gen
from xgserve.ops import _native, linear as L
from xgserve.ops._native import stream_ptr

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MODES = (G.MODE_PARTIAL, G.MODE_BF16, G.MODE_SILU)
KT = L.F8_KT


@pytest.fixture(scope="module")
def k():
    return _native.kernels()


def decode(q):
    return q.view(torch.float8_e4m3fn).double()


def launch(k, a, sx, q, sw, M, N, K, S, mode, cfg):
    """Two launches into fresh guarded buffers -> the interior result of the second."""
    shape = (S, M, N) if mode == G.MODE_PARTIAL else (M, N // 2 if mode == G.MODE_SILU else N)
    first = None
    for _ in range(2):
        flat, res = G.guarded(shape, torch.float32 if mode == G.MODE_PARTIAL else torch.bfloat16, DEV)
        part, out = (res.data_ptr(), 0) if mode == G.MODE_PARTIAL else (0, res.data_ptr())
        k.gemm_f8(a.data_ptr(), sx.data_ptr(), M, K, q.data_ptr(), sw.data_ptr(), N, part, out, S, mode, cfg,
                  stream_ptr())
        assert G.guards_intact(flat, math.prod(shape)), "wrote outside its output"
        assert first is None or torch.equal(first, flat), "two launches differ"
        first = flat
    return res


def on_device(a, sx, q, sw):
    """Operands as the leading rows of allocations whose tails hold code 0x7E and NaN scales."""
    code = G.TAIL_CODE[G.FP8]
    return (G.with_tail(a, DEV, code), G.with_tail(sx[:, None], DEV), G.with_tail(q, DEV, code),
            G.with_tail(sw[:, None], DEV))


def grid_problem(M, N, K, mode):
    """E4M3 values j / 2, |j| <= 16, on both sides; power-of-two scales that differ between
    neighbouring rows. Returns codes, scales and the exact float64 result."""
    for attempt in range(64):
        g = gen("f8-grid", M, N, K, mode, attempt)
        va, vw = G._ints(g, (M, K), -16, 16) / 2, G._ints(g, (N, K), -16, 16) / 2
        for smod in (7, 4, 2):
            sx = G.pow2_scales(g, G.FP8, M, K, smod)
            sw = G.pow2_scales(g, G.FP8, N, K, smod)
            units = ((va.abs() * sx.double()[:, None]) @ (vw.abs() * sw.double()[:, None]).t()).max()
            if float(units) / float(sx.min() * sw.min()) * 4 < G.EXACT:  # products are multiples of 1/4
                break
        assert float(units) / float(sx.min() * sw.min()) * 4 < G.EXACT
        y = (va @ vw.t()) * sx.double()[:, None] * sw.double()[None, :]
        if mode == G.MODE_SILU:
            ex = max(0, math.ceil(math.log2(max(float(y.abs().max()), 1.0) / G.SILU_MAX)))
            sx, y = sx * 2.0 ** -ex, y * 2.0 ** -ex
        if mode != G.MODE_BF16:
            break
        share, ties = G.bf16_rounding_stats(y)
        if share >= 0.25 and ties >= 1:
            break
    else:
        raise AssertionError("no draw exercises the bf16 rounding")
    return G.encode(va, G.FP8), sx.float(), G.encode(vw, G.FP8), sw, y


@pytest.mark.parametrize("mode", MODES, ids=lambda m: G.MODE_NAMES[m])
@pytest.mark.parametrize("cfg", sorted(L.F8_CFGS))
def test_exact(k, cfg, mode):
    bm, slots = L.F8_CFGS[cfg]
    K = KT * (5 if slots <= 3 else (slots + 2) | 1)
    for M in (1, bm - 1, bm + 1, 2 * bm + 17):
        for N in (256, 768):
            a, sx, q, sw, y = grid_problem(M, N, K, mode)
            p = G.Problem("quant", torch.zeros(M, K), y)
            want = G.Want(p, mode, DEV)
            ops = on_device(a, sx, q, sw)
            for S in ((1, 3) if mode == G.MODE_PARTIAL else (1,)):
                assert k.f8_supports(M, K, N, S, mode, cfg)
                want.check(launch(k, *ops, M, N, K, S, mode, cfg), f"cfg {cfg} M {M} N {N} S {S}")


@pytest.mark.parametrize("side", ("a", "w"))
def test_codes_one_hot(k, side):
    """One side's rows are unit vectors (code 0x38 = 1.0) at the first and last k and both sides of
    every K-tile (and split) boundary; the other side holds all 254 non-NaN codes at each probed k."""
    cfg, M, N, K, S = min(L.F8_CFGS, key=lambda c: L.F8_CFGS[c][0]), 256, 256, 3 * KT, 2
    g = gen("f8-onehot", side)
    hot = [0, KT - 1, KT, 2 * KT - 1, 2 * KT, K - 1]
    codes = torch.tensor([c for c in range(256) if c & 0x7F != 0x7F], dtype=torch.uint8)
    onehot = torch.zeros(256, K, dtype=torch.uint8)
    rows = torch.arange(256)
    onehot[rows, torch.tensor(hot)[rows % len(hot)]] = 0x38
    full = codes[torch.randint(0, 254, (256, K), generator=g)]
    for i, kk in enumerate(hot):   # every code at every probed k (256 rows >= 254 codes)
        full[:, kk] = codes[(rows + 41 * i) % 254]
    a, q = (onehot, full) if side == "a" else (full, onehot)
    sx, sw = G.pow2_scales(g, G.FP8, M, K, 7), G.pow2_scales(g, G.FP8, N, K, 7)
    y = (decode(a) @ decode(q).t()) * sx.double()[:, None] * sw.double()[None, :]
    res = launch(k, *on_device(a, sx, q, sw), M, N, K, S, G.MODE_PARTIAL, cfg)
    G.check_partial(res, y.float().to(DEV), f"one-hot {side}")
    assert torch.equal(y.float().double(), y)


@pytest.mark.parametrize("M", (1, 65, 300))
def test_quant_rows_bit_identical(k, M):
    K = 1024
    g = gen("f8-quant", M)
    x = (torch.randn(M, K, generator=g) * 2.0 ** torch.randint(-8, 4, (M, K), generator=g)).bfloat16()
    # row 0: holds 448 * 2^-3, so its scale is exactly 2^-3; the rest are that scale times the ties
    # between neighbouring E4M3 values (the subnormal range included), subnormals, and +-448
    e4 = torch.arange(0, 127, dtype=torch.uint8).view(torch.float8_e4m3fn).double()  # 0 .. 448 ascending
    vals = torch.cat([(e4[:-1] + e4[1:]) / 2, e4[:9], torch.tensor([448.0])])
    vals = torch.cat([vals, -vals])
    x[0] = (vals[torch.arange(K) % len(vals)] * 0.125).bfloat16()
    assert torch.equal(x[0].double(), vals[torch.arange(K) % len(vals)] * 0.125) and float(x[0].abs().max()) == 56.0
    if M > 2:
        x[1] = 0                       # the scale floor
        x[2, -1] = 2.0 ** 9            # the row maximum is its last element
    want_q, want_s = L.quantize_rows_fp8(x)
    assert float(want_s[0]) == 0.125 and (M < 3 or bool(want_s[1] == torch.tensor(1e-12)))
    flat_s, sx = G.guarded((M,), torch.float32, DEV)
    buf = torch.full((M + G.TAIL, K), 0xA5, dtype=torch.uint8, device=DEV)
    xd = x.to(DEV)
    k.quant_rows_fp8(xd.data_ptr(), M, K, buf.data_ptr(), sx.data_ptr(), stream_ptr())
    assert torch.equal(buf[:M].cpu(), want_q), "codes differ from quantize_rows_fp8"
    assert torch.equal(G.ibits(sx.cpu()), G.ibits(want_s)), "scales differ from quantize_rows_fp8"
    assert bool((buf[M:] == 0xA5).all()) and G.guards_intact(flat_s, M), "wrote past row M"
    got = L.quant_rows_fp8(xd)  # the wrapper
    assert torch.equal(got[0].cpu(), want_q) and torch.equal(G.ibits(got[1].cpu()), G.ibits(want_s))


def test_real_valued():
    M, N, K = 300, 768, 1024
    g = gen("f8-real", M, N, K)
    x = torch.randn(M, K, generator=g).bfloat16()
    q, sw = L.quantize_fp8((torch.randn(N, K, generator=g) * 0.02).bfloat16())
    a, sx = L.quantize_rows_fp8(x)
    av, wv = decode(a) * sx.double()[:, None], decode(q) * sw.double()[:, None]
    y = av @ wv.t()
    # fp32 accumulation in any order, plus the two scale multiplies
    p = G.Problem("real", x, y, q=q, scale=sw, fmt=G.FP8, bound=(K + 4) * 2.0 ** -23 * (av.abs() @ wv.abs().t()))
    for mode in MODES:
        got = L.f8_linear(x.to(DEV), q.to(DEV), sw.to(DEV), mode, plan=(3, 1) if mode == G.MODE_PARTIAL else None)
        res = got.part if mode == G.MODE_PARTIAL else got
        assert mode != G.MODE_PARTIAL or got.S == 3
        share = G.Want(p, mode, DEV).check(res, G.MODE_NAMES[mode])
        print(f"gemm_f8 real {G.MODE_NAMES[mode]}: {share:.3f} of the bound")


def test_refusals(k):
    M, N, K = 64, 256, 3 * KT
    a = torch.zeros(M, K, dtype=torch.uint8, device=DEV)
    q = torch.zeros(N + 64, K, dtype=torch.uint8, device=DEV)
    sx, sw = torch.ones(M, device=DEV), torch.ones(N + 64, device=DEV)
    P, B, SI = G.MODE_PARTIAL, G.MODE_BF16, G.MODE_SILU
    flat, res = G.guarded((4, M, N + 64), torch.float32, DEV)
    ptrs = [a.data_ptr(), sx.data_ptr(), q.data_ptr(), sw.data_ptr(), res.data_ptr()]
    # N % 256, K % 128, more splits than K tiles, S > 1 without partials, M = 0, unknown cfg / mode
    for m, kk, n, S, mode, cfg in [(M, K, N + 64, 1, P, 0), (M, K - 64, N, 1, P, 0), (M, K, N, 4, P, 0), (M, K, N, 2, B, 0),
                                   (M, K, N, 2, SI, 0), (0, K, N, 1, P, 0), (M, K, N, 1, P, len(L.F8_CFGS)),
                                   (M, K, N, 1, P, -1), (M, K, N, 1, 3, 0)]:
        assert not k.f8_supports(m, kk, n, S, mode, cfg) and not L._f8_valid(m, n, kk, mode, S, cfg)
        with pytest.raises(ValueError):
            k.gemm_f8(ptrs[0], ptrs[1], m, kk, ptrs[2], ptrs[3], n, ptrs[4], ptrs[4], S, mode, cfg, stream_ptr())
    for null in range(5):   # a, sx, w, sw, the mode's output
        p = [0 if i == null else v for i, v in enumerate(ptrs)]
        with pytest.raises(ValueError):
            k.gemm_f8(p[0], p[1], M, K, p[2], p[3], N, p[4], 0, 1, P, 0, stream_ptr())
    out = torch.empty(M, 2 * N, dtype=torch.bfloat16, device=DEV)
    # scale sizes, dtypes, non-contiguous operands and outputs, plans, modes, shapes
    for kw in [dict(sx=sx[:-1]), dict(sw=sw), dict(a=a.float()), dict(a=a.t().contiguous().t()),
               dict(mode=B, out=out[:, ::2]), dict(mode=B, out=out[:, :N].float()), dict(plan=(4, 0)),
               dict(plan=(1, 7)), dict(mode=5), dict(q=q)]:
        with pytest.raises(ValueError):
            L.f8_linear_codes(**{**dict(a=a, sx=sx, q=q[:N], sw=sw[:N], mode=P), **kw})
    with pytest.raises(ValueError):
        L.f8_linear(torch.zeros(M, K - 64, dtype=torch.bfloat16, device=DEV), q[:N, :K - 64].contiguous(), sw[:N])
    torch.cuda.synchronize()
    assert bool((G.ibits(res) == G.SENT32).all()) and G.guards_intact(flat, res.numel()), "a refused call wrote"
