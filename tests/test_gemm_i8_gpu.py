"""gemm_i8 and quant_rows_int8 (the int8 instantiations of csrc/kernels/gemm_f8.hip) against float64 and
int64, on the helpers of _gemm_ref: exact answers on small-integer grids with power-of-two row and
channel scales at every cfg x mode, sums past 2^24 that only an integer accumulator gets right,
one-hot probes of all 256 codes on both sides, the row quantizer bit for bit against
quantize_rows_int8, one real-valued problem at a derived bound, and every refused shape."""
import math

import pytest
import torch

import _gemm_ref as G
from _row_ref import gen
from xgserve.ops import _native, linear as L
from xgserve.ops._native import stream_ptr

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
P, B, SI = G.MODE_PARTIAL, G.MODE_BF16, G.MODE_SILU
KT = L.F8_KT
SMALL = min(L.F8_CFGS, key=lambda c: L.F8_CFGS[c][0])


@pytest.fixture(scope="module")
def k():
    return _native.kernels()


def decode(q):
    return q.view(torch.int8).double()


def on_device(a, sx, q, sw):
    """Operands as the leading rows of allocations whose tails hold code 0x7F and NaN scales."""
    code = G.TAIL_CODE[G.INT8]
    return (G.with_tail(a, DEV, code), G.with_tail(sx[:, None], DEV), G.with_tail(q, DEV, code),
            G.with_tail(sw[:, None], DEV))


def launch(k, a, sx, q, sw, S, mode, cfg):
    """Two launches into fresh guarded buffers -> the interior result of the second."""
    (M, K), N = a.shape, q.shape[0]
    shape = (S, M, N) if mode == P else (M, N // 2 if mode == SI else N)
    first = None
    for _ in range(2):
        flat, res = G.guarded(shape, torch.float32 if mode == P else torch.bfloat16, DEV)
        part, out = (res.data_ptr(), 0) if mode == P else (0, res.data_ptr())
        k.gemm_i8(a.data_ptr(), sx.data_ptr(), M, K, q.data_ptr(), sw.data_ptr(), N, part, out, S, mode, cfg, stream_ptr())
        assert G.guards_intact(flat, math.prod(shape)), "wrote outside its output"
        assert first is None or torch.equal(first, flat), "two launches differ"
        first = flat
    return res


def int_slabs(a, sx, q, sw, S):
    """What the kernel is specified to store: per split the int64 sum, rounded once to fp32, times
    the row scale, times the channel scale (fp32 [S, M, N])."""
    ia, iw = a.view(torch.int8).long(), q.view(torch.int8).long()
    return torch.stack([(ia[:, lo * KT:hi * KT] @ iw[:, lo * KT:hi * KT].t()).double().float() * sx[:, None] * sw[None, :]
                        for lo, hi in G.split_ranges(a.shape[1] // KT, S)])


def grid_problem(M, N, K, mode):
    """Codes |j| <= 16 on both sides and power-of-two scales that differ between neighbouring rows:
    the integer sum stays below 2^24, so its float, the scaled slabs and their sum are all exact."""
    for attempt in range(64):
        g = gen("i8-grid", M, N, K, mode, attempt)
        va, vw = G._ints(g, (M, K), -16, 16), G._ints(g, (N, K), -16, 16)
        sx, sw = G.pow2_scales(g, G.INT8, M, K, 7), G.pow2_scales(g, G.INT8, N, K, 7)
        y = (va @ vw.t()) * sx.double()[:, None] * sw.double()[None, :]
        if mode == SI:
            ex = max(0, math.ceil(math.log2(max(float(y.abs().max()), 1.0) / G.SILU_MAX)))
            sx, y = sx * 2.0 ** -ex, y * 2.0 ** -ex
        share, ties = G.bf16_rounding_stats(y)
        if mode != B or (share >= 0.25 and ties >= 1):
            return G.encode(va, G.INT8), sx.float(), G.encode(vw, G.INT8), sw, y
    raise AssertionError("no draw exercises the bf16 rounding")


@pytest.mark.parametrize("mode", (P, B, SI), ids=lambda m: G.MODE_NAMES[m])
@pytest.mark.parametrize("cfg", sorted(L.F8_CFGS))
def test_exact(k, cfg, mode):
    bm, K = L.F8_CFGS[cfg][0], 5 * KT
    for M in (1, bm - 1, bm + 1, 2 * bm + 17):
        for N in (256, 768):
            a, sx, q, sw, y = grid_problem(M, N, K, mode)
            want = G.Want(G.Problem("quant", torch.zeros(M, K), y), mode, DEV)
            ops = on_device(a, sx, q, sw)
            for S in ((1, 3) if mode == P else (1,)):
                assert k.i8_supports(M, K, N, S, mode, cfg)
                want.check(launch(k, *ops, S, mode, cfg), f"cfg {cfg} M {M} N {N} S {S}")


@pytest.mark.parametrize("mode,S", ((P, 1), (P, 2), (B, 1)))
def test_saturated_sums_need_an_integer_accumulator(k, mode, S):
    """Every product is +-127 x 127 over 24 K tiles: |sum| = 49,548,288 > 2^24 (per split of two:
    24,774,144), and the running sums on the way there are not fp32 numbers."""
    M, N, K = 17, 256, 24 * KT
    a = torch.full((M, K), 127, dtype=torch.int8).view(torch.uint8)
    q = (127 * (1 - 2 * (torch.arange(N) % 2)))[:, None].expand(N, K).to(torch.int8).contiguous().view(torch.uint8)
    sx, sw = torch.ones(M), torch.ones(N)
    want = int_slabs(a, sx, q, sw, S)
    assert float(want.sum(0).abs().max()) == 127 * 127 * K > G.EXACT
    res = launch(k, *on_device(a, sx, q, sw), S, mode, SMALL)
    if mode == P:
        G.check_partial(res, G.slab_sum(want).to(DEV), f"saturated S {S}")
    else:
        G.check_bf16(res, G.round_bf16(want[0].double()).to(DEV), "saturated bf16")


@pytest.mark.parametrize("side", ("a", "w"))
def test_codes_one_hot(k, side):
    """One side's rows are unit vectors (code 1) at the first and last k and both sides of every
    K-tile (and split) boundary; the other side holds all 256 codes, -128 included, at each probed k."""
    M = N = 256
    K, S = 3 * KT, 2
    g = gen("i8-onehot", side)
    hot = [0, KT - 1, KT, 2 * KT - 1, 2 * KT, K - 1]
    rows = torch.arange(256)
    onehot = torch.zeros(256, K, dtype=torch.uint8)
    onehot[rows, torch.tensor(hot)[rows % len(hot)]] = 1
    full = torch.randint(0, 256, (256, K), generator=g).to(torch.uint8)
    for i, kk in enumerate(hot):   # every code at every probed k
        full[:, kk] = ((rows + 41 * i) % 256).to(torch.uint8)
    a, q = (onehot, full) if side == "a" else (full, onehot)
    sx, sw = G.pow2_scales(g, G.INT8, M, K, 7), G.pow2_scales(g, G.INT8, N, K, 7)
    y = (decode(a) @ decode(q).t()) * sx.double()[:, None] * sw.double()[None, :]
    assert torch.equal(y.float().double(), y) and float(y.min()) < 0 and -128 in decode(full)[:, hot]
    G.check_partial(launch(k, *on_device(a, sx, q, sw), S, P, SMALL), y.float().to(DEV), f"one-hot {side}")


@pytest.mark.parametrize("M", (1, 65, 300))
def test_quant_rows_bit_identical(k, M):
    K = 1024
    g = gen("i8-quant", M)
    x = (torch.randn(M, K, generator=g) * 2.0 ** torch.randint(-8, 4, (M, K), generator=g)).bfloat16()
    # row 0: holds 127 * 2^-3, so its scale is exactly 2^-3; the rest are that scale times every tie k + 1/2
    vals = torch.cat([torch.arange(127).double() + 0.5, torch.tensor([127.0])])
    vals = torch.cat([vals, -vals])[torch.arange(K) % 256] * 0.125
    x[0] = vals.bfloat16()
    assert torch.equal(x[0].double(), vals)
    if M > 2:
        x[1] = 0                       # the scale floor
        x[2, -1] = 2.0 ** 9            # the row maximum is its last element
    want_q, want_s = L.quantize_rows_int8(x)
    assert float(want_s[0]) == 0.125 and (M < 3 or bool(want_s[1] == torch.tensor(1e-12)))
    assert want_q[0, :4].view(torch.int8).tolist() == [0, 2, 2, 4]   # half to even, not away from zero
    flat_s, sx = G.guarded((M,), torch.float32, DEV)
    buf = torch.full((M + G.TAIL, K), 0xA5, dtype=torch.uint8, device=DEV)
    xd = x.to(DEV)
    k.quant_rows_int8(xd.data_ptr(), M, K, buf.data_ptr(), sx.data_ptr(), stream_ptr())
    assert torch.equal(buf[:M].cpu(), want_q), "codes differ from quantize_rows_int8"
    assert torch.equal(G.ibits(sx.cpu()), G.ibits(want_s)), "scales differ from quantize_rows_int8"
    assert bool((buf[M:] == 0xA5).all()) and G.guards_intact(flat_s, M), "wrote past row M"
    got = L.quant_rows_int8(xd)  # the wrapper
    assert torch.equal(got[0].cpu(), want_q) and torch.equal(G.ibits(got[1].cpu()), G.ibits(want_s))


def test_real_valued():
    """The integer sum is exact, so a slab carries one int-to-float rounding and two fp32 multiplies
    (3 x 2^-24 of its |a| |w|) and the slab-order sum at most 2^-24 per add: under 4 x 2^-23 |A| |W|."""
    M, N, K = 300, 768, 1024
    g = gen("i8-real", M, N, K)
    x = torch.randn(M, K, generator=g).bfloat16()
    q, sw = L.quantize_int8((torch.randn(N, K, generator=g) * 0.02).bfloat16())
    a, sx = L.quantize_rows_int8(x)
    av, wv = decode(a) * sx.double()[:, None], decode(q) * sw.double()[:, None]
    p = G.Problem("real", x, av @ wv.t(), q=q, scale=sw, fmt=G.INT8, bound=4 * 2.0 ** -23 * (av.abs() @ wv.abs().t()))
    for mode in (P, B, SI):
        got = L.i8_linear(x.to(DEV), q.to(DEV), sw.to(DEV), mode, plan=(3, 1) if mode == P else None)
        assert mode != P or got.S == 3
        share = G.Want(p, mode, DEV).check(got.part if mode == P else got, G.MODE_NAMES[mode])
        print(f"gemm_i8 real {G.MODE_NAMES[mode]}: {share:.3f} of the bound")


def test_refusals(k):
    M, N, K = 64, 256, 3 * KT
    a = torch.zeros(M, K, dtype=torch.uint8, device=DEV)
    q = torch.zeros(N + 64, K, dtype=torch.uint8, device=DEV)
    sx, sw = torch.ones(M, device=DEV), torch.ones(N + 64, device=DEV)
    flat, res = G.guarded((4, M, N + 64), torch.float32, DEV)
    ptrs = [a.data_ptr(), sx.data_ptr(), q.data_ptr(), sw.data_ptr(), res.data_ptr()]
    big = L.I8_MAX_K + KT
    assert k.i8_supports(M, L.I8_MAX_K, N, 1, P, 0) and L._i8_valid(M, N, L.I8_MAX_K, P, 1, 0) and k.f8_supports(M, big, N, 1, P, 0)
    # N % 256, K % 128, more splits than K tiles, S > 1 without partials, M = 0, unknown cfg / mode, sums past int32
    for m, kk, n, S, mode, cfg in [(M, K, N + 64, 1, P, 0), (M, K - 64, N, 1, P, 0), (M, K, N, 4, P, 0), (M, K, N, 2, B, 0),
                                   (M, K, N, 2, SI, 0), (0, K, N, 1, P, 0), (M, K, N, 1, P, len(L.F8_CFGS)),
                                   (M, K, N, 1, P, -1), (M, K, N, 1, 3, 0), (M, big, N, 1, P, 0)]:
        assert not k.i8_supports(m, kk, n, S, mode, cfg) and not L._i8_valid(m, n, kk, mode, S, cfg)
        with pytest.raises(ValueError):
            k.gemm_i8(ptrs[0], ptrs[1], m, kk, ptrs[2], ptrs[3], n, ptrs[4], ptrs[4], S, mode, cfg, stream_ptr())
    for null in range(5):   # a, sx, w, sw, the mode's output
        p = [0 if i == null else v for i, v in enumerate(ptrs)]
        with pytest.raises(ValueError):
            k.gemm_i8(p[0], p[1], M, K, p[2], p[3], N, p[4], 0, 1, P, 0, stream_ptr())
    out = torch.empty(M, 2 * N, dtype=torch.bfloat16, device=DEV)
    # scale sizes, dtypes, non-contiguous operands and outputs, plans, modes, shapes
    for kw in [dict(sx=sx[:-1]), dict(sw=sw), dict(a=a.float()), dict(a=a.t().contiguous().t()),
               dict(mode=B, out=out[:, ::2]), dict(mode=B, out=out[:, :N].float()), dict(plan=(4, 0)),
               dict(plan=(1, 7)), dict(mode=5), dict(q=q)]:
        with pytest.raises(ValueError):
            L.i8_linear_codes(**{**dict(a=a, sx=sx, q=q[:N], sw=sw[:N], mode=P), **kw})
    with pytest.raises(ValueError):
        L.i8_linear(torch.zeros(M, K - 64, dtype=torch.bfloat16, device=DEV), q[:N, :K - 64].contiguous(), sw[:N])
    torch.cuda.synchronize()
    assert bool((G.ibits(res) == G.SENT32).all()) and G.guards_intact(flat, res.numel()), "a refused call wrote"
