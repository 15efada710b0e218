"""moe_gemm_f8 (the grouped form of csrc/kernels/gemm_f8.hip) against float64 by the method of
test_gemm_f8_gpu.py: E4M3 grid codes and power-of-two scales whose fp32 sums are exact, so split-K partials
compare exactly and the SiLU gate within one bf16 rounding. The layout is moe_align's by hand: an empty expert,
a one-row segment (63 pads), a full tile and a tile plus one row, in a shuffled expert order."""
import functools
import math

import pytest
import torch

import _gemm_ref as G
from _row_ref import gen
from xgserve.ops import _native, linear as L
from xgserve.ops._native import stream_ptr

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
E, N, K = 4, 512, 5 * L.F8_KT   # two column tiles; five K tiles: past both rings, uneven under S = 2 / 3
CASES = [(G.MODE_SILU, 1)] + [(G.MODE_PARTIAL, S) for S in (1, 2, 3)]


@functools.lru_cache(maxsize=None)
def problem(bm, mode):
    """Codes, scales, layout and the exact result of the real rows (in sorted order), on the CPU."""
    g = gen("moe-f8", bm, mode)
    real = [(0, 1, bm, bm + 1)[i] for i in torch.randperm(E, generator=g).tolist()]
    T = sum(real)
    src, rows, offs, expert = torch.randperm(T, generator=g).tolist(), [], [0], []
    for e, n in enumerate(real):
        seg = -(-n // 64) * 64
        rows += src[:n] + [-1] * (seg - n)
        expert += [e] * n
        src = src[n:]
        offs.append(offs[-1] + seg)
    P = offs[-1] + bm                       # capacity rows past offs[E], a whole tile of them: never written
    rows = torch.tensor(rows + [-1] * (P - offs[-1]), dtype=torch.int32)
    ridx, expert = (rows >= 0).nonzero()[:, 0], torch.tensor(expert)
    r = rows[ridx].long()
    va, vw = G._ints(g, (T, K), -16, 16) / 2, G._ints(g, (E, N, K), -16, 16) / 2
    sx, sw = G.pow2_scales(g, G.FP8, T, K, 4), G.pow2_scales(g, G.FP8, E * N, K, 4).view(E, N)
    y = torch.cat([va[r[expert == e]] @ vw[e].t() for e in range(E)]) * sx.double()[r, None] * sw.double()[expert]
    assert K * 64 * 4 * 2 ** 6 < G.EXACT    # |sum| <= 64 K, in units of 1/4 over the smallest scale pair 2^-6
    if mode == G.MODE_SILU:
        ex = max(0, math.ceil(math.log2(max(float(y.abs().max()), 1.0) / G.SILU_MAX)))
        sx, y = sx * 2.0 ** -ex, y * 2.0 ** -ex
    vs, ss = G._ints(g, (P, K), -16, 16) / 2, torch.ones(P)   # the sorted form: pads and capacity rows finite
    vs[ridx], ss[ridx] = va[r], sx[r]
    dev = lambda t, code=None: G.with_tail(t, DEV, code)  # noqa: E731  (tails: code 0x7E, NaN scales)
    code = G.TAIL_CODE[G.FP8]
    return dict(P=P, T=T, end=offs[-1], rows=rows.to(DEV), offs=torch.tensor(offs, dtype=torch.int32, device=DEV),
                ridx=ridx.to(DEV), y=y, q=dev(G.encode(vw.view(E * N, K), G.FP8), code), sw=dev(sw.reshape(-1, 1)),
                a=(dev(G.encode(vs, G.FP8), code), dev(G.encode(va, G.FP8), code)), sx=(dev(ss[:, None]), dev(sx[:, None])))


@pytest.mark.parametrize("gathered", (1, 0), ids=("rows", "sorted"))
@pytest.mark.parametrize("mode,S", CASES, ids=[f"{G.MODE_NAMES[m]}-S{s}" for m, s in CASES])
@pytest.mark.parametrize("cfg", sorted(L.F8_CFGS))
def test_exact(cfg, mode, S, gathered):
    k, p = _native.kernels(), problem(L.F8_CFGS[cfg][0], mode)
    P, partial = p["P"], mode == G.MODE_PARTIAL
    want = G.Want(G.Problem("quant", torch.zeros(len(p["ridx"]), K), p["y"]), mode, DEV)
    shape, dtype = ((S, P, N), torch.float32) if partial else ((P, N // 2), torch.bfloat16)
    assert k.moe_f8_supports(E, P, K, N, p["T"], S, mode, cfg)
    flat, res = G.guarded(shape, dtype, DEV)
    k.moe_gemm_f8(p["a"][gathered].data_ptr(), p["sx"][gathered].data_ptr(), p["rows"].data_ptr() if gathered else 0,
                  p["offs"].data_ptr(), E, P, K, p["q"].data_ptr(), p["sw"].data_ptr(), N, p["T"],
                  res.data_ptr() if partial else 0, 0 if partial else res.data_ptr(), S, mode, cfg, stream_ptr())
    want.check(res.index_select(-2, p["ridx"]), f"cfg {cfg} S {S}")
    assert bool((G.ibits(res[..., p["end"]:, :]) == (G.SENT32 if partial else G.SENT16)).all()), "wrote past offs[E]"
    assert G.guards_intact(flat, math.prod(shape)), "wrote outside its output"


def test_refusals():
    k, P, PA, SI = _native.kernels(), 128, G.MODE_PARTIAL, G.MODE_SILU
    b = torch.zeros(1024, device=DEV).data_ptr()   # refused before any pointer is read
    # K % 128, N % 256, the SiLU gate under a split, P % 64, more splits than K tiles, bf16 rows, cfg
    for pp, kk, n, S, mode, cfg in [(P, 576, N, 1, PA, 0), (P, K, 384, 1, PA, 0), (P, K, N, 2, SI, 0), (96, K, N, 1, PA, 0),
                                    (P, K, N, 6, PA, 0), (P, K, N, 1, G.MODE_BF16, 0), (P, K, N, 1, PA, len(L.F8_CFGS))]:
        assert not k.moe_f8_supports(E, pp, kk, n, 100, S, mode, cfg)
        with pytest.raises(ValueError):
            k.moe_gemm_f8(b, b, 0, b, E, pp, kk, b, b, n, 100, b, b, S, mode, cfg, stream_ptr())
    assert k.moe_f8_supports(E, P, K, N, 100, 1, SI, 1) and k.moe_f8_supports(E, P, K, N, 100, 5, PA, 0)
