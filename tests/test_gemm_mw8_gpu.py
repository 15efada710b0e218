"""gemm_mw8 (csrc/kernels/gemm_mw8.hip) through _native.kernels().gemm_mw8, on the problems and
checks of _gemm_ref: exact answers on the quantized grid (section 3 there) for every format x cfg x
mode, one real-valued problem per format at gemm_w8's bound (section 4), and every refused shape."""
import math

import pytest
import torch

import _gemm_ref as G
from xgserve import tune
from xgserve.ops import _native, linear as L
from xgserve.ops._native import stream_ptr

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FMTS = (G.FP8, G.INT8, G.INT4)
MODES = (G.MODE_PARTIAL, G.MODE_BF16, G.MODE_SILU)
CHUNKS = 5   # >= code ring slots + 2 (the rings wrap), odd (an uneven split of 3)


@pytest.fixture(scope="module")
def k():
    k = _native.kernels()
    yield k
    k.set_k_rotation(tune.get_int("krot", 1))


def launch(k, p, ops, M, N, K, S, mode, cfg, fmt):
    """Two launches into fresh guarded buffers -> the interior result of the second."""
    shape = (S, M, N) if mode == G.MODE_PARTIAL else (M, N // 2 if mode == G.MODE_SILU else N)
    first = None
    for _ in range(2):
        flat, res = G.guarded(shape, torch.float32 if mode == G.MODE_PARTIAL else torch.bfloat16, DEV)
        part, out = (res.data_ptr(), 0) if mode == G.MODE_PARTIAL else (0, res.data_ptr())
        k.gemm_mw8(ops.x.data_ptr(), M, K, ops.w.data_ptr(), ops.scale.data_ptr(), N, part, out, S, mode, cfg, fmt,
                   stream_ptr())
        assert G.guards_intact(flat, math.prod(shape)), "wrote outside its output"
        assert first is None or torch.equal(first, flat), "two launches differ"
        first = flat
    return res


@pytest.mark.parametrize("mode", MODES, ids=lambda m: G.MODE_NAMES[m])
@pytest.mark.parametrize("cfg", sorted(L.MW8_CFGS))
@pytest.mark.parametrize("fmt", FMTS, ids=("fp8", "int8", "int4"))
def test_exact(k, fmt, cfg, mode):
    cols, K = L.MW8_CFGS[cfg][0], CHUNKS * L.mw8_chunk(fmt)
    xkind = G.quant_x_kinds(fmt, K)[-1]   # "b" (odd |x| <= 255: 136 sum x matters) wherever it stays exact
    assert fmt != G.INT4 or xkind == "b"
    ran = 0
    for M in (65, 129, 320):
        for N in (cols, 2 * cols):
            if not k.mw8_supports(M, K, N, 1, mode, cfg, fmt):
                assert not L._mw8_fits(M, cfg, fmt), (M, N)   # only the (cfg, M, fmt) that do not exist
                continue
            p = G.quant_problem(fmt, xkind, M, N, K, mode)
            ops, want = G.DeviceOperands(p, DEV), G.Want(p, mode, DEV)
            for S in ((1, 3) if mode == G.MODE_PARTIAL else (1,)):
                for krot in (0, tune.get_int("krot", 1)):
                    k.set_k_rotation(krot)
                    want.check(launch(k, p, ops, M, N, K, S, mode, cfg, fmt),
                               f"mw8 fmt{fmt} cfg{cfg} {G.MODE_NAMES[mode]} M{M} N{N} K{K} S{S} krot{krot}")
                    ran += 1
    assert ran >= (4 if fmt == G.INT4 and cfg != 3 else 12)


@pytest.mark.parametrize("fmt", FMTS, ids=("fp8", "int8", "int4"))
def test_real_valued(k, fmt):
    M, N, K = 192, 256, 1024
    p = G.real_problem(M, N, K, fmt)
    ops = G.DeviceOperands(p, DEV)
    for mode, S, cfg in ((G.MODE_PARTIAL, 3, 0), (G.MODE_BF16, 1, 1), (G.MODE_SILU, 1, 2 if fmt != G.INT4 else 3)):
        used = G.Want(p, mode, DEV).check(launch(k, p, ops, M, N, K, S, mode, cfg, fmt), f"mw8 real fmt{fmt} mode{mode}")
        print(f"fmt {fmt} {G.MODE_NAMES[mode]}: {used:.3f} of the bound")


def test_refusals(k):
    M, N, K = 96, 256, 1024
    x = torch.zeros(M, K, dtype=torch.bfloat16, device=DEV)
    q = torch.zeros(N, K, dtype=torch.uint8, device=DEV)
    sc = torch.ones(K // 128, N, dtype=torch.float32, device=DEV)
    flat, res = G.guarded((3, M, N), torch.float32, DEV)
    P, B, SI = G.MODE_PARTIAL, G.MODE_BF16, G.MODE_SILU
    bad = [  # (M, K, N, S, mode, cfg, fmt, x, w, scale, out pointer)
        (M, K, N - 64, 1, P, 0, G.FP8),          # N not a multiple of the cfg's columns
        (M, K, 128, 1, P, 2, G.INT8),            # ... of 256 on cfg 2
        (M, K - 64, N, 1, P, 0, G.FP8),          # K not a multiple of the chunk
        (M, K - 128, N, 1, P, 0, G.INT4),        # int4: a chunk is two groups, 7 groups would cut one
        (M, 384, N, 3, P, 0, G.INT4),            # int4: three splits of one group and a half
        (M, K, N, 9, P, 0, G.FP8),               # more splits than chunks
        (320, K, N, 1, P, 0, G.INT4),            # LDS / registers at that M
        (321, K, N, 1, P, 0, G.FP8), (0, K, N, 1, P, 0, G.FP8),
        (M, K, N, 2, SI, 0, G.FP8), (M, K, N, 2, B, 0, G.FP8),   # SiLU / bf16 with S > 1
        (M, K, N, 1, 3, 0, G.FP8), (M, K, N, 1, P, len(L.MW8_CFGS), G.FP8), (M, K, N, 1, P, 0, 3),
    ]
    for a in bad:
        assert not k.mw8_supports(*a), a
        Mb, Kb, Nb, S, mode, cfg, fmt = a
        with pytest.raises(ValueError):
            k.gemm_mw8(x.data_ptr(), Mb, Kb, q.data_ptr(), sc.data_ptr(), Nb, res.data_ptr(), res.data_ptr(), S, mode, cfg,
                       fmt, stream_ptr())
    for ptrs in ((0, q.data_ptr(), sc.data_ptr(), res.data_ptr()), (x.data_ptr(), 0, sc.data_ptr(), res.data_ptr()),
                 (x.data_ptr(), q.data_ptr(), 0, res.data_ptr()), (x.data_ptr(), q.data_ptr(), sc.data_ptr(), 0)):
        with pytest.raises(ValueError):   # null pointers
            k.gemm_mw8(ptrs[0], M, K, ptrs[1], ptrs[2], N, ptrs[3], 0, 1, P, 0, G.FP8, stream_ptr())
    out = res[0].view(torch.bfloat16)[:, :N // 2]   # not the contiguous [M, N / 2] the mode needs
    for kw in (dict(mode=SI, plan=(2, 0)), dict(mode=P, plan=(1, 2), fmt=G.INT4), dict(mode=P, fmt=7),
               dict(mode=SI, out=out)):
        with pytest.raises(ValueError):
            L.mw8_linear(x, q if kw.get("fmt") != G.INT4 else q[:, :K // 2 - 64].contiguous(), sc[0].contiguous(), **kw)
    with pytest.raises(ValueError):   # scales of the wrong size
        L.mw8_linear(x, q, sc.view(-1), P)
    torch.cuda.synchronize()
    assert bool((flat == G.SENT32).all()), "a refused call wrote to its output"
