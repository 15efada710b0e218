"""Every hand-written GEMM kernel on inputs whose answer is known exactly, with guarded
operands and outputs: skinny_gemm (stream and slab variant), gemm_m64g (cfg x nw), gemm_w8
(cfg x fp8 / int8 / int4), gemm_mw, gemm_pf and gemm_pf_grouped, called directly through
_native.kernels() -- no planner and no fallback in the way -- in every mode the family's
no-launch predicate takes.

The older GEMM tests (test_skinny_gpu.py, test_pf_gpu.py, test_fp8_gpu.py, test_wq_gpu.py,
test_moe_gemm_gpu.py) compare one Frobenius norm over the whole output of unit-normal inputs
with 1e-2 / 2e-3 / 1e-5, which one wrong element, row or tile passes. Here a stale LDS slot, a
wait count that is one too small, a row clamp off by one, a swizzle on the wrong side, a wrong
scale index or a slab at the wrong offset changes elements whose exact value is known. Inputs,
float64 references, checks, the reasoning of each section and the case enumeration are in
tests/_gemm_ref.py; tests/test_gemm_refs_cpu.py holds a plain fp32 emulation to the same
checks and shows that the checks refuse ten planted errors.

Every launch reads operands that are the leading rows of larger NaN-tailed allocations, writes
an interior slice of a sentinel-filled buffer whose surroundings must keep the sentinel bit for
bit, and runs twice into fresh buffers with bit-identical results. gemm_m64g and gemm_mw run
with K rotation off and at its default, gemm_pf with set_pf_krot 0 and 1 (restored afterwards).
"""
import time

import pytest
import torch

import _gemm_ref as G
from xgserve.ops import _native
from xgserve.ops import linear as L
from xgserve.ops._native import stream_ptr

pytestmark = pytest.mark.gpu
DEV = "cuda"
FAMILIES = ("skinny", "m64g", "w8", "mw", "pf")


@pytest.fixture(scope="module")
def k():
    kern = _native.kernels()  # fail loudly: the HIP library must be the one that runs
    yield kern
    G.restore_rotation(kern)


def _sweep(k, cases, problem_of):
    cache, t0, worst = {}, time.perf_counter(), 0.0
    st = stream_ptr()
    for c in cases:
        for p in problem_of(c):
            worst = max(worst, G.run_case(k, c, p, DEV, st, cache))
    torch.cuda.synchronize()
    return time.perf_counter() - t0, worst


def _section13(c):
    if c.family == "w8":
        return [G.quant_problem(c.fmt, G.quant_xkind(c), c.M, c.N, c.K, c.mode)]
    return [G.grid_problem(G.grid_pair(c), c.M, c.N, c.K, c.mode)]


# ---------------------------------------------------------------- 1 and 3. grids (gemm_w8: quantized grids)
@pytest.mark.parametrize("family", FAMILIES)
def test_exact_grid(k, family):
    cases = G.family_cases(family)
    assert len(cases) >= G.FLOORS[family]
    if family != "skinny":  # every (cfg, mode, nw, fmt) the predicate takes at any listed shape is launched
        assert {c.combo for c in cases} == set(G._accepted_anywhere(family))
    if family in ("m64g", "mw", "pf"):
        assert {c.krot for c in cases} == {0, 1}
    sec, worst = _sweep(k, cases, _section13)
    print(f"{family}: {len(cases)} cases x 2 launches in {sec:.1f} s; largest share of the SiLU bound used {worst:.3f}")


# ---------------------------------------------------------------- 2. one-hot operands
@pytest.mark.parametrize("family", [f for f in FAMILIES if f != "w8"])
def test_one_hot(k, family):
    cases = G.onehot_cases(family)
    assert {c.combo for c in cases} == {c.combo for c in G.family_cases(family)}

    def problems(c):
        return [G.onehot_problem(c, side, r) for side in ("x", "w") for r in range(G.onehot_rounds(c, side))]

    sec, worst = _sweep(k, cases, problems)
    print(f"{family}: {len(cases)} one-hot cases in {sec:.1f} s; largest share of the SiLU bound used {worst:.3f}")


def test_w8_every_code(k):
    """All 254 non-NaN E4M3 codes, all 256 int8 codes, all 16 nibbles in all 8 word positions
    through the GEMM's own widening path, one code per probed (n, k)."""
    cases = G.onehot_cases("w8")
    t = k.gemm_cfgs()["w8"]
    assert {(c.cfg, c.fmt) for c in cases} == {(cfg, f) for cfg in range(len(t)) for f in (G.FP8, G.INT8, G.INT4)}
    sec, _ = _sweep(k, cases, lambda c: [G.codes_problem(c, r) for r in range(G.codes_rounds(c))])
    print(f"w8: {len(cases)} code cases in {sec:.1f} s")


# ---------------------------------------------------------------- 4. real-valued inputs, per-element bound
@pytest.mark.parametrize("family", FAMILIES)
def test_real_valued(k, family):
    cases = G.real_cases(family)
    st = stream_ptr()
    for c in cases:
        p = G.real_problem(c.M, c.N, c.K, c.fmt if family == "w8" else None)
        used = G.run_case(k, c, p, DEV, st)
        print(f"{c.tag}: share of the bound used {used:.4f}")


# ---------------------------------------------------------------- gemm_pf_grouped
def test_pf_grouped(k):
    cases = G.grouped_cases()
    assert len(cases) >= G.FLOORS["pf_grouped"]
    grouped = {cfg for cfg, row in enumerate(k.gemm_cfgs()["pf"]) if row[3]}
    assert {c[0] for c in cases} == grouped
    t0 = time.perf_counter()
    for case in cases:
        G.run_grouped(k, case, DEV, stream_ptr())
    print(f"pf_grouped: {len(cases)} cases x 2 launches in {time.perf_counter() - t0:.1f} s")


# ---------------------------------------------------------------- wrapper operands
def _wrappers():
    """name -> (call(x, w, out=None), M, N, K). The bad operands below stay in bounds even if a check
    were missing (views of LARGER device buffers, never smaller ones, never host memory), so a
    regression fails the test and does not fault the card."""
    def quant(w):
        return L.quantize_weight(w, L.WQ_INT8)

    return {
        "skinny": (lambda x, w, out=None: L.skinny_linear(x, w, None, L.MODE_BF16, out=out), 8, 64, 512),
        "m64": (lambda x, w, out=None: L.m64_linear(x, w, L.MODE_BF16, 1, 1, out=out, cfg=0), 32, 256, 512),
        "mw": (lambda x, w, out=None: L.mw_linear(x, w, L.MODE_BF16, plan=(1, 1), out=out), 100, 256, 256),
        "pf": (lambda x, w, out=None: L.pf_linear(x, w, L.MODE_BF16, plan=(1, 2), out=out), 300, 256, 256),
        "w8": (lambda x, w, out=None: L.w8_linear(x, *quant(w), L.MODE_SILU, plan=(1, 1), out=out, fmt=L.WQ_INT8), 8, 128, 256),
    }


@pytest.mark.parametrize("name", ["skinny", "m64", "mw", "pf", "w8"])
def test_wrappers_refuse_bad_operands(k, name):
    call, M, N, K = _wrappers()[name]
    p = G.grid_problem("b", M, N, K, G.MODE_SILU if name == "w8" else G.MODE_BF16)
    x, w = p.x.to(DEV), p.w.to(DEV)
    cols = N // 2 if name == "w8" else N
    got = call(x, w)                                    # the wrapper still runs what it ran
    assert got.shape == (M, cols)
    if name != "w8":
        G.check_bf16(got, p.want_bf16().to(DEV), name)
    else:  # (the package's quantizer: real scales, so section 4's kind of bound; here one part in 100)
        ref = p.silu_ref()[0].to(DEV)
        G.check_bound(got, ref, ref.abs() * 1e-2, name)
    out = torch.zeros(M + 8, cols, dtype=torch.bfloat16, device=DEV)
    assert call(x, w, out=out[:M]).data_ptr() == out.data_ptr()
    diff = G.ibits(out[:M]) != G.ibits(got)
    assert not bool(diff.any()), (name, int(diff.sum()), diff.nonzero()[:4].tolist(), out[:M][diff][:4], got[diff][:4])
    assert not bool(out[M:].any())                      # the rows behind the view stay as they were
    wide = torch.zeros(M, 2 * K, dtype=torch.bfloat16, device=DEV)
    wide[:, :K] = x
    bad = [
        ("strided x", lambda: call(wide[:, :K], w)),
        ("float32 x", lambda: call(x.float(), w)),
        ("larger out", lambda: call(x, w, out=out)),
        ("strided out", lambda: call(x, w, out=torch.zeros(M, 2 * cols, dtype=torch.bfloat16, device=DEV)[:, :cols])),
        ("float32 out", lambda: call(x, w, out=torch.zeros(M, cols, device=DEV))),
        ("3-d x", lambda: call(x[None], w)),
    ]
    if name != "w8":  # (w8's weight goes through the quantizer above; its own operands follow)
        wide_w = torch.zeros(N, 2 * K, dtype=torch.bfloat16, device=DEV)
        bad += [("strided w", lambda: call(x, wide_w[:, :K])), ("w of another K", lambda: call(x, wide_w)),
                ("float32 w", lambda: call(x, w.float()))]
    for what, fn in bad:
        with pytest.raises(ValueError):
            fn()
            pytest.fail(f"{name}: {what} was launched")


def test_w8_wrapper_refuses_bad_codes_and_scales():
    M, N, K = 8, 128, 256
    x = torch.zeros(M, K, dtype=torch.bfloat16, device=DEV)
    w = torch.zeros(N, K, dtype=torch.bfloat16, device=DEV)
    for fmt in (L.WQ_FP8, L.WQ_INT8, L.WQ_INT4):
        q, s = L.quantize_weight(w, fmt)
        L.w8_linear(x, q, s, L.MODE_PARTIAL, plan=(1, 1), fmt=fmt)
        wide = torch.zeros(N, 2 * q.shape[1], dtype=torch.uint8, device=DEV)
        for what, args in [("strided codes", (wide[:, :q.shape[1]], s)), ("codes of another K", (wide, s)),
                           ("int8-typed codes", (q.view(torch.int8), s)), ("float64 scales", (q, s.double()))]:
            with pytest.raises(ValueError):
                L.w8_linear(x, *args, L.MODE_PARTIAL, plan=(1, 1), fmt=fmt)
                pytest.fail(f"fmt {fmt}: {what} was launched")


def test_m64_linear_runs_the_named_configuration_or_raises():
    """An explicit (nw, split_k, cfg) that the kernel does not take is an error, never cfg 0 in its place."""
    M, N, K = 32, 192, 512
    x = torch.zeros(M, K, dtype=torch.bfloat16, device=DEV)
    w = torch.zeros(N, K, dtype=torch.bfloat16, device=DEV)
    assert L.m64_linear(x, w, L.MODE_PARTIAL, 2, 1, cfg=2).part.shape == (2, M, N)
    for nw, S, cfg in [(1, 1, 8), (1, 1, 11), (2, 1, 7), (1, 16, 0)]:  # deep ring at M > 16; no such cfg; N % 256; S > K / KC
        with pytest.raises(ValueError):
            L.m64_linear(x, w, L.MODE_PARTIAL, S, nw, cfg=cfg)
    with pytest.raises(ValueError):
        L.m64_linear(x, w, L.MODE_BF16, 2, 1, cfg=0)       # bf16 output has no split form
