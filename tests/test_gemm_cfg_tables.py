"""The GEMM families' configuration tables exist once in C++ (next to each kernel) and
once in Python (xgserve/ops/linear.py, read by the pure-Python planners). These checks
hold the two together: (a) tables and constants are equal, (b) the Python validity
predicates equal the library's no-launch predicates over a grid, and every plan a
planner returns is one the library takes, (c) the grid has both outcomes per family and
the named edge cases are rejected on both sides. Nothing is launched."""
import functools
import itertools

from xgserve.models.config import get_config, list_models
from xgserve.ops import linear as L
from xgserve.ops import moe as MOE
from xgserve.ops._native import kernels

TPS = (1, 2, 4, 8)
M64_ROWS = (1, 16, 17, 40, 64)      # gemm_m64g and gemm_w8
MW_ROWS = (65, 128, 256, 257, 320, 321)
PF_ROWS = (64, 575, 1536)
M64_MODES = (L.MODE_BF16, L.MODE_PARTIAL, L.MODE_SILU, L.MODE_RESID, 5)  # 5: GG_AR (4 is the grouped form's)
W8_MODES = (L.MODE_PARTIAL, L.MODE_SILU)                                # the kernel's two epilogues
MODES = (L.MODE_BF16, L.MODE_PARTIAL, L.MODE_SILU)
FMTS = (L.WQ_FP8, L.WQ_INT8, L.WQ_INT4)
MOE_PAIRS = (1, 2, 4, 8, 9, 16, 17, 63, 64, 256, 257, 1150, 16000)


@functools.lru_cache(maxsize=None)
def _shapes():
    """(N, K) of every tuned plan and of every llama / mixtral projection at TP 1-8."""
    out = set()
    for table in (L._M64_TUNED, L._W8_TUNED, L._W8_TUNED64, L._MW_TUNED):
        out.update((n, k) for n, k, _ in table)
    for name in list_models():
        c = get_config(name)
        if c.arch not in ("llama", "mixtral"):
            continue
        H, F, hd = c.hidden_size, c.intermediate_size, c.head_dim
        for tp in TPS:
            nh, kvh = max(1, c.num_heads // tp), max(1, c.num_kv_heads // tp)
            out.update({((nh + 2 * kvh) * hd, H), (H, nh * hd), (2 * F // tp, H), (H, F // tp), (c.vocab_size, H)})
    return sorted(out)


def _moe_layers():
    """(local experts, H, F) of every mixtral model at TP 1-8 (experts are sharded whole)."""
    for name in list_models():
        c = get_config(name)
        if c.arch == "mixtral":
            for tp in TPS:
                if c.num_experts % tp == 0:
                    yield c.num_experts // tp, c.hidden_size, c.intermediate_size


def _both(seen, what):
    assert seen == {True, False}, f"{what}: the grid only ever gives {seen}"


# ------------------------------------------------------------------ (a) tables and constants
def test_tables_and_constants_equal_the_librarys():
    k = kernels()
    t = k.gemm_cfgs()
    assert L.M64G_TABLE == dict(enumerate(t["m64g"]))
    assert L.M64G_CFGS == {c: row[:3] for c, row in enumerate(t["m64g"])}
    assert L.W8_GEOM == dict(enumerate(t["w8"]))
    assert L.W8_CFGS == {c: (16 * nw * wv, kc) for c, (nw, wv, kc) in enumerate(t["w8"])}
    assert L.MW_CFGS == dict(enumerate(t["mw"]))
    assert L.PF_CFGS == dict(enumerate(t["pf"]))
    assert L.PF_CFG_BM == {c: row[0] for c, row in enumerate(t["pf"])}
    assert set(L._PF_CFG_KT_US) <= set(L.PF_CFGS)
    assert L.M64G_SMALL_ONLY == tuple(c for c, row in enumerate(t["m64g"]) if row[3] != 3)
    assert (L.WQ_GROUP, L.WQ_SC_FLOATS) == (k.WQ_GROUP, k.WQ_SC_FLOATS)
    assert (L.M64_MAX_M, L.W8_MAX_M, L.MW_MAX_M) == (k.M64G_MAX_M, k.W8_MAX_M, k.MW_MAX_M)


# ------------------------------------------------------------------ (b) predicates and plans
def test_m64_valid_equals_the_library_on_the_grid():
    k, seen = kernels(), set()
    for (N, K), M, cfg, nw, S, mode in itertools.product(_shapes(), M64_ROWS, L.M64G_CFGS, (1, 2), L._SPLITS,
                                                         M64_MODES):
        py = L._m64_valid(N, K, mode, nw, S, cfg, M)
        assert py == k.m64g_supports(M, K, N, S, mode, nw, cfg), (M, N, K, mode, nw, S, cfg)
        seen.add(py)
    _both(seen, "gemm_m64g")


def test_w8_fits_equals_the_library_on_the_grid():
    k, seen = kernels(), set()
    for (N, K), M, cfg, S, mode, fmt in itertools.product(_shapes(), M64_ROWS, L.W8_CFGS, L._SPLITS, W8_MODES, FMTS):
        py = L._w8_fits(N, K, mode, S, cfg, M, fmt)
        assert py == k.w8_supports(M, K, N, S, mode, cfg, fmt), (M, N, K, mode, S, cfg, fmt)
        seen.add(py)
    _both(seen, "gemm_w8")


def test_mw_and_pf_grids_have_both_outcomes():
    k, mw, pf, pfg = kernels(), set(), set(), set()
    for (N, K), S, mode in itertools.product(_shapes(), L._SPLITS, MODES):
        for M, cfg in itertools.product(MW_ROWS, L.MW_CFGS):
            ok = k.mw_supports(M, K, N, S, mode, cfg)
            assert not ok or L._mw_fits(M, cfg), (M, N, K, mode, S, cfg)
            mw.add(ok)
        for M, cfg in itertools.product(PF_ROWS, L.PF_CFGS):
            pf.add(k.pf_supports(M, K, N, S, mode, cfg))
            pfg.add(k.pf_grouped_supports(8, 64 * 40, K, N, M, S, mode, cfg))
    for M, cfg in itertools.product(range(1, 330), L.MW_CFGS):  # the LDS rule alone, every row count
        assert L._mw_fits(M, cfg) == k.mw_supports(M, 4096, 4096, 1, L.MODE_PARTIAL, cfg), (M, cfg)
    _both(mw, "gemm_mw")
    _both(pf, "gemm_pf")
    _both(pfg, "gemm_pf_grouped")


def test_every_plan_is_one_the_library_takes():
    k, n = kernels(), 0
    for (N, K), mode in itertools.product(_shapes(), MODES):
        for M in M64_ROWS:
            p = L.m64_plan(M, N, K, mode)
            if p is not None:
                nw, S, cfg = p
                assert k.m64g_supports(M, K, N, S, mode, nw, cfg), ("m64", M, N, K, mode, p)
                n += 1
            for fmt in FMTS if mode in W8_MODES else ():
                p = L.w8_plan(M, N, K, mode, fmt)
                if p is not None:  # (w8_linear runs SiLU at split 1 whatever the plan's)
                    assert k.w8_supports(M, K, N, p[0] if mode == L.MODE_PARTIAL else 1, mode, p[1], fmt), \
                        ("w8", M, N, K, mode, fmt, p)
                    n += 1
        for M in MW_ROWS:
            p = L.mw_plan(M, N, K, mode)
            if p is not None:
                assert k.mw_supports(M, K, N, p[0], mode, p[1]), ("mw", M, N, K, mode, p)
                n += 1
        for M in PF_ROWS:
            p = L.pf_plan(M, N, K, mode)
            if p is not None:
                assert k.pf_supports(M, K, N, p[0], mode, p[1]), ("pf", M, N, K, mode, p)
                n += 1
    assert n > 1000  # (the planners do plan on this grid)


def test_every_moe_cfg_choice_is_one_the_library_takes():
    k, seen = kernels(), set()
    for (E, H, F), pairs in itertools.product(_moe_layers(), MOE_PAIRS):
        P = 64 * (-(-pairs // 64) + E)  # moe_align's capacity
        cfg13, nw2, cfg2, S = MOE.moe_m64_plan(pairs, E, H, F)
        assert k.moe_m64g_supports(E, H, 2 * F, P, 1, L.MODE_SILU, 2, cfg13, pairs), (E, H, F, pairs, cfg13)
        assert k.moe_m64g_supports(E, F, H, P, S, L.MODE_PARTIAL, nw2, cfg2, pairs), (E, H, F, pairs, nw2, cfg2, S)
        cols2 = 16 * nw2 * L.M64G_CFGS[cfg2][0]
        if pairs <= MOE.MOE_PREFILL_PAIRS and H // cols2 <= 64:  # fused_moe's in-launch combine (GG_MOE_RESID = 4)
            assert k.moe_m64g_supports(E, F, H, P, S, 4, nw2, cfg2, pairs), (E, H, F, pairs, nw2, cfg2, S)
        if pairs > MOE.MOE_PREFILL_PAIRS and MOE._moe_pf_ok(H, F):
            cfg = MOE._moe_pf_cfg(pairs, E)
            assert L.PF_CFGS[cfg][3]
            assert k.pf_grouped_supports(E, P, H, 2 * F, pairs, 1, L.MODE_SILU, cfg), (E, H, F, pairs, cfg)
            assert k.pf_grouped_supports(E, P, F, H, pairs, 2 if F % 128 == 0 else 1, L.MODE_PARTIAL, cfg)
        seen.update((cfg13, cfg2))
    assert seen and all(L.M64G_TABLE[c][4] for c in seen)
    # the grouped form's own rejections: a dense-only cfg, SiLU without gate / up pairs
    assert not k.moe_m64g_supports(8, 4096, 28672, 512, 1, L.MODE_SILU, 2, 7, 16)
    assert not k.moe_m64g_supports(8, 4096, 28672, 512, 1, L.MODE_SILU, 1, 5, 16)


# ------------------------------------------------------------------ (c) the named rejections
def test_named_cases_are_rejected_on_both_sides():
    k = kernels()
    P, SI, BF = L.MODE_PARTIAL, L.MODE_SILU, L.MODE_BF16

    def m64(M, N, K, mode, nw, S, cfg):
        return L._m64_valid(N, K, mode, nw, S, cfg, M), k.m64g_supports(M, K, N, S, mode, nw, cfg)

    def w8(M, N, K, mode, S, cfg, fmt):
        return L._w8_fits(N, K, mode, S, cfg, M, fmt), k.w8_supports(M, K, N, S, mode, cfg, fmt)

    assert m64(16, 4096, 4096, P, 1, 1, 8) == (True, True)
    assert m64(17, 4096, 4096, P, 1, 1, 8) == (False, False)          # deep ring: one x tile only
    assert m64(1, 28672, 4096, SI, 1, 1, 1) == (False, False)         # SiLU needs gate / up pairs
    assert m64(1, 4096, 4096, BF, 1, 2, 0) == (False, False)          # bf16 output has no split form
    assert m64(64, 4096, 4096, P, 2, 1, 7) == (True, True)
    assert m64(64, 4096 + 128, 4096, P, 2, 1, 7) == (False, False)    # 256-column tiles
    assert w8(16, 4096, 4096, P, 1, 3, L.WQ_FP8) == (True, True)
    assert w8(17, 4096, 4096, P, 1, 3, L.WQ_FP8) == (False, False)    # KC 256: one x tile only
    assert w8(1, 28672, 4096, SI, 1, 2, L.WQ_FP8) == (False, False)   # one 16-column tile per wave
    assert w8(1, 4096, 14336, P, 1, 0, L.WQ_INT8) == (True, True)
    assert w8(1, 4096, 14336, P, 1, 0, L.WQ_INT4) == (False, False)   # 112 groups x 128 columns > 4096 scales
    assert w8(1, 4096, 4096 + 256, P, 1, 3, L.WQ_INT8) == (True, True)
    assert w8(1, 4096, 4096 + 256, P, 4, 1, L.WQ_INT4) == (False, False)  # (K / S) % 128 = 1088 % 128 != 0
    # gemm_mw: beyond 320 rows; 320 rows beside the rings of a 256-column cfg
    assert L.mw_plan(320, 4096, 4096, P) is not None and k.mw_supports(320, 4096, 4096, 1, P, 2)
    assert L.mw_plan(321, 4096, 4096, P) is None and not any(
        k.mw_supports(321, 4096, 4096, 1, P, cfg) for cfg in L.MW_CFGS)
    assert L._mw_fits(256, 0) and k.mw_supports(256, 4096, 4096, 1, P, 0)
    assert not L._mw_fits(320, 0) and not k.mw_supports(320, 4096, 4096, 1, P, 0)
    # gemm_pf: 256-column tiles; the grouped form takes the lag-2 rows only
    assert L.pf_plan(575, 4096, 4096, P) is not None and k.pf_supports(575, 4096, 4096, 1, P, 2)
    assert L.pf_plan(575, 4096 + 128, 4096, P) is None and not any(
        k.pf_supports(575, 4096, 4096 + 128, 1, P, cfg) for cfg in L.PF_CFGS)
    assert L.PF_CFGS[6][3] and k.pf_grouped_supports(8, 1024, 4096, 28672, 600, 1, SI, 6)
    assert not L.PF_CFGS[5][3] and not k.pf_grouped_supports(8, 1024, 4096, 28672, 600, 1, SI, 5)
