"""The "mw8" step family (LayerDispatch, xgserve/models/llama.py) and the gemm_mw8 planner
(xgserve/ops/linear.py), the parts that need no GPU."""
import pytest

from xgserve.models import get_config
from xgserve.models import llama as ll
from xgserve.ops import linear as L

FMTS = (L.WQ_FP8, L.WQ_INT8, L.WQ_INT4)


def _dispatch(resident, fmt, model="llama3-70b"):
    d = ll.LayerDispatch.for_layer(get_config(model), tp=1, on_gpu=True)
    d.set_quantized(ll.PROJECTIONS, resident=resident, fmt=fmt)
    return d


def _today(resident, model="llama3-70b"):
    d = ll.LayerDispatch.for_layer(get_config(model), tp=1, on_gpu=True)
    d.set_quantized(ll.PROJECTIONS, resident=resident)
    return d


@pytest.fixture
def resident_takes_70b(monkeypatch):
    """A resident model takes gemm_mw8 only for measured (N, K, fmt): here every 70B one, any format."""
    shapes = ll.LayerDispatch.for_layer(get_config("llama3-70b"), 1, on_gpu=True).shapes.values()
    monkeypatch.setattr(ll, "MW8_RESIDENT", frozenset((N, K, f) for N, K, _ in shapes for f in FMTS))


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("resident", [True, False])
def test_select(resident, fmt, resident_takes_70b):
    d, today = _dispatch(resident, fmt), _today(resident)
    for T in (65, ll.MW_MAX_TOKENS):
        assert tuple(d.select(T, 0)) == ("mw8",) * 4 + ("from_partials",), T
    assert tuple(d.select(64, 0)) == ("w8",) * 4 + ("from_partials",)
    for T in (ll.MW_MAX_TOKENS + 1, 575, 4096):
        assert d.select(T, 0) == today.select(T, 0), T
    assert today.select(65, 0)[0] == ("mw" if resident else "dq")


def test_partly_quantized_keeps_todays_family_for_the_rest(resident_takes_70b):
    for resident, rest in ((True, "mw"), (False, "lib")):
        d = ll.LayerDispatch.for_layer(get_config("llama3-70b"), tp=1, on_gpu=True)
        d.set_quantized(("gate_up", "down"), resident=resident, fmt=L.WQ_INT4)
        assert tuple(d.select(200, 0)) == (rest, rest, "mw8", "mw8", "from_partials" if resident else "rope")


def test_shapes_held_back_and_shapes_without_a_plan(monkeypatch):
    # a resident model takes only MW8_RESIDENT (70B: fp8); a quantized-only one every shape with a plan
    assert _dispatch(True, L.WQ_FP8).select(200, 0)[:4] == ("mw8",) * 4
    assert _dispatch(False, L.WQ_INT8, "llama3-8b").select(200, 0)[:4] == ("mw8",) * 4
    for model in ("llama3-70b", "llama3-8b"):
        d, today = _dispatch(True, L.WQ_INT8, model), _today(True, model)
        assert all(d.select(T, 0) == today.select(T, 0) for T in (64, 65, 200, 320, 321))
    monkeypatch.setattr(ll, "mw8_plan", lambda *a: None)
    d, today = _dispatch(False, L.WQ_FP8), _today(False)
    assert all(d.select(T, 0) == today.select(T, 0) for T in (1, 64, 65, 320, 321))


def test_out_of_scope_steps_are_unchanged(resident_takes_70b):
    """TP > 1 and the bodies of the runner's mixed-step graphs keep the families they had."""
    for resident in (True, False):
        d, today = _dispatch(resident, L.WQ_FP8), _today(resident)
        assert d.select(200, 16)[0] == "mw8" and d.select(200, 16, mixed_graph=True) == today.select(200, 16)
        tp2 = ll.LayerDispatch.for_layer(get_config("llama3-70b"), tp=2, on_gpu=True)
        tp2.set_quantized(ll.PROJECTIONS, resident=resident, fmt=L.WQ_FP8)
        assert tp2.mw8 is None and "mw8" not in tp2.select(200, 16)


def test_a_tuned_plan_that_does_not_take_m_falls_back(monkeypatch):
    key = (1024, 2048, L.MODE_PARTIAL, L.WQ_INT4)
    default = [L.mw8_plan(M, *key) for M in (200, 250)]
    monkeypatch.setitem(L._MW8_TUNED, key, {192: (2, 2), 256: (99, 0)})   # cfg 2 has no int4 above 128 rows
    L.mw8_plan.cache_clear()
    try:
        assert [L.mw8_plan(M, *key) for M in (200, 250)] == default and None not in default
    finally:
        L.mw8_plan.cache_clear()


def test_tune_switch_restores_today(monkeypatch, resident_takes_70b):
    from xgserve import tune
    assert tune.get_bool("mw8", True) is True
    monkeypatch.setenv("XGS_TUNE", "mw8=0")
    assert tune.get_bool("mw8", True) is False   # what llama.MW8 reads at import
    monkeypatch.setattr(ll, "MW8", False)
    for resident in (True, False):
        d, today = _dispatch(resident, L.WQ_INT4), _today(resident)
        assert all(d.select(T, 0) == today.select(T, 0) for T in (1, 64, 65, 320, 321))


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("cfg", sorted(L.MW8_CFGS))
def test_lds_arithmetic(cfg, fmt):
    """160 KB hold `slots` code slots (int4: + 8 B of scales per column) and 2..5 x slots of
    128 B x M rounded up to 64 rows; the wave's accumulators (int4: twice) stay within 200 registers."""
    cols, slots, wn = L.MW8_CFGS[cfg]
    code = slots * cols * (136 if fmt == L.WQ_INT4 else 128)
    for M, rows in ((256, 256), (257, 320), (320, 320)):
        dx = min(5, (160 * 1024 - code) // (rows * 128))
        tiles = (cols // (16 * wn) + 1) * (rows // (16 * (8 // wn))) * (2 if fmt == L.WQ_INT4 else 1)
        want = code + dx * rows * 128 if dx >= 2 and 4 * tiles <= 200 else 0
        assert L._mw8_lds(M, cfg, fmt) == want and L._mw8_fits(M, cfg, fmt) == (want > 0), M
        plan = L.mw8_plan(M, 4 * cols, 2048, L.MODE_PARTIAL, fmt)
        assert plan is None or L._mw8_fits(M, plan[1], fmt)
    assert not L._mw8_fits(321, cfg, fmt) and L.mw8_plan(321, 4 * cols, 2048, L.MODE_PARTIAL, fmt) is None
    assert any(L._mw8_fits(320, c, fmt) for c in L.MW8_CFGS)
    assert L.mw8_plan(320, 4 * cols, 2048, L.MODE_PARTIAL, fmt) is not None
    assert L.mw8_plan(192, 4 * cols, 2048 + 64, L.MODE_PARTIAL, fmt) is None   # K off the chunk
    assert L.mw8_plan(192, 4 * cols, 2048, L.MODE_SILU, fmt)[0] == 1
