"""The "i4" step family, the gemm_i4 planner and the int8_activations key with int4 weights: no GPU launch."""
import itertools

import pytest

from xgserve.models import get_config, llama as ll
from xgserve.ops import _native, linear as L
from xgserve.server.config import ServerConfig
from xgserve.server.replica import engine_spec

ROWS = (1, 64, 65, 320, 321, 575, 2048)


def _dispatch(model="llama3-8b", tp=1, resident=False, fmt=L.WQ_INT4, on_gpu=True, **kw):
    d = ll.LayerDispatch.for_layer(get_config(model), tp=tp, on_gpu=on_gpu)
    d.set_quantized(ll.PROJECTIONS if "gate_up" in d.shapes else ("qkv", "o"), resident=resident, fmt=fmt, **kw)
    return d


def test_the_predicates_agree_and_the_tables_match():
    k, seen = _native.kernels(), set()
    shapes = {s for m in ("llama3-8b", "llama3-70b", "llama-tiny") for s in _dispatch(m).shapes.values()}
    for (N, K, _), M, mode in itertools.product(sorted(shapes), (321, 575, 2048, 8192), (L.MODE_BF16, L.MODE_PARTIAL, L.MODE_SILU)):
        for cfg, S in itertools.product((*L.I4_CFGS, len(L.I4_CFGS)), (1, 2, K // L.F8_KT + 1)):
            ok = L._i4_valid(M, N, K, mode, S, cfg)
            assert ok == k.i4_supports(M, K, N, S, mode, cfg), (M, N, K, mode, S, cfg)
            seen.add(ok)
        assert L._i4_valid(M, N, K, mode, *L.i4_plan(M, N, K, mode))
    assert seen == {True, False} and L._I4_TUNED == {} and L.i4_plan(321, 6144, 4096, L.MODE_PARTIAL) == (4, 1)
    assert [tuple(r) for r in k.gemm_cfgs()["i4"]] == [L.I4_CFGS[c] for c in sorted(L.I4_CFGS)]


@pytest.mark.parametrize("resident", [True, False])
def test_select(resident):
    on, off = _dispatch(resident=resident, aw4=True), _dispatch(resident=resident)
    assert on.i4 == ll.PROJECTIONS and off.i4 == on.i8 == on.f8 == ()
    for T in ROWS:
        if T > 320:
            assert tuple(on.select(T, 0)) == ("i4",) * 4 + ("from_partials",), T
            assert on.select(T, 0, mixed_graph=True) == off.select(T, 0, mixed_graph=True)
        else:
            assert on.select(T, 0) == off.select(T, 0) and on.select(T, T) == off.select(T, T), T
    # fp8 / int8 copies, TP 2, Mixtral and the CPU are unchanged
    for kw in (dict(fmt=L.WQ_FP8), dict(fmt=L.WQ_INT8), dict(tp=2), dict(model="mixtral-8x7b"), dict(on_gpu=False)):
        on, off = _dispatch(resident=resident, aw4=True, **kw), _dispatch(resident=resident, **kw)
        assert on.i4 == () and all(on.select(T, 0) == off.select(T, 0) for T in ROWS), kw


def test_config_accepts_int4_with_int8_activations():
    c = ServerConfig()
    c.worker.int8_activations, c.worker.quantization, c.worker.model = True, "int4", "llama3-8b"
    assert not [e for e in c.validate() if "activations" in e]
    assert engine_spec(c.worker)["int8_activations"] is True and engine_spec(c.worker)["weight_dtype"] == "int4"
    c.worker.quantization = "fp8"
    assert any("worker.int8_activations needs worker.quantization int8 or int4, got 'fp8'" in e for e in c.validate())
