"""The "i8" step family (LayerDispatch), the gemm_i8 planner and the int8_activations key from the
config file to the engine: the parts that need no GPU launch."""
import pytest

from xgserve.models import get_config
from xgserve.models import llama as ll
from xgserve.ops import _native, linear as L

MODES = (L.MODE_BF16, L.MODE_PARTIAL, L.MODE_SILU)
I8_STEP = ("i8",) * 4 + ("from_partials",)


def _dispatch(model="llama3-8b", tp=1, resident=False, fmt=L.WQ_INT8, **kw):
    d = ll.LayerDispatch.for_layer(get_config(model), tp=tp, on_gpu=True)
    d.set_quantized(ll.PROJECTIONS if "gate_up" in d.shapes else ("qkv", "o"), resident=resident, fmt=fmt, **kw)
    return d


def test_the_predicates_agree_and_the_plan_is_f8s():
    k = _native.kernels()
    shapes = {s for m in ("llama3-8b", "llama3-70b", "llama-tiny")
              for s in ll.LayerDispatch.for_layer(get_config(m), 1, on_gpu=True).shapes.values()}
    seen = set()
    for N, K, _ in sorted(shapes) + [(256, L.I8_MAX_K, 0), (256, L.I8_MAX_K + L.F8_KT, 0)]:
        for M in (321, 575, 2048, 8192):
            for mode in MODES:
                for cfg in (*L.F8_CFGS, len(L.F8_CFGS)):
                    for S in (1, 2, K // L.F8_KT + 1):
                        ok = L._i8_valid(M, N, K, mode, S, cfg)
                        assert ok == k.i8_supports(M, K, N, S, mode, cfg), (M, N, K, mode, S, cfg)
                        seen.add(ok)
                assert L.i8_plan(M, N, K, mode) == L.f8_plan(M, N, K, mode), (M, N, K, mode)
    assert seen == {True, False} and L._I8_TUNED == {} and L.i8_plan(321, 6144, 4096, L.MODE_PARTIAL) == (4, 1)
    assert not L._i8_valid(321, 256, L.I8_MAX_K + L.F8_KT, L.MODE_PARTIAL, 1, 0)
    assert [tuple(r) for r in k.gemm_cfgs()["i8"]] == [L.F8_CFGS[c] for c in sorted(L.F8_CFGS)]


@pytest.mark.parametrize("resident", [True, False])
def test_select(resident):
    on, off = _dispatch(resident=resident, ai8=True), _dispatch(resident=resident)
    for T in (321, 575, 2048):
        assert tuple(on.select(T, 0)) == I8_STEP, T
        assert on.select(T, 0, mixed_graph=True) == off.select(T, 0, mixed_graph=True)
    for T in (1, 16, 64, 65, 320):
        assert on.select(T, 0) == off.select(T, 0) and on.select(T, T) == off.select(T, T), T
    # off is exactly the dispatch of a model quantized without the argument
    plain = ll.LayerDispatch.for_layer(get_config("llama3-8b"), tp=1, on_gpu=True)
    plain.set_quantized(ll.PROJECTIONS, resident=resident, fmt=L.WQ_INT8)
    assert all(off.select(T, 0) == plain.select(T, 0) for T in (1, 64, 65, 320, 321, 575, 2048, 8192))


def test_ai8_changes_nothing_out_of_scope():
    for kw in (dict(fmt=L.WQ_FP8), dict(fmt=L.WQ_INT4), dict(tp=2), dict(model="mixtral-8x7b")):
        on, off = _dispatch(ai8=True, **kw), _dispatch(**kw)
        assert on.i8 == () and all(on.select(T, 0) == off.select(T, 0) for T in (64, 65, 320, 321, 575, 2048)), kw
    cpu = ll.LayerDispatch.for_layer(get_config("llama3-8b"), tp=1, on_gpu=False)
    cpu.set_quantized(ll.PROJECTIONS, resident=True, fmt=L.WQ_INT8, ai8=True)
    assert cpu.i8 == () and _dispatch(a8=True).f8 == () and _dispatch(ai8=True).f8 == ()


def test_config_key_cli_flag_and_engine_field():
    import argparse
    from xgserve import cli
    from xgserve.engine import EngineConfig
    from xgserve.server.config import ServerConfig
    from xgserve.server.replica import engine_spec
    c = ServerConfig()
    assert c.worker.int8_activations is False and EngineConfig().int8_activations is False
    assert engine_spec(c.worker)["int8_activations"] is False
    c.worker.int8_activations, c.worker.mock = True, True
    c.worker.quantization, c.worker.device, c.worker.tp = "fp8", "cpu", 2
    errs = "\n".join(c.validate())
    for text in ("worker.int8_activations needs worker.quantization int8", "worker.int8_activations needs a GPU",
                 "worker.int8_activations needs worker.tp = 1"):
        assert text in errs, errs
    c.worker.fp8_activations = True
    assert any("fp8_activations and worker.int8_activations exclude each other" in e for e in c.validate())
    c.worker.fp8_activations = False
    c.worker.quantization, c.worker.device, c.worker.tp, c.worker.mock = "int8", None, 1, False
    c.worker.model = "mixtral-8x7b"
    assert any("int8_activations" in e and "Mixtral" in e for e in c.validate())
    c.worker.model = "llama3-8b"
    assert not [e for e in c.validate() if "activations" in e]
    assert engine_spec(c.worker)["int8_activations"] is True
    p = argparse.ArgumentParser()
    cli._common(p)
    assert cli._overrides(p.parse_args(["--int8-activations"]))["worker"]["int8_activations"] is True
    assert cli._overrides(p.parse_args([]))["worker"]["int8_activations"] is None
