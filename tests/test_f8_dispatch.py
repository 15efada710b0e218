"""The "f8" step family (LayerDispatch), the gemm_f8 planner and the fp8_activations key from the
config file to the engine: the parts that need no GPU launch."""
import pytest

from xgserve.models import get_config
from xgserve.models import llama as ll
from xgserve.ops import _native, linear as L

MODES = (L.MODE_BF16, L.MODE_PARTIAL, L.MODE_SILU)
F8_STEP = ("f8",) * 4 + ("from_partials",)


def _dispatch(model="llama3-8b", tp=1, resident=False, fmt=L.WQ_FP8, **kw):
    d = ll.LayerDispatch.for_layer(get_config(model), tp=tp, on_gpu=True)
    d.set_quantized(ll.PROJECTIONS if "gate_up" in d.shapes else ("qkv", "o"), resident=resident, fmt=fmt, **kw)
    return d


def test_plans_are_valid_and_the_predicates_agree():
    k = _native.kernels()
    shapes = {s for m in ("llama3-8b", "llama3-70b", "llama-tiny")
              for s in ll.LayerDispatch.for_layer(get_config(m), 1, on_gpu=True).shapes.values()}
    seen = set()
    for N, K, _ in sorted(shapes):
        for M in (321, 575, 2048, 8192):
            for mode in MODES:
                for cfg in (*L.F8_CFGS, len(L.F8_CFGS)):
                    for S in (1, 2, K // L.F8_KT + 1):
                        ok = L._f8_valid(M, N, K, mode, S, cfg)
                        assert ok == k.f8_supports(M, K, N, S, mode, cfg), (M, N, K, mode, S, cfg)
                        seen.add(ok)
                p = L.f8_plan(M, N, K, mode)
                assert p is None or (L._f8_valid(M, N, K, mode, *p) and (mode == L.MODE_PARTIAL or p[0] == 1))
                assert p is None or p[0] == 1 or K // L.F8_KT // p[0] >= 2   # every split keeps two K tiles
    assert seen == {True, False}
    assert L.f8_plan(321, 6144, 4096, L.MODE_PARTIAL) == (4, 1) and L.f8_plan(512, 6144, 4096, L.MODE_BF16) == (1, 0)
    assert L.f8_plan(321, 4096 + 128, 4096) is None and L._F8_TUNED == {}
    assert [tuple(r) for r in k.gemm_cfgs()["f8"]] == [L.F8_CFGS[c] for c in sorted(L.F8_CFGS)]


@pytest.mark.parametrize("resident", [True, False])
def test_select(resident):
    on, off = _dispatch(resident=resident, a8=True), _dispatch(resident=resident)
    for T in (321, 575, 2048):
        assert tuple(on.select(T, 0)) == F8_STEP, T
        assert on.select(T, 0, mixed_graph=True) == off.select(T, 0, mixed_graph=True)
    for T in (1, 16, 64, 65, 320):
        assert on.select(T, 0) == off.select(T, 0) and on.select(T, T) == off.select(T, T), T
    # off is exactly the dispatch of a model quantized without the argument
    plain = ll.LayerDispatch.for_layer(get_config("llama3-8b"), tp=1, on_gpu=True)
    plain.set_quantized(ll.PROJECTIONS, resident=resident, fmt=L.WQ_FP8)
    assert all(off.select(T, 0) == plain.select(T, 0) for T in (1, 64, 65, 320, 321, 575, 2048, 8192))


def test_a8_changes_nothing_out_of_scope():
    for kw in (dict(fmt=L.WQ_INT8), dict(tp=2), dict(model="mixtral-8x7b")):
        on, off = _dispatch(a8=True, **kw), _dispatch(**kw)
        assert on.f8 == () and all(on.select(T, 0) == off.select(T, 0) for T in (64, 65, 320, 321, 575, 2048)), kw
    cpu = ll.LayerDispatch.for_layer(get_config("llama3-8b"), tp=1, on_gpu=False)
    cpu.set_quantized(ll.PROJECTIONS, resident=True, fmt=L.WQ_FP8, a8=True)
    assert cpu.f8 == ()


def test_config_key_cli_flag_and_engine_field():
    import argparse
    from xgserve import cli
    from xgserve.engine import EngineConfig
    from xgserve.server.config import ServerConfig
    from xgserve.server.replica import engine_spec
    c = ServerConfig()
    assert c.worker.fp8_activations is False and EngineConfig().fp8_activations is False
    assert engine_spec(c.worker)["fp8_activations"] is False
    c.worker.fp8_activations, c.worker.mock = True, True
    c.worker.quantization, c.worker.device, c.worker.tp = "int8", "cpu", 2
    errs = "\n".join(c.validate())
    for text in ("worker.fp8_activations needs worker.quantization fp8", "worker.fp8_activations needs a GPU",
                 "worker.fp8_activations needs worker.tp = 1"):
        assert text in errs, errs
    c.worker.quantization, c.worker.device, c.worker.tp, c.worker.mock = "fp8", None, 1, False
    c.worker.model = "mixtral-8x7b"
    assert any("fp8_activations" in e and "Mixtral" in e for e in c.validate())
    c.worker.model = "llama3-8b"
    assert not [e for e in c.validate() if "fp8_activations" in e]
    assert engine_spec(c.worker)["fp8_activations"] is True
    p = argparse.ArgumentParser()
    cli._common(p)
    assert cli._overrides(p.parse_args(["--fp8-activations"]))["worker"]["fp8_activations"] is True
    assert cli._overrides(p.parse_args([]))["worker"]["fp8_activations"] is None
