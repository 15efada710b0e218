"""Quantized-only serving (the model keeps only its fp8 / int8 / int4 projection
weights), the parts that need no GPU: the kernel selection of a layer whose bf16
weights are gone, the configuration plumbing down to the engine spec, and the
PyTorch form of dequantize_into."""
import pytest
import torch

from xgserve.cli import _common, _overrides
from xgserve.core.errors import ConfigError
from xgserve.models import get_config
from xgserve.models.llama import PROJECTIONS, LayerDispatch
from xgserve.ops.linear import WQ_FP8, WQ_INT4, WQ_INT8, dequantize_into, dequantize_weight, quantize_weight
from xgserve.server.config import WorkerSection, load_config
from xgserve.server.replica import engine_spec

SMALL, LARGE = (1, 16, 64), (65, 320, 575, 8192)


def _dispatch():
    return LayerDispatch.for_layer(get_config("llama3-8b"), tp=1, on_gpu=True)


def test_dispatch_without_bf16_weights():
    d = _dispatch()
    d.set_quantized(PROJECTIONS, resident=False)
    for T in SMALL:
        s = d.select(T, 0)
        assert (s.qkv, s.o, s.gate_up, s.down, s.attn) == ("w8", "w8", "w8", "w8", "from_partials"), T
    for T in LARGE:
        s = d.select(T, 0)
        assert (s.qkv, s.o, s.gate_up, s.down) == ("dq",) * 4, T
        assert s.attn == "rope", T
    for T in SMALL + LARGE:  # pure-decode steps too: no bf16 family for a released weight
        s = d.select(T, T)
        assert set(s[:4]) <= {"w8", "dq"}, (T, s)


def test_dispatch_partly_quantized_keeps_the_bf16_weight_of_the_rest():
    d = _dispatch()
    d.set_quantized(("gate_up", "down"), resident=False)
    s = d.select(512, 0)
    assert (s.qkv, s.o, s.gate_up, s.down, s.attn) == ("lib", "lib", "dq", "dq", "rope")


def test_dispatch_resident_is_unchanged():
    plain, d = _dispatch(), _dispatch()
    d.set_quantized(PROJECTIONS, resident=True)
    dflt = _dispatch()
    dflt.set_quantized(PROJECTIONS)
    for T in SMALL:
        assert d.select(T, 0) == dflt.select(T, 0) == ("w8", "w8", "w8", "w8", "from_partials")
    for T in LARGE:
        for nd in (0, T):
            assert d.select(T, nd) == dflt.select(T, nd) == plain.select(T, nd), (T, nd)
            assert "dq" not in d.select(T, nd)


def test_config_reports_both_misuses_together():
    with pytest.raises(ConfigError) as ei:
        load_config(env={}, cli=["worker.quantized_only=true", "worker.quantization=bf16", "worker.device=cpu"])
    msg = str(ei.value)
    assert "worker.quantized_only needs worker.quantization fp8|int8|int4" in msg
    assert "worker.quantized_only needs a GPU" in msg


def test_config_default_env_and_set():
    assert WorkerSection().quantized_only is False
    assert load_config(env={}).worker.quantized_only is False
    assert engine_spec(load_config(env={}).worker)["quantized_only"] is False
    cfg = load_config(env={"XGS_WORKER__QUANTIZED_ONLY": "1", "XGS_WORKER__QUANTIZATION": "int8"})
    assert cfg.worker.quantized_only is True
    cfg = load_config(env={}, cli=["worker.quantized_only=true", "worker.quantization=fp8"])
    assert cfg.worker.quantized_only is True and engine_spec(cfg.worker)["weight_dtype"] == "fp8"


def test_cli_shortcut_reaches_engine_spec():
    import argparse
    ap = argparse.ArgumentParser()
    _common(ap)
    a = ap.parse_args(["--quantized-only", "--quantization", "int4"])
    cfg = load_config(env={}, overrides=_overrides(a))
    spec = engine_spec(cfg.worker)
    assert spec["quantized_only"] is True and spec["weight_dtype"] == "int4"
    from xgserve.engine import EngineConfig
    assert "quantized_only" in EngineConfig.__dataclass_fields__ and EngineConfig().quantized_only is False
    a = ap.parse_args(["--quantization", "int4"])
    assert engine_spec(load_config(env={}, overrides=_overrides(a)).worker)["quantized_only"] is False


def test_cli_exit_status_2(capsys):
    from xgserve.cli import main
    assert main(["check-config", "--quantized-only"]) == 2
    assert "quantized_only" in capsys.readouterr().err


@pytest.mark.parametrize("fmt", [WQ_FP8, WQ_INT8, WQ_INT4])
def test_dequantize_into_cpu(fmt):
    torch.manual_seed(fmt)
    q, s = quantize_weight(torch.randn(5, 256) * 0.02, fmt)
    ref = dequantize_weight(q, s, fmt).to(torch.bfloat16)
    w = dequantize_into(q, s, fmt)
    assert w.dtype == torch.bfloat16 and tuple(w.shape) == (5, 256) and torch.equal(w, ref)
    buf = torch.full((5 * 256 + 64,), 7.0, dtype=torch.bfloat16)
    w = dequantize_into(q, s, fmt, out=buf)
    assert w.data_ptr() == buf.data_ptr() and torch.equal(w, ref) and bool((buf[5 * 256:] == 7.0).all())
    with pytest.raises(ValueError):
        dequantize_into(q, s, fmt, out=buf[:5 * 256 - 1])
    with pytest.raises(ValueError):
        dequantize_into(q, s[:-1].contiguous() if s.dim() == 1 else s[:, :-1].contiguous(), fmt)


def test_mock_engine_reports_weight_keys():
    from xgserve.engine.mock import MockEngine
    st = MockEngine().stats()
    assert (st["weight_bytes"], st["scratch_bytes"], st["weight_dtype"]) == (0, 0, "mock")


def test_server_stats_carry_the_weight_keys():
    import asyncio
    import time
    from _server_util import mock_config, run_with_client

    async def fn(c, srv):
        t_end = time.monotonic() + 10
        while True:  # the replica's first heartbeat brings its engine stats
            rep = (await (await c.get("/server/stats")).json())["replicas"][0]
            if rep["engine"] or time.monotonic() > t_end:
                break
            await asyncio.sleep(0.01)
        assert (rep["weight_bytes"], rep["scratch_bytes"], rep["weight_dtype"]) == (0, 0, "mock")
        assert rep["engine"]["weight_dtype"] == "mock"
        return True

    assert run_with_client(mock_config(), fn)


def test_save_checkpoint_refuses_a_quantized_only_model(tmp_path):
    from xgserve.models import save_checkpoint

    class Stub:
        tp, quantized_only = 1, True
    with pytest.raises(ValueError, match="quantized-only"):
        save_checkpoint(Stub(), str(tmp_path / "ck"))
