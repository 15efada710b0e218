"""The fp8_expert_activations key from the config file to the engine, its validation, and moe_f8_plan against
the library's predicate: the parts that need no GPU launch."""
import argparse

import pytest

from xgserve.models import build_model, get_config
from xgserve.ops import _native, linear as L, moe

KEY = "worker.fp8_expert_activations"


def test_config_key_cli_flag_env_and_engine_field(monkeypatch):
    from xgserve import cli
    from xgserve.engine import EngineConfig
    from xgserve.server.config import ServerConfig, load_config
    from xgserve.server.replica import engine_spec
    c = ServerConfig()
    w = c.worker
    assert not w.fp8_expert_activations and not EngineConfig().fp8_expert_activations
    assert engine_spec(w)["fp8_expert_activations"] is False
    w.fp8_expert_activations, w.mock, w.quantized_only, w.quantization, w.device, w.tp = True, True, True, "int8", "cpu", 2
    errs = "\n".join(c.validate())
    for text in ("needs worker.quantization fp8", "needs a GPU", "needs worker.tp = 1",
                 "cannot be combined with worker.quantized_only"):
        assert f"{KEY} {text}" in errs, errs
    w.mock, w.quantized_only, w.quantization, w.device, w.tp, w.model = False, False, "fp8", None, 1, "llama3-8b"
    assert any(KEY in e and "Mixtral only" in e and "worker.fp8_activations" in e for e in c.validate())
    w.model = "mixtral-8x7b"
    assert not [e for e in c.validate() if KEY in e] and engine_spec(w)["fp8_expert_activations"] is True
    p = argparse.ArgumentParser()
    cli._common(p)
    assert cli._overrides(p.parse_args(["--fp8-expert-activations"]))["worker"]["fp8_expert_activations"] is True
    monkeypatch.setenv("XGS_WORKER__FP8_EXPERT_ACTIVATIONS", "true")
    assert load_config(None, overrides={"worker": {"mock": True, "quantization": "fp8"}}).worker.fp8_expert_activations
    for name, why in (("llama-tiny", "Mixtral"), ("mixtral-tiny", "a GPU")):   # quantize_weights refuses the same
        with pytest.raises(ValueError, match=why):
            build_model(get_config(name), device="cpu").quantize_weights("fp8", ea8=True)


def test_plans_satisfy_the_predicate():
    k, cfg = _native.kernels(), get_config("mixtral-8x7b")
    E, H, F = cfg.num_experts, cfg.hidden_size, cfg.intermediate_size
    # few rows per expert: the 128-row tiles; a split of w2 while its tiles leave CUs idle
    for pairs, want in ((257, (1, 1, 2)), (1150, (0, 0, 2)), (16000, (0, 0, 1))):
        c13, c2, S = plan = moe.moe_f8_plan(pairs, E, H, F)
        P = -(-(pairs + 63 * E) // 64) * 64
        assert plan == want and k.moe_f8_supports(E, P, H, 2 * F, pairs, 1, L.MODE_SILU, c13), pairs
        assert k.moe_f8_supports(E, P, F, H, pairs, S, L.MODE_PARTIAL, c2), pairs
    assert moe.moe_f8_plan(256, E, H, F) is None and moe.moe_f8_plan(800, 8, 256 + 64, 256) is None
