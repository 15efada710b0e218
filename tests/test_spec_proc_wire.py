"""spec.processors on the wire and in the configuration: a speculating server started
with the key lets the five processor fields through on all four routes, the key travels
from the environment / --set into the replica's engine, and the three configurations it
cannot serve are refused at start-up."""
from __future__ import annotations

import json

import pytest

from _server_util import mock_config, run_with_client
from xgserve.engine import EngineConfig, SamplingParams

MSGS = [{"role": "user", "content": "hi"}]
ROUTES = [("/generate", {"prompt": "hello"}), ("/chat", {"messages": MSGS}),
          ("/v1/completions", {"prompt": "hello"}), ("/v1/chat/completions", {"messages": MSGS})]
FIELDS = [({"frequency_penalty": 0.5}, "frequency_penalty", 0.5), ({"min_p": 0.25}, "min_p", 0.25),
          ({"logit_bias": {"3": 1}}, "logit_bias", {3: 1.0}), ({"repetition_penalty": 1.5}, "repetition_penalty", 1.5),
          ({"presence_penalty": 1}, "presence_penalty", 1.0)]
SPEC = {"draft_model": "llama-tiny", "num_speculative_tokens": 2}


def _spy(srv):
    seen = []
    admit = srv.admit

    def spy(kind, ids, params, *a, **kw):
        seen.append(params)
        return admit(kind, ids, params, *a, **kw)

    srv.admit = spy
    return seen


@pytest.mark.parametrize("route,base", ROUTES)
def test_processor_fields_pass_with_the_key(route, base):
    async def fn(c, srv):
        seen = _spy(srv)
        for body, _, _ in FIELDS:
            r = await c.post(route, data=json.dumps({**base, "max_tokens": 2, **body}))
            assert r.status == 200, await r.text()
        return seen

    seen = run_with_client(mock_config(spec={**SPEC, "processors": True}), fn)
    assert len(seen) == len(FIELDS)
    for sp, (_, name, value) in zip(seen, FIELDS):
        assert isinstance(sp, SamplingParams) and not sp.plain and getattr(sp, name) == value


@pytest.mark.parametrize("route,base", ROUTES)
def test_range_checks_stay_with_the_key(route, base):
    async def fn(c, srv):
        r = await c.post(route, data=json.dumps({**base, "min_p": 1.5}))
        d = await r.json()
        assert r.status == 400 and "Invalid parameter 'min_p': must be between 0 and 1" in d["error"]["message"]
        return True

    assert run_with_client(mock_config(spec={**SPEC, "processors": True}), fn)


def test_config_key_env_and_set():
    from xgserve.server.config import SpecSection, load_config
    from xgserve.server.replica import engine_spec, make_engine  # noqa: F401
    assert SpecSection().processors is False and EngineConfig().spec_processors is False
    cfg = load_config(env={})
    assert cfg.spec.processors is False and engine_spec(cfg.worker, spec=cfg.spec)["spec_processors"] is False
    env = {"XGS_SPEC__DRAFT_MODEL": "llama-tiny", "XGS_SPEC__NUM_SPECULATIVE_TOKENS": "3", "XGS_SPEC__PROCESSORS": "1"}
    assert load_config(env=env).spec.processors is True
    cfg = load_config(env={}, cli=["spec.draft_model=llama-tiny", "spec.num_speculative_tokens=3",
                                   "spec.processors=true"])
    es = engine_spec(cfg.worker, spec=cfg.spec)
    assert cfg.spec.processors is True and es["spec_processors"] is True
    keys = set(EngineConfig.__dataclass_fields__)
    assert EngineConfig(**{k: v for k, v in es.items() if k in keys}).spec_processors is True


@pytest.mark.parametrize("cli,needle", [
    (["spec.processors=true"], "spec.processors requires spec.draft_model"),
    (["spec.processors=true", "spec.draft_model=llama-tiny"], "spec.processors requires spec.draft_model"),
    (["spec.processors=true", "spec.draft_model=llama-tiny", "spec.num_speculative_tokens=17"],
     "at most 16 speculative tokens (LOGIT_HIST_MAX)"),
    (["spec.processors=true", "spec.draft_model=llama-tiny", "spec.num_speculative_tokens=3", "worker.tp=2"],
     "spec.processors requires worker.tp = 1"),
])
def test_configuration_errors(cli, needle, capsys):
    from xgserve.cli import main
    from xgserve.server.config import ConfigError, load_config
    with pytest.raises(ConfigError) as e:
        load_config(env={}, cli=cli)
    assert needle in str(e.value)
    argv = ["check-config"]
    for kv in cli:
        argv += ["--set", kv]
    assert main(argv) == 2
    assert needle in capsys.readouterr().err


def test_valid_configuration_passes():
    from xgserve.cli import main
    assert main(["check-config", "--set", "spec.processors=true", "--set", "spec.draft_model=llama-tiny", "--set",
                 "spec.num_speculative_tokens=16"]) == 0
