"""Sampling extensions on the wire and in the engine (CPU): top_k, min_p,
repetition / presence / frequency penalties and logit_bias are parsed strictly on all
four routes, range-checked by the C++ validator (400 with the validator's message),
handed to SamplingParams, refused by a speculating engine, and honoured by a CPU engine
through the fallback ops."""
from __future__ import annotations

import json

import numpy as np
import pytest

from _logit_ref import greedy_reference, process_row
from _server_util import mock_config, run_with_client
from xgserve import _runtime as R
from xgserve.core.errors import ValidationError
from xgserve.core.wire import ChatRequest, GenerateRequest
from xgserve.engine import EngineConfig, LLMEngine, SamplingParams

EXT = {"top_k": 40, "min_p": 0.05, "repetition_penalty": 1.2, "presence_penalty": -0.5, "frequency_penalty": 1,
       "logit_bias": {"7": -100, "11": 2.5}}
MSGS = [{"role": "user", "content": "hi"}]


# ------------------------------------------------------------------ parsing
@pytest.mark.parametrize("cls,base", [(GenerateRequest, {"prompt": "x"}), (ChatRequest, {"messages": MSGS})])
def test_parse_extensions(cls, base):
    plain = cls.parse(dict(base))
    assert (plain.top_k, plain.min_p, plain.repetition_penalty, plain.presence_penalty, plain.frequency_penalty,
            plain.logit_bias) == (0, 0.0, 1.0, 0.0, 0.0, {})
    r = cls.parse(json.dumps({**base, **EXT}))
    assert r.top_k == 40 and r.frequency_penalty == 1.0 and r.presence_penalty == -0.5
    assert r.min_p == float(np.float32(0.05)) and r.repetition_penalty == float(np.float32(1.2))  # f32 like serde
    assert r.logit_bias == {7: -100.0, 11: 2.5}
    # null means absent, as for `seed`
    r = cls.parse({**base, **{k: None for k in EXT}})
    assert r.top_k == 0 and r.logit_bias == {} and r.repetition_penalty == 1.0


@pytest.mark.parametrize("field,bad", [
    ("top_k", -1), ("top_k", 1.5), ("top_k", True), ("top_k", "4"),
    ("min_p", "0.1"), ("min_p", True), ("repetition_penalty", [1.0]), ("presence_penalty", "1"),
    ("frequency_penalty", False), ("logit_bias", [1, 2]), ("logit_bias", "x"), ("logit_bias", {"a": 1.0}),
    ("logit_bias", {"-3": 1.0}), ("logit_bias", {"1.5": 1.0}), ("logit_bias", {"5": "1"}), ("logit_bias", {"5": True}),
    ("logit_bias", {" 5": 1.0}),
])
@pytest.mark.parametrize("cls,base", [(GenerateRequest, {"prompt": "x"}), (ChatRequest, {"messages": MSGS})])
def test_strict_types(cls, base, field, bad):
    with pytest.raises(ValidationError) as e:
        cls.parse({**base, field: bad})
    assert e.value.code == "invalid_json"


def test_duplicate_bias_ids_after_parsing():
    with pytest.raises(ValidationError) as e:
        GenerateRequest.parse({"prompt": "x", "logit_bias": {"7": 1.0, "007": 2.0}})
    assert e.value.code == "invalid_parameter" and "logit_bias" in str(e.value) and "twice" in str(e.value)


# ------------------------------------------------------------------ the C++ validator
def _check(**kw):
    a = dict(min_p=0.0, rp=1.0, pp=0.0, fp=0.0, ids=[], vals=[], vocab=1000)
    a.update(kw)
    return R.RequestValidator(R.ValidatorConfig()).check_processors(a["min_p"], a["rp"], a["pp"], a["fp"], a["ids"],
                                                                    a["vals"], a["vocab"])


def test_validator_accepts_the_ranges_ends():
    assert _check() is None
    assert _check(min_p=1.0, rp=2.0, pp=-2.0, fp=2.0, ids=[0, 999], vals=[-100.0, 100.0]) is None
    assert _check(min_p=0.0, rp=1e-3, pp=2.0, fp=-2.0, ids=list(range(128)), vals=[0.5] * 128) is None
    assert _check(ids=[5000], vals=[1.0], vocab=0) is None  # vocabulary unknown: not checked


@pytest.mark.parametrize("kw,field,msg", [
    (dict(min_p=-0.01), "min_p", "Invalid parameter 'min_p': must be between 0 and 1, got -0.01"),
    (dict(min_p=1.5), "min_p", "Invalid parameter 'min_p': must be between 0 and 1, got 1.5"),
    (dict(min_p=float("nan")), "min_p", "Invalid parameter 'min_p': must be between 0 and 1, got NaN"),
    (dict(rp=0.0), "repetition_penalty",
     "Invalid parameter 'repetition_penalty': must be greater than 0 and at most 2, got 0"),
    (dict(rp=2.5), "repetition_penalty",
     "Invalid parameter 'repetition_penalty': must be greater than 0 and at most 2, got 2.5"),
    (dict(rp=float("nan")), "repetition_penalty",
     "Invalid parameter 'repetition_penalty': must be greater than 0 and at most 2, got NaN"),
    (dict(pp=2.25), "presence_penalty", "Invalid parameter 'presence_penalty': must be between -2 and 2, got 2.25"),
    (dict(pp=float("nan")), "presence_penalty",
     "Invalid parameter 'presence_penalty': must be between -2 and 2, got NaN"),
    (dict(fp=-3.0), "frequency_penalty", "Invalid parameter 'frequency_penalty': must be between -2 and 2, got -3"),
    (dict(fp=float("nan")), "frequency_penalty",
     "Invalid parameter 'frequency_penalty': must be between -2 and 2, got NaN"),
    (dict(ids=[3], vals=[100.5]), "logit_bias",
     "Invalid parameter 'logit_bias': bias of token 3 must be between -100 and 100, got 100.5"),
    (dict(ids=[3], vals=[float("nan")]), "logit_bias",
     "Invalid parameter 'logit_bias': bias of token 3 must be between -100 and 100, got NaN"),
    (dict(ids=[1000], vals=[1.0]), "logit_bias",
     "Invalid parameter 'logit_bias': token id 1000 is outside the vocabulary of 1000"),
    (dict(ids=[4, 9, 4], vals=[1.0, 1.0, 2.0]), "logit_bias",
     "Invalid parameter 'logit_bias': token id 4 is given twice"),
    (dict(ids=list(range(129)), vals=[1.0] * 129), "logit_bias",
     "Invalid parameter 'logit_bias': must have at most 128 entries, got 129"),
])
def test_validator_ranges(kw, field, msg):
    res = _check(**kw)
    assert res is not None and res["field"] == field and res["message"] == msg


# ------------------------------------------------------------------ HTTP
ROUTES = [("/generate", {"prompt": "hello"}), ("/chat", {"messages": MSGS}),
          ("/v1/completions", {"prompt": "hello"}), ("/v1/chat/completions", {"messages": MSGS})]


def _spy(srv):
    seen = []
    admit = srv.admit

    def spy(kind, ids, params, *a, **kw):
        seen.append(params)
        return admit(kind, ids, params, *a, **kw)

    srv.admit = spy
    return seen


@pytest.mark.parametrize("route,base", ROUTES)
def test_routes_hand_the_values_to_sampling_params(route, base):
    async def fn(c, srv):
        seen = _spy(srv)
        r = await c.post(route, data=json.dumps({**base, "max_tokens": 3, **EXT}))
        assert r.status == 200, await r.text()
        r = await c.post(route, data=json.dumps({**base, "max_tokens": 3}))
        assert r.status == 200
        return seen

    sp, plain = run_with_client(mock_config(), fn)
    assert isinstance(sp, SamplingParams) and not sp.plain and sp.needs_counts
    assert sp.top_k == 40 and sp.logit_bias == {7: -100.0, 11: 2.5}
    assert (sp.min_p, sp.repetition_penalty) == (float(np.float32(0.05)), float(np.float32(1.2)))
    assert (sp.presence_penalty, sp.frequency_penalty) == (-0.5, 1.0)
    assert plain.plain and plain.top_k == 0 and plain.logit_bias == {}


@pytest.mark.parametrize("body,needle", [
    ({"min_p": 1.01}, "Invalid parameter 'min_p': must be between 0 and 1, got 1.01"),
    ({"repetition_penalty": 0}, "Invalid parameter 'repetition_penalty': must be greater than 0 and at most 2, got 0"),
    ({"repetition_penalty": 2.01}, "Invalid parameter 'repetition_penalty'"),
    ({"presence_penalty": -2.5}, "Invalid parameter 'presence_penalty': must be between -2 and 2, got -2.5"),
    ({"frequency_penalty": 2.5}, "Invalid parameter 'frequency_penalty': must be between -2 and 2, got 2.5"),
    ({"logit_bias": {"3": 101}}, "Invalid parameter 'logit_bias': bias of token 3 must be between -100 and 100"),
    ({"logit_bias": {"99999999": 1}}, "Invalid parameter 'logit_bias': token id 99999999 is outside the vocabulary"),
    ({"logit_bias": {"7": 1, "07": 1}}, "Invalid parameter 'logit_bias': token id 7 is given twice"),
    ({"logit_bias": {str(i): 1 for i in range(129)}},
     "Invalid parameter 'logit_bias': must have at most 128 entries, got 129"),
])
@pytest.mark.parametrize("route,base", ROUTES)
def test_range_violations_400(route, base, body, needle):
    async def fn(c, srv):
        seen = _spy(srv)
        r = await c.post(route, data=json.dumps({**base, **body}))
        d = await r.json()
        assert r.status == 400, d
        e = d["error"]
        assert e["type"] == "invalid_request_error" and e["code"] == "invalid_parameter"
        assert needle in e["message"], e["message"]
        assert not seen
        return True

    assert run_with_client(mock_config(), fn)


@pytest.mark.parametrize("route,base", ROUTES)
def test_wrong_types_400(route, base):
    async def fn(c, srv):
        for body in ({"top_k": 1.5}, {"min_p": "0.1"}, {"frequency_penalty": True}, {"logit_bias": [1]},
                     {"logit_bias": {"x": 1}}):
            r = await c.post(route, data=json.dumps({**base, **body}))
            d = await r.json()
            assert r.status == 400 and d["error"]["code"] == "invalid_json", (body, d)
        return True

    assert run_with_client(mock_config(), fn)


@pytest.mark.parametrize("route,base", ROUTES)
def test_speculating_server_answers_400(route, base):
    """`spec.draft_model` configured: the five processor fields are refused at the door,
    `top_k` and plain requests pass."""
    async def fn(c, srv):
        seen = _spy(srv)
        for body, field in (({"frequency_penalty": 0.5}, "frequency_penalty"), ({"min_p": 0.1}, "min_p"),
                            ({"logit_bias": {"3": 1}}, "logit_bias"), ({"repetition_penalty": 1.1}, "repetition_penalty"),
                            ({"presence_penalty": 1}, "presence_penalty")):
            r = await c.post(route, data=json.dumps({**base, **body}))
            d = await r.json()
            assert r.status == 400 and d["error"]["code"] == "invalid_parameter", d
            assert f"Invalid parameter '{field}': is not supported together with speculative decoding" in \
                d["error"]["message"]
        assert not seen
        r = await c.post(route, data=json.dumps({**base, "max_tokens": 2, "top_k": 5}))
        assert r.status == 200 and len(seen) == 1
        return True

    assert run_with_client(mock_config(spec={"draft_model": "llama-tiny", "num_speculative_tokens": 2}), fn)


def test_engine_side_rejection_is_a_400_too():
    """A server whose configuration does not say that its engine speculates: the engine's
    own refusal in add_request comes back as the same 400, not as an inference failure."""
    from xgserve.server.config import load_config
    eng = LLMEngine(EngineConfig(model="llama-tiny", device="cpu", dtype="float32", num_blocks=64, max_num_seqs=4,
                                 max_num_batched_tokens=128, use_graphs=False, seed=7, draft_model="llama-tiny",
                                 num_speculative_tokens=2))
    cfg = load_config(env={}, overrides={"worker": {"model": "llama-tiny", "in_process": True}})

    async def fn(c, srv):
        r = await c.post("/generate", data=json.dumps({"prompt": "hello", "max_tokens": 3, "presence_penalty": 0.5}))
        d = await r.json()
        assert r.status == 400, d
        assert d["error"]["code"] == "invalid_parameter" and d["error"]["type"] == "invalid_request_error"
        assert "Invalid parameter 'presence_penalty': is not supported together with speculative decoding" in \
            d["error"]["message"]
        r = await c.post("/generate", data=json.dumps({"prompt": "hello", "max_tokens": 3, "ignore_eos": True}))
        assert r.status == 200 and (await r.json())["usage"]["completion_tokens"] == 3
        return True

    assert run_with_client(cfg, fn, engine=eng, timeout=120)


# ------------------------------------------------------------------ engine (CPU, fallback ops)
def test_speculating_engine_rejects_processed_requests():
    eng = LLMEngine(EngineConfig(model="llama-tiny", device="cpu", dtype="float32", num_blocks=64, max_num_seqs=4,
                                 max_num_batched_tokens=128, use_graphs=False, seed=7, draft_model="llama-tiny",
                                 num_speculative_tokens=2))
    for kw in (dict(frequency_penalty=1.0), dict(min_p=0.1), dict(logit_bias={3: 1.0}), dict(repetition_penalty=1.1),
               dict(presence_penalty=0.5)):
        with pytest.raises(ValueError, match="speculative decoding"):
            eng.add_request("p", [1, 2, 3], SamplingParams(max_tokens=4, temperature=0.0, **kw))
    assert not eng.requests
    assert eng.generate([[1, 2, 3]], SamplingParams(max_tokens=4, temperature=0.0, top_k=5, ignore_eos=True))


def test_engine_rejects_what_the_device_path_cannot_take():
    eng = _gpt2()
    V = eng.mcfg.vocab_size
    for kw in (dict(logit_bias={V: 1.0}), dict(logit_bias={-1: 1.0}), dict(logit_bias={i: 1.0 for i in range(129)}),
               dict(logit_bias={3: float("nan")}), dict(min_p=2.0), dict(repetition_penalty=0.0),
               dict(frequency_penalty=float("inf"))):
        with pytest.raises(ValueError):
            eng.add_request("p", [1, 2, 3], SamplingParams(max_tokens=4, **kw))
    assert not eng.requests


def _gpt2(**kw):
    base = dict(model="gpt2-tiny", device="cpu", dtype="float32", num_blocks=64, max_num_seqs=4,
                max_num_batched_tokens=128, use_graphs=False, seed=11, async_schedule=False)
    base.update(kw)
    return LLMEngine(EngineConfig(**base))


PROMPT = [1, 17, 40, 41, 42, 300, 17]
TOL = 1e-3  # fp32 engine against the fp32 reference: far above their rounding, far below a logit gap that matters


def test_cpu_engine_force_and_ban():
    eng = _gpt2()
    assert eng.runner.p_state is None
    base = eng.generate([PROMPT], SamplingParams(max_tokens=10, temperature=0.0, ignore_eos=True))[0]
    assert eng.runner.p_state is None, "plain requests must not allocate the state table"
    forced = eng.generate([PROMPT], SamplingParams(max_tokens=10, temperature=0.0, ignore_eos=True,
                                                   logit_bias={77: 100.0}))[0]
    assert forced == [77] * 10
    banned = eng.generate([PROMPT], SamplingParams(max_tokens=10, temperature=0.0, ignore_eos=True,
                                                   logit_bias={t: -100.0 for t in set(base)}))[0]
    assert len(banned) == 10 and not set(banned) & set(base)
    assert eng.runner.p_state is not None


def test_cpu_engine_history_against_reference():
    from xgserve.models.reference import reference_logits
    eng = _gpt2()
    pen = dict(repetition_penalty=1.5, frequency_penalty=1.5, presence_penalty=1.0)
    bias = {t: 30.0 for t in (5, 60, 200, 17)}  # 17 is in the prompt

    def logits_fn(ids):
        return reference_logits(eng.model, ids)[-1].float().numpy()

    # the fp32 reference alone: penalised and unpenalised greedy sequences differ
    want = greedy_reference(logits_fn, PROMPT, 24, logit_bias=bias, **pen)
    unpen = greedy_reference(logits_fn, PROMPT, 24, logit_bias=bias)
    assert want != unpen and len(set(unpen[4:])) == 1, (want, unpen)
    # a second, plain request shares the steps
    plain_p = [1, 9, 8, 7]
    sp = SamplingParams(max_tokens=24, temperature=0.0, ignore_eos=True, logit_bias=dict(bias), **pen)
    eng.add_request("pen", PROMPT, sp)
    eng.add_request("plain", plain_p, SamplingParams(max_tokens=24, temperature=0.0, ignore_eos=True))
    outs = {"pen": [], "plain": []}
    while eng.has_work():
        for o in eng.step():
            outs[o.request_id].extend(o.new_token_ids)
    gen = outs["pen"]
    assert len(gen) == 24
    for i, tok in enumerate(gen):
        row = process_row(logits_fn(PROMPT + gen[:i]), PROMPT, gen[:i], logit_bias=bias, **pen)
        assert float(row.max() - row[tok]) < TOL, (i, tok, int(row.argmax()))
    assert gen != eng.generate([PROMPT], SamplingParams(max_tokens=24, temperature=0.0, ignore_eos=True,
                                                        logit_bias=dict(bias)))[0]
    for i, tok in enumerate(outs["plain"]):
        row = logits_fn(plain_p + outs["plain"][:i])
        assert float(row.max() - row[tok]) < TOL, ("plain", i)


def test_cpu_engine_min_p_masks_the_tail():
    """Seeded temperature sampling with min_p = 1 keeps only the maximum: greedy tokens."""
    eng = _gpt2()
    greedy = eng.generate([PROMPT], SamplingParams(max_tokens=8, temperature=0.0, ignore_eos=True))[0]
    got = eng.generate([PROMPT], SamplingParams(max_tokens=8, temperature=1.0, seed=3, min_p=1.0, ignore_eos=True))[0]
    assert got == greedy
    assert eng.runner.p_state is None  # min_p alone needs no token statistics: no state table
