"""top_logprobs on the wire (CPU): parsing and 400s on the four generation routes, the
response shapes streamed and not on the mock engine (whose lists are fixed: the emitted
token at -0.25, then ids 3, 4, ... at -1.0, -1.5, ...), one process-replica round trip, a
CPU llama-tiny engine held to torch.log_softmax(...).topk of the fp32 reference's logits,
and requests without the new fields answered exactly as before."""
from __future__ import annotations

import json

import pytest
import torch

from _server_util import mock_config, parse_sse, run_with_client
from xgserve import _runtime as R
from xgserve.core.errors import ValidationError
from xgserve.core.wire import ChatRequest, GenerateRequest, TokenEvent
from xgserve.engine import EngineConfig, LLMEngine, SamplingParams
from xgserve.engine.request import RequestOutput
from xgserve.server.orchestrator import ev_from_tuple, ev_to_tuple, sse_chunk
from xgserve.server.replica import encode_sse_chunk

MSGS = [{"role": "user", "content": "hi"}]
ROUTES = [("/generate", {"prompt": "hello"}), ("/chat", {"messages": MSGS}),
          ("/v1/completions", {"prompt": "hello"}), ("/v1/chat/completions", {"messages": MSGS})]
# fp32 engine against the fp32 reference (the bound of test_sampling_params_wire.py)
TOL = 1e-3


def _ask(route, k):
    """The route's way of asking for k alternatives."""
    if route == "/v1/completions":
        return {"logprobs": k}
    if route == "/v1/chat/completions":
        return {"logprobs": True, "top_logprobs": k}
    return {"top_logprobs": k}


# ------------------------------------------------------------------ parsing, validator
@pytest.mark.parametrize("cls,base", [(GenerateRequest, {"prompt": "x"}), (ChatRequest, {"messages": MSGS})])
def test_parse(cls, base):
    plain = cls.parse(dict(base))
    assert plain.top_logprobs == 0 and plain.logprobs is False
    r = cls.parse(json.dumps({**base, "top_logprobs": 5, "logprobs": True}))
    assert r.top_logprobs == 5 and r.logprobs is True
    assert cls.parse({**base, "top_logprobs": None}).top_logprobs == 0
    for bad in (1.5, "3", True, [2], {"n": 1}):
        with pytest.raises(ValidationError) as e:
            cls.parse({**base, "top_logprobs": bad})
        assert e.value.code == "invalid_parameter" and "Invalid parameter 'top_logprobs'" in str(e.value)


def test_validator_range():
    v = R.RequestValidator(R.ValidatorConfig())
    assert v.check_top_logprobs(0) is None and v.check_top_logprobs(20) is None
    for n in (-1, 21, 10**12):
        res = v.check_top_logprobs(n)
        assert res["field"] == "top_logprobs"
        assert res["message"] == f"Invalid parameter 'top_logprobs': must be an integer between 0 and 20, got {n}"


def test_sampling_params_and_output_defaults():
    assert SamplingParams().top_logprobs == 0
    assert RequestOutput("r", [1], "a", False).top_logprobs is None


def _spy(srv):
    seen = []
    admit = srv.admit

    def spy(kind, ids, params, *a, **kw):
        seen.append(params)
        return admit(kind, ids, params, *a, **kw)

    srv.admit = spy
    return seen


@pytest.mark.parametrize("route,base", ROUTES)
def test_routes_hand_the_value_to_sampling_params(route, base):
    async def fn(c, srv):
        seen = _spy(srv)
        for body in (_ask(route, 7), _ask(route, 0), {}):
            r = await c.post(route, data=json.dumps({**base, "max_tokens": 2, **body}))
            assert r.status == 200, await r.text()
        return seen

    asked, zero, plain = run_with_client(mock_config(), fn)
    assert asked.top_logprobs == 7 and asked.logprobs is True
    assert zero.top_logprobs == 0
    assert zero.logprobs is (route.startswith("/v1/"))  # the aliases' `logprobs` alone asks for the token's own
    assert plain.top_logprobs == 0 and plain.logprobs is False


@pytest.mark.parametrize("route,base", ROUTES)
def test_400s(route, base):
    async def fn(c, srv):
        seen = _spy(srv)
        for k in (-1, 21, 1000):
            r = await c.post(route, data=json.dumps({**base, **_ask(route, k)}))
            d = await r.json()
            assert r.status == 400, d
            assert d["error"]["code"] == "invalid_parameter" and d["error"]["type"] == "invalid_request_error"
            assert f"Invalid parameter 'top_logprobs': must be an integer between 0 and 20, got {k}" in \
                d["error"]["message"]
        for bad in (2.5, "5", [1]):
            r = await c.post(route, data=json.dumps({**base, **_ask(route, bad)}))
            d = await r.json()
            assert r.status == 400 and d["error"]["code"] == "invalid_parameter", d
            assert "must be an integer between 0 and 20" in d["error"]["message"]
        if route == "/v1/chat/completions":  # as at OpenAI
            for body in ({"top_logprobs": 3}, {"top_logprobs": 3, "logprobs": False}):
                r = await c.post(route, data=json.dumps({**base, **body}))
                d = await r.json()
                assert r.status == 400 and d["error"]["code"] == "invalid_parameter", d
                assert "Invalid parameter 'top_logprobs': requires logprobs to be true" in d["error"]["message"]
        assert not seen
        return True

    assert run_with_client(mock_config(), fn)


# ------------------------------------------------------------------ shapes on the mock engine
def _mock_list(tok, k):
    alt = [i for i in range(3, 3 + k + 1) if i != tok][:k - 1]
    return [(tok, -0.25)] + [(i, -1.0 - 0.5 * j) for j, i in enumerate(alt)]


@pytest.mark.parametrize("route,base", ROUTES[:2])
def test_native_routes(route, base):
    K, N = 4, 5

    async def fn(c, srv):
        body = {**base, "max_tokens": N, "ignore_eos": True, "top_logprobs": K}
        r = await c.post(route, data=json.dumps(body))
        d = await r.json()
        assert r.status == 200, d
        s = await c.post(route, data=json.dumps({**body, "stream": True}))
        assert s.status == 200
        only_lp = await (await c.post(route, data=json.dumps({**base, "max_tokens": N, "ignore_eos": True,
                                                              "logprobs": True}))).json()
        return d, parse_sse(await s.read()), only_lp, srv.tokenizer

    d, events, only_lp, tk = run_with_client(mock_config(), fn)
    lp = d["choices"][0]["logprobs"]
    assert sorted(lp) == ["token_ids", "token_logprobs", "tokens", "top_logprobs"]
    assert len(lp["token_ids"]) == N and lp["token_logprobs"] == [-0.25] * N
    assert lp["tokens"] == [tk.decode([t]) for t in lp["token_ids"]]
    for t, top in zip(lp["token_ids"], lp["top_logprobs"]):
        assert top == [{"token": tk.decode([i]), "token_id": i, "logprob": v} for i, v in _mock_list(t, K)]
    toks = [e for e in events if e["type"] == "token"]
    assert toks and events[-1]["type"] == "done"
    for e in toks:
        assert sorted(e) == ["index", "logprob", "token", "top_logprobs", "type"] and e["logprob"] == -0.25
        top = e["top_logprobs"]
        assert len(top) == K and all(sorted(x) == ["logprob", "token", "token_id"] for x in top)
        assert [(x["token_id"], x["logprob"]) for x in top] == _mock_list(top[0]["token_id"], K)
        assert all(x["token"] == tk.decode([x["token_id"]]) for x in top)
    # `logprobs: true` alone: the object without alternatives
    assert "logprobs" in only_lp["choices"][0] and all(t == [] for t in only_lp["choices"][0]["logprobs"]["top_logprobs"])


def test_v1_completions_shapes():
    K, N = 3, 4

    async def fn(c, srv):
        body = {"prompt": "hello", "max_tokens": N, "logprobs": K}
        d = await (await c.post("/v1/completions", data=json.dumps(body))).json()
        s = await c.post("/v1/completions", data=json.dumps({**body, "stream": True}))
        z = await (await c.post("/v1/completions", data=json.dumps({**body, "logprobs": 0}))).json()
        return d, parse_sse(await s.read()), z, srv.tokenizer

    d, events, z, tk = run_with_client(mock_config(), fn)
    lp = d["choices"][0]["logprobs"]
    assert sorted(lp) == ["text_offset", "token_logprobs", "tokens", "top_logprobs"]
    n = len(lp["tokens"])
    assert n == d["usage"]["completion_tokens"] and lp["token_logprobs"] == [-0.25] * n
    assert lp["text_offset"] == [sum(len(t) for t in lp["tokens"][:i]) for i in range(n)]
    for tok, top in zip(lp["tokens"], lp["top_logprobs"]):
        assert isinstance(top, dict) and top[tok] == -0.25 and 1 <= len(top) <= K
        assert sorted(top.values(), reverse=True)[1:] == [-1.0 - 0.5 * j for j in range(len(top) - 1)]
    assert z["choices"][0]["logprobs"]["top_logprobs"] == [{}] * len(z["choices"][0]["logprobs"]["tokens"])
    chunks = [e for e in events if e.get("object") == "text_completion"]
    got = [c["choices"][0]["logprobs"] for c in chunks if "logprobs" in c["choices"][0]]
    assert sum(len(g["tokens"]) for g in got) == n
    assert [t for g in got for t in g["tokens"]] == lp["tokens"]
    assert [o for g in got for o in g["text_offset"]] == lp["text_offset"]
    assert [t for g in got for t in g["top_logprobs"]] == lp["top_logprobs"]
    assert events[-1] == {"type": "[DONE]"}


def test_v1_chat_shapes():
    K, N = 2, 4

    async def fn(c, srv):
        body = {"messages": MSGS, "max_tokens": N, "logprobs": True, "top_logprobs": K}
        d = await (await c.post("/v1/chat/completions", data=json.dumps(body))).json()
        s = await c.post("/v1/chat/completions", data=json.dumps({**body, "stream": True}))
        return d, parse_sse(await s.read())

    d, events = run_with_client(mock_config(), fn)
    content = d["choices"][0]["logprobs"]["content"]
    assert len(content) == d["usage"]["completion_tokens"]
    for ent in content:
        assert sorted(ent) == ["bytes", "logprob", "token", "top_logprobs"]
        assert ent["logprob"] == -0.25 and ent["bytes"] == list(ent["token"].encode("utf-8"))
        assert len(ent["top_logprobs"]) == K
        assert ent["top_logprobs"][0] == {"token": ent["token"], "logprob": -0.25, "bytes": ent["bytes"]}
        assert ent["top_logprobs"][1]["logprob"] == -1.0
        assert all(sorted(t) == ["bytes", "logprob", "token"] for t in ent["top_logprobs"])
    chunks = [e for e in events if e.get("object") == "chat.completion.chunk"]
    got = [x for c in chunks if "logprobs" in c["choices"][0] for x in c["choices"][0]["logprobs"]["content"]]
    assert got == content


# ------------------------------------------------------------------ transport
def test_event_encodings_agree():
    top = [{"token": "a", "token_id": 5, "logprob": -0.25}, {"token": "é", "token_id": 9, "logprob": -1.5}]
    ev = TokenEvent.tok("he\"llo", 3, -0.25, top)
    assert encode_sse_chunk("he\"llo", 3, -0.25, top) == sse_chunk(ev)
    assert TokenEvent.from_dict(json.loads(ev.sse()[6:])).top_logprobs == top
    ev.detail = [(5, -0.25, [(5, -0.25), (9, -1.5)])]
    back = ev_from_tuple(ev_to_tuple(ev))
    assert back.top_logprobs == top and back.detail == ev.detail and back.sse() == ev.sse()
    # absent field: the bytes of before
    assert encode_sse_chunk("x", 0) == sse_chunk(TokenEvent.tok("x", 0)) == \
        b'2e\r\ndata: {"type":"token","token":"x","index":0}\n\n\r\n'
    assert encode_sse_chunk("x", 1, -0.5) == sse_chunk(TokenEvent.tok("x", 1, -0.5))


def test_process_replica_round_trip():
    cfg = mock_config(worker={"in_process": False, "replicas": 1, "mock_latency_ms": 1.0})

    async def fn(c, srv):
        assert srv.replicas[0].kind == "process"
        body = {"prompt": "x", "max_tokens": 4, "ignore_eos": True, "top_logprobs": 3}
        d = await (await c.post("/generate", data=json.dumps(body))).json()
        s = await c.post("/generate", data=json.dumps({**body, "stream": True}))
        return d, parse_sse(await s.read())

    d, events = run_with_client(cfg, fn)
    lp = d["choices"][0]["logprobs"]
    assert len(lp["token_ids"]) == 4
    assert [[(x["token_id"], x["logprob"]) for x in top] for top in lp["top_logprobs"]] == \
        [_mock_list(t, 3) for t in lp["token_ids"]]
    toks = [e for e in events if e["type"] == "token"]
    assert toks and all(len(e["top_logprobs"]) == 3 and e["top_logprobs"][0]["logprob"] == -0.25 for e in toks)


# ------------------------------------------------------------------ a real engine
def test_cpu_engine_lists_match_log_softmax_topk():
    from xgserve.models.reference import reference_logits
    from xgserve.server.config import load_config
    K, N = 5, 8
    eng = LLMEngine(EngineConfig(model="llama-tiny", device="cpu", dtype="float32", num_blocks=64, max_num_seqs=4,
                                 max_num_batched_tokens=128, use_graphs=False, seed=7))
    cfg = load_config(env={}, overrides={"worker": {"model": "llama-tiny", "in_process": True}})

    async def fn(c, srv):
        body = {"prompt": "The quick brown fox", "max_tokens": N, "temperature": 0.0, "ignore_eos": True,
                "top_logprobs": K}
        r = await c.post("/generate", data=json.dumps(body))
        d = await r.json()
        assert r.status == 200, d
        return d, srv.encode(body["prompt"])

    d, prompt = run_with_client(cfg, fn, engine=eng, timeout=120)
    lp = d["choices"][0]["logprobs"]
    gen = lp["token_ids"]
    assert len(gen) == N
    ref = torch.log_softmax(reference_logits(eng.model, prompt + gen[:-1]).float(), -1)
    worst = 0.0
    for i, (tok, tlp, top) in enumerate(zip(gen, lp["token_logprobs"], lp["top_logprobs"])):
        row = ref[len(prompt) - 1 + i]
        want = row.topk(K + 1)
        ids, vals = [x["token_id"] for x in top], [x["logprob"] for x in top]
        assert len(top) == K and ids[0] == tok and abs(vals[0] - tlp) <= TOL
        for t, v in zip(ids, vals):
            worst = max(worst, abs(v - float(row[t])))
        if float(want.values[K - 1] - want.values[K]) > 2 * TOL and float((want.values[:-1] - want.values[1:]).min()) > 2 * TOL:
            assert ids == want.indices[:K].tolist()  # no near-tie in the reference: the same ids in the same order
        else:
            assert float(min(vals)) >= float(want.values[K - 1]) - TOL
    print(f"worst |lp - log_softmax| = {worst:.3e}")
    assert worst <= TOL


# ------------------------------------------------------------------ nothing changes for anyone else
@pytest.mark.parametrize("route,base", ROUTES)
def test_requests_without_the_fields_are_answered_as_before(route, base):
    async def fn(c, srv):
        body = {**base, "max_tokens": 4, "ignore_eos": True}
        d = await (await c.post(route, data=json.dumps(body))).json()
        raw = await (await c.post(route, data=json.dumps({**body, "stream": True}))).read()
        return d, raw

    d, raw = run_with_client(mock_config(), fn)
    assert sorted(d) == ["choices", "created", "id", "model", "object", "usage"]
    keys = ["finish_reason", "index", "message"] if "chat" in route else ["finish_reason", "index", "text"]
    assert sorted(d["choices"][0]) == keys
    assert b"logprob" not in raw
    if not route.startswith("/v1/"):
        for e in parse_sse(raw):
            if e["type"] == "token":  # the event re-encoded from its three fields is the very bytes sent
                assert TokenEvent.tok(e["token"], e["index"]).sse() in raw
                assert sorted(e) == ["index", "token", "type"]
