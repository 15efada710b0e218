"""Prompt scores on the wire (CPU, llama-tiny in process): `echo` on /v1/completions, `prompt_logprobs` on
/generate streamed and not, the 400 of a non-bool, and `max_tokens: 0` without `echo` left as it was."""
import json

import pytest

from _server_util import mock_config, parse_sse, run_with_client
from xgserve.engine import EngineConfig, LLMEngine
from xgserve.server.config import load_config

PROMPT = "The quick brown fox"


def ask(route, *bodies):
    eng = LLMEngine(EngineConfig(model="llama-tiny", device="cpu", dtype="float32", num_blocks=64, max_num_seqs=4,
                                 max_num_batched_tokens=128, use_graphs=False, seed=7))

    async def fn(c, srv):
        res = [await c.post(route, data=json.dumps({"prompt": PROMPT, "temperature": 0.0, **b})) for b in bodies]
        return [(r.status, await r.read()) for r in res], srv.encode(PROMPT), srv.tokenizer

    cfg = load_config(env={}, overrides={"worker": {"model": "llama-tiny", "in_process": True}})
    return run_with_client(cfg, fn, engine=eng, timeout=120)


@pytest.mark.parametrize("n", (3, 0))
def test_v1_completions_echo(n):
    (echo, plain), ids, tk = ask("/v1/completions", {"max_tokens": n, "logprobs": 5, "echo": True},
                                 {"max_tokens": max(n, 1), "logprobs": 5})
    ch, want = json.loads(echo[1])["choices"][0], json.loads(plain[1])["choices"][0]
    tail = want if n else {"text": "", "logprobs": {k: [] for k in want["logprobs"]}}
    lp, P = ch["logprobs"], len(ids)
    assert echo[0] == 200 and ch["text"] == PROMPT + tail["text"] and ch["finish_reason"] == "length"
    assert json.loads(echo[1])["usage"]["completion_tokens"] == n
    assert lp["tokens"] == [tk.decode([t]) for t in ids] + tail["logprobs"]["tokens"]
    assert lp["token_logprobs"][0] is None and lp["top_logprobs"][0] is None
    # (the plain run hits the prefix cache the echo run filled: other chunks, fp32 round-off apart)
    assert lp["token_logprobs"][P:] == pytest.approx(tail["logprobs"]["token_logprobs"], abs=1e-4)
    assert [sorted(t) for t in lp["top_logprobs"][P:]] == [sorted(t) for t in tail["logprobs"]["top_logprobs"]]
    assert all(isinstance(x, float) and x <= 0 for x in lp["token_logprobs"][1:P])
    assert all(len(t) == 1 and max(t.values()) >= x - 1e-6 for t, x in zip(lp["top_logprobs"][1:P], lp["token_logprobs"][1:P]))
    assert lp["text_offset"] == [sum(len(t) for t in lp["tokens"][:i]) for i in range(len(lp["tokens"]))]


def test_generate_prompt_logprobs_and_absent_key():
    (full, stream, plain, bad), ids, tk = ask(
        "/generate", {"max_tokens": 2, "prompt_logprobs": True}, {"max_tokens": 2, "prompt_logprobs": True, "stream": True},
        {"max_tokens": 2}, {"max_tokens": 2, "prompt_logprobs": 1})
    obj = json.loads(full[1])["prompt_logprobs"]
    assert sorted(obj) == ["token_ids", "token_logprobs", "tokens", "top_logprobs"] and obj["token_ids"] == ids
    assert obj["token_logprobs"][0] is None and obj["top_logprobs"][0] == [] and None not in obj["token_logprobs"][1:]
    assert all(len(t) == 1 and sorted(t[0]) == ["logprob", "token", "token_id"] and t[0]["token"] == tk.decode([t[0]["token_id"]])
               for t in obj["top_logprobs"][1:])
    events = parse_sse(stream[1])
    assert events[-1]["type"] == "done" and events[-1]["prompt_logprobs"] == obj
    assert all("prompt_logprobs" not in e for e in events[:-1])
    assert plain[0] == 200 and b"prompt_logprobs" not in plain[1]
    assert bad[0] == 400 and "Invalid parameter 'prompt_logprobs': must be a boolean" in json.loads(bad[1])["error"]["message"]


def test_max_tokens_zero_without_echo_is_admitted_as_before():
    async def fn(c, srv):
        seen, admit = [], srv.admit
        srv.admit = lambda kind, ids, params, *a, **kw: (seen.append(params), admit(kind, ids, params, *a, **kw))[1]
        r = await c.post("/v1/completions", data=json.dumps({"prompt": PROMPT, "max_tokens": 0, "logprobs": 1}))
        return r.status, await r.json(), seen[0]

    status, d, sp = run_with_client(mock_config(), fn)
    assert status == 200 and sp.max_tokens == 0 and sp.prompt_logprobs is False
    assert not d["choices"][0]["text"].startswith(PROMPT) and None not in d["choices"][0]["logprobs"]["token_logprobs"]
