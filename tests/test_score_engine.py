"""SamplingParams.prompt_logprobs through the engine: llama-tiny with a prompt of three prefill chunks
(a target crosses each chunk boundary) against the fp32 reference model's log_softmax. On the CPU the
fp32 fallback of ops.score_rows carries the plumbing; the gpu case runs the HIP kernel on bf16 weights."""
import types

import pytest
import torch

from xgserve.engine import EngineConfig, LLMEngine, SamplingParams
from xgserve.engine import engine as engine_mod
from xgserve.engine.request import UnsupportedSampling
from xgserve.models.reference import reference_logits

PROMPT = [1] + [(37 * i + 11) % 500 + 3 for i in range(70)]  # 71 tokens; 32-token steps: chunks of 32, 32, 7
PLAIN = [1] + [(29 * i + 5) % 500 + 3 for i in range(20)]
# fp32 on both sides, sums of <= 256 products of O(1) terms in different orders: a few 1e-6 per logit
CPU_TOL = 1e-4
# bf16 model against the fp32 reference: twice the gap of GENERATED-token logprobs (8 greedy tokens after
# PROMPT), which measured 0.0052 on an MI355X (profiles/score.md)
GPU_TOL = 2 * 0.0052


def engine(device="cpu", dtype="float32", **kw):
    return LLMEngine(EngineConfig(model="llama-tiny", device=device, dtype=dtype, num_blocks=64, max_num_seqs=4,
                                  max_num_batched_tokens=32, use_graphs=False, **kw))


def run(eng, reqs):
    """reqs: {id: (prompt, params)} -> {id: (token ids, prompt_logprobs, last output)}"""
    for rid, (p, sp) in reqs.items():
        eng.add_request(rid, p, sp)
    res = {rid: [[], None, None] for rid in reqs}
    while any(r[2] is None or not r[2].finished for r in res.values()):
        for o in eng.step():
            r = res[o.request_id]
            r[0].extend(o.new_token_ids)
            r[1], r[2] = (o.prompt_logprobs if o.prompt_logprobs is not None else r[1]), o
    return res


def scored(max_tokens=3):
    return SamplingParams(max_tokens=max_tokens, temperature=0.0, ignore_eos=True, prompt_logprobs=True)


def check_against_reference(eng, scores, tol):
    ref = torch.log_softmax(reference_logits(eng.model, PROMPT).float().cpu(), dim=-1)
    assert len(scores) == len(PROMPT) and scores[0] is None and all(s is not None for s in scores[1:])
    worst = 0.0
    for i in range(1, len(PROMPT)):
        lp, best_id, best_lp = scores[i]
        row = ref[i - 1]
        worst = max(worst, abs(lp - float(row[PROMPT[i]])), abs(best_lp - float(row.max())))
        assert float(row.max() - row[best_id]) <= tol, (i, best_id, int(row.argmax()))
        if tol == CPU_TOL:
            assert best_id == int(row.argmax())
    print(f"prompt logprobs: worst gap {worst:.3e} of {tol:.1e}")
    assert worst <= tol


def test_prompt_logprobs_match_reference_across_chunks():
    eng = engine()
    toks, scores, last = run(eng, {"a": (PROMPT, scored())})["a"]
    assert len(toks) == 3 and last.finish_reason == "length"
    check_against_reference(eng, scores, CPU_TOL)
    toks, scores, last = run(eng, {"z": (PROMPT, scored(max_tokens=0))})["z"]  # scoring only
    assert toks == [] and last.finished and last.finish_reason == "length" and last.completion_tokens == 0
    check_against_reference(eng, scores, CPU_TOL)
    assert run(eng, {"b": (PROMPT, SamplingParams(max_tokens=2, temperature=0.0, ignore_eos=True))})["b"][1] is None


def test_prefix_cache_is_bypassed():
    eng = engine(enable_prefix_cache=True)
    first = run(eng, {"a": (PROMPT, scored())})["a"]
    second = run(eng, {"b": (PROMPT, scored())})["b"]
    assert all(s is not None for s in second[1][1:])
    assert second[1] == first[1] and second[0] == first[0]


def test_plain_request_unchanged_beside_a_scored_one():
    plain = SamplingParams(max_tokens=6, temperature=0.0, ignore_eos=True)
    alone = run(engine(), {"p": (PLAIN, plain)})["p"][0]
    both = run(engine(), {"s": (PROMPT, scored()), "p": (PLAIN, plain)})
    assert both["p"][0] == alone and both["p"][1] is None
    assert all(s is not None for s in both["s"][1][1:])


def test_refused_with_tp_or_draft_model(monkeypatch):
    eng = engine()
    with pytest.raises(UnsupportedSampling):
        eng.add_request("x", PROMPT, SamplingParams(prompt_logprobs=1))
    monkeypatch.setattr(eng, "spec", object())
    with pytest.raises(UnsupportedSampling):
        eng.add_request("d", PROMPT, scored())
    monkeypatch.setattr(eng, "spec", None)
    monkeypatch.setattr(engine_mod, "get_state", lambda: types.SimpleNamespace(tp_size=2))
    with pytest.raises(UnsupportedSampling):
        eng.add_request("t", PROMPT, scored())
    assert not eng.requests


@pytest.mark.gpu
def test_prompt_logprobs_gpu_bf16():
    eng = engine(device="cuda:0", dtype="bfloat16")
    toks, scores, _ = run(eng, {"a": (PROMPT, scored())})["a"]
    assert len(toks) == 3
    check_against_reference(eng, scores, GPU_TOL)
