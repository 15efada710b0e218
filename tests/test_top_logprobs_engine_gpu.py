"""top_logprobs through the engine on the GPU: a llama-tiny engine with graphs and
asynchronous scheduling, four concurrent requests of 12 tokens, one of them asking.

The lists must describe the distribution the emitted logprob refers to (entry 0 of a greedy
row is the emitted token, within LP_TOL = 1e-3 of its logprob -- two kernels' fp32
log-sum-exp of one row), be sorted, hold at most the whole probability mass, not depend on
how many entries were asked, and leave every request's tokens exactly as they are."""
import math

import pytest
import torch

from xgserve.engine import EngineConfig, LLMEngine, SamplingParams
from xgserve.ops import _native

pytestmark = pytest.mark.gpu
LP_TOL = 1e-3
PROMPTS = {"A": [1] + list(range(10, 40)), "B": [1, 5, 9, 200, 300], "C": [1] + list(range(100, 160)),
           "D": [1] + list(range(300, 317))}


def _engine(**kw):
    _native.kernels()
    base = dict(model="llama-tiny", device="cuda:0", num_blocks=256, max_num_seqs=8, max_num_batched_tokens=512,
                max_model_len=256, graph_batch_sizes=[1, 2, 4, 8], seed=7, enable_prefix_cache=False)
    base.update(kw)
    return LLMEngine(EngineConfig(**base))


def _params(a_top, a_kw):
    def sp(**kw):
        return SamplingParams(max_tokens=12, ignore_eos=True, **kw)
    a = dict(temperature=0.0, seed=1)
    a.update(a_kw)
    return {"A": sp(top_logprobs=a_top, **a), "B": sp(temperature=0.0, seed=2),
            "C": sp(temperature=0.8, top_k=40, seed=11), "D": sp(temperature=0.0, seed=4)}


def _run(eng, params):
    toks, lps, tops = {}, {}, {}
    for rid, sp in params.items():
        eng.add_request(rid, PROMPTS[rid], sp)
    while eng.has_work():
        for o in eng.step():
            toks.setdefault(o.request_id, []).extend(o.new_token_ids)
            if o.top_logprobs is not None:
                # one list per new token of this very output (a verify step emits several)
                assert len(o.top_logprobs) == len(o.new_token_ids) == len(o.logprobs)
                tops.setdefault(o.request_id, []).extend(o.top_logprobs)
                lps.setdefault(o.request_id, []).extend(o.logprobs)
            else:
                assert o.request_id != "A" or not o.new_token_ids or not params["A"].top_logprobs
    torch.cuda.synchronize()
    return toks, lps, tops


def _check_lists(toks, lps, tops, k, greedy):
    assert len(tops) == len(toks) == len(lps) == 12
    worst = 0.0
    for tok, lp, top in zip(toks, lps, tops):
        assert len(top) == k
        ids, vals = [t[0] for t in top], [t[1] for t in top]
        assert len(set(ids)) == k and all(0 <= i < 512 for i in ids)
        assert all(a >= b for a, b in zip(vals, vals[1:])), vals
        assert sum(math.exp(v) for v in vals) <= 1 + LP_TOL
        if greedy:
            assert ids[0] == tok
        if tok in ids:  # a drawn token that is listed carries the emitted logprob
            worst = max(worst, abs(vals[ids.index(tok)] - lp))
    print(f"worst |listed lp - emitted logprob| = {worst:.3e}")
    assert worst <= LP_TOL
    return worst


CONFIGS = {
    "graphs_async": dict(),
    "eager": dict(use_graphs=False),
    "speculating": dict(draft_model="llama-tiny", num_speculative_tokens=2),
}
REQUEST_A = {
    "greedy": dict(),
    "sampled": dict(temperature=0.9, seed=5),
    "penalised": dict(repetition_penalty=1.3),
}


# logit processors are refused on a speculating engine, so that pair does not exist
COMBOS = [(c, a) for c in sorted(CONFIGS) for a in sorted(REQUEST_A) if (c, a) != ("speculating", "penalised")]


@pytest.mark.parametrize("config,a_kind", COMBOS)
def test_only_the_asking_request_gets_lists(config, a_kind):
    a_kw = REQUEST_A[a_kind]
    eng = _engine(**CONFIGS[config])
    if config == "graphs_async":
        assert eng._async and eng.runner.graphs
    if config == "speculating":
        assert eng.spec is not None
    base, _, none = _run(eng, _params(0, a_kw))
    assert not none and eng.runner.t_out is None  # nobody asked: nothing allocated, nothing launched
    toks5, lps5, tops5 = _run(eng, _params(5, a_kw))
    assert toks5 == base and all(len(v) == 12 for v in base.values())
    assert sorted(tops5) == ["A"]
    _check_lists(toks5["A"], lps5["A"], tops5["A"], 5, greedy=a_kind != "sampled")
    toks20, lps20, tops20 = _run(eng, _params(20, a_kw))
    assert toks20 == base
    _check_lists(toks20["A"], lps20["A"], tops20["A"], 20, greedy=a_kind != "sampled")
    assert [t[:5] for t in tops20["A"]] == tops5["A"]  # bit for bit: ids and logprobs
    if config == "speculating":
        st = eng.stats()["speculative"]
        assert st["draft_tokens_proposed"] > 0 and st["mean_tokens_per_verify"] > 1.0
    if a_kind == "penalised" and config == "graphs_async":
        assert eng.runner.proc_graphs


def test_every_row_asking_through_the_mixed_and_decode_graphs():
    """All four ask for different counts, so one launch serves rows with different K."""
    eng = _engine()
    ks = {"A": 3, "B": 20, "C": 1, "D": 7}
    params = {rid: SamplingParams(max_tokens=12, temperature=0.0, ignore_eos=True, top_logprobs=k)
              for rid, k in ks.items()}
    toks, lps, tops = _run(eng, params)
    base, _, _ = _run(eng, {rid: SamplingParams(max_tokens=12, temperature=0.0, ignore_eos=True) for rid in ks})
    assert toks == base
    for rid, k in ks.items():
        _check_lists(toks[rid], lps[rid], tops[rid], k, greedy=True)
