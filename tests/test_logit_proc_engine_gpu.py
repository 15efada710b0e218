"""Logit processors through the engine on the GPU (the 2-layer llama3-8b of
test_engine_gpu.py): forced / banned tokens, penalties that follow the generated history
step by step against the fp32 reference, the same tokens with graphs on and off, with and
without asynchronous scheduling, through the mixed-step graphs and across a pre-emption,
and an engine that only ever sees plain requests staying exactly as it was."""
from dataclasses import replace

import pytest
import torch

from _logit_ref import greedy_reference, process_row
from xgserve.engine import EngineConfig, LLMEngine, SamplingParams
from xgserve.models import build_model, get_config
from xgserve.models.reference import reference_logits
from xgserve.ops import _native

pytestmark = pytest.mark.gpu

NEAR_TIE = 0.15  # the near-tie bound of test_engine_gpu.py for this model (bf16 engine vs fp32 reference)
PEN = dict(repetition_penalty=1.5, frequency_penalty=1.5, presence_penalty=1.0)
BIAS = {1000: 30.0, 2000: 30.0, 50000: 30.0, 128255: 30.0}  # without penalties the output repeats
PROMPT = [128000] + list(range(1000, 1040))                  # token 1000 is in the prompt and biased


def _engine(model, **kw):
    base = dict(model=model.cfg.name, device="cuda:0", num_blocks=512, max_num_seqs=16,
                max_num_batched_tokens=2048, max_model_len=1024, graph_batch_sizes=[1, 2, 4, 8])
    base.update(kw)
    return LLMEngine(EngineConfig(**base), model=model)


@pytest.fixture(scope="module")
def llama_small():
    _native.kernels()
    cfg = replace(get_config("llama3-8b"), num_layers=2, name="llama3-8b-2l")
    return build_model(cfg, device="cuda:0", seed=3)


def _greedy(n, **kw):
    return SamplingParams(max_tokens=n, temperature=0.0, ignore_eos=True, **kw)


def _run(eng, reqs, late=None, late_at=3):
    """reqs / late: {id: (prompt, params)}; late ones arrive after `late_at` steps."""
    outs = {}
    for rid, (p, sp) in reqs.items():
        eng.add_request(rid, p, sp)
    n = 0
    while eng.has_work():
        for o in eng.step():
            outs.setdefault(o.request_id, []).extend(o.new_token_ids)
        n += 1
        if late and n == late_at:
            for rid, (p, sp) in late.items():
                eng.add_request(rid, p, sp)
    assert eng.sched.num_inflight() == 0 and eng.sched.num_running() == 0
    return outs


def _check_against_reference(model, prompt, gen, **params):
    """Teacher-forced: every token within NEAR_TIE of the maximum of its processed fp32 reference row."""
    ref = reference_logits(model, prompt + gen[:-1]).float().cpu().numpy()
    for i, tok in enumerate(gen):
        row = process_row(ref[len(prompt) - 1 + i], prompt, gen[:i], **params)
        gap = float(row.max() - row[tok])
        assert gap < NEAR_TIE, (i, tok, int(row.argmax()), gap)


def test_force_and_ban(llama_small):
    eng = _engine(llama_small)
    base = eng.generate([PROMPT], _greedy(12))[0]
    forced = eng.generate([PROMPT], _greedy(12, logit_bias={4242: 100.0}))[0]
    assert forced == [4242] * 12
    banned = eng.generate([PROMPT], _greedy(12, logit_bias={t: -100.0 for t in set(base)}))[0]
    assert len(banned) == 12 and not set(banned) & set(base)
    _check_against_reference(llama_small, PROMPT, banned, logit_bias={t: -100.0 for t in set(base)})


def test_history_across_steps(llama_small):
    def logits_fn(ids):
        return reference_logits(llama_small, ids)[-1].float().cpu().numpy()

    # the fp32 reference alone: its penalised and unpenalised greedy sequences differ
    want = greedy_reference(logits_fn, PROMPT, 24, logit_bias=BIAS, **PEN)
    unpen = greedy_reference(logits_fn, PROMPT, 24, logit_bias=BIAS)
    assert want != unpen
    eng = _engine(llama_small)
    plain_p = [128000] + list(range(300, 330))
    outs = _run(eng, {"pen": (PROMPT, _greedy(24, logit_bias=dict(BIAS), **PEN)), "plain": (plain_p, _greedy(24))})
    assert len(outs["pen"]) == 24 and len(outs["plain"]) == 24
    _check_against_reference(llama_small, PROMPT, outs["pen"], logit_bias=BIAS, **PEN)
    # a plain request that shared every step with the penalised one: untouched
    _check_against_reference(llama_small, plain_p, outs["plain"])
    assert eng.runner.proc_graphs, "the processed decode graphs were not used"
    nopen = _engine(llama_small).generate([PROMPT], _greedy(24, logit_bias=dict(BIAS)))[0]
    assert outs["pen"] != nopen


def _request_set(temperature):
    """Penalised, biased, min_p and plain requests in one batch; equal lengths, so the steps'
    batch composition (hence their bf16 rounding) is the same in every run mode."""
    def sp(n, seed, **kw):
        return SamplingParams(max_tokens=n, temperature=temperature, ignore_eos=True, seed=seed, **kw)

    return {
        "pen": (PROMPT, sp(12, 21, logit_bias=dict(BIAS), **PEN)),
        "bias": ([128000] + list(range(500, 523)), sp(12, 22, logit_bias={7: 25.0, 8: 24.0, 128000: -100.0})),
        "minp": ([128000] + list(range(700, 745)), sp(12, 23, min_p=0.2, repetition_penalty=1.3, top_k=50)),
        "freq": ([128000] + list(range(900, 917)), sp(12, 24, frequency_penalty=2.0, logit_bias={11: 28.0, 12: 27.0})),
        "plain": ([128000] + list(range(300, 330)), sp(12, 25)),
    }


@pytest.mark.parametrize("temperature", [0.0, 0.8])
def test_graphs_and_async_schedule_give_the_same_tokens(llama_small, temperature):
    want = _run(_engine(llama_small), _request_set(temperature))
    assert sorted(want) == ["bias", "freq", "minp", "pen", "plain"] and all(len(v) == 12 for v in want.values())
    eager = _engine(llama_small, use_graphs=False)
    assert _run(eager, _request_set(temperature)) == want
    assert not eager.runner.proc_graphs and eager.runner.p_state is not None
    sync = _engine(llama_small, async_schedule=False)
    assert not sync._async
    assert _run(sync, _request_set(temperature)) == want
    if temperature == 0.0:
        for rid, (p, sp) in _request_set(0.0).items():
            _check_against_reference(llama_small, p, want[rid], logit_bias=sp.logit_bias,
                                     repetition_penalty=sp.repetition_penalty, frequency_penalty=sp.frequency_penalty,
                                     presence_penalty=sp.presence_penalty)


def _mixed_run(model, use_graphs, async_schedule, strip=False):
    """16 rows decoding, every other one penalised, while two long prompts arrive and ride the
    decode steps in 128-token chunks. strip: the same prompts and lengths with every request
    plain -- the same schedule and batch composition through the unprocessed graphs."""
    eng = _engine(model, decode_prefill_cap=128, decode_prefill_seqs=1, graph_batch_sizes=[1, 2, 4, 8, 16, 24, 32],
                  max_num_seqs=32, use_graphs=use_graphs, async_schedule=async_schedule)
    reqs = {}
    for i in range(16):
        kw = dict(logit_bias={100 + i: 30.0, 200 + i: 29.0}, **PEN) if i % 2 == 0 else {}
        reqs[f"d{i}"] = ([128000] + list(range(900 + 3 * i, 940 + 3 * i)), _greedy(16, **kw))
    late = {"p0": ([128000] + list(range(2000, 2300)), _greedy(6, logit_bias={2000: 30.0, 2001: 29.5}, **PEN)),
            "p1": ([128000] + list(range(3000, 3337)), _greedy(6))}
    if strip:
        reqs = {rid: (p, _greedy(sp.max_tokens)) for rid, (p, sp) in reqs.items()}
        late = {rid: (p, _greedy(sp.max_tokens)) for rid, (p, sp) in late.items()}
    return reqs, late, _run(eng, reqs, late), eng


def test_mixed_step_graphs(llama_small):
    """The same request set through the captured mixed graphs (decode rows + one prompt
    chunk), token for token:
    * its plain rows against the same schedule with every request plain, through the
      unprocessed mixed graphs: the same kernels on the same batch composition, and the
      bf16 -> fp32 conversion of a plain row is exact, so the logits are bit-equal;
    * its penalised rows against the eager run of the same schedule (graphs off);
    * under asynchronous scheduling the plain rows against the all-plain asynchronous run
      and the penalised rows against the synchronous mixed-graph run.
    Every token of both processed runs is also held to the fp32 reference, the prompt
    chunk's first generated token included (bias and prompt repetition)."""
    reqs, late, outs, eng = _mixed_run(llama_small, True, False)
    every = {**reqs, **late}
    plain = [rid for rid, (_, sp) in every.items() if sp.plain]
    pen = [rid for rid, (_, sp) in every.items() if not sp.plain]
    assert len(plain) == 9 and len(pen) == 9
    assert eng.runner.mixed_graphs and eng.runner.proc_mixed_graphs, "no processed mixed graph was used"
    assert eng.runner.mixed_replays >= 4
    _, _, eager, _ = _mixed_run(llama_small, False, False)
    _, _, unproc, e2 = _mixed_run(llama_small, True, False, strip=True)
    assert e2.runner.mixed_replays == eng.runner.mixed_replays and not e2.runner.proc_mixed_graphs
    assert sorted(outs) == sorted(eager) == sorted(unproc)
    assert {rid: outs[rid] for rid in pen} == {rid: eager[rid] for rid in pen}
    assert {rid: outs[rid] for rid in plain} == {rid: unproc[rid] for rid in plain}
    _, _, ahead, eng = _mixed_run(llama_small, True, True)
    assert eng._async and eng.runner.proc_mixed_graphs and eng.stats()["lookahead_launches"] > 0
    _, _, unproc_ahead, e3 = _mixed_run(llama_small, True, True, strip=True)
    assert e3._async and e3.runner.mixed_replays == eng.runner.mixed_replays
    assert {rid: ahead[rid] for rid in plain} == {rid: unproc_ahead[rid] for rid in plain}
    assert {rid: ahead[rid] for rid in pen} == {rid: outs[rid] for rid in pen}
    for got in (outs, ahead):
        assert all(len(got[f"d{i}"]) == 16 for i in range(16)) and len(got["p0"]) == 6 and len(got["p1"]) == 6
        for rid, (p, sp) in every.items():
            kw = PEN if sp.logit_bias else {}
            _check_against_reference(llama_small, p, got[rid], logit_bias=sp.logit_bias, **kw)


TIGHT = dict(repetition_penalty=1.2, frequency_penalty=0.3, presence_penalty=0.5)


def _tight_run(model, num_blocks):
    eng = _engine(model, num_blocks=num_blocks, enable_prefix_cache=False)
    reqs = {f"s{i}": ([128000] + list(range(1500 + 40 * i, 1540 + 40 * i)),
                      _greedy(30, logit_bias={10 + i: 30.0, 20 + i: 29.0, 30 + i: 28.0}, **TIGHT)) for i in range(4)}
    return reqs, _run(eng, reqs), eng


def test_preempted_sequence_carries_its_history(llama_small):
    """A pool too small for four sequences of 71 tokens (5 pages each, 17 pages in all): one
    is pre-empted, resumed later and must continue as if nothing had happened."""
    reqs, want, roomy = _tight_run(llama_small, 512)
    assert roomy.sched.total_preemptions() == 0
    _, got, tight = _tight_run(llama_small, 17)
    assert tight.sched.total_preemptions() > 0
    assert got == want
    for rid, (p, sp) in reqs.items():
        _check_against_reference(llama_small, p, got[rid], logit_bias=sp.logit_bias, **TIGHT)


def test_plain_engine_has_no_processor_state(llama_small):
    eng = _engine(llama_small, decode_prefill_cap=128, graph_batch_sizes=[1, 2, 4, 8, 16], max_num_seqs=16)
    n_graphs, n_mixed = len(eng.runner.graphs), len(eng.runner.mixed_graphs)
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    outs = eng.generate([PROMPT, [128000, 5, 6, 7]], SamplingParams(max_tokens=8, temperature=0.8, top_k=40, seed=1,
                                                                    ignore_eos=True))
    assert all(len(o) == 8 for o in outs)
    r = eng.runner
    assert r.p_state is None and r.p_scratch is None and not r.proc_graphs and not r.proc_mixed_graphs
    assert r.g_pi is None and not eng._resets
    assert (len(r.graphs), len(r.mixed_graphs)) == (n_graphs, n_mixed)
    torch.cuda.synchronize()
    assert torch.cuda.memory_allocated() - before < (8 << 20)  # nothing the size of a state table or a scratch
    # min_p alone: the processed form without token statistics, so still no state table
    eng.generate([PROMPT], SamplingParams(max_tokens=4, temperature=0.8, min_p=0.1, seed=2, ignore_eos=True))
    assert r.proc_graphs and r.p_scratch is not None and r.p_state is None and r.p_bias_ids is None
    n_proc = len(r.proc_graphs)
    # ... until the first request that needs counts
    eng.generate([PROMPT], _greedy(4, presence_penalty=0.5))
    assert len(r.proc_graphs) > n_proc  # captured again, now with the table
    assert r.p_state is not None and tuple(r.p_state.shape) == (16, llama_small.cfg.vocab_size) and r.proc_graphs
    assert (len(r.graphs), len(r.mixed_graphs)) == (n_graphs, n_mixed)
