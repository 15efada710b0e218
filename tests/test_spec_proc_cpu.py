"""Speculating requests that use logit processors, on the CPU: the op with per-row extra
history and the commit op against numpy, and the speculating engine (spec_processors)
against the non-speculating engine's processed output, token for token."""
from __future__ import annotations

import numpy as np
import pytest
import torch

from _logit_ref import process_row
from _spec_proc_ref import CMAX, FLAG, history_row_ref, state_add_ref
from xgserve import ops
from xgserve.engine import EngineConfig, LLMEngine, SamplingParams
from xgserve.engine.request import UnsupportedSampling

PROMPTS = [[1] + list(range(10, 40)), [1, 5, 9, 200, 300], [1] + list(range(100, 160))]
PROC = dict(repetition_penalty=1.3, frequency_penalty=0.4, presence_penalty=0.3, logit_bias={7: 2.0, 300: -100.0})


def _greedy(n=20, **kw):
    return SamplingParams(max_tokens=n, temperature=0.0, ignore_eos=True, **kw)


def _engine(draft=None, k=0, **kw):
    base = dict(model="llama-tiny", device="cpu", dtype="float32", num_blocks=128, max_num_seqs=8,
                max_num_batched_tokens=256, use_graphs=False, seed=7, draft_model=draft, num_speculative_tokens=k)
    base.update(kw)
    return LLMEngine(EngineConfig(**base))


def _run(eng, reqs):
    outs = {}
    for rid, (p, sp) in reqs.items():
        eng.add_request(rid, p, sp)
    while eng.has_work():
        for o in eng.step():
            outs.setdefault(o.request_id, []).extend(o.new_token_ids)
    return outs


# ------------------------------------------------------------------ ops
def test_history_rows_equal_the_row_reference():
    """Row i of a block with the list's first i tokens as extra history == process_row on
    the table's history plus those tokens, bit for bit."""
    V, k = 512, 6
    rng = np.random.default_rng(0)
    x = (rng.standard_normal((k + 1, V)) * 3).astype(np.float32)
    prompt, gen = [3, 4, 5, 400], [4, 9, 9, 77]
    ids, cells = ops.logit_state_cells(prompt, gen)
    state = ops.logit_state_alloc(2, V, "cpu")
    packed, nres, total = ops.pack_state_resets([(1, ids, cells)])
    ops.logit_state_reset(state, torch.from_numpy(packed), nres, total)
    lst = [9, 200, 200, 3, -1, V]  # seen again, new twice, a prompt token, two ids outside [0, V)
    bias = {200: 1.5, 11: -2.0}
    params = dict(repetition_penalty=1.3, frequency_penalty=0.4, presence_penalty=0.3, logit_bias=bias)
    R = k + 1
    pi = torch.zeros(3, R, dtype=torch.int32)
    pi[0], pi[1], pi[2] = 1, 0, len(bias)
    pf = torch.tensor([[1.3] * R, [0.4] * R, [0.3] * R, [-np.inf] * R], dtype=torch.float32)
    hp = torch.zeros(2, R, dtype=torch.int32)
    hp[1] = torch.arange(R, dtype=torch.int32)
    out = torch.empty(R, V)
    ops.process_logits(torch.from_numpy(x), out, state, pi, pf, torch.zeros(R),
                       torch.tensor(list(bias), dtype=torch.int32), torch.tensor(list(bias.values())),
                       hist_ids=torch.tensor(lst, dtype=torch.int32), hist_pos=hp)
    differ = 0
    for i in range(R):
        want = history_row_ref(x[i], prompt, gen, lst[:i], V, **params)
        assert np.array_equal(out[i].numpy().view(np.uint32), want.view(np.uint32)), i
        if i:
            base = process_row(x[i], prompt, gen, **params)
            differ += not np.array_equal(base, want)
    assert differ >= 3  # the reference itself: extra history changes the row
    # without the list: the call of before
    out0 = torch.empty(R, V)
    ops.process_logits(torch.from_numpy(x), out0, state, pi, pf, torch.zeros(R),
                       torch.tensor(list(bias), dtype=torch.int32), torch.tensor(list(bias.values())))
    for i in range(R):
        assert np.array_equal(out0[i].numpy(), process_row(x[i], prompt, gen, **params))


def test_history_positions_are_validated():
    V = 64
    x, out = torch.zeros(2, V), torch.empty(2, V)
    pi = torch.zeros(3, 2, dtype=torch.int32)
    pi[0] = -1
    pf = torch.tensor([[1.0] * 2, [0.0] * 2, [0.0] * 2, [-np.inf] * 2])
    lst = torch.zeros(ops.LOGIT_HIST_MAX + 4, dtype=torch.int32)
    for off, ln in ((0, ops.LOGIT_HIST_MAX + 1), (10, 11), (-1, 2), (0, -1)):
        hp = torch.tensor([[off, 0], [ln, 0]], dtype=torch.int32)
        with pytest.raises(ValueError):
            ops.process_logits(x, out, None, pi, pf, torch.zeros(2), hist_ids=lst, hist_pos=hp)
    assert ops.LOGIT_HIST_MAX == 16


def test_state_add_repeats_saturation_flag_and_range():
    S, V = 3, 100
    state = ops.logit_state_alloc(S, V, "cpu")
    t = state.numpy().view(np.uint16)
    t[0, 5] = CMAX - 1          # two adds: ends at 0x7fff
    t[1, 6] = FLAG | 3          # the flag is kept
    t[2, 7] = FLAG | CMAX       # saturated: stays
    before = t.copy()
    slots = [0, 0, 0, 1, 1, 2, 1, 3, -1, 1, 1, 0]
    toks = [5, 5, 5, 6, 6, 7, 9, 1, 1, V, -1, 5]
    ops.logit_state_add(state, torch.tensor(slots, dtype=torch.int32), torch.tensor(toks, dtype=torch.int32), len(slots))
    want = state_add_ref(before, slots, toks)
    assert np.array_equal(t, want)
    assert t[0, 5] == CMAX and t[1, 6] == (FLAG | 5) and t[2, 7] == (FLAG | CMAX) and t[1, 9] == 1
    assert int(t.astype(np.int64).sum() - before.astype(np.int64).sum()) == 1 + 2 + 1
    ops.logit_state_add(state, torch.zeros(0, dtype=torch.int32), torch.zeros(0, dtype=torch.int32), 0)
    assert np.array_equal(t, want)


# ------------------------------------------------------------------ engine
@pytest.fixture(scope="module")
def baseline():
    """The non-speculating engine: its processed and its plain greedy outputs."""
    proc = _engine().generate(PROMPTS, _greedy(**PROC))
    plain = _engine().generate(PROMPTS, _greedy())
    return proc, plain


def test_processors_change_the_plain_output(baseline):
    proc, plain = baseline
    assert all(a != b for a, b in zip(proc, plain))
    # the plain output repeats tokens inside windows of k + 1: intra-block history decides tokens
    assert any(len(set(o[i:i + 4])) < 4 for o in plain for i in range(len(o) - 3))


@pytest.mark.parametrize("k", [1, 3, 5])
def test_self_draft_is_exact_and_fully_accepted(baseline, k):
    eng = _engine("llama-tiny", k, spec_processors=True)
    assert eng.generate(PROMPTS, _greedy(**PROC)) == baseline[0]
    st = eng.stats()["speculative"]
    # the draft and the target saw the same history: every draft token is the target's choice
    assert st["acceptance_rate"] == 1.0 and st["processed_draft_tokens_proposed"] > 0
    assert st["processed_draft_tokens_accepted"] == st["processed_draft_tokens_proposed"]
    assert eng.spec.runner.p_state is eng.runner.p_state and eng.runner.p_state is not None


def test_weak_draft_is_exact(baseline):
    eng = _engine("llama-tiny-draft", 4, spec_processors=True)
    assert eng.generate(PROMPTS, _greedy(**PROC)) == baseline[0]
    assert eng.stats()["speculative"]["processed_draft_tokens_proposed"] > 0


def _mixed_requests():
    return {"proc": (PROMPTS[0], _greedy(16, **PROC)),
            "plain": (PROMPTS[1], _greedy(14)),
            "samp": (PROMPTS[2], SamplingParams(max_tokens=18, temperature=0.8, seed=11, ignore_eos=True,
                                                repetition_penalty=1.2, presence_penalty=0.4, logit_bias={9: 1.0}))}


def test_mixed_batch(baseline):
    def run():
        eng = _engine("llama-tiny", 3, spec_processors=True, spec_sampled=True)
        return _run(eng, _mixed_requests()), eng.stats()["speculative"]

    outs, st = run()
    assert {r: len(o) for r, o in outs.items()} == {"proc": 16, "plain": 14, "samp": 18}
    assert outs["plain"] == _engine().generate([PROMPTS[1]], _greedy(14))[0]
    assert outs["proc"] == _engine().generate([PROMPTS[0]], _greedy(16, **PROC))[0]
    assert st["sampled_draft_tokens_proposed"] > 0 and st["processed_draft_tokens_proposed"] > 0
    again, _ = run()
    assert again["samp"] == outs["samp"]


def test_plain_sampled_draws_the_same_tokens_with_the_key_on():
    sp = SamplingParams(max_tokens=16, temperature=0.9, seed=5, ignore_eos=True)
    off = _engine("llama-tiny-draft", 3, spec_sampled=True).generate(PROMPTS, sp)
    on = _engine("llama-tiny-draft", 3, spec_sampled=True, spec_processors=True)
    assert on.generate(PROMPTS, sp) == off
    assert on.spec.q_buf.dtype == torch.float32 and on.runner.p_state is None


def test_preempted_sequence_carries_its_history():
    """A pool too small for the four sequences: one is pre-empted, bound again later (a
    state reset from its committed tokens) and continues as in the roomy run."""
    def run(num_blocks):
        eng = _engine("llama-tiny", 3, spec_processors=True, num_blocks=num_blocks, enable_prefix_cache=False)
        reqs = {f"s{i}": ([1] + list(range(20 + 40 * i, 60 + 40 * i)),
                          _greedy(30, logit_bias={10 + i: 2.0, 300: -100.0}, repetition_penalty=1.3,
                                  frequency_penalty=0.4, presence_penalty=0.3)) for i in range(4)}
        return _run(eng, reqs), eng

    want, roomy = run(128)
    assert roomy.sched.total_preemptions() == 0
    got, tight = run(13)  # four sequences of 71 tokens need 20 pages
    assert tight.sched.total_preemptions() > 0
    assert got == want
    plain = _engine(enable_prefix_cache=False)
    ref = {f"s{i}": plain.generate([[1] + list(range(20 + 40 * i, 60 + 40 * i))],
                                   _greedy(30, logit_bias={10 + i: 2.0, 300: -100.0}, repetition_penalty=1.3,
                                           frequency_penalty=0.4, presence_penalty=0.3))[0] for i in range(4)}
    assert want == ref


def test_key_off_keeps_the_refusal():
    eng = _engine("llama-tiny", 3)
    with pytest.raises(UnsupportedSampling) as ei:
        eng.add_request("r", PROMPTS[0], _greedy(**PROC))
    assert "is not supported together with speculative decoding" in str(ei.value)
    assert "repetition_penalty" in str(ei.value)


def test_engine_config_errors():
    with pytest.raises(ValueError, match="draft model"):
        _engine(spec_processors=True)
    with pytest.raises(ValueError, match="LOGIT_HIST_MAX"):
        _engine("llama-tiny", 17, spec_processors=True)
