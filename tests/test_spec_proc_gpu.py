"""Speculating requests that use logit processors, on the GPU.

(a) ops.process_logits with per-row extra history, bit-identical to the numpy reference
    (-inf positions included): a block of k = 16, a block of k = 3, two single rows without
    a list and a row with slot -1 and a list in one call.
(b) a call without the list against the reference of the plain kernel.
(c) ops.logit_state_add against the numpy loop, 64 slots x 17 entries of one token each
    included (what a non-atomic update loses).
(d) ops.spec_verify_sample on processed rows with -inf entries against the float64
    reference, by the margin rule of test_spec_sample_gpu.py.
(e) the engine: 2-layer llama3-8b, self draft, graphs on, k = 3.
"""
from dataclasses import replace

import numpy as np
import pytest
import torch

import _spec_ref as R
from _spec_proc_ref import CMAX, FLAG, cells_row_ref, state_add_ref
from test_logit_proc_engine_gpu import BIAS, NEAR_TIE, PEN, PROMPT, _check_against_reference
from test_logit_proc_gpu import ref_row
from xgserve import ops
from xgserve.engine import EngineConfig, LLMEngine, SamplingParams
from xgserve.models import build_model, get_config
from xgserve.ops import _native

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module")
def native():
    _native.kernels()  # fail loudly: the GPU path must run the native library


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ------------------------------------------------------------------ (a), (b)
T_ZERO, T_DUP, T_FLAG, T_SAT, T_FSAT1, T_BIAS, T_MAX, T_ZERO2 = 11, 23, 37, 41, 53, 67, 71, 29
PENS = (1.3, 0.4, 0.3)


def _proc_case(V, bf16, pad):
    """24 rows: block A (slot 0, k = 16: rows 0..16), block B (slot 1, k = 3: rows 17..20),
    single rows 21 (slot 2) and 22 (slot -1) without a list, row 23 with slot -1 and a list."""
    rng = np.random.default_rng(V + 2 * bf16 + pad)
    S, rows = 4, 24
    table = np.zeros((S, V), np.uint16)
    for s in range(S):
        ids = rng.permutation(V)[:200]
        table[s, ids[:60]] = FLAG
        table[s, ids[60:120]] = rng.integers(1, 9, 60)
        table[s, ids[120:200]] = FLAG | rng.integers(1, 5, 80).astype(np.uint16)
    b0, b1 = 4095 % V, 4096 % V  # either side of the chunk boundary where V > 4096
    for s in (0, 1):
        table[s, [T_ZERO, T_ZERO2, T_MAX, T_BIAS, b0, b1]] = 0
        table[s, T_DUP], table[s, T_FLAG], table[s, T_SAT], table[s, T_FSAT1] = 2, FLAG, CMAX, FLAG | (CMAX - 1)
    list_a = [T_ZERO, T_DUP, T_FLAG, T_DUP, T_SAT, T_FSAT1, T_BIAS, T_MAX, -1, V, b0, b1, T_ZERO2, T_FSAT1, T_MAX,
              T_FSAT1]
    list_b = [T_MAX, T_MAX, 5]
    list_c = [7, 7, 9]
    assert len(list_a) == ops.LOGIT_HIST_MAX
    hist = np.asarray(list_a + list_b + list_c, np.int32)
    hp = np.zeros((2, rows), np.int32)
    hp[1, :17] = np.arange(17)
    hp[0, 17:21], hp[1, 17:21] = 16, np.arange(4)
    hp[0, 23], hp[1, 23] = 19, 3
    slots = np.asarray([0] * 17 + [1] * 4 + [2, -1, -1], np.int32)
    x = (rng.standard_normal((rows, V)) * 3).astype(np.float32)
    x[:, T_MAX] = 16.0  # the row maximum until the history penalises it: min_p's threshold moves
    x[:, T_BIAS] = 1.0
    dt = torch.bfloat16 if bf16 else torch.float32
    buf = torch.full((rows, V + pad), 1e30, dtype=dt)
    buf[:, :V] = torch.from_numpy(x).to(dt)
    xin = buf[:, :V]
    bias = {0: {T_BIAS: 1.5, 100: -2.0}, 1: {T_MAX: -0.5}}
    nb = ops.LOGIT_BIAS_MAX
    bias_ids, bias_vals = np.zeros(S * nb, np.int32), np.zeros(S * nb, np.float32)
    pi = np.zeros((3, rows), np.int32)
    pi[0] = slots
    for s, d in bias.items():
        bias_ids[s * nb:s * nb + len(d)], bias_vals[s * nb:s * nb + len(d)] = list(d), list(d.values())
        pi[1, slots == s], pi[2, slots == s] = s * nb, len(d)
    pf = np.zeros((4, rows), np.float32)
    pf[0], pf[1], pf[2], pf[3] = PENS[0], PENS[1], PENS[2], np.float32(np.log(0.05))
    return dict(V=V, rows=rows, table=table, hist=hist, hp=hp, slots=slots, xin=xin, pad=pad, bias=bias,
                bias_ids=bias_ids, bias_vals=bias_vals, pi=pi, pf=pf)


def _to_dev(view):
    V = view.shape[1]
    base = torch.as_strided(view, (view.shape[0], view.stride(0)), (view.stride(0), 1))
    return base.to(DEV)[:, :V]


def _run_proc(c, temp, with_hist):
    rows, V = c["rows"], c["V"]
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)  # noqa: E731
    state = t(c["table"].view(np.int16))
    out = ops.process_scratch(rows, V, DEV)
    if c["pad"]:
        out = torch.empty(rows, V + c["pad"], dtype=torch.float32, device=DEV)[:, :V]
    kw = dict(hist_ids=t(c["hist"]), hist_pos=t(c["hp"])) if with_hist else {}
    ops.check_hist_pos(c["hp"], len(c["hist"]), rows)
    ops.process_logits(_to_dev(c["xin"]), out, state, t(c["pi"]), t(c["pf"]), t(np.full(rows, temp, np.float32)),
                       t(c["bias_ids"]), t(c["bias_vals"]), **kw)
    torch.cuda.synchronize()
    assert np.array_equal(state.cpu().numpy().view(np.uint16), c["table"])  # read-only
    return out.cpu().numpy()


def _want(c, i, temp, with_hist):
    V, s = c["V"], int(c["slots"][i])
    cells = c["table"][s] if s >= 0 else np.zeros(V, np.uint16)
    o, n = (int(c["hp"][0, i]), int(c["hp"][1, i])) if with_hist else (0, 0)
    return cells_row_ref(c["xin"][i].float().numpy(), cells, rep=PENS[0], freq=PENS[1], pres=PENS[2],
                         bias=c["bias"].get(s), min_p=0.05, temperature=temp, extra=c["hist"][o:o + n].tolist())


@pytest.mark.parametrize("pad", [0, 3])
@pytest.mark.parametrize("bf16", [True, False])
@pytest.mark.parametrize("V", [1000, 4104, 128256])
def test_history_rows_are_bit_identical(native, V, bf16, pad):
    c = _proc_case(V, bf16, pad)
    assert c["xin"].stride(0) == V + pad
    for temp in (0.0, 0.7):
        got = _run_proc(c, temp, True)
        changed = 0
        for i in range(c["rows"]):
            want = _want(c, i, temp, True)
            assert np.array_equal(_bits(got[i]), _bits(want)), (temp, i, np.nonzero(_bits(got[i]) != _bits(want))[0][:8])
            changed += not np.array_equal(want, _want(c, i, temp, False))
            if temp > 0:
                assert np.isneginf(want).any() and np.array_equal(np.isneginf(got[i]), np.isneginf(want))
        # the reference itself: unmasked (T = 0), every row with a list differs from its plain form
        assert changed >= 16 + 3 + 1 or temp > 0
    # the threshold of min_p moved with the history: T_MAX is row 16's maximum only without its list
    assert _want(c, 16, 0.7, False).max() == 16.0 and _want(c, 16, 0.7, True).max() != 16.0


@pytest.mark.parametrize("bf16,pad", [(True, 0), (False, 3)])
@pytest.mark.parametrize("V", [1000, 4104, 128256])
def test_call_without_a_list_is_the_plain_call(native, V, bf16, pad):
    c = _proc_case(V, bf16, pad)
    for temp in (0.0, 0.7):
        got = _run_proc(c, temp, False)
        for i in range(c["rows"]):
            s = int(c["slots"][i])
            cells = c["table"][s] if s >= 0 else np.zeros(V, np.uint16)
            b = c["bias"].get(s, {})
            want = ref_row(c["xin"][i].float().numpy(), cells, PENS[0], PENS[1], PENS[2], list(b), list(b.values()),
                           temp, np.float32(np.log(0.05)))
            assert np.array_equal(_bits(got[i]), _bits(want)), (temp, i)


# ------------------------------------------------------------------ (c)
def test_state_add_equals_the_loop(native):
    S, V = 64, 1000
    rng = np.random.default_rng(3)
    table = np.zeros((S, V), np.uint16)
    table[rng.integers(0, S, 500), rng.integers(0, V, 500)] = rng.integers(0, 1 << 16, 500).astype(np.uint16)
    table[5, 77] = CMAX - 1
    table[6, 78] = FLAG | (CMAX - 1)
    # 64 slots x 17 entries, every entry of a slot the same token (odd and even cells, so both halves of a word)
    slots = np.repeat(np.arange(S), 17)
    toks = np.repeat((np.arange(S) * 7 + 1) % V, 17)
    table[np.arange(S), (np.arange(S) * 7 + 1) % V] &= 0x8003
    extra_s = np.concatenate([rng.integers(0, S, 300), [5, 5, 5, 6, 6, 6, -1, S, 3, 3]])
    extra_t = np.concatenate([rng.integers(0, 40, 300), [77, 77, 77, 78, 78, 78, 4, 4, -1, V]])
    slots, toks = np.concatenate([slots, extra_s]).astype(np.int32), np.concatenate([toks, extra_t]).astype(np.int32)
    perm = rng.permutation(len(slots))
    slots, toks = slots[perm], toks[perm]
    want = state_add_ref(table, slots, toks)
    assert want[5, 77] == CMAX and want[6, 78] == (FLAG | CMAX)
    assert all(want[s, (s * 7 + 1) % V] >= (table[s, (s * 7 + 1) % V] + 17) for s in range(S))
    state = torch.from_numpy(table.view(np.int16).copy()).to(DEV)
    ops.logit_state_add(state, torch.from_numpy(slots).to(DEV), torch.from_numpy(toks).to(DEV), len(slots))
    torch.cuda.synchronize()
    got = state.cpu().numpy().view(np.uint16)
    assert np.array_equal(got, want), np.argwhere(got != want)[:8]
    ops.logit_state_add(state, torch.from_numpy(slots).to(DEV), torch.from_numpy(toks).to(DEV), 0)
    torch.cuda.synchronize()
    assert np.array_equal(state.cpu().numpy().view(np.uint16), want)


# ------------------------------------------------------------------ (d)
def _masked_case():
    """Blocks of k = 1 and k = 3 on fp32 rows masked as min_p = 0.05 masks them at T = 0.8
    (about nine tenths of a row are -inf); draft tokens are the draft's own draws, and in
    every fourth block the first one sits on a token the target masked."""
    V, nblocks, T = 4104, 48, np.float32(0.8)
    g = torch.Generator().manual_seed(41)
    ks = np.array([1, 3], np.int64)[np.arange(nblocks) % 2]
    Lp, Lq = int((ks + 1).sum()), int(ks.sum())
    p_row0 = np.concatenate([[0], np.cumsum(ks + 1)[:-1]])
    q_row0 = np.concatenate([[0], np.cumsum(ks)[:-1]])
    tp = (torch.randn(Lp, V, generator=g) * 3).numpy()
    src = np.concatenate([np.arange(p_row0[j], p_row0[j] + ks[j]) for j in range(nblocks)])
    tq = tp[src] + torch.randn(Lq, V, generator=g).numpy() * 0.5

    def mask(x):
        y = (x * (np.float32(1) / T)).astype(np.float32)
        return np.where(y < (y.max(axis=1, keepdims=True) + np.float32(np.log(0.05))), np.float32(-np.inf), x)

    tp, tq = mask(tp.astype(np.float32)), mask(tq.astype(np.float32))
    seeds = ((np.arange(1, Lp + 1, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15)) >> np.uint64(1)).astype(np.int64)
    draft = np.empty(Lq, np.int32)
    on_masked = 0
    for j in range(nblocks):
        for i in range(int(ks[j])):
            draft[q_row0[j] + i] = R.draft_draw(tq[q_row0[j] + i], T, int(seeds[p_row0[j] + i]))
        if j % 4 == 0:
            both = np.nonzero(np.isneginf(tp[p_row0[j]]) & ~np.isneginf(tq[q_row0[j]]))[0]
            if len(both):
                draft[q_row0[j]] = both[0]
        on_masked += int(np.isneginf(tp[p_row0[j], draft[q_row0[j]]]))
    assert on_masked >= 4 and np.isneginf(tp).mean() > 0.5
    return {"p": torch.from_numpy(tp), "q": torch.from_numpy(tq), "ks": ks, "temps": np.full(nblocks, T, np.float32),
            "p_row0": p_row0, "q_row0": q_row0, "d_off": q_row0.copy(), "draft": draft, "seeds": seeds,
            "blocks": [(int(p_row0[j]), int(q_row0[j]), int(q_row0[j]), int(ks[j]), float(T)) for j in range(nblocks)]}


def _verify(c, dev):
    tok, lp, acc = ops.spec_verify_sample(c["p"].to(dev), c["q"].to(dev), c["draft"], c["p_row0"], c["q_row0"],
                                          c["d_off"], c["ks"], c["temps"], c["seeds"])
    if dev != "cpu":
        torch.cuda.synchronize()
    return tok.cpu().numpy(), lp.cpu().numpy(), acc.cpu().numpy()


def test_verify_kernels_take_masked_rows(native):
    """Processed rows hold -inf where min_p masked a token. The kernels and the CPU path of
    ops.spec_verify_sample against the float64 reference of the contract: tokens, accepted
    and logprobs wherever the reference's margins decide; no NaN in the emitted logprobs.
    Sampled requests with min_p > 0 are speculated (spec_decode.SAMPLED_MIN_P) because this holds."""
    from xgserve.engine import spec_decode
    c = _masked_case()
    refs = R.verify(c["p"].numpy(), c["q"].numpy(), c["blocks"], c["draft"], c["seeds"])
    for dev in ("cpu", DEV):
        tok, lp, acc = _verify(c, dev)
        emitted = np.concatenate([np.arange(p0, p0 + int(a) + 1) for (p0, _, _, _, _), a in zip(c["blocks"], acc)])
        assert not np.isnan(lp[emitted]).any() and np.isfinite(lp[emitted]).all()
        R.check_against(c, tok, lp, acc, refs, f"masked rows on {dev}")
        for (p0, _, _, _, _), a in zip(c["blocks"], acc):  # no emitted token is one the target masked
            assert not np.isneginf(c["p"].numpy()[np.arange(p0, p0 + int(a) + 1), tok[p0:p0 + int(a) + 1]]).any()
    assert spec_decode.SAMPLED_MIN_P is True


# ------------------------------------------------------------------ (e)
@pytest.fixture(scope="module")
def llama_small(native):
    cfg = replace(get_config("llama3-8b"), num_layers=2, name="llama3-8b-2l")
    return build_model(cfg, device="cuda:0", seed=3)


def _engine(model, **kw):
    base = dict(model=model.cfg.name, device="cuda:0", num_blocks=512, max_num_seqs=16, max_num_batched_tokens=2048,
                max_model_len=1024, graph_batch_sizes=[1, 2, 4, 8], draft_model=model, num_speculative_tokens=3,
                spec_processors=True)
    base.update(kw)
    return LLMEngine(EngineConfig(**base), model=model)


def _greedy(n, **kw):
    return SamplingParams(max_tokens=n, temperature=0.0, ignore_eos=True, **kw)


def _run(eng, reqs):
    outs = {}
    for rid, (p, sp) in reqs.items():
        eng.add_request(rid, p, sp)
    while eng.has_work():
        for o in eng.step():
            outs.setdefault(o.request_id, []).extend(o.new_token_ids)
    torch.cuda.synchronize()
    return outs


def test_forced_token_is_drafted_and_accepted(llama_small):
    """logit_bias of +100 on one token: the processed target emits it 12 times, and the
    draft, processed the same way, proposes nothing else -- every draft token accepted
    (observed on an MI355X: acceptance_rate 1.0)."""
    eng = _engine(llama_small)
    assert eng.runner.graphs and eng.spec.runner.graphs
    assert eng.generate([PROMPT], _greedy(12, logit_bias={4242: 100.0}))[0] == [4242] * 12
    st = eng.stats()["speculative"]
    assert st["acceptance_rate"] == 1.0 and st["processed_draft_tokens_proposed"] > 0, st
    assert eng.spec.runner.p_state is eng.runner.p_state and eng.runner.p_state is not None
    assert eng.spec.runner.p_bias_ids is eng.runner.p_bias_ids
    assert eng.spec.runner.proc_graphs, "the draft's processed graphs were not used"


def test_penalised_greedy_follows_the_reference(llama_small):
    """PEN and BIAS of test_logit_proc_engine_gpu.py over 24 tokens, self draft, k = 3: every
    token within NEAR_TIE of the maximum of its processed fp32 reference row. The acceptance
    rate is asserted above the engine's disable floor (0.5) only: draft and verify rows go
    through different attention kernels, so a near-tie may reject a draft token.
    Observed on an MI355X: 17 draft tokens proposed, 17 accepted (acceptance_rate 1.0),
    6 verify steps, mean_tokens_per_verify 3.83."""
    eng = _engine(llama_small)
    out = eng.generate([PROMPT], _greedy(24, logit_bias=dict(BIAS), **PEN))[0]
    assert len(out) == 24
    _check_against_reference(llama_small, PROMPT, out, logit_bias=BIAS, **PEN)
    st = eng.stats()["speculative"]
    print(f"[spec-proc] penalised greedy, self draft k=3: {st}")
    assert st["processed_draft_tokens_proposed"] > 0 and st["acceptance_rate"] > 0.5, st
    assert NEAR_TIE == 0.15


def test_plain_sampled_request_draws_the_same_tokens(llama_small):
    """A plain sampled request that shares its batch with a processed one draws what it
    draws with spec_processors off (same seed): fp32 q rows and the processed verify step
    change no value."""
    plain_p = [128000] + list(range(300, 330))
    sp = SamplingParams(max_tokens=16, temperature=0.9, seed=11, ignore_eos=True)
    off = _run(_engine(llama_small, spec_processors=False, spec_sampled=True), {"s": (plain_p, sp)})
    eng = _engine(llama_small, spec_sampled=True)
    on = _run(eng, {"s": (plain_p, sp), "pen": (PROMPT, _greedy(16, logit_bias=dict(BIAS), **PEN))})
    assert on["s"] == off["s"] and len(on["pen"]) == 16
    st = eng.stats()["speculative"]
    assert st["sampled_draft_tokens_proposed"] > 0 and st["processed_draft_tokens_proposed"] > 0
    assert eng.spec.q_buf.dtype == torch.float32


def test_plain_speculating_engine_has_no_processor_state(llama_small):
    eng = _engine(llama_small, spec_sampled=True)
    n_graphs, n_draft = len(eng.runner.graphs), len(eng.spec.runner.graphs)
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    outs = eng.generate([PROMPT, [128000, 5, 6, 7]], _greedy(8))
    assert all(len(o) == 8 for o in outs)
    torch.cuda.synchronize()
    assert torch.cuda.memory_allocated() - before < (8 << 20)  # nothing the size of a state table or a scratch
    outs = eng.generate([PROMPT, [128000, 5, 6, 7]], SamplingParams(max_tokens=8, temperature=0.8, seed=1,
                                                                    ignore_eos=True))
    assert all(len(o) == 8 for o in outs) and eng.stats()["speculative"]["sampled_draft_tokens_proposed"] > 0
    for r in (eng.runner, eng.spec.runner):
        assert r.p_state is None and r.p_scratch is None and not r.proc_graphs and not r.proc_mixed_graphs
        assert r.g_pi is None and r.p_bias_ids is None
    assert not eng._resets
    assert (len(eng.runner.graphs), len(eng.spec.runner.graphs)) == (n_graphs, n_draft)
