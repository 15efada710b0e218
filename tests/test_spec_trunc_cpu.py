"""Speculative sampling of top-p / top-k requests without a GPU: the float64 bracket
reference (tests/_spec_trunc_ref.py), the CPU path of ops.spec_verify_sample(top_ps=,
top_ks=), the host guards and the workspace cap, and the engine / configuration plumbing of
spec.truncated.

Exact cases: `trunc_case` (the inputs of _spec_ref.exact_case, (top_p, top_k) cycling per
block over (0.9, 0), (1.0, 40), (0.95, 64), (1.0, 0), draft tokens drawn from the truncated
q on stream 0). The CPU path keeps the CPU sampler's exact sets (k-th value, smallest sorted
prefix), which must lie inside the reference's bracket. Ambiguous positions of the
reference: 0 of 510 at V = 1003 bf16, 0 of 510 at V = 4099 fp32, 0 of 20 at V = 128256 bf16
(6 blocks); no mismatch, worst logprob error 4.0e-7.

Distribution: the inputs of test_spec_sample_cpu.dist_inputs (V = 203, T = 0.8, 60 000
blocks of k = 1) with (top_p 0.9, top_k 0) and (0.8, 20); L == U on both rows; the first
emitted token must follow p' = norm(p on K_p): chi-square over the kept tokens, z <= 4, and
acceptance within 0.01 of 1 - TV(p', q'). Reference: z = -0.74 / -0.84, acceptance 0.2639
against 0.2654 / 0.1299 against 0.1296. With q left untruncated in the accept / residual
step the same reference gives z = 90.5 / 203, so the bound has power.
"""
import functools

import numpy as np
import pytest
import torch

import _spec_ref as R
import _spec_trunc_ref as TR
from test_spec_sample_cpu import DIST_N, DIST_T, dist_inputs
from xgserve import ops
from xgserve.engine import EngineConfig, LLMEngine, SamplingParams
from xgserve.ops import sampling as SP

DIST_PARAMS = [(0.9, 0), (0.8, 20)]
DIST_LAUNCH = 2048  # blocks per call: three truncated rows each, inside the workspace cap


def run_case(c, p=None, q=None, trunc=True, **kw):
    return ops.spec_verify_sample(c["p"] if p is None else p, c["q"] if q is None else q, c["draft"], c["p_row0"],
                                  c["q_row0"], c["d_off"], c["ks"], c["temps"], c["seeds"],
                                  **(dict(top_ps=c["top_ps"], top_ks=c["top_ks"]) if trunc else {}), **kw)


def case_refs(c):
    return TR.verify(c["p"].float().numpy(), c["q"].float().numpy(), c["blocks"], c["draft"], c["seeds"],
                     c["top_ps"], c["top_ks"])


# ------------------------------------------------------------------ exact
@pytest.mark.parametrize("V,bf16,pad,nblocks", [(1003, True, 2, 153), (4099, False, 0, 153), (128256, True, 0, 6)])
def test_fallback_against_reference(V, bf16, pad, nblocks):
    c = TR.trunc_case(V, bf16, nblocks, pad)
    tok, lp, acc = run_case(c)
    R.check_against(c, tok.numpy(), lp.numpy(), acc.numpy(), case_refs(c), f"cpu truncated V={V}")


def test_reference_p_equals_q_accepts_everything():
    c = TR.trunc_case(1003, True, 12, 2)
    P = c["p"].float().numpy()
    Q = P[np.concatenate([np.arange(p0, p0 + k) for p0, _, _, k, _ in c["blocks"]])]
    draft = c["draft"].copy()
    for j, (p0, q0, d0, k, T) in enumerate(c["blocks"]):
        for i in range(k):
            draft[d0 + i] = TR.trunc_draw(Q[q0 + i], T, int(c["seeds"][p0 + i]), c["top_ps"][j], c["top_ks"][j])
    refs = TR.verify(P, Q, c["blocks"], draft, c["seeds"], c["top_ps"], c["top_ks"])
    for r, (_, _, _, k, _) in zip(refs, c["blocks"]):
        assert r.accepted == k


def test_call_without_the_arrays_is_untouched():
    c = TR.trunc_case(1003, True, 9, 2)
    base = run_case(c, trunc=False)
    off = ops.spec_verify_sample(c["p"], c["q"], c["draft"], c["p_row0"], c["q_row0"], c["d_off"], c["ks"],
                                 c["temps"], c["seeds"], top_ps=np.ones(9, np.float32), top_ks=np.zeros(9, np.int32))
    wide = ops.spec_verify_sample(c["p"], c["q"], c["draft"], c["p_row0"], c["q_row0"], c["d_off"], c["ks"],
                                  c["temps"], c["seeds"], top_ps=[1.0] * 9, top_ks=[1003] * 9)  # top_k >= V: off
    for got in (off, wide):
        for a, b in zip(base, got):
            assert torch.equal(a, b)


# ------------------------------------------------------------------ distribution
@functools.lru_cache(maxsize=None)
def dist_ref(top_p, top_k):
    xp, xq, seeds, _, _ = dist_inputs()
    ref = TR.DistRef(xp, xq, DIST_T, top_p, top_k)
    return ref, ref.first_tokens(seeds)


def dist_run_ops(device, top_p, top_k):
    """The distribution inputs through ops.spec_verify_sample: every block reads target row
    0 twice (position 0 and the bonus position) and draft row 0."""
    xp, xq, seeds, _, _ = dist_inputs()
    _, (draft, _, _) = dist_ref(top_p, top_k)
    P = torch.from_numpy(np.stack([xp, xp])).to(device)
    Q = torch.from_numpy(xq[None, :]).to(device)
    first, acc = [], []
    for s in range(0, DIST_N, DIST_LAUNCH):
        n = min(DIST_LAUNCH, DIST_N - s)
        z = np.zeros(n, np.int64)
        sd = np.stack([seeds[s:s + n], seeds[s:s + n] ^ np.uint64(0x5555)], axis=1).reshape(-1).view(np.int64)
        tok, _, a = ops.spec_verify_sample(P, Q, draft[s:s + n].astype(np.int32), z, z, np.arange(n), z + 1,
                                           np.full(n, DIST_T, np.float32), sd,
                                           top_ps=np.full(n, top_p, np.float32), top_ks=np.full(n, top_k, np.int32))
        first.append(tok.cpu().numpy()[0::2])
        acc.append(a.cpu().numpy())
    return np.concatenate(first), np.concatenate(acc)


def dist_check(name, ref, first, accepted):
    assert ref.Kp[first].all(), f"{name}: an emitted token lies outside K_p"
    z, chi2, df = ref.chi_square_z(first)
    rate = float(np.mean(accepted))
    print(f"[spec-trunc] {name}: kept p {int(ref.Kp.sum())} q {int(ref.Kq.sum())} chi2={chi2:.1f} df={df} z={z:.2f} "
          f"acceptance={rate:.4f} 1-TV={ref.one_minus_tv:.4f}")
    assert z <= 4, (name, chi2, df, z)
    assert abs(rate - ref.one_minus_tv) <= 0.01, (name, rate, ref.one_minus_tv)


@pytest.mark.parametrize("top_p,top_k", DIST_PARAMS)
def test_distribution_reference_and_its_power(top_p, top_k):
    ref, (draft, acc, first) = dist_ref(top_p, top_k)
    assert ref.exact, "L != U on a distribution row: the kept sets are not determined"
    assert ref.Kq[draft].all()
    dist_check(f"reference ({top_p}, {top_k})", ref, first, acc)
    _, _, seeds, _, _ = dist_inputs()
    _, _, wrong = ref.first_tokens(seeds, untruncated_q=True)
    z, chi2, df = ref.chi_square_z(wrong)
    print(f"[spec-trunc] reference, q left untruncated: chi2={chi2:.1f} df={df} z={z:.1f}")
    assert z > 40, "the bound has no power against an untruncated q"


@pytest.mark.parametrize("top_p,top_k", DIST_PARAMS)
def test_distribution_cpu_fallback(top_p, top_k):
    ref, (_, racc, rfirst) = dist_ref(top_p, top_k)
    first, acc = dist_run_ops("cpu", top_p, top_k)
    dist_check(f"ops cpu ({top_p}, {top_k})", ref, first, acc)
    assert np.array_equal(acc == 1, racc) and np.array_equal(first, rfirst)


# ------------------------------------------------------------------ guards
def test_wrapper_guards_on_cpu():
    p, q = torch.zeros(3, 50), torch.zeros(2, 50)
    ok = dict(draft=np.zeros(2, np.int32), p_row0=[0], q_row0=[0], d_off=[0], ks=[2], temps=[1.0], seeds=[1, 2, 3])
    ops.spec_verify_sample(p, q, **ok, top_ps=[0.9], top_ks=[5])
    ops.spec_verify_sample(p, q, **ok, top_ps=[1.0])
    ops.spec_verify_sample(p, q, **ok, top_ks=[0])
    for bad in (dict(top_ps=[0.9, 0.9]), dict(top_ks=[]), dict(top_ps=[0.0]), dict(top_ps=[-0.5]), dict(top_ps=[1.5]),
                dict(top_ps=[float("nan")]), dict(top_ps=[float("inf")]), dict(top_ks=[-1])):
        with pytest.raises(ValueError):
            ops.spec_verify_sample(p, q, **{**ok, **bad})


def test_workspace_cap_raises_instead_of_allocating():
    """Blocks may share logits rows, scratch rows they may not: three TRows per truncated
    block of k = 1, so 3 700 such blocks pass the 256 MiB cap and 3 500 do not."""
    from xgserve.ops._native import kernels
    K = kernels()
    assert SP.SPEC_TROW == K.spec_trow_bytes() and K.spec_block_words() == 10
    for Lp, Lq, V, nT in [(2, 1, 203, 0), (2, 1, 203, 3), (510, 357, 4099, 400), (20, 14, 128256, 34), (7000, 3500, 203, 10500)]:
        assert SP.spec_ws_need(Lp, Lq, V, nT) == K.spec_ws_bytes(Lp, Lq, V, nT)
    assert K.spec_ws_bytes(20, 14, 128256) == K.spec_ws_bytes(20, 14, 128256, 0)  # untruncated: as before
    assert K.spec_ws_bytes(20, 14, 128256, 34) - K.spec_ws_bytes(20, 14, 128256) >= 34 * SP.SPEC_TROW
    assert SP.spec_ws_need(7000, 3500, 203, 10500) < SP.SPEC_WS_CAP < SP.spec_ws_need(7400, 3700, 203, 11100)
    p, q = torch.zeros(2, 50), torch.zeros(1, 50)
    n = 3700
    z = np.zeros(n, np.int64)
    args = (np.zeros(n, np.int32), z, z, np.arange(n), z + 1, np.ones(n, np.float32), np.arange(2 * n))
    with pytest.raises(ValueError, match="workspace"):
        ops.spec_verify_sample(p, q, *args, top_ps=np.full(n, 0.9, np.float32))
    ops.spec_verify_sample(p, q, *args)  # the same call untruncated needs no such scratch


def _guard_call(blocks, V=100, ws_bytes=1 << 30):
    """The binding with dummy device pointers: the guards throw before anything is launched.
    blocks: (p_row0, q_row0, d_off, k, lrow0, out_row0, T, top_k, top_p, trow0)."""
    from xgserve.ops._native import kernels
    K = kernels()
    b = np.zeros((len(blocks), K.spec_block_words()), np.int32)
    for j, blk in enumerate(blocks):
        b[j, :6] = blk[:6]
        b[j, 6] = np.float32(blk[6]).view(np.int32)
        b[j, 7] = blk[7]
        b[j, 8] = np.float32(blk[8]).view(np.int32)
        b[j, 9] = blk[9]
    return K.spec_verify_sample(16, 1 << 20, V, 16, 1 << 20, V, 0, V, len(blocks), b.ctypes.data, 16, 16, 16, 16,
                                1 << 20, 16, 16, 1 << 20, 16, 16, ws_bytes, 0)


@pytest.mark.parametrize("blocks,kw", [
    (((0, 0, 0, 1, 0, 0, 1.0, 0, 0.0, -1),), {}),            # top_p = 0
    (((0, 0, 0, 1, 0, 0, 1.0, 0, -0.5, -1),), {}),
    (((0, 0, 0, 1, 0, 0, 1.0, 0, 1.5, -1),), {}),
    (((0, 0, 0, 1, 0, 0, 1.0, 0, float("nan"), -1),), {}),
    (((0, 0, 0, 1, 0, 0, 1.0, -1, 1.0, -1),), {}),           # top_k < 0
    (((0, 0, 0, 1, 0, 0, 1.0, 0, 0.9, -1),), {}),            # truncated, trow0 not the running sum
    (((0, 0, 0, 1, 0, 0, 1.0, 0, 0.9, 0), (0, 0, 0, 2, 2, 0, 1.0, 5, 1.0, 2)), {}),  # second block: 3 expected
    (((0, 0, 0, 1, 0, 0, 1.0, 0, 0.9, 0),), dict(ws_bytes=3 * 24624)),  # holds the TRows, not the rest
])
def test_binding_guards_raise_before_any_launch(blocks, kw):
    with pytest.raises(ValueError):
        _guard_call(blocks, **kw)


def test_binding_accepts_what_the_guards_allow():
    """The same descriptors pass the checks once the faulty field is right: the guard tests
    above fail for the reason they name (the workspace check comes last)."""
    for blocks in (((0, 0, 0, 1, 0, 0, 1.0, 0, 1.0, -1),), ((0, 0, 0, 1, 0, 0, 1.0, 100, 1.0, -1),),
                   ((0, 0, 0, 1, 0, 0, 1.0, 0, 0.9, 0), (0, 0, 0, 2, 2, 0, 1.0, 5, 1.0, 3))):
        with pytest.raises(ValueError, match="workspace too small"):
            _guard_call(blocks, ws_bytes=16)


# ------------------------------------------------------------------ engine (CPU, fp32)
def _engine(draft=None, k=0, **kw):
    return LLMEngine(EngineConfig(model="llama-tiny", device="cpu", dtype="float32", num_blocks=128, max_num_seqs=8,
                                  max_num_batched_tokens=256, use_graphs=False, seed=7, draft_model=draft,
                                  num_speculative_tokens=k, **kw))


PROMPTS = [[1] + list(range(10, 40)), [1, 5, 9, 200, 300], [1] + list(range(100, 160))]


@pytest.mark.parametrize("kw", [dict(top_p=0.9), dict(top_k=5)])
def test_engine_self_draft_accepts_every_truncated_token(kw):
    sp = SamplingParams(max_tokens=20, temperature=0.8, seed=3, ignore_eos=True, **kw)
    plain = _engine()
    plain.generate(PROMPTS, sp)
    eng = _engine("llama-tiny", 3, spec_sampled=True, spec_truncated=True)  # p == q bit for bit
    got = eng.generate(PROMPTS, sp)
    st = eng.stats()["speculative"]
    assert st["draft_tokens_proposed"] > 0
    assert st["truncated_draft_tokens_proposed"] == st["sampled_draft_tokens_proposed"] == st["draft_tokens_proposed"]
    assert st["truncated_draft_tokens_accepted"] == st["sampled_draft_tokens_accepted"] == st["draft_tokens_accepted"]
    assert st["acceptance_rate"] == 1.0
    assert eng.stats()["steps"] < plain.stats()["steps"]
    assert all(len(o) == 20 for o in got)
    assert _engine("llama-tiny", 3, spec_sampled=True, spec_truncated=True).generate(PROMPTS, sp) == got


def test_truncated_needs_sampled_in_the_engine():
    eng = _engine("llama-tiny", 3, spec_truncated=True)  # without spec_sampled nothing sampled is speculated
    got = eng.generate(PROMPTS[:1], SamplingParams(max_tokens=8, temperature=0.8, seed=3, ignore_eos=True, top_p=0.9))
    assert len(got[0]) == 8 and eng.stats()["speculative"]["draft_tokens_proposed"] == 0


def test_untruncated_requests_are_not_counted_as_truncated():
    eng = _engine("llama-tiny", 3, spec_sampled=True, spec_truncated=True)
    eng.generate(PROMPTS[:1], SamplingParams(max_tokens=10, temperature=0.8, seed=3, ignore_eos=True))
    st = eng.stats()["speculative"]
    assert st["sampled_draft_tokens_proposed"] > 0 and st["truncated_draft_tokens_proposed"] == 0


def _run_requests(eng, reqs):
    """reqs: {id: (prompt, SamplingParams)} -> {id: tokens}, stepping the engine itself."""
    for rid, (prompt, sp) in reqs.items():
        eng.add_request(rid, prompt, sp)
    toks = {rid: [] for rid in reqs}
    for _ in range(400):
        if not eng.has_work():
            break
        for o in eng.step():
            toks[o.request_id] += o.new_token_ids
    return toks


@pytest.mark.parametrize("top_p", [0.0, 1e-46, -0.5, float("nan")])  # 1e-46 is 0 in float32
def test_top_p_outside_the_kernels_range_decodes_plainly(top_p):
    """The samplers serve top_p = 0 (they keep one token); the verify kernels take (0, 1]
    only. Such a request must not be speculated, must complete, and must not disturb the
    request next to it, which is speculated as usual."""
    odd = SamplingParams(max_tokens=10, temperature=0.8, seed=3, ignore_eos=True, top_p=top_p)
    normal = SamplingParams(max_tokens=12, temperature=0.8, seed=4, ignore_eos=True, top_p=0.9)
    eng = _engine("llama-tiny", 3, spec_sampled=True, spec_truncated=True)
    toks = _run_requests(eng, {"odd": (PROMPTS[0], odd), "normal": (PROMPTS[1], normal)})
    assert len(toks["odd"]) == 10 and len(toks["normal"]) == 12
    st = eng.stats()["speculative"]
    assert st["truncated_draft_tokens_proposed"] == st["draft_tokens_proposed"] > 0  # the normal request's
    assert st["acceptance_rate"] == 1.0
    alone = _engine("llama-tiny", 3, spec_sampled=True, spec_truncated=True)
    assert _run_requests(alone, {"odd": (PROMPTS[0], odd)})["odd"] == toks["odd"]
    assert alone.stats()["speculative"]["draft_tokens_proposed"] == 0
    assert toks["odd"] == _run_requests(_engine(), {"odd": (PROMPTS[0], odd)})["odd"]  # the plain engine's draws


def test_top_p_above_one_and_top_k_at_vocab_run_untruncated():
    eng = _engine("llama-tiny", 3, spec_sampled=True, spec_truncated=True)
    V = eng.mcfg.vocab_size
    sp = SamplingParams(max_tokens=10, temperature=0.8, seed=3, ignore_eos=True, top_p=1.5, top_k=V)
    toks = _run_requests(eng, {"a": (PROMPTS[0], sp), "b": (PROMPTS[1], replace_top(sp, 0.9, 0))})
    assert len(toks["a"]) == 10 and len(toks["b"]) == 10
    st = eng.stats()["speculative"]
    assert 0 < st["truncated_draft_tokens_proposed"] < st["sampled_draft_tokens_proposed"]
    only = _engine("llama-tiny", 3, spec_sampled=True, spec_truncated=True)
    _run_requests(only, {"a": (PROMPTS[0], sp)})
    st = only.stats()["speculative"]
    assert st["sampled_draft_tokens_proposed"] > 0 and st["truncated_draft_tokens_proposed"] == 0


def replace_top(sp, top_p, top_k):
    from dataclasses import replace
    return replace(sp, top_p=top_p, top_k=top_k)


def test_engine_refuses_a_configuration_whose_verify_step_would_pass_the_cap():
    """max_num_seqs blocks of k draft tokens may meet in one verify call: (2 k + 1) scratch
    rows each. 2048 sequences at k = 3 need 337 MiB."""
    with pytest.raises(ValueError, match="spec_truncated"):
        LLMEngine(EngineConfig(model="llama-tiny", device="cpu", dtype="float32", num_blocks=128, max_num_seqs=2048,
                               max_num_batched_tokens=256, use_graphs=False, seed=7, draft_model="llama-tiny",
                               num_speculative_tokens=3, spec_sampled=True, spec_truncated=True))
    assert SP.spec_ws_need(2048 * 4, 2048 * 3, 32000, 2048 * 7) > SP.SPEC_WS_CAP


# ------------------------------------------------------------------ configuration and CLI
def test_config_key_env_and_set():
    from xgserve.server.config import ConfigError, SpecSection, load_config
    from xgserve.server.replica import engine_spec
    assert SpecSection().truncated is False and EngineConfig().spec_truncated is False
    cfg = load_config(env={})
    assert cfg.spec.truncated is False and engine_spec(cfg.worker, spec=cfg.spec)["spec_truncated"] is False
    cfg = load_config(env={"XGS_SPEC__SAMPLED": "1", "XGS_SPEC__TRUNCATED": "1"})
    assert cfg.spec.sampled is True and cfg.spec.truncated is True
    cfg = load_config(env={}, cli=["spec.sampled=true", "spec.truncated=true"])
    es = engine_spec(cfg.worker, spec=cfg.spec)
    assert cfg.spec.truncated is True and es["spec_truncated"] is True and es["spec_sampled"] is True
    with pytest.raises(ConfigError, match="spec.truncated"):
        load_config(env={}, cli=["spec.sampled=true", "spec.truncated=maybe"])
    with pytest.raises(ConfigError, match="spec.truncated requires spec.sampled"):
        load_config(env={}, cli=["spec.truncated=true"])
    with pytest.raises(ConfigError, match="spec.truncated requires spec.sampled"):
        load_config(env={"XGS_SPEC__TRUNCATED": "1"})


def test_cli_rejects_bad_values_with_status_2(capsys):
    from xgserve.cli import main
    assert main(["check-config", "--set", "spec.sampled=true", "--set", "spec.truncated=maybe"]) == 2
    assert "spec.truncated" in capsys.readouterr().err
    assert main(["check-config", "--set", "spec.truncated=true"]) == 2
    assert "spec.truncated requires spec.sampled" in capsys.readouterr().err
    assert main(["check-config", "--set", "spec.sampled=true", "--set", "spec.truncated=true"]) == 0
