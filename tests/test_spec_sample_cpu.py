"""Speculative sampling without a GPU: the float64 reference (tests/_spec_ref.py) and the
CPU path of ops.spec_verify_sample (same contract, same counter hash), the binding's host
guards, and the engine / server plumbing of spec.sampled on the CPU engine.

Distribution test: one target row and one draft row shared by N = 60 000 blocks of k = 1
(V = 203, T = 0.8). The first emitted token must follow p whatever q is: chi-square against
p with the bins of expected count < 20 pooled, z = (chi2 - df) / sqrt(2 df) <= 4, and the
acceptance rate within 0.01 of 1 - TV(p, q). The reference gives chi2 = 112.7 at df = 118
(z = -0.35) and acceptance 0.3196 against 1 - TV = 0.3209; with the residual wrongly drawn
from p the same reference gives z = 455, so the bound has power.
"""
import functools
import json

import numpy as np
import pytest
import torch

import _spec_ref as R
from xgserve import ops
from xgserve.engine import EngineConfig, LLMEngine, SamplingParams

DIST_N, DIST_V, DIST_T = 60000, 203, 0.8


@functools.lru_cache(maxsize=1)
def dist_inputs():
    rng = np.random.default_rng(0)
    xp = rng.normal(0, 2, DIST_V).astype(np.float32)
    xq = (xp + rng.normal(0, 1.5, DIST_V)).astype(np.float32)
    seeds = (np.arange(1, DIST_N + 1, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15))
    yp, yq = R.scaled(xp, DIST_T), R.scaled(xq, DIST_T)
    p, q = np.exp(yp - R.log_z(yp)), np.exp(yq - R.log_z(yq))
    return xp, xq, seeds, p, 1.0 - 0.5 * np.abs(p - q).sum()


@functools.lru_cache(maxsize=1)
def dist_reference():
    xp, xq, seeds, _, _ = dist_inputs()
    return R.first_tokens_shared(xp, xq, DIST_T, seeds)


def dist_run_ops(device, launches):
    """The distribution inputs through ops.spec_verify_sample: every block reads target row
    0 twice (position 0 and the bonus position) and draft row 0."""
    xp, xq, seeds, _, _ = dist_inputs()
    draft, _, _ = dist_reference()
    P = torch.from_numpy(np.stack([xp, xp])).to(device)
    Q = torch.from_numpy(xq[None, :]).to(device)
    first, acc = [], []
    per = DIST_N // launches
    for s in range(0, DIST_N, per):
        n = min(per, DIST_N - s)
        z = np.zeros(n, np.int64)
        sd = np.stack([seeds[s:s + n], seeds[s:s + n] ^ np.uint64(0x5555)], axis=1).reshape(-1).view(np.int64)
        tok, _, a = ops.spec_verify_sample(P, Q, draft[s:s + n].astype(np.int32), z, z, np.arange(n), z + 1,
                                           np.full(n, DIST_T, np.float32), sd)
        first.append(tok.cpu().numpy()[0::2])
        acc.append(a.cpu().numpy())
    return np.concatenate(first), np.concatenate(acc)


def dist_check(name, first, accepted):
    _, _, _, p, one_minus_tv = dist_inputs()
    z, chi2, df = R.chi_square_z(first, p)
    rate = float(np.mean(accepted))
    print(f"[spec] {name}: chi2={chi2:.1f} df={df} z={z:.2f} acceptance={rate:.4f} 1-TV={one_minus_tv:.4f}")
    assert z <= 4, (name, chi2, df, z)
    assert abs(rate - one_minus_tv) <= 0.01, (name, rate, one_minus_tv)


def test_distribution_reference_and_its_power():
    xp, xq, seeds, p, _ = dist_inputs()
    _, acc, first = dist_reference()
    dist_check("reference", first, acc)
    _, _, wrong = R.first_tokens_shared(xp, xq, DIST_T, seeds, wrong_residual=True)
    z, chi2, df = R.chi_square_z(wrong, p)
    print(f"[spec] reference, residual drawn from p: chi2={chi2:.1f} df={df} z={z:.1f}")
    assert z > 40, "the bound has no power against a wrong residual"


def test_distribution_cpu_fallback():
    first, acc = dist_run_ops("cpu", 2)
    dist_check("ops cpu", first, acc)
    d, racc, rfirst = dist_reference()
    assert np.array_equal(acc == 1, racc) and np.array_equal(first, rfirst)


@pytest.mark.parametrize("V,bf16,pad,nblocks", [(1003, True, 2, 153), (4099, False, 0, 153), (128256, True, 0, 6)])
def test_fallback_equals_reference(V, bf16, pad, nblocks):
    c = R.exact_case(V, bf16, nblocks, pad)
    refs = R.verify(c["p"].float().numpy(), c["q"].float().numpy(), c["blocks"], c["draft"], c["seeds"])
    tok, lp, acc = ops.spec_verify_sample(c["p"], c["q"], c["draft"], c["p_row0"], c["q_row0"], c["d_off"], c["ks"],
                                          c["temps"], c["seeds"])
    tok, lp, acc = tok.numpy(), lp.numpy(), acc.numpy()
    for j, (r, (p0, _, _, k, _)) in enumerate(zip(refs, c["blocks"])):  # float64 both: every position, exactly
        assert acc[j] == r.accepted, j
        assert tok[p0:p0 + r.accepted + 1].tolist() == r.toks, j
        np.testing.assert_allclose(lp[p0:p0 + r.accepted + 1], r.lps, atol=1e-5)
    R.check_against(c, tok, lp, acc, refs, f"cpu V={V}")


def test_reference_p_equals_q_accepts_everything():
    c = R.exact_case(1003, True, 9, 2)
    P = c["p"].float().numpy()
    Q = P[np.concatenate([np.arange(p0, p0 + k) for p0, _, _, k, _ in c["blocks"]])]
    draft = c["draft"].copy()
    for (p0, q0, d0, k, T) in c["blocks"]:
        for i in range(k):
            draft[d0 + i] = R.draft_draw(Q[q0 + i], T, int(c["seeds"][p0 + i]))
    for r, (_, _, _, k, _) in zip(R.verify(P, Q, c["blocks"], draft, c["seeds"]), c["blocks"]):
        assert r.accepted == k


# ------------------------------------------------------------------ binding guards
def _guard_call(V=100, ps=100, qs=100, blocks=((0, 0, 0, 1, 0, 0, 1.0),), ws=16, p_rows=1 << 20, q_rows=1 << 20,
                n_draft=1 << 20, n_out=1 << 20):
    from xgserve.ops._native import kernels
    K = kernels()
    b = np.zeros((len(blocks), K.spec_block_words()), np.int32)
    for j, blk in enumerate(blocks):
        b[j, :6] = blk[:6]
        b[j, 6] = np.float32(blk[6]).view(np.int32)
    # every device pointer is a dummy: the guards throw before anything is launched
    return K.spec_verify_sample(16, p_rows, ps, 16, q_rows, qs, 0, V, len(blocks), b.ctypes.data if len(blocks) else 0,
                                16, 16, 16, 16, n_draft, 16, 16, n_out, 16, ws, 1 << 30, 0)


@pytest.mark.parametrize("kw", [
    dict(V=0), dict(V=-4), dict(ps=99), dict(qs=99), dict(ws=0), dict(ws=8),
    dict(blocks=((0, 0, 0, 0, 0, 0, 1.0),)), dict(blocks=((0, 0, 0, -1, 0, 0, 1.0),)),
    dict(blocks=((0, 0, 0, 1, 0, 0, 0.0),)), dict(blocks=((0, 0, 0, 1, 0, 0, float("nan")),)),
    dict(blocks=((0, 0, 0, 2, 0, 0, 1.0),), p_rows=2), dict(blocks=((0, 0, 0, 2, 0, 0, 1.0),), q_rows=1),
    dict(blocks=((-1, 0, 0, 1, 0, 0, 1.0),)), dict(blocks=((0, 0, 3, 2, 0, 0, 1.0),), n_draft=4),
    dict(blocks=((0, 0, 0, 1, 0, 0, 1.0), (0, 0, 0, 1, 3, 0, 1.0))),
    dict(blocks=((0, 0, 0, 1, 0, 5, 1.0),), n_out=6),
    dict(blocks=tuple((0, 0, 0, 1, 2 * j, 0, 1.0) for j in range(32768))),   # 65536 target rows
])
def test_binding_guards_raise_before_any_launch(kw):
    with pytest.raises(ValueError):
        _guard_call(**kw)


def test_binding_zero_blocks_is_a_noop():
    _guard_call(blocks=())


def test_wrapper_guards_on_cpu():
    p, q = torch.zeros(3, 50), torch.zeros(2, 50)
    ok = dict(draft=np.zeros(2, np.int32), p_row0=[0], q_row0=[0], d_off=[0], ks=[2], temps=[1.0], seeds=[1, 2, 3])
    ops.spec_verify_sample(p, q, **ok)
    for bad in (dict(ks=[0]), dict(ks=[3]), dict(temps=[0.0]), dict(q_row0=[1]), dict(d_off=[1]), dict(seeds=[1, 2])):
        with pytest.raises(ValueError):
            ops.spec_verify_sample(p, q, **{**ok, **bad})
    with pytest.raises(ValueError):
        ops.spec_verify_sample(p, torch.zeros(2, 51), **ok)
    tok, lp, acc = ops.spec_verify_sample(p, q, np.zeros(0, np.int32), [], [], [], [], [], [])
    assert tok.numel() == 0 and acc.numel() == 0


# ------------------------------------------------------------------ engine (CPU, fp32)
def _engine(draft=None, k=0, **kw):
    return LLMEngine(EngineConfig(model="llama-tiny", device="cpu", dtype="float32", num_blocks=128, max_num_seqs=8,
                                  max_num_batched_tokens=256, use_graphs=False, seed=7, draft_model=draft,
                                  num_speculative_tokens=k, **kw))


PROMPTS = [[1] + list(range(10, 40)), [1, 5, 9, 200, 300], [1] + list(range(100, 160))]
SAMPLED = SamplingParams(max_tokens=20, temperature=0.8, seed=3, ignore_eos=True)


def test_engine_self_draft_accepts_every_sampled_token():
    plain = _engine()
    plain.generate(PROMPTS, SAMPLED)
    eng = _engine("llama-tiny", 3, spec_sampled=True)  # p == q bit for bit
    got = eng.generate(PROMPTS, SAMPLED)
    st = eng.stats()["speculative"]
    assert st["sampled_draft_tokens_proposed"] > 0
    assert st["sampled_draft_tokens_proposed"] == st["draft_tokens_proposed"]
    assert st["acceptance_rate"] == 1.0 and st["sampled_draft_tokens_accepted"] == st["draft_tokens_accepted"]
    assert eng.stats()["steps"] < plain.stats()["steps"]
    assert all(len(o) == 20 for o in got)
    assert _engine("llama-tiny", 3, spec_sampled=True).generate(PROMPTS, SAMPLED) == got
    V = eng.mcfg.vocab_size
    assert eng.stats()["scratch_bytes"] == plain.stats()["scratch_bytes"] + 8 * 3 * V * 4  # q_buf, fp32


def test_engine_weak_draft_completes_and_gets_disabled():
    eng = _engine("llama-tiny-draft", 4, spec_sampled=True)
    got = eng.generate(PROMPTS, SAMPLED)
    assert all(len(o) == 20 for o in got)
    st = eng.stats()["speculative"]
    assert st["sampled_draft_tokens_proposed"] > 0 and st["acceptance_rate"] < 1.0
    assert st["active"] == 0 or all(d.disabled for d in eng.spec.seqs.values())
    assert any(d.disabled for d in eng.spec.seqs.values())  # low acceptance switched a request off
    assert _engine("llama-tiny-draft", 4, spec_sampled=True).generate(PROMPTS, SAMPLED) == got


@pytest.mark.parametrize("kw", [dict(top_p=0.9), dict(top_k=5)])
def test_truncated_request_is_not_speculated(kw):
    eng = _engine("llama-tiny", 3, spec_sampled=True)
    got = eng.generate(PROMPTS[:1], SamplingParams(max_tokens=10, temperature=0.8, seed=3, ignore_eos=True, **kw))
    assert len(got[0]) == 10
    st = eng.stats()["speculative"]
    assert st["sampled_draft_tokens_proposed"] == 0 and st["draft_tokens_proposed"] == 0


def test_opt_in_off_speculates_no_sampled_request():
    eng = _engine("llama-tiny", 3)
    got = eng.generate(PROMPTS[:1], SAMPLED)
    st = eng.stats()["speculative"]
    assert st["sampled_draft_tokens_proposed"] == 0 and st["draft_tokens_proposed"] == 0
    assert eng.spec.q_buf is None and eng.spec.scratch_bytes() == 0
    assert got == _engine().generate(PROMPTS[:1], SAMPLED)  # exactly the plain engine's draws


def test_mixed_step_keeps_greedy_exact():
    eng = _engine("llama-tiny", 3, spec_sampled=True)
    greedy = SamplingParams(max_tokens=12, temperature=0.0, ignore_eos=True)
    eng.add_request("g", PROMPTS[0], greedy)
    eng.add_request("s", PROMPTS[1], SamplingParams(max_tokens=12, temperature=0.8, seed=3, ignore_eos=True))
    toks = {"g": [], "s": []}
    for _ in range(200):
        if not eng.has_work():
            break
        for o in eng.step():
            toks[o.request_id] += o.new_token_ids
    assert len(toks["g"]) == 12 and len(toks["s"]) == 12
    assert toks["g"] == _engine().generate([PROMPTS[0]], greedy)[0]
    st = eng.stats()["speculative"]
    assert 0 < st["sampled_draft_tokens_proposed"] < st["draft_tokens_proposed"]
    assert st["acceptance_rate"] == 1.0


# ------------------------------------------------------------------ configuration and HTTP
def test_config_key_env_and_set():
    from xgserve.server.config import ConfigError, SpecSection, load_config
    from xgserve.server.replica import engine_spec
    assert SpecSection().sampled is False and EngineConfig().spec_sampled is False
    cfg = load_config(env={})
    assert cfg.spec.sampled is False and engine_spec(cfg.worker, spec=cfg.spec)["spec_sampled"] is False
    assert load_config(env={"XGS_SPEC__SAMPLED": "1"}).spec.sampled is True
    cfg = load_config(env={}, cli=["spec.sampled=true"])
    assert cfg.spec.sampled is True and engine_spec(cfg.worker, spec=cfg.spec)["spec_sampled"] is True
    with pytest.raises(ConfigError, match="spec.sampled"):
        load_config(env={}, cli=["spec.sampled=maybe"])


def test_cli_rejects_a_non_bool_with_status_2(capsys):
    from xgserve.cli import main
    assert main(["check-config", "--set", "spec.sampled=maybe"]) == 2
    assert "spec.sampled" in capsys.readouterr().err
    assert main(["check-config", "--set", "spec.sampled=true"]) == 0


def test_http_server_speculates_a_sampled_request():
    from _server_util import run_with_client
    from xgserve.server.config import load_config
    eng = _engine("llama-tiny", 3, spec_sampled=True)
    cfg = load_config(env={}, overrides={"worker": {"model": "llama-tiny", "in_process": True},
                                         "spec": {"draft_model": "llama-tiny", "num_speculative_tokens": 3,
                                                  "sampled": True},
                                         "scheduler": {"health_check_interval_s": 0.1}})

    async def fn(c, srv):
        r = await c.post("/generate", data=json.dumps({"prompt": "hello there", "max_tokens": 12, "temperature": 0.8,
                                                       "seed": 3, "ignore_eos": True}))
        d = await r.json()
        assert r.status == 200 and d["usage"]["completion_tokens"] == 12, d
        for rep in srv.replicas.values():  # what the next heartbeat would carry
            rep.stats = dict(rep.stats or {}, speculative=eng.stats()["speculative"])
        srv.check_health()
        d = await (await c.get("/server/stats")).json()
        s = d["metrics"]["speculative"]
        assert s["sampled_draft_tokens_proposed"] > 0 and s["sampled_draft_tokens_accepted"] > 0, s
        e = d["replicas"][0]["engine"]["speculative"]
        assert e["sampled_draft_tokens_proposed"] == s["sampled_draft_tokens_proposed"]
        return True

    assert run_with_client(cfg, fn, engine=eng, timeout=120)
