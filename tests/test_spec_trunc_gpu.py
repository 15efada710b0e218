"""spec_verify_sample with top_ps / top_ks (csrc/kernels/spec_sample.hip, the truncated
kernels) on the GPU against the float64 bracket reference (tests/_spec_trunc_ref.py), and
the engine speculating top-p / top-k requests with graphs on.

(a) exact: truncated and untruncated blocks mixed in one launch; unambiguous positions match
    the reference (token, accepted, logprob within 1e-3); at most 3 % may be ambiguous.
(b) q == p bit for bit: everything accepted, the bonus token is ops.sample_tokens(step=2)
    with the same top_p / top_k.
(c) a draft certain of a token that the target's top_k = 8 excludes: always rejected.
(d) the CPU distribution test's inputs through the kernels, 2048 blocks per launch.
(e) a truncated launch, an untruncated one, the first again: identical / the parent contract.
(f) the engine, self-draft, graphs on, spec_truncated.

Figures (MI355X; the tests print them before they assert):
(a) 0 ambiguous positions and 0 mismatches of 510 (V = 1003 bf16), 510 (V = 4099 fp32) and
    25 (V = 128256 bf16, 8 blocks); worst logprob error 1.0e-6.
(b) every block unambiguous and fully accepted at the three shapes, the bonus tokens equal
    to sample_tokens'.
(c) 128 positions, 0 ambiguous, 0 of 64 accepted, no mismatch.
(d) (0.9, 0): chi2 = 39.8 at df = 47 (z = -0.74), acceptance 0.2639 against 1 - TV = 0.2654;
    (0.8, 20): chi2 = 13.8 at df = 19 (z = -0.84), acceptance 0.1299 against 0.1296; all
    60 000 first tokens and accept decisions equal to the float64 reference's, both times.
(e) first and third launch identical; 0 ambiguous, 0 mismatches of 510 in the second.
(f) top_p 0.9: 44 proposed, 44 accepted; top_k 40: 45 proposed, 43 accepted (0.956).
"""
from dataclasses import replace

import numpy as np
import pytest
import torch

import _spec_ref as R
import _spec_trunc_ref as TR
from test_spec_trunc_cpu import DIST_PARAMS, case_refs, dist_check, dist_ref, dist_run_ops, run_case
from xgserve import ops
from xgserve.engine import EngineConfig, LLMEngine, SamplingParams
from xgserve.models import build_model, get_config
from xgserve.ops import _native

pytestmark = pytest.mark.gpu
DEV = "cuda"
LP_TOL = 1e-3


@pytest.fixture(scope="module")
def native():
    _native.kernels()  # fail loudly: the GPU path must run the native library


def _to_dev(view):
    """The same [rows, V] view of a padded buffer on the device (row stride kept)."""
    V = view.shape[1]
    base = torch.as_strided(view, (view.shape[0], view.stride(0)), (view.stride(0), 1))
    return base.to(DEV)[:, :V]


def _run(c, p, q, trunc=True):
    tok, lp, acc = run_case(c, p, q, trunc)
    torch.cuda.synchronize()
    return tok.cpu().numpy(), lp.cpu().numpy(), acc.cpu().numpy()


# ------------------------------------------------------------------ (a)
@pytest.mark.parametrize("V,bf16,pad,nblocks", [(1003, True, 2, 153), (4099, False, 0, 153), (128256, True, 0, 8)])
def test_exact_against_reference(native, V, bf16, pad, nblocks):
    """V = 1003 bf16 with an odd row stride (one chunk, the scalar path); V = 4099 fp32 (two
    chunks: the row ticket decides); V = 128256 bf16 (21 chunks per row); k = 1, 2, 4,
    T = 0.7, 1.0, 1.3 and the four (top_p, top_k) of the cycle mixed in one launch."""
    c = TR.trunc_case(V, bf16, nblocks, pad)
    p, q = _to_dev(c["p"]), _to_dev(c["q"])
    assert p.stride(0) == V + pad and q.stride(0) == V + pad
    tok, lp, acc = _run(c, p, q)
    assert ((acc >= 0) & (acc <= c["ks"])).all()
    R.check_against(c, tok, lp, acc, case_refs(c), f"gpu truncated V={V} {'bf16' if bf16 else 'fp32'}")


# ------------------------------------------------------------------ (b)
@pytest.mark.parametrize("V,bf16", [(1003, True), (128256, True), (4099, False)])
def test_q_equals_p_accepts_everything(native, V, bf16):
    c = TR.trunc_case(V, bf16, 8)
    rows = np.concatenate([np.arange(p0, p0 + k) for p0, _, _, k, _ in c["blocks"]])
    c["q"] = c["p"][torch.from_numpy(rows)].contiguous()
    Qf = c["q"].float().numpy()
    for j, (p0, q0, d0, k, T) in enumerate(c["blocks"]):  # the draft's tokens: drawn from q' = p'
        for i in range(k):
            c["draft"][d0 + i] = TR.trunc_draw(Qf[q0 + i], T, int(c["seeds"][p0 + i]), c["top_ps"][j], c["top_ks"][j])
    refs = case_refs(c)
    p = c["p"].to(DEV)
    tok, lp, acc = _run(c, p, c["q"].to(DEV))
    clean = np.array([r.clean for r in refs])
    print(f"[spec-trunc] q == p V={V}: accepted {acc.tolist()} of {c['ks'].tolist()}, unambiguous blocks "
          f"{int(clean.sum())} of {len(refs)}")
    assert clean.sum() >= 6 and np.array_equal(acc[clean], c["ks"][clean])
    last = c["p_row0"] + c["ks"]
    per_row = lambda a: torch.from_numpy(np.repeat(a, c["ks"] + 1)).to(DEV)  # noqa: E731
    btok, blp = ops.sample_tokens(p, per_row(c["temps"]), per_row(c["top_ps"]), per_row(c["top_ks"]),
                                  torch.from_numpy(c["seeds"]).to(DEV), step=2)
    torch.cuda.synchronize()
    assert np.array_equal(tok[last][clean], btok.cpu().numpy()[last][clean])
    np.testing.assert_allclose(lp[last][clean], blp.cpu().numpy()[last][clean], atol=LP_TOL)
    for ok, (p0, _, d0, k, _) in zip(clean, c["blocks"]):
        if ok:
            assert tok[p0:p0 + k].tolist() == c["draft"][d0:d0 + k].tolist()


# ------------------------------------------------------------------ (c)
def test_draft_token_outside_the_targets_kept_set_is_rejected(native):
    V, nb, bad = 4099, 64, 1234
    g = torch.Generator().manual_seed(5)
    tp = torch.randn(2 * nb, V, generator=g) * 3
    tp[:, bad] = tp.median(dim=1).values  # far outside the target's top 8
    tq = torch.randn(nb, V, generator=g) * 3
    tq[:, bad] = 30.0                      # the draft is certain of it
    c = {"p": tp, "q": tq, "ks": np.ones(nb, np.int64), "temps": np.ones(nb, np.float32),
         "p_row0": 2 * np.arange(nb), "q_row0": np.arange(nb), "d_off": np.arange(nb),
         "draft": np.full(nb, bad, np.int32), "seeds": np.arange(1, 2 * nb + 1, dtype=np.int64) * 7919,
         "top_ps": np.ones(nb, np.float32), "top_ks": np.full(nb, 8, np.int32),
         "blocks": [(2 * j, j, j, 1, 1.0) for j in range(nb)]}
    refs = case_refs(c)
    assert all(r.accepted == 0 for r in refs)
    tok, lp, acc = _run(c, tp.to(DEV), tq.to(DEV))
    assert (acc == 0).all()
    assert (tok[0::2] != bad).all()
    R.check_against(c, tok, lp, acc, refs, "draft token outside K_p")
    # a figure, nothing asserted: untruncated, p(bad) / q(bad) is small but not zero
    _, _, plain = _run(c, tp.to(DEV), tq.to(DEV), trunc=False)
    print(f"[spec-trunc] draft outside K_p: accepted without truncation {int(plain.sum())} of {nb}")


# ------------------------------------------------------------------ (d)
@pytest.mark.parametrize("top_p,top_k", DIST_PARAMS)
def test_distribution_on_the_gpu(native, top_p, top_k):
    ref, (_, racc, rfirst) = dist_ref(top_p, top_k)
    assert ref.exact
    first, acc = dist_run_ops(DEV, top_p, top_k)
    agree = float(np.mean(first == rfirst))
    print(f"[spec-trunc] gpu ({top_p}, {top_k}) == float64 reference on {agree:.5f} of the first tokens, "
          f"{float(np.mean((acc == 1) == racc)):.5f} of the accept decisions")
    dist_check(f"ops gpu ({top_p}, {top_k})", ref, first, acc)
    assert agree >= 0.97 and float(np.mean((acc == 1) == racc)) >= 0.97


# ------------------------------------------------------------------ (e)
def test_workspace_reuse_between_truncated_and_untruncated_launches(native):
    c = TR.trunc_case(4099, False, 153)
    p, q = c["p"].to(DEV), c["q"].to(DEV)
    first = _run(c, p, q)
    plain = R.exact_case(4099, False, 153)  # the parent contract: its own draft tokens, no truncation
    tok, lp, acc = _run(plain, p, q, trunc=False)
    third = _run(c, p, q)
    for a, b in zip(first, third):
        assert np.array_equal(a, b)
    refs = R.verify(plain["p"].float().numpy(), plain["q"].float().numpy(), plain["blocks"], plain["draft"],
                    plain["seeds"])
    R.check_against(plain, tok, lp, acc, refs, "untruncated between two truncated launches")
    R.check_against(c, *third, case_refs(c), "truncated, third launch")


# ------------------------------------------------------------------ (f)
@pytest.fixture(scope="module")
def llama_small(native):
    cfg = replace(get_config("llama3-8b"), num_layers=2, name="llama3-8b-2l")
    return build_model(cfg, device="cuda:0", seed=3)


def _engine(model, **kw):
    base = dict(model=model.cfg.name, device="cuda:0", num_blocks=512, max_num_seqs=16,
                max_num_batched_tokens=2048, max_model_len=1024, graph_batch_sizes=[1, 2, 4, 8],
                draft_model=model, num_speculative_tokens=3, spec_sampled=True, spec_truncated=True)
    base.update(kw)
    return LLMEngine(EngineConfig(**base), model=model)


def _generate(eng, prompts, **kw):
    out = {}
    for i, p in enumerate(prompts):
        eng.add_request(f"r{i}", p, SamplingParams(max_tokens=16, temperature=0.9, seed=11 + i, ignore_eos=True, **kw))
    while eng.has_work():
        for o in eng.step():
            out.setdefault(o.request_id, []).extend(o.new_token_ids)
    torch.cuda.synchronize()
    return out


ENGINE_PROMPTS = [[128000] + list(range(300 + 13 * i, 340 + 13 * i)) for i in range(4)]


def test_engine_speculates_top_p_requests(llama_small):
    """Self-draft, graphs on, k = 3, temperature 0.9, top_p 0.9. Draft and verify rows go
    through different attention kernels, so p and q differ by bf16 rounding only; the bound
    is that of the untruncated self-draft test. Observed on an MI355X (4 requests of 16
    tokens): 44 draft tokens proposed, all counted as truncated, 44 accepted, 16 verify
    steps, mean_tokens_per_verify 3.75."""
    eng = _engine(llama_small)
    assert eng.runner.graphs and eng.spec.runner.graphs
    got = _generate(eng, ENGINE_PROMPTS, top_p=0.9)
    st = eng.stats()["speculative"]
    print(f"[spec-trunc] engine top_p=0.9: {st}")
    assert st["draft_tokens_proposed"] > 0
    assert st["truncated_draft_tokens_proposed"] == st["sampled_draft_tokens_proposed"] == st["draft_tokens_proposed"]
    assert st["truncated_draft_tokens_accepted"] == st["draft_tokens_accepted"]
    assert st["acceptance_rate"] > 0.8, st
    assert all(len(v) == 16 for v in got.values()) and len(got) == 4
    assert _generate(_engine(llama_small), ENGINE_PROMPTS, top_p=0.9) == got


def test_engine_speculates_top_k_requests(llama_small):
    """The same with top_k = 40. On nearly flat random weights K_p and K_q differ at the
    rank-40 near-ties, so a draft token may fall outside K_p; only proposals, some
    acceptance, completion and reproducibility are asserted. Observed on an MI355X: 45
    proposed, 43 accepted (acceptance_rate 0.956), 16 verify steps."""
    eng = _engine(llama_small)
    got = _generate(eng, ENGINE_PROMPTS, top_k=40)
    st = eng.stats()["speculative"]
    print(f"[spec-trunc] engine top_k=40: {st}")
    assert st["truncated_draft_tokens_proposed"] == st["draft_tokens_proposed"] > 0
    assert st["draft_tokens_accepted"] > 0
    assert all(len(v) == 16 for v in got.values()) and len(got) == 4
    assert _generate(_engine(llama_small), ENGINE_PROMPTS, top_k=40) == got
