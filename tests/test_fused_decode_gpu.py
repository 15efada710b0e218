"""Fused decode layer on the MI355X: gemm_m64g's RMSNorm row-scale and residual
(GG_RESID) epilogues, the fused QKV -> RoPE -> KV-append attention prologue, and
the fused model path -- each against a plain fp32 PyTorch reference (or the
unfused kernel chain that is itself checked against fp32 elsewhere)."""
import math
from dataclasses import replace

import pytest
import torch
import torch.nn.functional as F

from xgserve import ops
from xgserve.ops import _native
from xgserve.ops import linear as lin
from xgserve.ops.linear import (MODE_PARTIAL, MODE_SILU, PendingSum, ResidWorkspace, RowStats, interleave_gate_up,
                                m64_linear, m64_resid_linear)

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(autouse=True, scope="module")
def _k():
    _native.kernels()  # fail loudly: the HIP library must be the one that runs
    torch.manual_seed(0)


def rnd(*s, scale=1.0):
    return (torch.randn(*s, device=DEV) * scale).bfloat16()


def rel_err(a, b):
    return float((a.float() - b.float()).norm() / b.float().norm().clamp_min(1e-6))


@pytest.mark.parametrize("M,n_parts", [(1, 1), (5, 4), (16, 8), (24, 1), (64, 4), (64, 8), (1, 64), (9, 64),
                                        (16, 32), (33, 64), (64, 64), (64, 32), (40, 16)])
def test_norm_linear_row_scale(M, n_parts):
    K = 4096
    x = rnd(M, K)
    sq = x.float() ** 2
    st = RowStats(sq.view(M, n_parts, -1).sum(-1).t().contiguous(), n_parts, M)
    h = x.float() * torch.rsqrt(sq.sum(-1, keepdim=True) / K + 1e-5)
    w = rnd(6144, K, scale=0.02)
    pend = m64_linear(x, w, MODE_PARTIAL, stats=st, eps=1e-5)
    assert rel_err(pend.part.sum(0), h @ w.float().t()) < 2e-3
    g, u = rnd(14336, K, scale=0.02), rnd(14336, K, scale=0.02)
    y = m64_linear(x, interleave_gate_up(g, u), MODE_SILU, stats=st, eps=1e-5)
    ref = F.silu(h @ g.float().t()) * (h @ u.float().t())
    assert rel_err(y, ref) < 1e-2


@pytest.mark.parametrize("M", [1, 4, 16])
@pytest.mark.parametrize("n_parts", [128])
@pytest.mark.parametrize("N,K,mode", [(1280, 8192, MODE_PARTIAL), (7168, 8192, MODE_SILU), (6144, 4096, MODE_PARTIAL),
                                      (28672, 4096, MODE_SILU)])
def test_norm_linear_128_partial_sums(M, n_parts, N, K, mode):
    """M <= 16 consumers combine up to 128 per-tile statistics (the wide path at 2 / 4
    waves: 70B TP8 and 8B decode plans), so a 128-tile GG_AR / GG_RESID producer needs
    no pair combine."""
    x = rnd(M, K)
    sq = x.float() ** 2
    st = RowStats(sq.view(M, n_parts, -1).sum(-1).t().contiguous(), n_parts, M)
    h = x.float() * torch.rsqrt(sq.sum(-1, keepdim=True) / K + 1e-5)
    if mode == MODE_PARTIAL:
        w = rnd(N, K, scale=0.02)
        pend = m64_linear(x, w, MODE_PARTIAL, stats=st, eps=1e-5)
        assert rel_err(pend.part.sum(0), h @ w.float().t()) < 2e-3
    else:
        g, u = rnd(N // 2, K, scale=0.02), rnd(N // 2, K, scale=0.02)
        y = m64_linear(x, interleave_gate_up(g, u), MODE_SILU, stats=st, eps=1e-5)
        assert rel_err(y, F.silu(h @ g.float().t()) * (h @ u.float().t())) < 1e-2


@pytest.mark.parametrize("M", [1, 17, 64])
@pytest.mark.parametrize("S,cfg", [(1, 7), (2, 7), (4, 7), (2, 1), (2, 5), (2, 6), (4, 6), (4, 0), (4, 1), (4, 3)])
@pytest.mark.parametrize("normed", [False, True])
def test_split_silu_and_wide_tile(M, S, cfg, normed):
    """Split-K SiLU-gate (fp32 slabs, per-tile tickets, last arriver reduces + gates)
    and the 8-wave 256-column tile, against fp32; the tickets must be re-armed (zero)
    after every launch, so a second launch on the same counters gives the same result."""
    K, F2 = 4096, 2 * 4096
    x = rnd(M, K)
    g, u = rnd(F2 // 2, K, scale=0.02), rnd(F2 // 2, K, scale=0.02)
    w = interleave_gate_up(g, u)
    h = x.float()
    st = None
    if normed:
        sq = h ** 2
        st = RowStats(sq.view(M, 4, -1).sum(-1).t().contiguous(), 4, M)
        h = h * torch.rsqrt(sq.sum(-1, keepdim=True) / K + 1e-5)
    ref = F.silu(h @ g.float().t()) * (h @ u.float().t())
    lin._M64_TUNED[(F2, K, MODE_SILU)] = {64: (2, S, cfg), 32: (2, S, cfg), 16: (2, S, cfg)}
    try:
        for _ in range(2):
            if normed:
                y = m64_linear(x, w, MODE_SILU, stats=st, eps=1e-5)
            else:
                y = lin.m64_linear(x, w, MODE_SILU)
            assert rel_err(y, ref) < 1e-2
    finally:
        del lin._M64_TUNED[(F2, K, MODE_SILU)]
    torch.cuda.synchronize()
    assert int(lin.tile_counters(x.device, F2).abs().sum()) == 0


@pytest.mark.parametrize("M", [65, 575, 1536])
def test_splitk_prefill_down_into_add_rmsnorm(M):
    """Prefill-sized down projection as one K-split batched GEMM with fp32 partials,
    reduced by the consumer (add + RMSNorm prologue), against fp32."""
    N, K = 4096, 14336
    x, w, r0 = rnd(M, K, scale=0.5), rnd(N, K, scale=0.02), rnd(M, N)
    nw = (torch.rand(N, device=DEV) + 0.5).bfloat16()
    assert lin.splitk_prefill_ok(x, w)
    pend = lin.splitk_linear(x, w, 2)
    d = x.float() @ w.float().t()
    assert rel_err(pend.part.sum(0), d) < 1e-5
    h, r = ops.fused_add_rmsnorm(pend, r0.clone(), nw, 1e-5)
    rr = r0.float() + d
    assert rel_err(r, rr) < 1e-2
    ref = rr.bfloat16().float() * torch.rsqrt((rr.bfloat16().float() ** 2).mean(-1, keepdim=True) + 1e-5) * nw.float()
    assert rel_err(h, ref) < 1e-2


@pytest.mark.parametrize("M", [1, 40, 64])
@pytest.mark.parametrize("N,K,S", [(6144, 4096, 4), (4096, 14336, 8), (4096, 4096, 2)])
def test_wide_tile_partials(M, N, K, S):
    x, w = rnd(M, K), rnd(N, K, scale=0.02)
    pend = lin.m64_linear(x, w, MODE_PARTIAL, split_k=S, nw=2, cfg=7)
    assert rel_err(pend.part.sum(0), x.float() @ w.float().t()) < 2e-3


@pytest.mark.parametrize("M", [1, 7, 16, 33, 64])
@pytest.mark.parametrize("N,K", [(4096, 4096), (4096, 14336)])
@pytest.mark.parametrize("inlaunch", [True, False])
def test_resid_linear(M, N, K, inlaunch, monkeypatch):
    """inlaunch True: last-arriver ticket reduce; False: separate add_partials_resid."""
    monkeypatch.setattr(lin, "RESID_INLAUNCH_MAX_BYTES", (1 << 30) if inlaunch is True else 0)
    x, w, r0 = rnd(M, K), rnd(N, K, scale=0.02), rnd(M, N)
    ws = ResidWorkspace(4, 64, N, DEV)
    ref = (r0.float() + x.float() @ w.float().t()).bfloat16().float()
    runs = []
    for _ in range(3):  # the tickets are re-armed by their winners: repeated launches stay exact
        r = r0.clone()
        st = m64_resid_linear(x, w, r, ws, 1, 1e-5)
        torch.testing.assert_close(r.float(), ref, atol=3e-2, rtol=2e-2)
        ss = st.ss.reshape(-1)[: st.n * st.stride].view(st.n, st.stride)[:, :M].sum(0)
        nw, S, cfg = lin.m64_plan(M, N, K, MODE_PARTIAL)
        if inlaunch is True:  # one partial sum per column tile
            assert st.n == N // (16 * nw * lin.M64G_CFGS[cfg][0])
        else:
            assert st.n == N // 1024
        assert rel_err(ss, (r.float() ** 2).sum(-1)) < 1e-5
        runs.append((r.clone(), ss.clone()))
    assert all(torch.equal(runs[0][0], a) and torch.equal(runs[0][1], b) for a, b in runs)  # deterministic
    assert int(ws.counters.abs().sum()) == 0


def _paged(lens, Hkv, D, bs, extra_pages=8):
    pages_per = [(L + bs - 1) // bs for L in lens]
    NB = sum(pages_per) + extra_pages
    kc = rnd(NB, Hkv, bs, D)
    vc = rnd(NB, Hkv, bs, D)
    perm = torch.randperm(NB).tolist()
    bt = torch.zeros(len(lens), max(pages_per), dtype=torch.int32)
    i = 0
    for s, n in enumerate(pages_per):
        bt[s, :n] = torch.tensor(perm[i:i + n])
        i += n
    return kc, vc, bt.to(DEV)


@pytest.mark.parametrize("Hq,Hkv", [(32, 8), (64, 8), (8, 8)])
@pytest.mark.parametrize("S", [1, 4, 8, 12])
@pytest.mark.parametrize("splits", [1, 3, 16])
@pytest.mark.parametrize("depth", [2, 3, 4])
def test_decode_attention_fused_prologue(Hq, Hkv, S, splits, depth):
    """S <= 8 runs the split prologue (partial loads issued ahead of the K/V
    preloads), S = 12 and depth 4 the classic one."""
    import xgserve.ops.attention as A
    D, bs = 128, 16
    lens = [1, 17, 300, 64, 0, 129]  # row 4: a graph padding row (no KV write, no attention)
    kc, vc, bt = _paged([max(1, L) for L in lens], Hkv, D, bs)
    B = len(lens)
    part = torch.randn(S, B, (Hq + 2 * Hkv) * D, device=DEV) * 0.3
    pos = torch.tensor([max(0, L - 1) for L in lens], dtype=torch.int32, device=DEV)
    slots = torch.tensor([int(bt[b, (L - 1) // bs]) * bs + (L - 1) % bs if L > 0 else -1
                          for b, L in enumerate(lens)], dtype=torch.int32, device=DEV)
    sl = torch.tensor(lens, dtype=torch.int32, device=DEV)
    cs = ops.build_cos_sin(D, 4096, 500000.0, device=DEV)
    scale = 1.0 / math.sqrt(D)
    kc1, vc1, kc2, vc2 = kc.clone(), vc.clone(), kc.clone(), vc.clone()
    ws = A.DecodeWorkspace(B, Hq, D, splits, DEV)
    out = ops.decode_attention_fused(PendingSum(part, S), pos, slots, cs, kc1, vc1, bt, sl, Hq, scale, splits,
                                     workspace=ws, depth=depth)
    # reference: the unfused chain (rope_cache_partials -> fp32 attention reference)
    q = torch.empty(B, Hq * D, dtype=torch.bfloat16, device=DEV)
    ops.rope_cache_partials(PendingSum(part, S), q, pos, cs, kc2, vc2, slots, Hq, Hkv, D)
    ref = ops.decode_attention_ref(q.view(B, Hq, D).cpu(), kc2.cpu(), vc2.cpu(), bt.cpu(), sl.cpu(), scale)
    torch.testing.assert_close(out.view(B, Hq, D).cpu().float(), ref.float(), atol=2e-2, rtol=2e-2)
    torch.testing.assert_close(kc1.float(), kc2.float(), atol=2e-2, rtol=2e-2)
    torch.testing.assert_close(vc1.float(), vc2.float(), atol=0, rtol=0)
    assert out[4].float().abs().max().item() == 0.0


@pytest.fixture(scope="module")
def llama_small():
    from xgserve.models import build_model, get_config
    cfg = replace(get_config("llama3-8b"), num_layers=2, name="llama3-8b-2l")
    return build_model(cfg, device="cuda:0", seed=3)


@pytest.mark.parametrize("M", [1, 17])
@pytest.mark.parametrize("name,mode", [("qkv", MODE_PARTIAL), ("gate_up", MODE_SILU)])
def test_m64_linear_stats_matches_prenormed(llama_small, M, name, mode):
    """m64_linear with `stats` (the RMSNorm as an epilogue row scale of the raw x) against
    the same wrapper on rmsnorm(x), on the 8B QKV [6144, 4096] and gate_up [28672, 4096]."""
    w = getattr(llama_small.layers[0], name)
    K = w.shape[1]
    assert tuple(w.shape) == ((6144, 4096) if name == "qkv" else (28672, 4096))
    x = rnd(M, K)
    st = RowStats((x.float() ** 2).view(M, 4, -1).sum(-1).t().contiguous(), 4, M)
    got = m64_linear(x, w, mode, stats=st, eps=1e-5)
    ref = m64_linear(ops.rmsnorm(x, torch.ones(K, device=DEV, dtype=torch.bfloat16), 1e-5), w, mode)
    if mode == MODE_PARTIAL:
        assert rel_err(got.part.sum(0), ref.part.sum(0)) < 2e-3
    else:
        assert got.shape == ref.shape == (M, w.shape[0] // 2)
        assert rel_err(got, ref) < 1e-2


@pytest.mark.parametrize("fused", [True, False])
def test_decode_step_logits_match_reference(llama_small, fused, monkeypatch):
    """One eager pure-decode step through the fused (or unfused) layer chain vs the
    dense fp32 reference forward with the same weights."""
    import xgserve.models.llama as ll
    from xgserve.engine import EngineConfig, LLMEngine, SamplingParams
    from xgserve.models.reference import reference_logits
    monkeypatch.setattr(ll, "FUSED_DECODE", fused)
    assert llama_small._fused_ok and llama_small.norms_folded
    eng = LLMEngine(EngineConfig(model=llama_small.cfg.name, device="cuda:0", num_blocks=256, max_num_seqs=8,
                                 max_num_batched_tokens=1024, max_model_len=512, use_graphs=False),
                    model=llama_small)
    eng.runner.capture_logits = True
    prompt = [128000] + list(range(700, 790))
    eng.add_request("d", prompt, SamplingParams(max_tokens=2, temperature=0.0, ignore_eos=True))
    toks = []
    while eng.has_work():
        for o in eng.step():
            toks += o.new_token_ids
    assert len(toks) == 2
    got = eng.runner.last_logits[-1]
    ref = reference_logits(llama_small, prompt + toks[:1])[-1].float().cpu()
    assert float((got - ref).norm() / ref.norm()) < 2e-2


def test_fused_batch_decode_matches_unfused(llama_small, monkeypatch):
    """A 5-sequence greedy decode (graphs on): the first decode token of every
    sequence from the fused chain matches the unfused chain's (bf16 rounding order
    differs, so one near-tie flip is tolerated)."""
    import xgserve.models.llama as ll
    from xgserve.engine import EngineConfig, LLMEngine, SamplingParams
    prompts = [[128000] + list(range(1200 + 9 * i, 1260 + 4 * i)) for i in range(5)]
    sp = SamplingParams(max_tokens=4, temperature=0.0, ignore_eos=True)
    outs = {}
    for fused in (True, False):
        monkeypatch.setattr(ll, "FUSED_DECODE", fused)
        eng = LLMEngine(EngineConfig(model=llama_small.cfg.name, device="cuda:0", num_blocks=256, max_num_seqs=8,
                                     max_num_batched_tokens=1024, max_model_len=512, graph_batch_sizes=[1, 2, 4, 8]),
                        model=llama_small)
        outs[fused] = eng.generate(prompts, sp)
    agree = sum(a[1] == b[1] for a, b in zip(outs[True], outs[False]))
    assert agree >= 4, outs


@pytest.fixture(scope="module")
def mixtral_small():
    from xgserve.models import build_model, get_config
    cfg = replace(get_config("mixtral-8x7b"), num_layers=2, intermediate_size=1792, name="mixtral-2l")
    return build_model(cfg, device="cuda:0", seed=5)


@pytest.mark.parametrize("T", [1, 5, 64])
def test_moe_route_norm_and_combine_resid(T):
    """Fused MoE decode pieces vs their unfused forms: router with the RMSNorm in its
    prologue (normalised rows, weights, ids) and the combine that adds into the
    residual stream and writes the next norm's per-1024-column statistics."""
    H, E, k, F = 4096, 8, 2, 1792
    resid = rnd(T, H)
    norm_w = (1 + 0.1 * torch.randn(H, device=DEV)).bfloat16()
    router = rnd(E, H, scale=0.05)
    hn, w, ids = ops.moe_route_norm(resid, norm_w, 1e-5, router, k)
    want_hn = ops.rmsnorm(resid, norm_w, 1e-5)
    torch.testing.assert_close(hn.float(), want_hn.float(), atol=2e-2, rtol=1e-2)
    w2_, ids2 = ops.moe_route(hn, router, k)
    assert torch.equal(ids.cpu(), ids2.cpu())
    torch.testing.assert_close(w, w2_, atol=1e-5, rtol=1e-5)
    from xgserve.ops.linear import interleave_gate_up
    w13 = torch.stack([interleave_gate_up(rnd(F, H, scale=0.05), rnd(F, H, scale=0.05)) for _ in range(E)])
    w2 = rnd(E, H, F, scale=0.05)
    out = ops.fused_moe(hn, w13, w2, w, ids)
    # separate combine kernel (1024-column statistics), then the combine inside the
    # w2 launch (per-128-column-tile statistics; twice: the tickets must re-arm)
    counters = torch.zeros(128, dtype=torch.int32, device=DEV)
    for use_ctr, reps in ((False, 1), (True, 2)):
        for _ in range(reps):
            r = resid.clone()
            ss = torch.full((64 * T,), -1.0, device=DEV)
            n = ops.fused_moe(hn, w13, w2, w, ids, resid=r, ss=ss, counters=counters if use_ctr else None)
            from xgserve.ops import moe as MO
            pairs = T * k
            small = pairs <= MO.MOE_W2_SMALL_LOW or MO.MOE_W2_SMALL_HIGH <= pairs <= MO.MOE_PREFILL_PAIRS
            tile = 64 if (MO.MOE_W2_SMALL and small) else 128  # decode-sized w2 tiles
            assert n == (H // tile if use_ctr else H // 1024)
            want = (resid.float() + out.float()).bfloat16()
            assert rel_err(r, want) < 1e-2
            want_ss = r.float().view(T, n, H // n).pow(2).sum(-1).t().reshape(-1)
            torch.testing.assert_close(ss[: n * T], want_ss, rtol=1e-4, atol=1e-2)
        torch.cuda.synchronize()
        assert int(counters.abs().sum()) == 0


@pytest.mark.parametrize("fused", [True, False])
def test_mixtral_decode_step_logits_match_reference(mixtral_small, fused, monkeypatch):
    """Mixtral on the fused decode layer (attention half as for dense models, router
    with the post-attention norm, combine into the residual) vs the fp32 reference."""
    import xgserve.models.llama as ll
    from xgserve.engine import EngineConfig, LLMEngine, SamplingParams
    from xgserve.models.reference import reference_logits
    monkeypatch.setattr(ll, "FUSED_DECODE", fused)
    assert mixtral_small._fused_ok and mixtral_small.norms_folded
    eng = LLMEngine(EngineConfig(model=mixtral_small.cfg.name, device="cuda:0", num_blocks=256, max_num_seqs=8,
                                 max_num_batched_tokens=1024, max_model_len=512, use_graphs=False),
                    model=mixtral_small)
    eng.runner.capture_logits = True
    prompt = [1] + list(range(300, 380))
    eng.add_request("m", prompt, SamplingParams(max_tokens=2, temperature=0.0, ignore_eos=True))
    toks = []
    while eng.has_work():
        for o in eng.step():
            toks += o.new_token_ids
    assert len(toks) == 2
    got = eng.runner.last_logits[-1]
    ref = reference_logits(mixtral_small, prompt + toks[:1])[-1].float().cpu()
    # top-2 routing is discontinuous: a near-tie expert choice of one prompt token that
    # flips between the bf16 engine and the fp32 reference moves the logits by a few %
    # (bench/diag_moe_mw.py: 1.5-4.8 % across prompts, the same with the prompt step on
    # gemm_mw or on the library GEMMs), so the bound is looser than the dense model's
    # and the greedy choice must agree
    assert float((got - ref).norm() / ref.norm()) < 6e-2
    assert int(got.argmax()) == int(ref.argmax())


def test_mixtral_fused_batch_decode_matches_unfused(mixtral_small, monkeypatch):
    """6 sequences, graphs on: the fused MoE decode chain's greedy tokens agree with the
    unfused chain's (one near-tie flip tolerated)."""
    import xgserve.models.llama as ll
    from xgserve.engine import EngineConfig, LLMEngine, SamplingParams
    prompts = [[1] + list(range(500 + 7 * i, 540 + 3 * i)) for i in range(6)]
    sp = SamplingParams(max_tokens=4, temperature=0.0, ignore_eos=True)
    outs = {}
    for fused in (True, False):
        monkeypatch.setattr(ll, "FUSED_DECODE", fused)
        eng = LLMEngine(EngineConfig(model=mixtral_small.cfg.name, device="cuda:0", num_blocks=256, max_num_seqs=8,
                                     max_num_batched_tokens=1024, max_model_len=512, graph_batch_sizes=[1, 2, 4, 8]),
                        model=mixtral_small)
        outs[fused] = eng.generate(prompts, sp)
    agree = sum(a[1] == b[1] for a, b in zip(outs[True], outs[False]))
    assert agree >= 5, outs
