"""A mixed step's attention in one launch (ops.mixed_attention, csrc/kernels/mixed_attention.hip)
against the three-launch form it replaces (rope_cache + decode_attention + prefill_attention)
and against the float64 references of tests/_attn_ref.py.

A step is a Case of _attn_ref: decode rows first (sequences of one query row), then the prompt
chunks, as the runner packs them; the block tables and lengths of the two sides are slices of one
table. The rows that the step appends are NaN in the cache before the call and travel in the K / V
columns of the QKV buffer, so the launch's own rope_cache must put them where the attention reads
them. Both forms run through PagedAttention.__call__, switched by attention.MIXED_ATTN (what
XGS_TUNE mixed_attn sets):
  * the one launch runs every row on the code of its own kernel in the configuration of the
    separate launch: output and caches bit for bit, with RoPE on;
  * both forms against float64 with _attn_ref's row-scaled bounds, RoPE off so that the appended
    rows are exact and the written pages can be compared bit for bit with the reference's cache.
"""
from __future__ import annotations

import functools

import pytest
import torch

import _attn_ref as R
from _row_ref import bits

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
D = 128


def dec_lens(n, bs):
    """n decode contexts: 1, 15, 16, 17, a page boundary +- 1, about 700, then more of the kind."""
    base = [700, 1, 15, 16, 17, bs - 1, bs + 1, 2 * bs - 1, 2 * bs, 2 * bs + 1, 333, 64, 65, 127, 129]
    return [base[i % len(base)] + 3 * (i // len(base)) for i in range(n)]


# (decode rows, prompts as (qlen, cached prefix)): every prompt length and row count of the issue
STEPS = [(1, [(1, 0)]), (3, [(33, 0)]), (63, [(64, 0)]), (3, [(65, 0)]), (63, [(512, 0)]),
         (3, [(33, 0), (130, 0)]), (63, [(130, 0), (33, 0)]), (1, [(64, 16)]), (3, [(65, 48)]),
         # eight prompts under a 512-row grid: with 32 query heads the prefill side is the one-key-phase,
         # three-slot configuration (8 * 4 row tiles * 16 head groups = 512 workgroups), else the two-phase one
         (3, [(512, 0), (1, 0), (33, 0), (64, 0), (65, 0), (130, 0), (5, 16), (7, 48)])]
HEADS = [(8, 2), (32, 8)]
PAGES = [16, 32]
# one kv head: 1, 3 or 63 decode rows are an ODD number of (sequence, kv head) items, so the last
# decode block of the grid holds one item and its waves 4-7 exit before the block's barrier
ODD_ITEMS = [(4, 1, 16), (4, 1, 32)]  # Hq, Hkv, page size


def step_case(nd, prompts, Hq, Hkv, bs):
    lens = dec_lens(nd, bs)
    qlens = (1,) * nd + tuple(q for q, _ in prompts)
    ctxs = tuple(L - 1 for L in lens) + tuple(c for _, c in prompts)
    return R.rand_case(qlens, ctxs, Hq, Hkv, D, bs, tag="mixed_step")


class Step:
    """Device inputs of one step: the cache without the step's own rows, the QKV buffer that
    holds them, and the metadata as the runner builds it."""

    def __init__(self, c, nd):
        from xgserve import ops
        from xgserve.models.base import AttnMeta
        self.c, self.nd = c, nd
        ks0, vs0 = [], []
        W = (c.Hq + 2 * c.Hkv) * D
        qkv = torch.full((c.T, W), R.NAN, dtype=torch.bfloat16)
        qkv[:, :c.Hq * D] = c.q.reshape(c.T, -1)
        for s, a, b, ctx, L in c.seqs():
            k, v = c.ks[s].clone(), c.vs[s].clone()
            qkv[a:b, c.Hq * D:(c.Hq + c.Hkv) * D] = k[ctx:L].reshape(b - a, -1)
            qkv[a:b, (c.Hq + c.Hkv) * D:] = v[ctx:L].reshape(b - a, -1)
            k[ctx:L] = R.NAN
            v[ctx:L] = R.NAN
            ks0.append(k)
            vs0.append(v)
        before = R.Case(c.q, ks0, vs0, c.qlens, c.ctxs, c.bs, c.scale, c.tag)
        self.kc0, self.vc0, self.bt = R.build_cache(before, DEV)
        self.kc_ref, self.vc_ref, bt_ref = R.build_cache(c, "cpu")
        assert torch.equal(bt_ref, self.bt.cpu())
        btc = self.bt.cpu()
        slots = [int(btc[int(c.seq[t]), int(c.lim[t]) // c.bs]) * c.bs + int(c.lim[t]) % c.bs for t in range(c.T)]
        self.qkv0 = qkv.to(DEV)
        self.cos_sin = ops.build_cos_sin(D, int(c.lim.max()) + 2, 500000.0).to(DEV)
        sl = R._i32(c.lens, DEV)
        qsl = R._i32([x - nd for x in c.start[nd:]], DEV)
        self.meta = AttnMeta(num_tokens=c.T, num_decodes=nd, positions=c.lim.to(torch.int32).to(DEV),
                             slot_mapping=R._i32(slots, DEV), dec_block_tables=self.bt[:nd], dec_seq_lens=sl[:nd],
                             num_splits=1, workspace=None, pre_block_tables=self.bt[nd:], pre_qsl=qsl,
                             pre_seq_lens=sl[nd:], pre_max_q=max(c.qlens[nd:], default=0))

    def run(self, monkeypatch, mode, rope, expect):
        """-> out [T, Hq, D], k cache, v cache on the CPU; `expect`: the path that must run."""
        from xgserve import ops
        from xgserve.models.base import PagedAttention
        from xgserve.ops import attention
        monkeypatch.setattr(attention, "MIXED_ATTN", mode)
        # which entries the layer calls: the one-launch form, or rope_cache and the separate launches
        ran = []
        for name, orig in (("mixed_attention", attention.mixed_attention), ("rope_cache", ops.rope.rope_cache)):
            monkeypatch.setattr(ops, name, lambda *a, _n=name, _f=orig, **k: (ran.append(_n), _f(*a, **k))[1])
        c = self.c
        attn = PagedAttention(c.Hq, c.Hkv, D, use_rope=rope)
        kc, vc, qkv = self.kc0.clone(), self.vc0.clone(), self.qkv0.clone()
        buf, out = R._out_slice(c, DEV)
        r = attn(qkv, self.meta, (kc, vc), self.cos_sin, out=out)
        assert ran == [{"mixed": "mixed_attention", "separate": "rope_cache"}[expect]], (ran, expect)
        assert r.data_ptr() == out.data_ptr()
        R._sentinel_kept(buf, c.T)
        return out.cpu(), kc.cpu(), vc.cpu()


@functools.lru_cache(maxsize=None)
def make_step(i, Hq, Hkv, bs):
    """STEPS[i], built once for the tests that run it (its inputs are cloned per run)."""
    nd, prompts = STEPS[i]
    return Step(step_case(nd, prompts, Hq, Hkv, bs), nd)


@pytest.mark.parametrize("bs", PAGES)
@pytest.mark.parametrize("Hq,Hkv", HEADS)
def test_one_launch_equals_three_bit_for_bit(monkeypatch, Hq, Hkv, bs):
    for i, (nd, prompts) in enumerate(STEPS):
        st = make_step(i, Hq, Hkv, bs)
        o0, k0, v0 = st.run(monkeypatch, 0, True, "separate")
        assert not bool(torch.isnan(o0.float()).any())
        o1, k1, v1 = st.run(monkeypatch, 1, True, "mixed")
        what = f"nd={nd} prompts={prompts}"
        assert torch.equal(o1, o0), f"{what}: {int((bits(o1) != bits(o0)).sum())} output elements differ"
        assert torch.equal(bits(k1), bits(k0)) and torch.equal(bits(v1), bits(v0)), f"{what}: cache pages differ"


@pytest.mark.parametrize("bs", PAGES)
@pytest.mark.parametrize("Hq,Hkv", HEADS)
def test_one_launch_against_float64(monkeypatch, Hq, Hkv, bs):
    used = {}
    for i, (nd, prompts) in enumerate(STEPS):
        st = make_step(i, Hq, Hkv, bs)
        c = st.c
        for mode in (0, 1):
            o, k, v = st.run(monkeypatch, mode, False, "mixed" if mode else "separate")
            note = f" mixed_attn={mode} nd={nd} prompts={prompts}"
            for key, u in R.check_rand(c, o, note).items():
                used[key] = max(used.get(key, 0.0), u)
            # the pages hold the reference's cache: the appended rows exactly, the others untouched
            assert torch.equal(bits(k), bits(st.kc_ref)) and torch.equal(bits(v), bits(st.vc_ref)), note
    print(f"Hq={Hq} Hkv={Hkv} bs={bs}: largest share of the bounds used {used}")


@pytest.mark.parametrize("Hq,Hkv,bs", ODD_ITEMS)
def test_odd_number_of_decode_items(monkeypatch, Hq, Hkv, bs):
    """Bit for bit against the three launches and against float64 where nd * Hkv is odd."""
    for i, (nd, prompts) in enumerate(STEPS[:7]):
        assert (nd * Hkv) % 2 == 1
        st = make_step(i, Hq, Hkv, bs)
        o0, k0, v0 = st.run(monkeypatch, 0, True, "separate")
        o1, k1, v1 = st.run(monkeypatch, 1, True, "mixed")
        what = f"nd={nd} prompts={prompts}"
        assert not bool(torch.isnan(o0.float()).any())
        assert torch.equal(o1, o0), f"{what}: {int((bits(o1) != bits(o0)).sum())} output elements differ"
        assert torch.equal(bits(k1), bits(k0)) and torch.equal(bits(v1), bits(v0)), f"{what}: cache pages differ"
        o, k, v = st.run(monkeypatch, 1, False, "mixed")
        R.check_rand(st.c, o, " " + what)
        assert torch.equal(bits(k), bits(st.kc_ref)) and torch.equal(bits(v), bits(st.vc_ref)), what


def test_other_steps_take_the_separate_launches(monkeypatch):
    """No decode row, no prompt row, or a split decode: the three launches, whatever mixed_attn says."""
    c = step_case(0, [(33, 0)], 8, 2, 16)
    o, _, _ = Step(c, 0).run(monkeypatch, 1, False, "separate")
    R.check_rand(c, o)
    c = R.rand_case((1, 1, 1), (0, 15, 699), 8, 2, D, 16, tag="mixed_step")
    o, _, _ = Step(c, 3).run(monkeypatch, 1, False, "separate")
    R.check_rand(c, o)
    c = step_case(3, [(33, 0)], 8, 2, 16)
    st = Step(c, 3)
    from xgserve.ops.attention import DecodeWorkspace
    st.meta.num_splits, st.meta.workspace = 2, DecodeWorkspace(3, 8, D, 2, DEV)
    o, _, _ = st.run(monkeypatch, 1, False, "separate")
    R.check_rand(c, o)


def _native_call(st, T, nd, Hq, Hkv, d, num_pre, kc, vc, qkv, out):
    from xgserve.ops._native import kernels, stream_ptr
    m = st.meta
    kernels().mixed_attention(qkv.data_ptr(), qkv.stride(0), m.positions.data_ptr(), st.cos_sin.data_ptr(),
                              kc.data_ptr(), vc.data_ptr(), m.slot_mapping.data_ptr(), T, nd,
                              st.bt.data_ptr(), st.bt.stride(0), m.dec_seq_lens.data_ptr(), st.bt.data_ptr(),
                              st.bt.stride(0), m.pre_qsl.data_ptr(), m.pre_seq_lens.data_ptr(), num_pre, 33,
                              out.data_ptr(), out.stride(0), Hq, Hkv, d, kc.shape[2], 0.088, 1, stream_ptr())


@pytest.mark.parametrize("what,T,nd,Hq,Hkv,d,num_pre", [
    ("no decode row", 36, 0, 8, 2, 128, 1), ("no prompt row", 3, 3, 8, 2, 128, 1), ("no prompt", 36, 3, 8, 2, 128, 0),
    ("D = 64", 36, 3, 16, 4, 64, 1), ("GQA group of 16", 36, 3, 16, 1, 128, 1), ("GQA group of 3", 36, 3, 6, 2, 128, 1)])
def test_native_entry_refuses_what_it_does_not_cover(what, T, nd, Hq, Hkv, d, num_pre):
    """An error and no launch: neither the output nor the cache nor the QKV rows change."""
    st = Step(step_case(3, [(33, 0)], 8, 2, 16), 3)
    kc, vc, qkv = st.kc0.clone(), st.vc0.clone(), st.qkv0.clone()
    buf, out = R._out_slice(st.c, DEV)
    with pytest.raises(ValueError, match="mixed_attention"):
        _native_call(st, T, nd, Hq, Hkv, d, num_pre, kc, vc, qkv, out)
    torch.cuda.synchronize()
    assert torch.equal(bits(buf), bits(torch.full_like(buf, R.SENT))), what
    assert torch.equal(bits(kc), bits(st.kc0)) and torch.equal(bits(vc), bits(st.vc0)), what
    assert torch.equal(bits(qkv), bits(st.qkv0)), what


# ---------------------------------------------------------------- the engine
@pytest.fixture(scope="module")
def llama_256():
    from dataclasses import replace
    from xgserve.models import build_model, get_config
    from xgserve.ops import _native
    _native.kernels()
    # llama-tiny (2 layers, hidden 256, vocabulary 512) with two heads of 128 on one kv head
    cfg = replace(get_config("llama-tiny"), num_heads=2, num_kv_heads=1, head_dim=128, name="llama-256-2l")
    return build_model(cfg, device=DEV, seed=11)


def _serve(model, monkeypatch, mode, graphs):
    """Three rows decoding, then a 400-token prompt joins them: greedy tokens of every request,
    and how often the model took the one-launch path."""
    from xgserve import ops
    from xgserve.engine import EngineConfig, LLMEngine, SamplingParams
    from xgserve.ops import attention
    monkeypatch.setattr(attention, "MIXED_ATTN", mode)
    # the few kv heads of this model would split the decode rows' keys: the fused launch is the unsplit form
    monkeypatch.setenv("XGS_TUNE", "decode_max_splits=1")
    calls = []
    orig = attention.mixed_attention
    monkeypatch.setattr(ops, "mixed_attention", lambda *a, **k: (calls.append(1), orig(*a, **k))[1])
    eng = LLMEngine(EngineConfig(model=model.cfg.name, device=DEV, num_blocks=256, max_num_seqs=16,
                                 max_num_batched_tokens=1024, max_model_len=1024, use_graphs=graphs,
                                 graph_batch_sizes=[16], decode_prefill_cap=512 if graphs else 0), model=model)
    sp = SamplingParams(max_tokens=6, temperature=0.0, ignore_eos=True)
    outs, mixed_steps = {}, 0
    for i in range(3):
        eng.add_request(f"d{i}", [1] + list(range(100 + 9 * i, 117 + 13 * i)), sp)  # (vocabulary: 512)
    n = 0
    while eng.has_work():
        for o in eng.step():
            outs.setdefault(o.request_id, []).extend(o.new_token_ids)
        n += 1
        if n == 2:
            eng.add_request("p", [1] + [3 + (7 * j) % 500 for j in range(399)], sp)
    assert all(len(v) == 6 for v in outs.values()) and len(outs) == 4, outs
    return outs, len(calls), eng


@pytest.mark.parametrize("graphs", [False, True])
def test_engine_tokens_do_not_move(llama_256, monkeypatch, graphs):
    want, n0, _ = _serve(llama_256, monkeypatch, 0, graphs)
    assert n0 == 0
    got, n1, eng = _serve(llama_256, monkeypatch, 1, graphs)
    assert n1 >= 2, "the mixed step did not take the one-launch path"  # once per layer
    if graphs:
        assert eng.runner.mixed_replays >= 1
    assert got == want
