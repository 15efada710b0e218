"""Logit processors (csrc/kernels/logit_proc.hip) against a numpy fp32 reference.

The contract leaves no rounding freedom -- every step is one fp32 operation, in a fixed
order, no fma -- so the processed logits must be bit-identical to the reference, -inf
positions included:

  seen (in prompt or generated):  x = x > 0 ? x / r : x * r
  x = x - (f * float(c));  where c > 0: x = x - p
  listed tokens: x = x + b
  T > 0 and min_p > 0:  y = x * (1 / T);  y < max(y) + fp32(ln min_p)  ->  x = -inf

The samplers then read the processed rows: every drawn token must be unmasked, greedy
rows must return the numpy argmax (the inputs keep the processed maximum at least
MARGIN = 1e-3 ahead of the runner-up, the sampler tests' own margin; asserted on the
CPU), and a plain row inside a processed step must return what the unprocessed call
returns.
"""
import functools
import math

import numpy as np
import pytest
import torch

from xgserve import ops
from xgserve.ops import _native
from xgserve.ops import sampling as SP

gpu = pytest.mark.gpu
DEV = "cuda:0"
F32 = np.float32
NEG_INF = F32(-np.inf)
MARGIN = 1e-3
SAT = 0x7FFF
FLAG = 0x8000

KINDS = ["all", "plain", "rep", "freq", "pres", "bias", "minp", "minp_greedy", "bias_on_max", "bias_new_max",
         "untracked_minp", "neg_pen", "all_greedy"]


# ------------------------------------------------------------------ reference
def ref_row(x, cell, r, f, p, bias_ids, bias_vals, temp, lm):
    """Steps 1-4 on one row: np.float32 operations in the stated order."""
    x = x.astype(F32).copy()
    r, f, p, lm = F32(r), F32(f), F32(p), F32(lm)
    c = (cell & SAT).astype(np.int32)
    with np.errstate(all="ignore"):
        seen = cell != 0
        x = np.where(seen, np.where(x > 0, x / r, x * r), x).astype(F32)
        fc = (f * c.astype(F32)).astype(F32)
        x = (x - fc).astype(F32)
        x = np.where(c > 0, (x - p).astype(F32), x)
        for t, b in zip(bias_ids, bias_vals):
            x[t] = F32(x[t] + F32(b))
        if temp > 0 and lm > NEG_INF:
            it = F32(1) / F32(temp)
            y = (x * it).astype(F32)
            thr = F32(y.max() + lm)
            x = np.where(y < thr, NEG_INF, x)
    return x.astype(F32)


def ln32(m):
    return F32(math.log(m)) if m > 0 else NEG_INF


# ------------------------------------------------------------------ inputs
def make_table(rng, S, V):
    """State cells per slot: prompt-only tokens, generated 1x / 7x, one token both in the
    prompt and generated, one cell at the saturation value."""
    st = np.zeros((S, V), np.uint16)
    special = {}
    for s in range(S):
        ids = rng.permutation(V)[:min(V // 4, 300)]
        n = len(ids) // 5
        st[s, ids[:n]] = FLAG
        st[s, ids[n:2 * n]] = 1
        st[s, ids[2 * n:3 * n]] = 7
        st[s, ids[3 * n:4 * n]] = FLAG | 3
        st[s, ids[4 * n]] = SAT
        st[s, ids[4 * n + 1]] = FLAG | SAT
        special[s] = ids
    return st, special


@functools.lru_cache(maxsize=None)
def build_case(V, rows, dtype_name, pad, seed=0):
    """Everything of one case on the host: input logits (already rounded to the input
    dtype), the state table, per-row parameters and the reference output."""
    rng = np.random.default_rng(1000 * seed + V + 7 * rows + pad)
    dtype = getattr(torch, dtype_name)
    S = rows + 2
    st, special = make_table(rng, S, V)
    x = (rng.standard_normal((rows, V)) * 3).astype(F32)
    x[:, rng.permutation(V)[:V // 50]] = 0.0          # exact zeros, seen tokens among them
    x[:, rng.permutation(V)[:4]] = -0.0
    kinds = [KINDS[(i + seed) % len(KINDS)] for i in range(rows)]
    for i, kind in enumerate(kinds):
        if kind == "plain" and i % 2 == 0:             # a greedy plain row: a clear winner in the input
            x[i, int(x[i].argmax())] += 6.0
    x = torch.from_numpy(x).to(dtype).float().numpy()  # what the kernel reads, exactly
    pi = np.zeros((3, rows), np.int32)
    pf = np.zeros((4, rows), F32)
    pf[0], pf[3] = 1.0, NEG_INF
    temps = np.zeros(rows, F32)
    bias_ids = np.zeros(rows * SP.LOGIT_BIAS_MAX, np.int32)
    bias_vals = np.zeros(rows * SP.LOGIT_BIAS_MAX, F32)
    slots = rng.permutation(S)
    ref = np.empty((rows, V), F32)
    for i, kind in enumerate(kinds):
        slot, r, f, p, m, temp, bias = int(slots[i]), 1.0, 0.0, 0.0, 0.0, 0.0, {}
        cell = st[slot]
        order = np.argsort(-x[i], kind="stable")
        if kind == "plain":
            slot, temp = -1, (0.8 if i % 2 else 0.0)
        elif kind == "rep":
            r, temp = 1.3, 0.9
        elif kind == "freq":
            f = 0.7
        elif kind == "pres":
            p, temp = 1.1, 1.0
        elif kind == "bias":
            ids = rng.permutation(V)[:SP.LOGIT_BIAS_MAX - 8]
            bias = {int(t): float(F32(rng.uniform(-100, 100))) for t in ids}
            bias[int(special[slot][0])] = -3.5    # a seen token, biased too
        elif kind == "minp":
            m, temp = 0.05, 0.8
        elif kind == "minp_greedy":
            m, temp = 0.5, 0.0
        elif kind == "bias_on_max":               # the maximum goes down: the threshold follows
            m, temp, bias = 0.1, 0.7, {int(order[0]): -2.0, int(order[5]): 0.25}
        elif kind == "bias_new_max":              # a low token becomes the maximum
            m, temp, bias = 0.1, 1.3, {int(order[V // 2]): 40.0}
        elif kind == "untracked_minp":
            slot, m, temp = -1, 0.02, 0.6
        elif kind == "neg_pen":
            r, f, p, temp = 0.8, -0.01, -0.5, 0.5
        elif kind in ("all", "all_greedy"):
            r, f, p, m = 1.5, 0.4, 0.6, 0.03
            temp = 0.0 if kind == "all_greedy" else 0.75
            bias = {int(order[1]): 4.0, int(special[slot][1]): 2.0, int(order[V // 3]): -100.0}
        if temp <= 0 and kind != "plain":
            # greedy: a clear winner the processors leave in front (checked below)
            top = int(order[0])
            bias[top] = bias.get(top, 0.0) + 60.0
        b_ids = list(bias.keys())
        b_vals = [bias[t] for t in b_ids]
        pi[:, i] = (slot, i * SP.LOGIT_BIAS_MAX, len(b_ids))
        pf[:, i] = (r, f, p, ln32(m))
        temps[i] = temp
        bias_ids[i * SP.LOGIT_BIAS_MAX:i * SP.LOGIT_BIAS_MAX + len(b_ids)] = b_ids
        bias_vals[i * SP.LOGIT_BIAS_MAX:i * SP.LOGIT_BIAS_MAX + len(b_ids)] = b_vals
        cell = st[slot] if slot >= 0 else np.zeros(V, np.uint16)
        ref[i] = ref_row(x[i], cell, r, f, p, b_ids, b_vals, temp, ln32(m))
        if temp <= 0:
            top2 = np.sort(ref[i])[-2:]
            assert top2[1] - top2[0] >= MARGIN, (kind, top2)
    return dict(V=V, rows=rows, dtype=dtype, x=x, st=st, pi=pi, pf=pf, temps=temps, bias_ids=bias_ids,
                bias_vals=bias_vals, ref=ref, kinds=kinds, pad=pad)


def test_reference_cases_are_sound():
    """CPU: the hand-made inputs hit what they claim to (masked rows, moved thresholds,
    clear greedy winners) before any kernel is judged by them."""
    c = build_case(4000, 65, "bfloat16", 0)
    assert set(c["kinds"]) == set(KINDS)
    for i, kind in enumerate(c["kinds"]):
        masked = int(np.isneginf(c["ref"][i]).sum())
        if kind in ("minp", "bias_on_max", "bias_new_max", "untracked_minp", "all"):
            assert 0 < masked < c["V"], (kind, masked)
        else:
            assert masked == 0, (kind, masked)
        if kind == "bias_new_max":
            assert masked >= c["V"] - 4    # the +40 token leaves (almost) nothing above the threshold
    # the row maximum always survives min_p
    for i in range(c["rows"]):
        assert np.isfinite(c["ref"][i].max())


# ------------------------------------------------------------------ GPU plumbing
@pytest.fixture(scope="module")
def native():
    _native.kernels()  # fail loudly: the GPU path must run the native library
    assert SP.SAMPLE_SPLIT


def dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).to(DEV)


def dev_table(st):
    return torch.from_numpy(st.view(np.int16).copy()).to(DEV)


def host_table(state):
    return state.cpu().numpy().view(np.uint16)


def run_process(c):
    V, rows, pad = c["V"], c["rows"], c["pad"]
    big = torch.zeros(rows, V + pad, dtype=c["dtype"], device=DEV)
    big[:, :V] = dev(c["x"], c["dtype"])
    logits = big[:, :V]
    state = dev_table(c["st"])
    out = ops.process_scratch(rows, V, DEV)
    out.fill_(float("nan"))
    temps = dev(c["temps"])
    ops.process_logits(logits, out, state, dev(c["pi"]), dev(c["pf"]), temps, dev(c["bias_ids"]),
                       dev(c["bias_vals"]))
    torch.cuda.synchronize()
    assert np.array_equal(host_table(state), c["st"]), "process_logits wrote to the state table"
    return logits, out, temps


def assert_bits(got, ref, kinds):
    same = got.view(np.uint32) == ref.view(np.uint32)
    bad = np.argwhere(~same)
    print(f"rows {got.shape[0]} V {got.shape[1]}: {bad.shape[0]} differing cells, "
          f"{int(np.isneginf(ref).sum())} masked")
    assert bad.shape[0] == 0, [(int(i), kinds[i], int(t), float(got[i, t]), float(ref[i, t])) for i, t in bad[:8]]


# ------------------------------------------------------------------ process_logits
@gpu
@pytest.mark.parametrize("dtype", ["bfloat16", "float32"])
@pytest.mark.parametrize("rows", [1, 5, 65])
@pytest.mark.parametrize("V", [1003, 4000, 128256])
def test_process_logits_bit_exact(native, V, rows, dtype):
    c = build_case(V, rows, dtype, 0)
    _, out, _ = run_process(c)
    assert_bits(out.cpu().numpy(), c["ref"], c["kinds"])


@gpu
@pytest.mark.parametrize("pad", [24, 3])
@pytest.mark.parametrize("dtype", ["bfloat16", "float32"])
def test_process_logits_row_stride(native, dtype, pad):
    """Rows further apart than V: 16-byte aligned rows (pad 24) and unaligned ones (pad 3)."""
    c = build_case(4000, 5, dtype, pad, seed=1)
    logits, out, _ = run_process(c)
    assert logits.stride(0) == 4000 + pad
    assert_bits(out.cpu().numpy(), c["ref"], c["kinds"])


@gpu
def test_process_logits_every_kind_at_one_row(native):
    """rows = 1 with each parameter set in turn (the split over workgroups has no other row to hide in)."""
    for seed in range(len(KINDS)):
        c = build_case(128256, 1, "bfloat16", 0, seed=seed)
        _, out, _ = run_process(c)
        assert_bits(out.cpu().numpy(), c["ref"], c["kinds"])


# ------------------------------------------------------------------ state table
@gpu
@pytest.mark.parametrize("V", [1003, 128256])
def test_state_reset_and_update(native, V):
    rng = np.random.default_rng(V)
    S = 5
    state = ops.logit_state_alloc(S, V, DEV)
    state.fill_(0x1111)  # stale cells of earlier owners everywhere
    ref = np.full((S, V), 0x1111, np.uint16)

    def expected_row(prompt, gen, preset=()):
        """The contract, from the sequence alone: saturating count of the generated
        tokens, bit 15 where the token occurs in the prompt."""
        row = np.minimum(np.bincount(np.asarray(gen, np.int64), minlength=V), SAT).astype(np.uint16)
        row[np.asarray(prompt, np.int64)] |= FLAG
        for t, cell in preset:
            row[t] = cell
        return row

    def reset(entries, owners):
        """entries: what the host code under test packs; owners: (prompt, gen, preset cells) per entry."""
        packed, nres, total = ops.pack_state_resets(entries)
        ops.logit_state_reset(state, dev(packed), nres, total)
        for (slot, _, _), (prompt, gen, preset) in zip(entries, owners):
            ref[slot] = expected_row(prompt, gen, preset)

    def update(slots, toks):
        ops.logit_state_update(state, dev(np.asarray(slots, np.int32)), dev(np.asarray(toks, np.int32)), len(slots))
        for s, t in zip(slots, toks):
            if s >= 0 and (ref[s, t] & SAT) < SAT:
                ref[s, t] += 1

    def owner(n_prompt, n_gen):
        prompt = rng.integers(0, V, n_prompt)
        gen = rng.integers(0, V, n_gen)
        if n_gen:
            gen[:3] = prompt[:3]  # in the prompt and generated
            gen[3:9] = gen[9]     # one token seven times
        return prompt, gen

    pa, ga = owner(700, 40)
    pb, gb = owner(30, 0)
    ia, ca = ops.logit_state_cells(pa, ga)
    ib, cb = ops.logit_state_cells(pb, gb)
    assert ca[np.searchsorted(ia, ga[9])] & SAT == int((ga == ga[9]).sum()) >= 7
    assert ca[np.searchsorted(ia, pa[0])] & FLAG and ca[np.searchsorted(ia, pa[0])] & SAT
    sat_tok = int(ib[0])
    cb[0] = FLAG | SAT  # a cell at the saturation value: the update leaves it there
    reset([(0, ia, ca), (3, ib, cb)], [(pa, ga, ()), (pb, gb, [(sat_tok, FLAG | SAT)])])
    torch.cuda.synchronize()
    assert np.array_equal(host_table(state), ref)
    for step in range(6):
        update([0, -1, 3, -1], [int(ga[9]) if step % 2 else int(rng.integers(0, V)), 5, sat_tok, V - 1])
    torch.cuda.synchronize()
    assert np.array_equal(host_table(state), ref)
    assert ref[3, sat_tok] == FLAG | SAT
    # slot 0 gets a second owner: nothing of the first may survive
    pc, gc = owner(50, 12)
    ic, cc = ops.logit_state_cells(pc, gc)
    reset([(0, ic, cc)], [(pc, gc, ())])
    update([3, 0], [int(pb[1]), int(gc[0])])
    update([0], [int(pa[0])])
    torch.cuda.synchronize()
    got = host_table(state)
    assert np.array_equal(got, ref)
    assert np.array_equal(got[1], np.full(V, 0x1111, np.uint16))  # untouched slots stay untouched
    assert int((got[0] != 0).sum()) <= len(ic) + 2


# ------------------------------------------------------------------ through the samplers
def sample_v1(logits, temps, seeds):
    """The one-workgroup-per-row kernel: the raw binding without a workspace."""
    B, V = logits.shape
    tok = torch.empty(B, dtype=torch.int32, device=DEV)
    lp = torch.empty(B, dtype=torch.float32, device=DEV)
    _native.kernels().sample_tokens(logits.data_ptr(), 1 if logits.dtype == torch.float32 else 0, logits.stride(0), B,
                                    V, temps.data_ptr(), 0, 0, seeds.data_ptr(), 0, tok.data_ptr(), lp.data_ptr(),
                                    _native.stream_ptr(), 0, 0)
    return tok, lp


def sample_v2(logits, temps, seeds):
    return ops.sample_tokens(logits, temps, None, None, seeds, 0)


SAMPLERS = {"v1": sample_v1, "v2": sample_v2}


@gpu
@pytest.mark.parametrize("sampler", ["v2", "v1"])
@pytest.mark.parametrize("V,rows", [(1003, 65), (128256, 13)])
def test_samplers_read_processed_rows(native, V, rows, sampler):
    c = build_case(V, rows, "bfloat16", 0, seed=2)
    _, out, temps = run_process(c)
    assert_bits(out.cpu().numpy(), c["ref"], c["kinds"])
    for rnd in range(3):
        seeds = dev(np.arange(rows, dtype=np.int64) * 7919 + 101 * rnd)
        tok, lp = SAMPLERS[sampler](out, temps, seeds)
        torch.cuda.synchronize()
        tok, lp = tok.cpu().numpy(), lp.cpu().numpy()
        for i in range(rows):
            t = int(tok[i])
            assert 0 <= t < V and np.isfinite(c["ref"][i, t]), (i, c["kinds"][i], t)
            assert np.isfinite(lp[i]) and lp[i] <= 1e-6
            if c["temps"][i] <= 0:
                assert t == int(c["ref"][i].argmax()), (i, c["kinds"][i])
    # the all-greedy path (argmax_logprob) on the same scratch
    tok, _ = ops.argmax_logprob(out)
    torch.cuda.synchronize()
    tok = tok.cpu().numpy()
    for i in range(rows):
        if c["temps"][i] <= 0:
            assert int(tok[i]) == int(c["ref"][i].argmax())
        assert np.isfinite(c["ref"][i, int(tok[i])])


@gpu
@pytest.mark.parametrize("sampler", ["v2", "v1"])
@pytest.mark.parametrize("V", [4000, 128256])
def test_plain_rows_keep_their_token(native, V, sampler):
    """A plain row of a processed step is the bf16 -> fp32 conversion and nothing else:
    same token as the same row through the unprocessed call, greedy and seeded T = 0.8."""
    rows = 26
    c = build_case(V, rows, "bfloat16", 0, seed=3)
    logits, out, temps = run_process(c)
    plain = [i for i, k in enumerate(c["kinds"]) if k == "plain"]
    assert {float(c["temps"][i]) for i in plain} == {0.0, float(F32(0.8))}
    assert np.array_equal(out.cpu().numpy()[plain].view(np.uint32), c["x"][plain].view(np.uint32))
    seeds = dev(np.arange(rows, dtype=np.int64) + 12345)
    a, alp = SAMPLERS[sampler](out, temps, seeds)
    b, blp = SAMPLERS[sampler](logits, temps, seeds)
    torch.cuda.synchronize()
    a, b = a.cpu().numpy(), b.cpu().numpy()
    assert [int(a[i]) for i in plain] == [int(b[i]) for i in plain]
    # the logprob's log-sum-exp runs over 4-wide vectors on fp32 rows and 8-wide ones on
    # bf16 rows, so its fp32 sum is taken in another order: a few ulp of a value near 10
    # (1e-5 at most), against the 1e-3 the sampler tests allow a logprob
    np.testing.assert_allclose(alp.cpu().numpy()[plain], blp.cpu().numpy()[plain], rtol=0, atol=1e-4)
