"""Both samplers of csrc/kernels/sampling.hip against an exact CPU reference.

The draw is Gumbel-max over a counter hash of (seed, step, index), so a float64 numpy
reference reproduces it and the kernels are held to the exact token. The split-row
sampler ("v2", `ops.sample_tokens`) and the one-workgroup sampler ("v1", the raw binding
without a workspace) run every case unless noted.

Reference (`ref_row`, no device code):
  * hash32 and the key mix below are the written contract that a fixed seed reproduces;
    u = ((hsh >> 9) + 0.5) / 2^23, g = -log(-log u), y = fp32(x) * fp32(1 / temp).
  * the kernels keep whole sub-bins, so the kept set is bracketed: L (certainly kept) and
    U (possibly kept), W = 2 * 40 / 2^20 (two v2 sub-bins), EPS on the top-p mass. The
    expected token is the argmax of y + g over U.
  * a row is ambiguous when that winner is not in L or the two best scores over U are
    closer than MARGIN = 1e-3 (> 100x the fp32 rounding of a score plus two __logf).
    Unambiguous rows must match exactly; every row's token lies in U and its logprob is
    y[tok] - logZ within 1e-3. Each case asserts that at most 3 % of its rows are
    ambiguous.

Figures (MI355X, both samplers, 21 929 checked rows in all):
  * EPS = 2e-5 was enough and was never widened: with it no unambiguous row mismatched
    and no token fell outside U, so the kernels' top-p boundary was never observed more
    than 2e-5 of mass away from the exact one. The worst logprob error was 2.1e-6.
  * ambiguous rows of the reference alone, 512 rows of `sweep_inputs` per shape:
    V = 128256 bf16: 4; 50257 fp32: 2; 4000 fp32: 1; 1000 bf16: 1 (under 1 %).
  * ambiguous rows in the cases below (the same for v1 and v2, it is a property of the
    reference): 0 in most; 1 of 48 (V = 50257 bf16), 2 of 200 (16387 bf16), 8 of 600 and
    1 of 600 (4000 bf16 / fp32) in the sweep; 1 or 2 of 2048 in the crafted cases. The
    crafted top-k 3 tie is ambiguous by construction (580 of 2048) and has no cap.
  * case (f), step 0, V = 128256: the 24-bit index is all ones first at (seed 70, index
    34171); the first 23-bit-only hit (hsh >> 8 == 0xFFFFFE) is (seed 82, index 46367).
    With the old formula (u rounded to 1.0f, score +inf) v1 returned 34171 from 25 and
    from 12 below the maximum; v2 returned it only from 12 below, because its GMAX
    early-out skips a token more than 17.5 under the thread's best without hashing it.
  * what the sweep found besides: v2 computed the bin of `M - x * (1 / T)` with one fma in
    the histogram kernels and with a rounded product in the draw kernel, so a boundary
    token next to a (sub-)bin edge was counted as kept and then dropped: 7 of 2 412
    sweep rows, all with T != 1, drew the row maximum instead of the reference token.
"""
import functools
import math

import numpy as np
import pytest
import torch

from xgserve import ops
from xgserve.ops import _native
from xgserve.ops import sampling as SP

DEV = "cuda"

# ------------------------------------------------------------------ the CPU reference
M32 = np.uint64(0xFFFFFFFF)
DEFAULT_SEED = 0x9E3779B97F4A7C15
U_BITS = 23              # u = ((hsh >> (32 - U_BITS)) + 0.5) / 2^U_BITS
W = 2 * 40.0 / 2 ** 20   # two sub-bins of the split-row sampler, in y
EPS = 2e-5               # slack on the top-p mass
MARGIN = 1e-3            # two best scores closer than this: ambiguous
MAX_AMBIGUOUS = 0.03


def hash32(x):
    x = np.asarray(x, dtype=np.uint64) & M32
    x = x ^ (x >> np.uint64(16))
    x = (x * np.uint64(0x7FEB352D)) & M32
    x = x ^ (x >> np.uint64(15))
    x = (x * np.uint64(0x846CA68B)) & M32
    return x ^ (x >> np.uint64(16))


def stream_key(seed, step):
    """The per-(seed, step) key; seed may be an array (int64 seeds wrap to uint64)."""
    s = np.asarray(seed).astype(np.int64).astype(np.uint64) if not isinstance(seed, int) else np.uint64(seed % 2 ** 64)
    lo, hi = s & M32, s >> np.uint64(32)
    st = np.uint64(step % 2 ** 32)
    return hash32(lo ^ hash32((hi + np.uint64(0x85EBCA6B)) & M32)
                  ^ hash32((st * np.uint64(0x27D4EB2F) + np.uint64(0x165667B1)) & M32))


def hash_bits(key, V, bits=U_BITS):
    """hsh >> (32 - bits) for indices 0..V-1; key scalar or [S, 1] -> [V] or [S, V]."""
    i = np.arange(V, dtype=np.uint64)
    h = hash32(np.asarray(key, dtype=np.uint64) ^ hash32((i * np.uint64(0x9E3779B9)) & M32))
    return h >> np.uint64(32 - bits)


def gumbel(key, V, bits=None):
    bits = U_BITS if bits is None else bits
    u = (hash_bits(key, V, bits).astype(np.float64) + 0.5) / float(2 ** bits)
    return -np.log(-np.log(u))


def scaled(x, temp):
    """y of the kernels: fp32(x) * fp32(1 / temp) rounded to fp32 (greedy: x), as float64."""
    x = np.asarray(x, dtype=np.float32)
    t = np.float32(temp)
    it = np.float32(1.0) / t if t > 0 else np.float32(1.0)
    return (x * it).astype(np.float64)


def bracket(y, top_p, top_k, eps=None):
    """(L, U, logZ): the certainly-kept and possibly-kept sets of a non-greedy row."""
    eps = EPS if eps is None else eps
    V = y.size
    ys = np.sort(y)[::-1]
    m = ys[0]
    logZ = m + math.log(np.exp(ys - m).sum())
    L = np.ones(V, dtype=bool)
    U = np.ones(V, dtype=bool)
    top_p = float(np.float32(top_p))
    if top_p < 1.0:
        cum = np.cumsum(np.exp(ys - logZ))
        n_lo = min(int(np.searchsorted(cum, top_p - eps, side="left")), V - 1)
        n_hi = min(int(np.searchsorted(cum, top_p + eps, side="left")), V - 1)
        L &= y >= ys[n_lo]
        U &= y >= ys[n_hi] - W
    k = int(top_k)
    if 0 < k < V:
        L &= y > ys[k] + W
        U &= y >= ys[k - 1]
    L |= y == m
    U |= y == m
    return L, U, logZ


class RowRef:
    __slots__ = ("tok", "ambiguous", "logZ", "y", "U")

    def __init__(self, tok, ambiguous, logZ, y, U):
        self.tok, self.ambiguous, self.logZ, self.y, self.U = tok, ambiguous, logZ, y.astype(np.float32), U


def draw(y, L, U, key, bits=None):
    """(expected token, ambiguous) of one row from its bracket and stream key."""
    score = np.where(U, y + gumbel(key, y.size, bits), -np.inf)
    w = int(np.argmax(score))
    best = score[w]
    score[w] = -np.inf
    return w, bool(not L[w] or best - score.max() < MARGIN)


def ref_row(x, temp, top_p=1.0, top_k=0, seed=None, step=0):
    y = scaled(x, temp)
    if not np.float32(temp) > 0:  # greedy: lowest index of the maximum, no noise
        m = y.max()
        logZ = m + math.log(np.exp(y - m).sum())
        return RowRef(int(np.argmax(y)), False, logZ, y, y == m)
    L, U, logZ = bracket(y, top_p, top_k)
    tok, amb = draw(y, L, U, stream_key(DEFAULT_SEED if seed is None else int(seed), step))
    return RowRef(tok, amb, logZ, y, U)


def ref_rows(logits, temps, top_ps, top_ks, seeds, step, rows=None):
    x = logits.detach().float().cpu().numpy()
    rows = range(x.shape[0]) if rows is None else rows
    return {b: ref_row(x[b], float(temps[b]), 1.0 if top_ps is None else float(top_ps[b]),
                       0 if top_ks is None else int(top_ks[b]), None if seeds is None else int(seeds[b]), step)
            for b in rows}


def find_all_ones(bits, V=128256, step=0, max_seed=5000, skip=()):
    """First (seed, index), not in `skip`, whose `bits`-bit uniform index is all ones."""
    for seed in range(max_seed):
        for i in np.nonzero(hash_bits(stream_key(seed, step), V, bits) == np.uint64(2 ** bits - 1))[0]:
            if (seed, int(i)) not in skip:
                return seed, int(i)
    return None


# (seed, index) at step 0, V = 128256: the search below must still find exactly these
OLD_ALL_ONES = (70, 34171)    # 24-bit index: (n + 0.5) / 2^24 rounded to 1.0f before the fix
NEW_ALL_ONES = (82, 46367)   # 23-bit index only (hsh >> 8 == 0xFFFFFE): u = 1 - 2^-24, the largest draw


# ------------------------------------------------------------------ CPU tests of the reference
def test_reference_follows_softmax_and_stays_in_bracket():
    """20 000 seeds on one 50-token row: the reference's draws follow softmax (chi-square,
    p > 1e-4), and with top-p and top-k set every draw lies in U."""
    rng = np.random.default_rng(5)
    x = rng.standard_normal(50).astype(np.float32)
    N, V = 20000, 50
    y = scaled(x, 0.9)
    keys = stream_key(np.arange(N, dtype=np.int64) * 7919, 3)[:, None]
    g = gumbel(keys, V)
    tok = np.argmax(y[None, :] + g, axis=1)
    p = np.exp(y - y.max())
    p /= p.sum()
    cnt = np.bincount(tok, minlength=V)
    assert (N * p).min() > 5  # the chi-square approximation holds
    chi2 = float(((cnt - N * p) ** 2 / (N * p)).sum())
    # chi-square, 49 degrees of freedom: P(X > 94.60) = 1e-4
    assert chi2 < 94.60, chi2
    L, U, _ = bracket(y, 0.8, 12)
    assert L.sum() <= U.sum() <= 12 and L[np.argmax(y)]
    tk = np.argmax(np.where(U[None, :], y[None, :] + g, -np.inf), axis=1)
    assert U[tk].all() and set(tk.tolist()) == set(np.nonzero(U)[0].tolist())
    # the per-row entry point draws the same tokens
    for s in (0, 1, 77):
        assert ref_row(x, 0.9, 1.0, 0, s * 7919, 3).tok == tok[s]
        assert ref_row(x, 0.9, 0.8, 12, s * 7919, 3).tok == tk[s]
    # u never reaches 0 or 1: the noise is bounded on both sides
    gmin, gmax = -math.log(-math.log(2.0 ** -24)), -math.log(-math.log(1 - 2.0 ** -24))
    assert g.min() >= gmin > -2.82 and g.max() <= gmax < 16.64


def test_reference_all_ones_seeds_still_hit():
    """The hard-coded case (f) seeds are what the deterministic search finds."""
    assert find_all_ones(24) == OLD_ALL_ONES
    assert find_all_ones(23) == OLD_ALL_ONES  # 24 ones are 23 ones too: the next one differs
    assert find_all_ones(23, skip=(OLD_ALL_ONES,)) == NEW_ALL_ONES
    # what made the old formula harmful: the sum is a tie in fp32 and rounds to 2^24
    assert np.float32(0xFFFFFF) + np.float32(0.5) == np.float32(16777216.0)
    assert (np.float32(0x7FFFFF) + np.float32(0.5)) * np.float32(1 / 8388608.0) == np.float32(1 - 2.0 ** -24)


# ------------------------------------------------------------------ GPU plumbing
gpu = pytest.mark.gpu


@pytest.fixture(scope="module")
def native():
    _native.kernels()  # fail loudly: the GPU path must run the native library
    assert SP.SAMPLE_SPLIT


def sample_v1(logits, temps, top_ps, top_ks, seeds, step):
    """The one-workgroup-per-row kernel: the raw binding without a workspace."""
    B, V = logits.shape
    tok = torch.empty(B, dtype=torch.int32, device=DEV)
    lp = torch.empty(B, dtype=torch.float32, device=DEV)
    _native.kernels().sample_tokens(logits.data_ptr(), 1 if logits.dtype == torch.float32 else 0, logits.stride(0), B,
                                    V, temps.data_ptr(), _native.ptr(top_ps), _native.ptr(top_ks), _native.ptr(seeds),
                                    step, tok.data_ptr(), lp.data_ptr(), _native.stream_ptr(), 0, 0)
    return tok, lp


def sample_v2(logits, temps, top_ps, top_ks, seeds, step):
    return ops.sample_tokens(logits, temps, top_ps, top_ks, seeds, step)


SAMPLERS = {"v1": sample_v1, "v2": sample_v2}
both = pytest.mark.parametrize("sampler", ["v2", "v1"])


def dev(a, dtype):
    return None if a is None else torch.as_tensor(np.asarray(a), dtype=dtype).to(DEV)


def run(sampler, logits, temps, top_ps, top_ks, seeds, step):
    tok, lp = SAMPLERS[sampler](logits, dev(temps, torch.float32), dev(top_ps, torch.float32),
                                dev(top_ks, torch.int32), dev(seeds, torch.int64), step)
    torch.cuda.synchronize()
    return tok.cpu().numpy(), lp.cpu().numpy()


def check(name, tok, lp, refs, max_ambiguous=MAX_AMBIGUOUS):
    """Exact tokens on unambiguous rows, tokens in U and logprobs on every row, and the
    cap on the ambiguous share. Prints the figures before it asserts."""
    V = next(iter(refs.values())).y.size
    bad_range = [(b, int(tok[b])) for b in refs if not 0 <= tok[b] < V]
    assert not bad_range, f"{name}: token outside [0, V): {bad_range[:5]}"
    amb = [b for b, r in refs.items() if r.ambiguous]
    mism = [(b, int(tok[b]), r.tok) for b, r in refs.items() if not r.ambiguous and tok[b] != r.tok]
    outside = [(b, int(tok[b])) for b, r in refs.items() if not r.U[tok[b]]]
    lp_ref = np.array([float(r.y[tok[b]]) - r.logZ for b, r in refs.items()])
    lp_got = np.array([float(lp[b]) for b in refs])
    lp_err = np.abs(lp_got - lp_ref)
    lp_bad = [(b, float(g), float(e)) for b, g, e in zip(refs, lp_got, lp_ref)
              if not abs(g - e) <= 1e-3 + 1e-3 * abs(e)]
    print(f"[sampling] {name}: rows={len(refs)} ambiguous={len(amb)} mismatches={len(mism)} "
          f"outside_U={len(outside)} max_lp_err={np.nanmax(lp_err) if lp_err.size else 0:.2e} lp_bad={len(lp_bad)}")
    assert not outside, f"{name}: tokens outside the possibly-kept set (row, token): {outside[:5]}"
    assert not mism, f"{name}: {len(mism)} unambiguous mismatches (row, got, expected): {mism[:5]}"
    assert not lp_bad, f"{name}: logprobs off (row, got, expected): {lp_bad[:5]}"
    assert len(amb) <= max_ambiguous * len(refs), f"{name}: {len(amb)} of {len(refs)} rows ambiguous"


def sweep_inputs(V, dtype, B, seed=0):
    """The sweep's inputs: logits randn * 3 and the parameter cycles of the issue."""
    g = torch.Generator().manual_seed(1000003 * seed + V)
    logits = (torch.randn(B, V, generator=g) * 3).to(dtype)
    b = np.arange(B)
    temps = np.array([0.3, 0.7, 1.0, 1.3], dtype=np.float32)[b % 4]
    top_ps = np.array([0.1, 0.5, 0.9, 0.95, 0.999], dtype=np.float32)[b % 5]
    top_ks = np.array([0, 1, 2, 7, 50, 200, 0, V - 1], dtype=np.int32)[b % 8]
    return logits, temps, top_ps, top_ks, b.astype(np.int64) * 7919


@functools.lru_cache(maxsize=2)
def sweep_case(V, dtype, B, padded=False):
    logits, temps, top_ps, top_ks, seeds = sweep_inputs(V, dtype, B)
    refs = ref_rows(logits, temps, top_ps, top_ks, seeds, 11)  # every row: cheap at these V
    if padded:
        buf = torch.full((B, V + 24), 1e30, dtype=dtype)
        buf[:, :V] = logits
        logits = buf
    return logits, temps, top_ps, top_ks, seeds, refs


# ------------------------------------------------------------------ (a) exact tokens, shape sweep
SWEEP = [(V, dt, B) for V in (5, 1000, 2049, 4000, 16387, 50257, 128256) for dt in (torch.bfloat16, torch.float32)
         for B in (1, 9, 48)]
SWEEP += [(16387, dt, 200) for dt in (torch.bfloat16, torch.float32)]
SWEEP += [(4000, dt, 600) for dt in (torch.bfloat16, torch.float32)]


@gpu
@both
@pytest.mark.parametrize("V,dtype,B", SWEEP)
def test_exact_tokens_sweep(native, V, dtype, B, sampler):
    """P = 1, 2, 3, 9, 11, 25, 57, 63 workgroups per row; odd V puts odd rows off 16-B
    alignment (v2's scalar path) and leaves empty trailing chunks."""
    logits, temps, top_ps, top_ks, seeds, refs = sweep_case(V, dtype, B)
    tok, lp = run(sampler, logits.to(DEV), temps, top_ps, top_ks, seeds, 11)
    check(f"sweep {sampler} V={V} {dtype} B={B}", tok, lp, refs)


# ------------------------------------------------------------------ (b) row stride
@gpu
@both
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("V", [16387, 4000])
def test_row_stride(native, V, dtype, sampler):
    """Rows are a [:, :V] view of a [B, V + 24] buffer whose padding holds +1e30."""
    B = 9
    buf, temps, top_ps, top_ks, seeds, refs = sweep_case(V, dtype, B, True)
    view = buf.to(DEV)[:, :V]
    assert view.stride(0) == V + 24
    tok, lp = run(sampler, view, temps, top_ps, top_ks, seeds, 11)
    assert (tok < V).all() and (tok >= 0).all()
    check(f"stride {sampler} V={V} {dtype}", tok, lp, refs)


# ------------------------------------------------------------------ (c) crafted kept sets
CRAFT_V, CRAFT_N = 4000, 2048
# batches of 256 rows run v2 with two workgroups per row: chunks [0, 2000) and [2000, 4000)
CRAFT_IDX = (1999, 2000, 7, 3999)


def crafted_row(probs):
    x = np.full(CRAFT_V, math.log(min(probs)) - 30.0, dtype=np.float32)
    x[list(CRAFT_IDX)] = np.log(np.array(probs, dtype=np.float64)).astype(np.float32)
    return x


@gpu
@both
@pytest.mark.parametrize("what", ["top_p0.65", "top_p0.85", "top_k2", "top_k3_tied"])
def test_crafted_kept_sets(native, what, sampler):
    tied = what == "top_k3_tied"
    x = crafted_row((0.4, 0.3, 0.15, 0.15) if tied else (0.4, 0.3, 0.2, 0.1))
    top_p = float(what[5:]) if what.startswith("top_p") else 1.0
    top_k = int(what[5]) if what.startswith("top_k") else 0
    N = CRAFT_N
    seeds = np.arange(N, dtype=np.int64)
    y = scaled(x, 1.0)
    L, U, logZ = bracket(y, top_p, top_k)
    refs = {}
    for b in range(N):
        t, amb = draw(y, L, U, stream_key(int(seeds[b]), 5))
        refs[b] = RowRef(t, amb, logZ, y, U)
    rows = torch.from_numpy(x).to(DEV)[None, :].expand(256, CRAFT_V).contiguous()
    tok = np.empty(N, dtype=np.int64)
    lp = np.empty(N, dtype=np.float32)
    for s in range(0, N, 256):
        tok[s:s + 256], lp[s:s + 256] = run(sampler, rows, np.ones(256), None if top_p == 1.0 else np.full(256, top_p),
                                            None if top_k == 0 else np.full(256, top_k), seeds[s:s + 256], 5)
    # the tied pair is ambiguous by construction (about 30 % of the rows): no cap there
    check(f"crafted {sampler} {what}", tok, lp, refs, max_ambiguous=1.0 if tied else MAX_AMBIGUOUS)
    got = set(tok.tolist())
    first = list(CRAFT_IDX)
    if tied:
        assert set(first[:2]) <= got <= set(first)
    else:
        assert got == set(first[:{"top_p0.65": 2, "top_p0.85": 3, "top_k2": 2}[what]])
    # frequencies within 4 sigma of the probabilities renormalised over the drawn set
    keep = sorted(got)
    p = np.exp(y[keep] - y[keep].max())
    p /= p.sum()
    freq = np.array([(tok == k).mean() for k in keep])
    sigma = np.sqrt(p * (1 - p) / N)
    print(f"[sampling] crafted {sampler} {what}: set={keep} freq={freq.round(4)} p={p.round(4)}")
    assert (np.abs(freq - p) <= 4 * sigma).all(), (keep, freq, p, sigma)


# ------------------------------------------------------------------ (d) parameter edges
def edge_rows(V):
    """(temp, top_p, top_k) per row: the edges mixed with greedy and plain-temperature rows."""
    return [(1.0, 1.0, V + 5), (0.8, 1.0, 0), (1.0, 1.0, V), (0.7, 1.0, V - 1), (0.0, 0.5, 3), (1.0, 1.0, 0),
            (1.0, 1e-6, 0), (0.01, 1.0, 0), (0.01, 0.9, 50), (-1.0, 0.9, 0), (50.0, 1.0, 0), (50.0, 0.95, 200),
            (1.3, 1.0, 0), (0.0, 1.0, 0), (0.7, 0.9, V - 1), (-0.5, 0.1, V - 1), (50.0, 0.5, V - 1), (0.01, 1e-6, 1)]


@functools.lru_cache(maxsize=1)
def edge_case(dtype, absent):
    V = 16387
    rows = edge_rows(V)
    B = len(rows)
    g = torch.Generator().manual_seed(17)
    logits = (torch.randn(B, V, generator=g) * 3).to(dtype)
    temps = np.array([r[0] for r in rows], dtype=np.float32)
    top_ps = None if absent == "top_ps" else np.array([r[1] for r in rows], dtype=np.float32)
    top_ks = None if absent == "top_ks" else np.array([r[2] for r in rows], dtype=np.int32)
    seeds = None if absent == "seeds" else np.arange(B, dtype=np.int64) * 104729 + 1
    return rows, logits, temps, top_ps, top_ks, seeds, ref_rows(logits, temps, top_ps, top_ks, seeds, 2)


@gpu
@both
@pytest.mark.parametrize("absent", ["none", "top_ps", "top_ks", "seeds"])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_parameter_edges(native, dtype, absent, sampler):
    """top_k >= V, V - 1; top_p 1.0, 1e-6; temp 0.01, 50, 0, < 0; each optional argument
    absent in turn (without seeds every row draws from the default seed's stream)."""
    rows, logits, temps, top_ps, top_ks, seeds, refs = edge_case(dtype, absent)
    tok, lp = run(sampler, logits.to(DEV), temps, top_ps, top_ks, seeds, 2)
    check(f"edges {sampler} {dtype} absent={absent}", tok, lp, refs)
    x = logits.float().numpy()
    for b, (t, p, k) in enumerate(rows):
        greedy = not t > 0
        argmax_only = (top_ps is not None and p == 1e-6) or (top_ks is not None and k == 1)
        if greedy or (argmax_only and not refs[b].ambiguous):
            assert tok[b] == int(np.argmax(x[b])), (b, rows[b])


# ------------------------------------------------------------------ (e) workspace re-arming
@gpu
def test_workspace_rearmed_between_calls(native):
    """Seven split-row calls back to back on one device, no synchronisation between them:
    B, V (so P), and the filters change from call to call; each is exact, and the seventh
    repeats the first call's inputs and tokens. (v2 only: v1 has no workspace.)"""
    g = torch.Generator().manual_seed(23)
    big = (torch.randn(48, 128256, generator=g) * 3).to(torch.bfloat16)
    small = (torch.randn(48, 1000, generator=g) * 3).to(torch.float32)
    calls = [(big, 48, None, 20000), (small, 3, None, None), (big, 48, 0.9, None), (small, 3, None, 50),
             (small, 48, None, None), (big, 3, 0.5, 200)]
    calls.append(calls[0])
    dbig, dsmall = big.to(DEV), small.to(DEV)
    args, outs = [], []
    for i, (lg, B, p, k) in enumerate(calls):
        temps = np.array([0.7, 1.0, 1.3], dtype=np.float32)[np.arange(B) % 3]
        top_ps = None if p is None else np.full(B, p, dtype=np.float32)
        top_ks = None if k is None else np.full(B, k, dtype=np.int32)
        seeds = np.arange(B, dtype=np.int64) * 31 + (0 if i == 6 else i)
        args.append((lg[:B], temps, top_ps, top_ks, seeds))
        d = dbig if lg is big else dsmall
        outs.append(ops.sample_tokens(d[:B], dev(temps, torch.float32), dev(top_ps, torch.float32),
                                      dev(top_ks, torch.int32), dev(seeds, torch.int64), 9))
    torch.cuda.synchronize()
    for i, ((lg, temps, top_ps, top_ks, seeds), (tok, lp)) in enumerate(zip(args[:6], outs)):
        check(f"rearm call {i}", tok.cpu().numpy(), lp.cpu().numpy(), ref_rows(lg, temps, top_ps, top_ks, seeds, 9))
    assert torch.equal(outs[6][0], outs[0][0]) and torch.equal(outs[6][1], outs[0][1])


# ------------------------------------------------------------------ (f) the u = 1.0 draw
@gpu
@both
@pytest.mark.parametrize("top_p", [None, 0.9])
@pytest.mark.parametrize("depth", [25.0, 12.0])
@pytest.mark.parametrize("which", ["old_index", "new_index"])
def test_all_ones_draw_never_wins(native, which, depth, top_p, sampler):
    """Token i, whose uniform index is all ones, sits `depth` below the single maximum and
    the rest 5 below it. Bounded noise (g < 16.64) cannot lift it over the maximum from 25
    below. From 12 below it reaches M + 4.64, under the best of the 128 254 others (the
    reference confirms it for these seeds), and 12 is inside GMAX, so the split-row
    sampler hashes the token instead of skipping it."""
    V = 128256
    seed, i = OLD_ALL_ONES if which == "old_index" else NEW_ALL_ONES
    bits = 24 if which == "old_index" else 23
    assert hash_bits(stream_key(seed, 0), V, bits)[i] == 2 ** bits - 1
    for dtype in (torch.bfloat16, torch.float32):
        x = torch.full((1, V), 5.0)
        x[0, (i + V // 2) % V] = 10.0
        x[0, i] = 10.0 - depth
        x = x.to(dtype)
        refs = ref_rows(x, [1.0], None if top_p is None else [top_p], None, [seed], 0)
        assert refs[0].tok != i and not refs[0].ambiguous
        tok, lp = run(sampler, x.to(DEV), [1.0], None if top_p is None else [top_p], None, [seed], 0)
        assert tok[0] != i, f"{sampler} drew the all-ones token {i} (logprob {lp[0]})"
        check(f"all-ones {sampler} {which} depth={depth} top_p={top_p} {dtype}", tok, lp, refs)


# ------------------------------------------------------------------ (g) -inf logits
def masked_logits(V, dtype, B=8):
    g = torch.Generator().manual_seed(29 + V)
    x = torch.randn(B, V, generator=g) * 3
    mask = torch.zeros(B, V, dtype=torch.bool)
    mask[0::2] = torch.rand(B // 2, V, generator=g) < 0.3   # even rows: a random 30 %
    mask[1::2, :min(2000, V // 2)] = True                   # odd rows: the head of the row
    mask[2::4, :min(2000, V // 2)] = True                   # rows 2, 6: both
    if V % 2:
        mask[:, V - 1] = True
    return x.masked_fill(mask, float("-inf")).to(dtype), mask.numpy()


@functools.lru_cache(maxsize=1)
def masked_case(V, dtype, filtered):
    logits, mask = masked_logits(V, dtype)
    B = logits.shape[0]
    b = np.arange(B)
    temps = np.array([0.7, 1.0, 1.3, 0.0], dtype=np.float32)[b % 4]
    top_ps = np.array([0.9, 1.0, 0.5, 0.95, 1.0], dtype=np.float32)[b % 5] if filtered else None
    top_ks = np.array([0, 50, 0, 7, 200, V - 1], dtype=np.int32)[b % 6] if filtered else None
    seeds = b.astype(np.int64) * 7919 + 5
    return logits, mask, temps, top_ps, top_ks, seeds, ref_rows(logits, temps, top_ps, top_ks, seeds, 4)


@gpu
@both
@pytest.mark.parametrize("filtered", [False, True])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("V", [1000, 16387, 128256])
def test_masked_logits(native, V, dtype, filtered, sampler):
    """-inf entries: every logprob finite, no masked index returned, tokens exact."""
    logits, mask, temps, top_ps, top_ks, seeds, refs = masked_case(V, dtype, filtered)
    tok, lp = run(sampler, logits.to(DEV), temps, top_ps, top_ks, seeds, 4)
    name = f"masked {sampler} V={V} {dtype} filtered={filtered}"
    print(f"[sampling] {name}: finite_lp={int(np.isfinite(lp).sum())}/{lp.size}")
    assert np.isfinite(lp).all(), f"{name}: logprobs {lp}"
    assert not mask[np.arange(len(tok)), np.clip(tok, 0, V - 1)].any(), f"{name}: a masked index was returned: {tok}"
    check(name, tok, lp, refs)


@gpu
@pytest.mark.parametrize("kernel", ["one_workgroup", "split"])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("V", [5, 13, 1000, 16387, 128256])
def test_argmax_logprob_masked(native, V, dtype, kernel):
    """Both greedy kernels on the same rows (and rows shorter than one vector pass, whose
    threads see only the scalar tail) against argmax_logprob_ref."""
    logits, mask = masked_logits(V, dtype)
    d = logits.to(DEV)
    B = d.shape[0]
    tok = torch.empty(B, dtype=torch.int32, device=DEV)
    lp = torch.empty(B, dtype=torch.float32, device=DEV)
    ws = cnt = 0
    if kernel == "split":
        w, c = SP._argmax_ws(d.device, B)
        ws, cnt = w.data_ptr(), c.data_ptr()
    _native.kernels().argmax_logprob(d.data_ptr(), 1 if dtype == torch.float32 else 0, d.stride(0), B, V,
                                     tok.data_ptr(), lp.data_ptr(), _native.stream_ptr(), ws, cnt)
    torch.cuda.synchronize()
    rt, rl = ops.argmax_logprob_ref(logits)
    assert torch.isfinite(lp).all(), lp
    assert torch.equal(tok.cpu(), rt)
    torch.testing.assert_close(lp.cpu(), rl, atol=1e-3, rtol=1e-3)
