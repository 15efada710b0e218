"""float64 references, bounds and shared inputs of the row-kernel tests: the norms,
activations, embedding / pooling kernels and the MoE routing and layout kernels.

tests/test_row_kernels_gpu.py runs the HIP kernels on these inputs, and
tests/test_row_refs_cpu.py runs the package's fp32 CPU paths on the same inputs, so a
bound that a correct fp32 implementation cannot meet shows up without a GPU.

Every reference takes the bf16 / fp32 tensors the kernel saw, upcasts them to float64
and computes the operation in float64 on the CPU. Inputs are drawn on the CPU from
generators seeded by the case, so both modules see the same numbers.
"""
from __future__ import annotations

import math

import torch

# ---------------------------------------------------------------- bounds
# a bf16 output rounded once from an fp32 value: one bf16 ulp, twice the half ulp of a
# round to nearest (as tests/test_paged_kv_gpu.py)
ULP = dict(atol=1e-5, rtol=2.0 ** -7)
# fp32 sums of squares (as tests/test_partials_gpu.py)
SS = dict(rtol=1e-4, atol=1e-2)
# routing weights as an expert -> weight map [T, E]
ROUTE = dict(atol=1e-5, rtol=1e-4)
# mean_l2norm_rows (fp32 in, fp32 out): the sum of squares of H positive terms is a tree of
# depth <= ceil(H / 256) + 6 + 4 <= 27 additions at H = 4097, each within u = 2^-24, so
# the norm is within 13.5 u; the scaling (1 / n, square root, divide, multiply) adds <= 4 u.
# 32 u covers both; zero rows must come out exactly zero (atol 0).
L2N = dict(atol=0.0, rtol=32 * 2.0 ** -24)
# a row's k-th and (k+1)-th float64 router logits closer than this may legitimately be
# chosen differently by an fp32 router; at most ROUTE_TIE_CAP of a case's rows may be
ROUTE_TIE, ROUTE_TIE_CAP = 1e-3, 0.05

GRID_THREADS = 2048 * 256  # silu_and_mul / gelu_tanh: threads of the capped grid

# H -> (threads, VPT) of the norm kernels: every pair, a partly filled last pass, the smallest row
NORM_H = [8, 128, 520, 1536, 2048, 2056, 4096, 4104, 8192, 8200, 16384]
# the reduced cross for fused_add_rmsnorm / layernorm: every VPT, the 192-thread and the smallest row
NORM_H_REDUCED = [8, 1536, 2056, 4104, 8200, 16384]
# (name, scale of x, eps, spike)
NORM_REGIMES = {
    "unit": (1.0, 1e-5, False),
    "small_eps1e-5": (1e-3, 1e-5, False),  # eps is ten times the variance
    "small_eps1e-6": (1e-3, 1e-6, False),  # the same rows, eps equal to the variance
    "spike": (1.0, 1e-5, True),            # one element of 2000 among N(0, 1)
    "shifted": (1.0, 1e-5, False),         # layernorm only: 16 + N(0, 1)
}
RMS_REGIMES = ["unit", "small_eps1e-5", "small_eps1e-6", "spike"]
LN_REGIMES = RMS_REGIMES + ["shifted"]


def gen(*key) -> torch.Generator:
    seed = 0
    for v in key:
        for ch in (str(v) + "|"):
            seed = (seed * 131 + ord(ch)) % (2 ** 31 - 1)
    return torch.Generator().manual_seed(seed)


# ---------------------------------------------------------------- helpers
def bits(t: torch.Tensor) -> torch.Tensor:
    """The raw bits of a tensor (NaN-safe equality with torch.equal)."""
    t = t.detach().cpu().contiguous()
    return t.view({2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def round_bf16(x64: torch.Tensor) -> torch.Tensor:
    """float64 -> bf16 with ONE round to nearest even (a cast through fp32 rounds twice).
    Values in bf16's normal range, or zero."""
    b = x64.contiguous().view(torch.int64)
    drop = 52 - 7
    b = b + ((1 << (drop - 1)) - 1) + ((b >> drop) & 1)
    b = b & ~((1 << drop) - 1)
    return b.view(torch.float64).float().bfloat16()


def used(got: torch.Tensor, want64: torch.Tensor, atol: float, rtol: float) -> float:
    """The largest share of the bound |got - want| <= atol + rtol |want| that is used."""
    if got.numel() == 0:
        return 0.0
    d = (got.detach().cpu().double() - want64).abs()
    lim = atol + rtol * want64.abs()
    return float(torch.where(d == 0, torch.zeros_like(d), d / lim).max())


def check(got: torch.Tensor, want64: torch.Tensor, atol: float, rtol: float, msg: str = "") -> float:
    """assert_close in float64; returns the share of the bound that was used."""
    g = got.detach().cpu().double()
    torch.testing.assert_close(g, want64, atol=atol, rtol=rtol, msg=lambda m: f"{msg}: {m}")
    return used(got, want64, atol, rtol)


# ---------------------------------------------------------------- norms
def norm_inputs(T: int, H: int, regime: str, tag: str = "norm"):
    """x, residual, w, b (bf16) and eps of a norm case. The two `small` regimes share rows."""
    scale, eps, spike = NORM_REGIMES[regime]
    g = gen(tag, T, H, "small" if regime.startswith("small") else regime)
    x = torch.randn(T, H, generator=g)
    res = torch.randn(T, H, generator=g)
    w = 0.5 + torch.rand(H, generator=g)
    b = torch.randn(H, generator=g)
    if regime == "shifted":
        x = x + 16.0
    if spike:
        x[T // 2, H // 3] = 2000.0
    return dict(x=(x * scale).bfloat16(), res=(res * scale).bfloat16(), w=w.bfloat16(), b=b.bfloat16(), eps=eps)


def rmsnorm64(x, w, eps):
    xd = x.double()
    return xd * torch.rsqrt(xd.pow(2).mean(-1, keepdim=True) + eps) * w.double()


def layernorm64(x, w, b, eps):
    xd = x.double()
    mean = xd.mean(-1, keepdim=True)
    var = (xd - mean).pow(2).mean(-1, keepdim=True)
    return (xd - mean) * torch.rsqrt(var + eps) * w.double() + b.double()


def add_bf16(x, res):
    """bf16(float64(x) + float64(res)): the residual fused_add_rmsnorm stores."""
    return round_bf16(x.double() + res.double())


def sumsq64(x):
    return x.double().pow(2).sum(-1)


# ---------------------------------------------------------------- activations
SILU_SHAPES = [(1, 8), (3, 24), (2, 16), (5, 14336), (300, 14336)]
GELU_SHAPES = [(1, 8), (4, 3072), (1400, 3072)]
SILU_PLANTED = [0.0, -0.0, 20.0, -20.0, 88.0, -88.0, 30000.0, -30000.0, 1e-30]


def silu_inputs(T: int, F: int):
    return (torch.randn(T, 2 * F, generator=gen("silu", T, F)) * 4).bfloat16()


def silu_planted_inputs(interleave16: bool):
    """One row, F = 16: the planted gates with u = 1, N(0, 1) * 4 elsewhere."""
    F = 16
    g = (torch.randn(F, generator=gen("silu_planted")) * 4)
    g[:len(SILU_PLANTED)] = torch.tensor(SILU_PLANTED)
    u = torch.ones(F)
    row = torch.stack([g, u]).reshape(1, 2 * F)  # gate | up: with F = 16 also the block-16 interleaved layout
    return row.bfloat16()


def gelu_inputs(T: int, N: int):
    x = torch.randn(T, N, generator=gen("gelu", T, N)) * 4
    x.view(-1)[:2] = torch.tensor([100.0, -100.0])
    return x.bfloat16()


def split_gate_up(x, interleave16: bool):
    F = x.shape[-1] // 2
    if interleave16:
        v = x.reshape(*x.shape[:-1], F // 16, 2, 16)
        return v[..., 0, :].reshape(*x.shape[:-1], F), v[..., 1, :].reshape(*x.shape[:-1], F)
    return x[..., :F], x[..., F:]


def silu_mul64(x, interleave16: bool = False):
    g, u = split_gate_up(x.double(), interleave16)
    return g / (1 + torch.exp(-g)) * u


def gelu64(x):
    v = x.double()
    return 0.5 * v * (1 + torch.tanh(math.sqrt(2 / math.pi) * (v + 0.044715 * v ** 3)))


# ---------------------------------------------------------------- embedding and pooling
EMBED_H = [8, 2040, 2048, 4096]
EMBED_V = 11


def embed_inputs(H: int):
    """The table as a view of a larger allocation with NaN rows on both sides, and ids
    with both ends of the table, one past it, a negative one and INT32_MAX."""
    V, pad = EMBED_V, 2
    buf = torch.full(((V + 2 * pad) * H,), float("nan")).bfloat16()
    buf[pad * H:(pad + V) * H] = torch.randn(V * H, generator=gen("embed", H)).bfloat16()
    ids = torch.tensor([0, V - 1, V, -1, 2 ** 31 - 1, 3, 3, V - 2], dtype=torch.int32)
    return buf, pad, ids


def embed64(table, ids):
    """(rows bf16: the table row or zero, float64 sums of squares)."""
    V = table.shape[0]
    ok = (ids >= 0) & (ids < V)
    rows = table[ids.long().clamp(0, V - 1)].clone()
    rows[~ok] = 0
    return rows, sumsq64(rows)


SEG_H = [8, 2056, 4096]
SEG_LENS = [3, 0, 300, 1, 17]  # an empty and a 300-row segment
SEG_OUT_ROWS = [-1, 4, 0, 6, 2]  # a skipped (non-empty) segment, a permutation, rows 1, 3, 5, 7 not named
SEG_R = 8


def segment_inputs(H: int):
    g = gen("segsum", H)
    cu = torch.tensor([0] + torch.tensor(SEG_LENS).cumsum(0).tolist(), dtype=torch.int32)
    hidden = torch.randn(int(cu[-1]), H, generator=g).bfloat16()
    out0 = torch.randn(SEG_R, H, generator=g)
    return hidden, cu, out0


def segment_sum64(hidden, cu, out0, out_rows=None):
    out = out0.double().clone()
    for s in range(cu.shape[0] - 1):
        r = s if out_rows is None else int(out_rows[s])
        if r >= 0:
            out[r] += hidden[int(cu[s]):int(cu[s + 1])].double().sum(0)
    return out


def segment_sum_atol(hidden, cu, out0) -> float:
    """The absolute bound of segment_sum, next to rtol = 1e-5: the kernel adds the n rows of a
    segment one after the other in fp32 and then adds the sum to out, n + 1 additions, each
    within u = 2^-24 of its result. No partial result exceeds P = max |prefix sum| + max |out0|,
    so the error is at most (n + 1) * u * P (first order). With the 300-row segment of
    N(0, 1) here (P about 60): 1.0e-3 at H = 8, 1.3e-3 at H = 2056, 1.2e-3 at H = 4096."""
    n = int((cu[1:] - cu[:-1]).max())
    p = 0.0
    for s in range(cu.shape[0] - 1):
        seg = hidden[int(cu[s]):int(cu[s + 1])].double()
        if seg.shape[0]:
            p = max(p, float(seg.cumsum(0).abs().max()))
    return (n + 1) * 2.0 ** -24 * (p + float(out0.abs().max()))


L2N_H = [1, 100, 4097]
L2N_ROWS = [5, 0, 2, 7]        # accumulator rows (of 9) named by the call
L2N_COUNTS = [0, 1, 1000, 3]   # 0 is treated like 1; row 7 is all zero


def l2norm_inputs(H: int):
    g = gen("l2n", H)
    acc = torch.randn(9, H, generator=g) * torch.tensor([1., 3., 700., 1., 1., 2., 1., 1., 1.])[:, None]
    acc[7] = 0
    return acc, torch.tensor(L2N_ROWS, dtype=torch.int32), torch.tensor(L2N_COUNTS, dtype=torch.int32)


def mean_l2norm64(acc, rows, counts):
    v = acc.double()[rows.long()] / counts.clamp_min(1).double()[:, None]
    return v / v.norm(dim=-1, keepdim=True).clamp_min(1e-12)


# ---------------------------------------------------------------- MoE routing
TOPK_EK = [(2, 1), (2, 2), (8, 2), (16, 4), (60, 6), (64, 8), (64, 16), (16, 16)]
TOPK_T = [1, 129, 300]  # 128 threads per block
# moe_route: the shapes of test_moe_route_matches_fp32, and E <= 8 with H > 16384
# (the one-round-trip router does not take it: route_kernel)
ROUTE_CASES = [(1, 8, 2, 4096), (64, 8, 2, 4096), (5, 16, 4, 512), (3, 64, 6, 1024), (2, 4, 1, 8192),
               (7, 8, 2, 14336), (1, 6, 2, 1000), (3, 8, 2, 16392)]
ROUTE_NORM_CASES = [(1, 8, 2, 4096), (33, 8, 2, 4096), (2, 4, 1, 8192), (3, 8, 2, 14336), (3, 8, 2, 16392)]


def topk_logits(T: int, E: int):
    """Tie-free rows: a random permutation per row of E distinct multiples of 1/8
    (exact in bf16 and fp32)."""
    vals = (torch.arange(E, dtype=torch.float32) - E // 2) * 0.125
    perm = torch.rand(T, E, generator=gen("topk", T, E)).argsort(-1)
    return vals[perm]


def dense(w, ids, E: int):
    """[T, k] weights and expert ids -> [T, E] float64 weights; the ids of a row must be
    distinct and in range."""
    ids = ids.detach().cpu().long()
    assert bool(((ids >= 0) & (ids < E)).all()), "expert id out of range"
    T, k = ids.shape
    mask = torch.zeros(T, E, dtype=torch.bool).scatter_(1, ids, torch.ones(T, k, dtype=torch.bool))
    assert bool((mask.sum(-1) == k).all()), "an expert chosen twice in a row"
    return torch.zeros(T, E, dtype=torch.float64).scatter_(1, ids, w.detach().cpu().double())


def topk_softmax64(logits, k: int, renorm: bool, ids=None):
    """float64 softmax + top-k as [T, E] weights (zero where not chosen). With `ids` the
    choice is given and only the weights are computed."""
    p = torch.softmax(logits.double(), -1)
    if ids is None:
        ids = p.topk(k, dim=-1).indices
    mask = torch.zeros_like(p, dtype=torch.bool).scatter_(1, ids.cpu().long(), True)
    w = p * mask
    return w / w.sum(-1, keepdim=True) if renorm else w


def near_tie_rows(logits64, k: int):
    """Rows whose k-th and (k+1)-th logits are closer than ROUTE_TIE."""
    if k >= logits64.shape[-1]:
        return torch.zeros(logits64.shape[0], dtype=torch.bool)
    s = logits64.sort(-1, descending=True).values
    return (s[:, k - 1] - s[:, k]) < ROUTE_TIE


def route_inputs(T: int, E: int, k: int, H: int, scale: float = 1.0, tag: str = "route"):
    g = gen(tag, T, E, k, H)
    h = (torch.randn(T, H, generator=g) * scale).bfloat16()
    router = (torch.randn(E, H, generator=g) * 0.05).bfloat16()
    norm_w = (1 + 0.1 * torch.randn(H, generator=g)).bfloat16()
    return h, router, norm_w


def check_route(w, ids, logits64, k: int, renorm: bool, msg: str = "") -> float:
    """Routing of an fp32 router against float64 logits: the chosen experts equal the
    reference's on every row that is not a near tie (at most ROUTE_TIE_CAP of the rows
    are), and each weight belongs to its expert: [T, E] against the reference's, on
    near-tie rows against the float64 weights of the experts the kernel chose."""
    T, E = logits64.shape
    got = dense(w, ids, E)
    want = topk_softmax64(logits64, k, renorm)
    tie = near_tie_rows(logits64, k)
    assert int(tie.sum()) <= ROUTE_TIE_CAP * T, f"{msg}: {int(tie.sum())} of {T} rows are near ties"
    assert torch.equal((got != 0)[~tie], (want != 0)[~tie]), f"{msg}: chosen experts differ"
    want = torch.where(tie[:, None], topk_softmax64(logits64, k, renorm, ids=ids), want)
    return check(got, want, **ROUTE, msg=msg)


# ---------------------------------------------------------------- MoE layout
BLOCK_M = 64


def align_cap(n_pairs: int, E: int, block_m: int) -> int:
    return (n_pairs + E * (block_m - 1) + block_m - 1) // block_m * block_m


def align_cases():
    """name -> (ids [T, k] int32 global expert ids, E_local, expert_offset)."""
    def rand(T, k, E, lo=0, hi=None, tag=""):
        return torch.randint(lo, E if hi is None else hi, (T, k), generator=gen("align", T, k, E, tag),
                             dtype=torch.int32)
    c = {}
    c["1x1_E1"] = (torch.zeros(1, 1, dtype=torch.int32), 1, 0)
    c["3x2_E4"] = (rand(3, 2, 4), 4, 0)
    c["64x2_E8"] = (rand(64, 2, 8), 8, 0)
    c["575x2_E8"] = (rand(575, 2, 8), 8, 0)            # 1150 pairs: past the 1024 threads
    c["625x8_E64"] = (rand(625, 8, 64), 64, 0)
    c["100x6_E256"] = (rand(100, 6, 256), 256, 0)
    c["shard_4of8"] = (rand(300, 2, 8), 4, 4)          # half the pairs are another rank's
    c["shard_low"] = (rand(40, 2, 8), 4, 0)
    neg = rand(50, 2, 8, tag="neg")
    neg[::7, 0] = -1                                   # negative ids are foreign too
    neg[3, 1] = -5
    c["negative_ids"] = (neg, 8, 0)
    c["neg_shard"] = (neg.clone(), 4, 4)
    c["one_expert"] = (torch.full((650, 2), 5, dtype=torch.int32), 8, 0)
    ex = torch.full((96, 2), 2, dtype=torch.int32)     # expert 1: exactly 64 pairs, 2: 128, 0 and 3: none
    ex[:64, 0] = 1
    c["exact_block"] = (ex, 4, 0)
    c["exact_block_1150"] = (torch.cat([ex, torch.full((479, 2), 3, dtype=torch.int32)]), 6, 0)
    return c


def align_ref(ids, E: int, expert_offset: int, block_m: int):
    """A plain implementation of moe_align's contract (pairs placed in order)."""
    flat = ids.reshape(-1).tolist()
    k = ids.shape[1]
    loc = [e - expert_offset if 0 <= e - expert_offset < E else -1 for e in flat]
    cnt = [sum(1 for e in loc if e == j) for j in range(E)]
    offs = [0]
    for j in range(E):
        offs.append(offs[-1] + -(-cnt[j] // block_m) * block_m)
    rows = [-1] * align_cap(len(flat), E, block_m)
    dest, fill = [], [0] * E
    for i, e in enumerate(loc):
        if e < 0:
            dest.append(-1)
            continue
        dest.append(offs[e] + fill[e])
        rows[dest[-1]] = i // k
        fill[e] += 1
    return (torch.tensor(rows, dtype=torch.int32), torch.tensor(offs, dtype=torch.int32),
            torch.tensor(dest, dtype=torch.int32))


def check_align(ids, E: int, expert_offset: int, block_m: int, sorted_rows, offsets, dest):
    """The documented contract of moe_align; the slot order inside an expert is free."""
    ids, sorted_rows, offsets, dest = (t.detach().cpu().long() for t in (ids, sorted_rows, offsets, dest))
    T, k = ids.shape
    n = T * k
    assert sorted_rows.shape == (align_cap(n, E, block_m),) and offsets.shape == (E + 1,) and dest.shape == (n,)
    loc = ids.reshape(-1) - expert_offset
    local = (loc >= 0) & (loc < E)
    cnt = torch.bincount(loc[local], minlength=E)
    assert int(offsets[0]) == 0
    assert torch.equal(offsets[1:] - offsets[:-1], (cnt + block_m - 1) // block_m * block_m)
    assert bool((dest[~local] == -1).all()), "a foreign pair was placed"
    pairs = torch.arange(n)[local]
    d = dest[local]
    lo = offsets[loc[local]]
    assert bool(((d >= lo) & (d < lo + cnt[loc[local]])).all()), "dest outside its expert's rows"
    assert d.unique().numel() == d.numel(), "two pairs share a row"
    assert torch.equal(sorted_rows[d], pairs // k), "sorted_rows[dest[i]] != i // k"
    rest = torch.ones_like(sorted_rows, dtype=torch.bool)
    rest[d] = False
    assert bool((sorted_rows[rest] == -1).all()), "padding is not -1"


# ---------------------------------------------------------------- the cases
# Each run_* draws a case, runs xgserve.ops on `dev` ("cuda": the HIP kernels, "cpu": the
# package's fp32 paths) into poisoned buffers, checks the result against float64 and
# returns the share of each bound that was used (for the record; the checks assert).
NAN = float("nan")


def _nan(*shape, dtype=torch.bfloat16):
    return torch.full(shape, NAN, dtype=dtype)


def run_rmsnorm(dev, T, H, regime):
    from xgserve import ops
    c = norm_inputs(T, H, regime)
    buf = _nan(T + 2, H).to(dev)
    y = ops.rmsnorm(c["x"].to(dev), c["w"].to(dev), c["eps"], out=buf[:T])
    assert y.shape == (T, H)
    assert torch.equal(bits(buf[T:]), bits(_nan(2, H))), "rows past T were written"
    return {"ULP": check(buf[:T], rmsnorm64(c["x"], c["w"], c["eps"]), **ULP, msg=f"rmsnorm {T}x{H} {regime}")}


def run_rmsnorm_strided(dev, T, H, regime):
    """x and out are views of wider buffers (row stride H + 24); the gaps stay as they were."""
    from xgserve import ops
    c = norm_inputs(T, H, regime, tag="strided")
    xb, ob = _nan(T, H + 24), _nan(T, H + 24)
    xb[:, 8:8 + H] = c["x"]
    xb, ob = xb.to(dev), ob.to(dev)
    y = ops.rmsnorm(xb[:, 8:8 + H], c["w"].to(dev), c["eps"], out=ob[:, 16:16 + H])
    assert torch.equal(bits(ob[:, :16]), bits(_nan(T, 16))) and torch.equal(bits(ob[:, 16 + H:]), bits(_nan(T, 8)))
    return {"ULP": check(y, rmsnorm64(c["x"], c["w"], c["eps"]), **ULP, msg=f"strided rmsnorm {T}x{H} {regime}")}


def run_fused_add_rmsnorm(dev, T, H, regime):
    from xgserve import ops
    c = norm_inputs(T, H, regime)
    rbuf = _nan(T + 1, H)
    rbuf[:T] = c["res"]
    rbuf, ybuf = rbuf.to(dev), _nan(T + 1, H).to(dev)
    y, r = ops.fused_add_rmsnorm(c["x"].to(dev), rbuf[:T], c["w"].to(dev), c["eps"], out=ybuf[:T])
    assert r.data_ptr() == rbuf.data_ptr()
    assert torch.equal(bits(rbuf[:T]), bits(add_bf16(c["x"], c["res"]))), "residual != bf16(x + residual)"
    assert torch.equal(bits(rbuf[T:]), bits(_nan(1, H))) and torch.equal(bits(ybuf[T:]), bits(_nan(1, H)))
    # the kernel normalises the residual it stored
    want = rmsnorm64(rbuf[:T].cpu(), c["w"], c["eps"])
    return {"ULP": check(ybuf[:T], want, **ULP, msg=f"fused_add_rmsnorm {T}x{H} {regime}")}


def run_layernorm(dev, T, H, regime):
    from xgserve import ops
    c = norm_inputs(T, H, regime)
    y = ops.layernorm(c["x"].to(dev), c["w"].to(dev), c["b"].to(dev), c["eps"])
    return {"ULP": check(y, layernorm64(c["x"], c["w"], c["b"], c["eps"]), **ULP, msg=f"layernorm {T}x{H} {regime}")}


def partials_inputs(T=3, H=4096, S=3, scale=1e-3):
    g = gen("partials", T, H, S)
    part = torch.randn(S, T, H, generator=g) * scale
    res = (torch.randn(T, H, generator=g) * scale).bfloat16()
    w = (0.5 + torch.rand(H, generator=g)).bfloat16()
    return part, res, w


def check_add_partials_rmsnorm(part, res0, w, eps, res, y):
    """res = bf16(res0 + sum_s part[s]) (one rounding of an fp32 sum), y = RMSNorm of the stored res."""
    u = check(res, res0.double() + part.double().sum(0), **ULP, msg="add_partials_rmsnorm residual")
    return {"ULP": max(u, check(y, rmsnorm64(res.cpu(), w, eps), **ULP, msg=f"add_partials_rmsnorm eps={eps}"))}


def run_row_sumsq(dev, T, H):
    from xgserve import ops
    x = torch.randn(T, H, generator=gen("sumsq", T, H)).bfloat16()
    out = torch.full((T + 3,), -7.0).to(dev)
    ops.row_sumsq(x.to(dev), out)
    assert torch.equal(out[T:].cpu(), torch.full((3,), -7.0))
    return {"SS": check(out[:T], sumsq64(x), **SS, msg=f"row_sumsq {T}x{H}")}


def run_silu(dev, x, interleave16, msg):
    from xgserve import ops
    T, F = x.shape[0], x.shape[1] // 2
    buf = _nan(T + 2, F).to(dev)
    y = ops.silu_and_mul(x.to(dev), out=buf[:T], interleave16=interleave16)
    assert y.data_ptr() == buf.data_ptr()
    assert torch.equal(bits(buf[T:]), bits(_nan(2, F))), "rows past T were written"
    assert bool(torch.isfinite(buf[:T]).all())
    return {"ULP": check(buf[:T], silu_mul64(x, interleave16), **ULP, msg=msg)}


def run_gelu(dev, x):
    from xgserve import ops
    y = ops.gelu_tanh(x.to(dev))
    assert y.shape == x.shape and bool(torch.isfinite(y).all())
    return {"ULP": check(y, gelu64(x), **ULP, msg=f"gelu_tanh {tuple(x.shape)}")}


def run_embed_gather(dev, H):
    from xgserve import ops
    buf, pad, ids = embed_inputs(H)
    T = ids.shape[0]
    dbuf = buf.to(dev)
    table = dbuf[pad * H:(pad + EMBED_V) * H].view(EMBED_V, H)
    ss = torch.full((T + 2,), -7.0).to(dev)
    out = ops.embed_gather(ids.to(dev), table, ss)
    rows, ss64 = embed64(table.cpu(), ids)
    assert torch.equal(bits(out), bits(rows)), "gathered rows differ from the table"
    assert torch.equal(ss[T:].cpu(), torch.full((2,), -7.0))
    bad = (ids < 0) | (ids >= EMBED_V)
    assert bool((ss[:T].cpu()[bad] == 0).all())
    out2 = ops.embed_gather(ids.to(dev), table)  # without the statistic
    assert torch.equal(bits(out2), bits(rows))
    return {"SS": check(ss[:T], ss64, **SS, msg=f"embed_gather ss H={H}")}


def run_segment_sum(dev, H, with_rows):
    from xgserve import ops
    hidden, cu, out0 = segment_inputs(H)
    rows = torch.tensor(SEG_OUT_ROWS, dtype=torch.int32) if with_rows else None
    out = out0.clone().to(dev)
    ops.segment_sum(hidden.to(dev), cu.to(dev), out, rows if rows is None else rows.to(dev))
    named = [r for r in SEG_OUT_ROWS if r >= 0] if with_rows else list(range(len(SEG_LENS)))
    rest = [r for r in range(SEG_R) if r not in named]
    assert torch.equal(bits(out[rest]), bits(out0[rest])), "a row that no segment names was written"
    if not with_rows:
        assert torch.equal(bits(out[1]), bits(out0[1])), "the empty segment changed its row"
    atol = segment_sum_atol(hidden, cu, out0)
    return {"SEG": check(out, segment_sum64(hidden, cu, out0, rows), atol=atol, rtol=1e-5,
                         msg=f"segment_sum H={H} rows={with_rows} atol={atol:.2e}")}


def run_mean_l2norm(dev, H):
    from xgserve import ops
    acc0, rows, counts = l2norm_inputs(H)
    acc = acc0.clone().to(dev)
    out = ops.mean_l2norm_rows(acc, rows.to(dev), counts.to(dev))
    assert out.shape == (len(L2N_ROWS), H) and bool(torch.isfinite(out).all())
    assert bool((out[L2N_ROWS.index(7)] == 0).all()), "an all-zero row must give an all-zero output"
    assert bool((acc[rows.long().to(dev)] == 0).all()), "the named accumulator rows are re-zeroed"
    rest = [r for r in range(acc0.shape[0]) if r not in L2N_ROWS]
    assert torch.equal(bits(acc[rest]), bits(acc0[rest])), "another accumulator row was written"
    return {"L2N": check(out, mean_l2norm64(acc0, rows, counts), **L2N, msg=f"mean_l2norm_rows H={H}")}


def run_topk_softmax(dev, T, E, k):
    """fp32 and bf16 logits, renorm on and off; tie-free rows, so the choice is exact."""
    from xgserve import ops
    worst = 0.0
    base = topk_logits(T, E)
    for dtype in (torch.float32, torch.bfloat16):
        logits = base.to(dtype)
        assert torch.equal(logits.float(), base)
        for renorm in (True, False):
            msg = f"moe_topk_softmax T={T} E={E} k={k} {dtype} renorm={renorm}"
            w, ids = ops.moe_topk_softmax(logits.to(dev), k, renorm)
            assert w.shape == (T, k) and ids.shape == (T, k) and ids.dtype == torch.int32
            got, want = dense(w, ids, E), topk_softmax64(logits, k, renorm)
            assert torch.equal(got != 0, want != 0), f"{msg}: chosen experts differ"
            worst = max(worst, check(got, want, **ROUTE, msg=msg))
    return {"ROUTE": worst}


def run_topk_softmax_ties(dev, E, k):
    """All-equal logits: distinct experts in range, every weight 1/k (renorm) or 1/E; no rule for the winners."""
    from xgserve import ops
    worst = 0.0
    for dtype in (torch.float32, torch.bfloat16):
        logits = torch.tensor([0.0, 1.5, -3.0])[:, None].expand(3, E).contiguous().to(dtype)
        for renorm in (True, False):
            w, ids = ops.moe_topk_softmax(logits.to(dev), k, renorm)
            got = dense(w, ids, E)  # asserts distinct and in range
            want = (got != 0).double() * (1.0 / k if renorm else 1.0 / E)
            worst = max(worst, check(got, want, **ROUTE, msg=f"tied logits E={E} k={k} {dtype} renorm={renorm}"))
    return {"ROUTE": worst}


def run_moe_route(dev, T, E, k, H):
    from xgserve import ops
    h, router, _ = route_inputs(T, E, k, H)
    logits64 = h.double() @ router.double().t()
    worst = 0.0
    for renorm in (True, False):
        w, ids = ops.moe_route(h.to(dev), router.to(dev), k, renorm)
        worst = max(worst, check_route(w, ids, logits64, k, renorm, msg=f"moe_route {(T, E, k, H)} renorm={renorm}"))
    return {"ROUTE": worst}


def run_moe_route_norm(dev, T, E, k, H, scale=1.0, eps=1e-5):
    from xgserve import ops
    h, router, norm_w = route_inputs(T, E, k, H, scale=scale, tag="route_norm")
    out = {"ROUTE": 0.0, "ULP": 0.0}
    for renorm in (True, False):
        msg = f"moe_route_norm {(T, E, k, H)} scale={scale} eps={eps} renorm={renorm}"
        hn, w, ids = ops.moe_route_norm(h.to(dev), norm_w.to(dev), eps, router.to(dev), k, renorm)
        out["ULP"] = max(out["ULP"], check(hn, rmsnorm64(h, norm_w, eps), **ULP, msg=msg))
        # the kernel routes on the bf16 rows it wrote
        logits64 = hn.cpu().double() @ router.double().t()
        out["ROUTE"] = max(out["ROUTE"], check_route(w, ids, logits64, k, renorm, msg=msg))
    return out
