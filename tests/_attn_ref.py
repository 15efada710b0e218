"""Inputs, float64 references and checks of the attention tests that can see ONE wrong key:
ops.prefill_attention (both kernels), ops.decode_attention and ops.decode_attention_fused.

tests/test_attn_exact_gpu.py runs the HIP kernels through the run_* functions below and
tests/test_attn_refs_cpu.py runs the package's fp32 CPU paths through the same functions,
plants wrong answers and checks that every check refuses them.

  1. staircase: K[j] = (j // 128, j % 128, random ...), q = +-512 * (128, 1, 0, ...): the raw
     score of key j is exactly +-512 j, neighbouring keys are 45 (D = 128) or 64 (D = 64)
     nats apart, so the answer is ONE V row: V[lim] (the diagonal key) for sign +, V[0] for
     sign -. Compared with ULP: the exponent's -m * scale_log2 term is rounded at
     magnitudes up to 1e5, which can move the normaliser by about 1e-3, less than one bf16
     step but not always zero steps.
  2. counted keys: q = 0, V integers in -2..2: every weight is exactly 1, the fp32
     accumulator holds the exact integer O = sum V[0..lim], the answer is O / n.
     out * n is compared with O under ULP on max(|O|, 1).
  3. the fused decode's own row: q = 200 k_new / (|k_new|^2 scale), so the key that the
     launch's own prologue appends has score 200 and the answer is the new V row.
  4. random inputs against float64 with bounds that scale with the row:
     |out - ref| <= 2^-6 B + 1e-6 with B = sum_j p_j |v_j| (the kernels round P to bf16,
     2^-8, round the output once, 2^-8, normalise by a sum of unrounded P, 2^-8, and a
     fourth 2^-8 covers the fp32 scores and exp2), and rms(out - ref) / rms(ref) over the
     D coordinates of a row <= RMS_LIMIT = 3 RMS_EMU, where RMS_EMU is the largest value
     of a float64 emulation of the kernels' arithmetic (emulate=True in attend64) over
     the committed seeds and shapes. Rounding errors of independent P entries add in
     quadrature and the kernels' order of summation differs: hence the factor 3.

A decode row is a sequence with one query row and ctx = L - 1 (ctx = -1: an empty row, no
key visible, answer exactly 0), so one Case and one set of checks serve all three ops.
Caches are paged with a shuffled block table; K rows past a sequence's end continue the
sequence's construction with every second row NaN, V rows past it hold +Inf; pages that
no sequence names hold NaN / +Inf too. Q is a strided view into a wider QKV row whose
other columns are NaN, and `out` is a row slice of a larger buffer filled with SENT.
"""
from __future__ import annotations

import functools
import math

import torch

from _row_ref import ULP, bits, gen, round_bf16

NAN, INF = float("nan"), float("inf")
SENT = -7.0  # exact in bf16
# section 4's rms limit: tests/test_attn_refs_cpu.py re-derives RMS_EMU and fails if it drifts
RMS_EMU = 0.0034457523564279213  # 0.882 * 2^-8
RMS_LIMIT = 3 * RMS_EMU
EB = dict(atol=1e-6, rtol=2.0 ** -6)  # section 4's elementwise bound, rtol on B
# section 3: the appended key's score leads every other key's by at least this many nats
# (computed in float64 from the bf16 q and keys the kernel attends with). 1100 keys at
# e^-40 each are 5e-15 of the row sum, far below fp32 resolution (6e-8).
FUSED_GAP_MIN = 40.0

# ---------------------------------------------------------------- shapes and configurations
# 30 and 62 (ctx % 32 == 30): a 32-row block of prefill_attn2_kernel whose smallest causal limit
# is the last key but one of a 64-key tile, the edge of its need_mask test
PF_CTX = [0, 1, 30, 31, 32, 33, 62, 63, 64, 65, 127, 128, 129, 191]
PF_QLEN = [1, 31, 32, 33, 63, 64, 65, 129]
PF_LONG = [(5, 1000), (64, 960)]  # (qlen, ctx)


def prefill_shapes(long_only=False):
    """(qlens, ctxs) of one varlen launch: the ctx x qlen cross with two empty sequences in
    the middle of the batch, then the two long-context sequences."""
    if long_only:
        pairs = [PF_LONG[0], (0, 17)] + PF_LONG[1:]
    else:
        pairs = [(ql, c) for c in PF_CTX for ql in PF_QLEN]
        half = len(pairs) // 2
        pairs = pairs[:half] + [(0, 0), (0, 17)] + pairs[half:] + PF_LONG
    return tuple(p[0] for p in pairs), tuple(p[1] for p in pairs)


# 24 short sequences: with Hq = 8 the launcher's own choice (gh = 0) is KS = 2 here and KS = 1 on
# the full cross: num_seqs * ceil(max_q_len / 128) * Hq / 2 = 24 * 2 * 4 = 192 < 512 <= 116 * 2 * 4
PF_KS2 = ((1, 33, 64, 129, 0, 65, 32, 5) * 3, tuple([0, 63, 64, 1, 17, 129, 191, 1000] + PF_CTX[:8] + PF_CTX[6:]))

# (Hq, Hkv, D, gh): every prefill_attn2_kernel case of the launcher's switch, its own choice, and
# the 16-row kernel
PF2_CFGS = [(8, 2, 128, g) for g in (-84, -82, -81, -44, -42, -41, -1284, -1282, -1281)] + [(8, 1, 128, -88)]
PF16_CFGS = [(8, 2, 128, 1), (8, 2, 128, 2), (8, 2, 128, 4), (8, 2, 64, 0), (8, 2, 64, 1), (8, 2, 64, 2)]
PF_BS = [16, 48]

DG = [(128, 1), (128, 2), (128, 4), (128, 8), (128, 16), (64, 1), (64, 2), (64, 4), (64, 8)]
DEC_LENS = [1, 15, 16, 17, 127, 128, 129, 333, 1100, 0]
DEC_SPLITS = [1, 5, 17, 64]
DEC_LENS_LONG = [333, 1100, 0]  # section 2, the (D, G) pairs between the first and the last

# section 4: the suite's random construction, ctx % 64 in {0, 1, 63} and the long sequences
RAND_QLENS = (64, 1, 130, 7, 33, 65, 2, 5, 64)
RAND_CTXS = (0, 5, 40, 300, 64, 129, 191, 1000, 960)
RAND_PF = [(8, 2, 128, -82, 16), (8, 2, 128, -1282, 48), (8, 2, 128, 2, 48), (8, 2, 64, 0, 16)]  # .., gh, bs
RAND_DEC = [(128, 4, 16), (64, 1, 48)]  # D, G, bs; splits 1 and 5
RAND_FUSED = (4, 3, 2, 16, 3, True)  # G, S, depth, bs, splits, rope

# section 3: half of G x S x depth (18 cases); the page size moves with G and the depth, the
# split count with S and the depth, RoPE with G and S
_GS, _SS, _DEPTHS = [1, 2, 4, 8], [2, 5, 9], [2, 3, 4]
FUSED_CASES = [(G, S, dp, (16, 48)[(ig + idp) % 2], (1, 3, 17)[(i_s + idp) % 3], (ig + i_s) % 2 == 0)
               for ig, G in enumerate(_GS) for i_s, S in enumerate(_SS) for idp, dp in enumerate(_DEPTHS)
               if (ig + i_s + idp) % 2 == 0]


def fused_lens(bs):
    return (1, bs, bs + 1, 0, 2 * bs + 5, 300, 1100)


# ---------------------------------------------------------------- a case
def _pages(L, bs):
    return (max(1, L) + bs - 1) // bs  # an empty row still owns one page


class Case:
    """One launch. q [T, Hq, D] bf16 packed; ks / vs: per sequence [pages * bs, Hkv, D] bf16
    (rows past L poisoned); a sequence's queries sit at positions ctx .. ctx + qlen - 1."""

    def __init__(self, q, ks, vs, qlens, ctxs, bs, scale, tag):
        self.q, self.ks, self.vs, self.qlens, self.ctxs, self.bs, self.scale, self.tag = q, ks, vs, qlens, ctxs, bs, scale, tag
        self.T, self.Hq, self.D = q.shape
        self.Hkv = ks[0].shape[1]
        self.G = self.Hq // self.Hkv
        self.lens = [a + c for a, c in zip(qlens, ctxs)]
        self.start = [0]
        for n in qlens:
            self.start.append(self.start[-1] + n)
        lim = [c + i for n, c in zip(qlens, ctxs) for i in range(n)]
        self.lim = torch.tensor(lim, dtype=torch.long)         # [T] causal limit of every row
        self.seq = torch.tensor([s for s, n in enumerate(qlens) for _ in range(n)], dtype=torch.long)
        self.want = None   # sections 1 and 3: [T, Hq, D] bf16
        self.O = None      # section 2: [T, Hq, D] float64 integer sums
        self.ref = self.B = None  # section 4: float64

    def seqs(self):
        for s, n in enumerate(self.qlens):
            yield s, self.start[s], self.start[s + 1], self.ctxs[s], self.lens[s]

    def where(self, t, h, note=""):
        s = int(self.seq[t])
        return (f"{self.tag}{note}: row {t} (sequence {s}: qlen {self.qlens[s]}, ctx {self.ctxs[s]}, "
                f"row {t - self.start[s]} of it, causal limit {int(self.lim[t])}), head {h}")


def _poison(k, v, L):
    k[L::2] = NAN
    v[L:] = INF


def _kv_head(x, G):
    """[n, Hkv, D] -> [n, Hq, D]."""
    return x.repeat_interleave(G, dim=1)


def _signs(T, Hq, Hkv):
    """+1 / -1 per (row, head): by head, or by row when every query head has its own kv head."""
    if Hq == Hkv:
        s = 1 - 2 * (torch.arange(T) % 2)
        return s[:, None].expand(T, Hq).clone()
    s = 1 - 2 * (torch.arange(Hq) % 2)
    return s[None, :].expand(T, Hq).clone()


@functools.lru_cache(maxsize=None)
def stair_case(qlens, ctxs, Hq, Hkv, D, bs, tag="stair"):
    g = gen(tag, Hq, Hkv, D, bs, len(qlens), sum(ctxs))
    T = sum(qlens)
    sign = _signs(T, Hq, Hkv)
    q = torch.zeros(T, Hq, D)
    q[..., 0] = sign * (512.0 * 128.0)
    q[..., 1] = sign * 512.0
    ks, vs = [], []
    for ql, ctx in zip(qlens, ctxs):
        cap = _pages(ql + ctx, bs) * bs
        k = torch.randn(cap, Hkv, D, generator=g)
        j = torch.arange(cap, dtype=torch.float32)
        k[:, :, 0] = (j // 128)[:, None]
        k[:, :, 1] = (j % 128)[:, None]
        v = torch.randn(cap, Hkv, D, generator=g)
        k, v = k.bfloat16(), v.bfloat16()
        _poison(k, v, ql + ctx)
        ks.append(k)
        vs.append(v)
    c = Case(q.bfloat16(), ks, vs, qlens, ctxs, bs, 1.0 / math.sqrt(D), f"staircase {tag} Hq={Hq} Hkv={Hkv} D={D} bs={bs}")
    want = torch.zeros(T, Hq, D, dtype=torch.bfloat16)
    for s, a, b, ctx, L in c.seqs():
        if b == a or L == 0:
            continue
        lim = c.lim[a:b]
        up = _kv_head(vs[s][lim], c.G)                       # the diagonal key
        down = _kv_head(vs[s][torch.zeros_like(lim)], c.G)   # key 0
        want[a:b] = torch.where((sign[a:b] > 0)[..., None], up, down)
    c.want, c.sign = want, sign
    return c


@functools.lru_cache(maxsize=None)
def count_case(qlens, ctxs, Hq, Hkv, D, bs, tag="count"):
    g = gen(tag, Hq, Hkv, D, bs, len(qlens), sum(ctxs))
    T = sum(qlens)
    ks, vs = [], []
    for ql, ctx in zip(qlens, ctxs):
        cap = _pages(ql + ctx, bs) * bs
        k = torch.randn(cap, Hkv, D, generator=g).bfloat16()
        v = torch.randint(-2, 3, (cap, Hkv, D), generator=g).bfloat16()
        _poison(k, v, ql + ctx)
        ks.append(k)
        vs.append(v)
    c = Case(torch.zeros(T, Hq, D, dtype=torch.bfloat16), ks, vs, qlens, ctxs, bs, 1.0 / math.sqrt(D),
             f"counted keys {tag} Hq={Hq} Hkv={Hkv} D={D} bs={bs}")
    c.O = torch.zeros(T, Hq, D, dtype=torch.float64)
    for s, a, b, ctx, L in c.seqs():
        if b > a and L > 0:
            c.O[a:b] = _kv_head(vs[s][:L].double().cumsum(0)[c.lim[a:b]], c.G)
    return c


def count_precondition(c):
    """For every (row, kv head) and every visible key j (and key lim + 1, which a mask that is
    one too wide would add) there is a coordinate d with V[j, d] != 0 and |O[d]| <= 64: a
    missing or doubled key then moves out * n by >= 1 where the bound is <= 2^-7 * 64."""
    for s, a, b, ctx, L in c.seqs():
        if b == a or L == 0:
            continue
        lim = c.lim[a:b]
        for kvh in range(c.Hkv):
            small = (c.O[a:b, kvh * c.G].abs() <= 64).double()          # [n, D]
            nz = (c.vs[s][:L, kvh].double() != 0).double()              # [L, D]
            hit = small @ nz.t() > 0                                    # [n, L]
            need = torch.arange(L)[None, :] <= (lim[:, None] + 1)
            if not bool((hit | ~need).all()):
                return False
    return True


@functools.lru_cache(maxsize=None)
def rand_case(qlens, ctxs, Hq, Hkv, D, bs, tag="rand"):
    g = gen(tag, Hq, Hkv, D, bs, len(qlens), sum(ctxs))
    T = sum(qlens)
    q = torch.randn(T, Hq, D, generator=g).bfloat16()
    ks, vs = [], []
    for ql, ctx in zip(qlens, ctxs):
        cap = _pages(ql + ctx, bs) * bs
        k = torch.randn(cap, Hkv, D, generator=g).bfloat16()
        v = torch.randn(cap, Hkv, D, generator=g).bfloat16()
        _poison(k, v, ql + ctx)
        ks.append(k)
        vs.append(v)
    c = Case(q, ks, vs, qlens, ctxs, bs, 1.0 / math.sqrt(D), f"random {tag} Hq={Hq} Hkv={Hkv} D={D} bs={bs}")
    c.ref, c.B = attend_case(c)
    return c


def decode_shape(lens):
    """Decode rows as sequences of one query row."""
    return (1,) * len(lens), tuple(L - 1 for L in lens)


# ---------------------------------------------------------------- float64 attention
def attend64(q, k, v, lim, scale, vis=None, vmap=None, emulate=False):
    """q [n, Hq, D], k / v [L, Hkv, D] (the first L rows of a sequence), lim [n]: softmax and
    PV in float64 from the bf16 inputs -> ref [n, Hq, D], B = sum_j p_j |v_j| [n, Hq, D].
    vis [n, L] replaces the causal mask j <= lim and vmap [L] the V row read for key j (the
    planted errors of the CPU tests). A row that sees no key gives 0. emulate: the kernels'
    arithmetic: P rounded to bf16 for PV, the normaliser a sum of unrounded P, the
    quotient rounded once to bf16."""
    n, Hq, D = q.shape
    L, Hkv = k.shape[0], k.shape[1]
    if L == 0:
        z = torch.zeros(n, Hq, D, dtype=torch.float64)
        return z, z.clone()
    G = Hq // Hkv
    kd = _kv_head(k.double(), G)
    vd = _kv_head((v if vmap is None else v[vmap]).double(), G)
    s = torch.einsum("nhd,lhd->hnl", q.double(), kd) * scale
    if vis is None:
        vis = torch.arange(L)[None, :] <= lim[:, None]
    s = s.masked_fill(~vis[None], -INF)
    m = s.amax(-1, keepdim=True)
    p = torch.exp(s - torch.where(torch.isinf(m), torch.zeros_like(m), m))
    l = p.sum(-1, keepdim=True)
    w = p / torch.where(l > 0, l, torch.ones_like(l))
    B = torch.einsum("hnl,lhd->nhd", w, vd.abs())
    if emulate:
        pr = round_bf16(torch.where(p < 1e-30, torch.zeros_like(p), p)).double()
        o = torch.einsum("hnl,lhd->nhd", pr, vd) / torch.where(l > 0, l, torch.ones_like(l)).permute(1, 0, 2)
        return round_bf16(o).double(), B
    return torch.einsum("hnl,lhd->nhd", w, vd), B


def attend_case(c, wrong=None, emulate=False):
    ref = torch.zeros(c.T, c.Hq, c.D, dtype=torch.float64)
    B = torch.zeros_like(ref)
    for s, a, b, ctx, L in c.seqs():
        if b == a:
            continue
        vis = vmap = None
        if wrong is not None:
            vis, vmap = wrong_vis(wrong, c.lim[a:b], L)
        ref[a:b], B[a:b] = attend64(c.q[a:b], c.ks[s][:L], c.vs[s][:L], c.lim[a:b], c.scale, vis, vmap, emulate)
    return ref, B


# ---------------------------------------------------------------- planted errors
WRONG = ["no_diag", "one_past", "drop_64_127", "v70_as_71", "drop_last16"]


def wrong_vis(name, lim, L):
    """(vis [n, L], vmap [L]) of a planted error: the diagonal key not seen, key lim + 1 seen,
    keys 64..127 dropped, V[70] read as V[71], the last 16 visible keys dropped."""
    j = torch.arange(L)[None, :]
    lm = lim[:, None]
    vis = j <= lm
    vmap = torch.arange(L)
    if name == "no_diag":
        vis = j < lm
    elif name == "one_past":
        vis = j <= lm + 1
    elif name == "drop_64_127":
        vis = vis & ~((j >= 64) & (j < 128))
    elif name == "v70_as_71":
        if L > 71:
            vmap[70] = 71
    elif name == "drop_last16":
        vis = j <= lm - 16
    else:
        raise KeyError(name)
    return vis, vmap


def touched(c, name):
    """[T] bool: the planted error changes the set of (key, V row) pairs that the row sees."""
    out = torch.zeros(c.T, dtype=torch.bool)
    for s, a, b, ctx, L in c.seqs():
        if b == a or L == 0:
            continue
        vis, vmap = wrong_vis(name, c.lim[a:b], L)
        ok = torch.arange(L)[None, :] <= c.lim[a:b, None]
        t = (vis != ok).any(-1)
        moved = vmap != torch.arange(L)
        out[a:b] = t | (ok & moved[None, :]).any(-1)
    return out


def touched_stair(c, name):
    """[T, Hq] bool: the planted error changes the V row that wins the staircase (the visible
    key of the largest index for sign +, of the smallest for sign -), or leaves no key."""
    out = torch.zeros(c.T, c.Hq, dtype=torch.bool)
    for s, a, b, ctx, L in c.seqs():
        if b == a or L == 0:
            continue
        vis, vmap = wrong_vis(name, c.lim[a:b], L)
        idx = torch.arange(L)[None, :].expand_as(vis)
        hi = torch.where(vis, idx, torch.full_like(idx, -1)).amax(-1)
        lo = torch.where(vis, idx, torch.full_like(idx, L)).amin(-1)
        none = ~vis.any(-1)
        up = none | (vmap[hi.clamp(0, L - 1)] != c.lim[a:b])
        down = none | (vmap[lo.clamp(0, L - 1)] != 0)
        out[a:b] = torch.where(c.sign[a:b] > 0, up[:, None], down[:, None])
    return out


# ---------------------------------------------------------------- the checks
# Each returns ([T, Hq] bool: the (row, head) pairs that miss the bound, NaN included, and the
# largest share of the bound that is used).
def _judge(d, lim):
    bad = ~(d <= lim)
    share = torch.where(d == 0, torch.zeros_like(d), d / lim)
    share = torch.where(torch.isnan(share), torch.full_like(share, INF), share)
    return bad.any(-1), (float(share.max()) if share.numel() else 0.0)


def close_bad(c, got):
    """Sections 1 and 3: got against the named V row, ULP."""
    w = c.want.double()
    return _judge((got.double() - w).abs(), ULP["atol"] + ULP["rtol"] * w.abs())


def count_bad(c, got):
    n = (c.lim + 1).clamp_min(0).double()[:, None, None]
    return _judge((got.double() * n - c.O).abs(), ULP["atol"] + ULP["rtol"] * c.O.abs().clamp_min(1.0))


def rms_ratio(c, got):
    """rms(out - ref) / rms(ref) over D per (row, head); 0 where ref is 0 (empty rows: checked elementwise)."""
    e = (got.double() - c.ref).pow(2).mean(-1).sqrt()
    r = c.ref.pow(2).mean(-1).sqrt()
    return torch.where(r > 0, e / r.clamp_min(1e-300), torch.zeros_like(e))


def elem_bad(c, got):
    return _judge((got.double() - c.ref).abs(), EB["atol"] + EB["rtol"] * c.B)


def rms_bad(c, got, limit=None):
    limit = RMS_LIMIT if limit is None else limit
    r = rms_ratio(c, got)
    r = torch.where(torch.isnan(r), torch.full_like(r, INF), r)
    return ~(r <= limit), (float(r.max()) / limit if r.numel() else 0.0)


def _assert_none_bad(c, got, bad, what, want=None, note=""):
    if bool(bad.any()):
        t, h = (int(x) for x in bad.nonzero()[0])
        msg = f"{what}: {int(bad.sum())} of {bad.numel()} (row, head) pairs miss the bound; first: {c.where(t, h, note)}\n got  {got[t, h, :8].float().tolist()} ..."
        if want is not None:
            msg += f"\n want {want[t, h, :8].float().tolist()} ..."
        raise AssertionError(msg)


def check_close(c, got, note=""):
    bad, u = close_bad(c, got)
    _assert_none_bad(c, got, bad, "ULP against the named V row", c.want, note)
    return {"ULP": u}


def check_count(c, got, note=""):
    bad, u = count_bad(c, got)
    n = (c.lim + 1).clamp_min(1).double()[:, None, None]
    _assert_none_bad(c, got, bad, "out * n against the integer sum", c.O / n, note)
    return {"COUNT": u}


def check_rand(c, got, note=""):
    bad, u = elem_bad(c, got)
    _assert_none_bad(c, got, bad, "|out - ref| <= 2^-6 B + 1e-6", c.ref, note)
    badr, ur = rms_bad(c, got)
    _assert_none_bad(c, got, badr, f"row rms(out - ref) / rms(ref) <= {RMS_LIMIT:.3e}", c.ref, note)
    return {"EB": u, "RMS": ur}


# ---------------------------------------------------------------- launches
def _i32(x, dev):
    return torch.tensor(x, dtype=torch.int32, device=dev)


def build_cache(c, dev, extra_pages=3):
    """Paged caches [NB, Hkv, bs, D] and a shuffled block table; the pages that no sequence
    names hold NaN (K) and +Inf (V)."""
    bs = c.bs
    n = [k.shape[0] // bs for k in c.ks]
    NB = sum(n) + extra_pages
    kc = torch.full((NB, c.Hkv, bs, c.D), NAN, dtype=torch.bfloat16)
    vc = torch.full((NB, c.Hkv, bs, c.D), INF, dtype=torch.bfloat16)
    perm = torch.randperm(NB, generator=gen("pages", c.tag))
    bt = torch.zeros(len(n), max(n), dtype=torch.int32)
    i = 0
    for s, m in enumerate(n):
        pg = perm[i:i + m]
        kc[pg] = c.ks[s].view(m, bs, c.Hkv, c.D).permute(0, 2, 1, 3)
        vc[pg] = c.vs[s].view(m, bs, c.Hkv, c.D).permute(0, 2, 1, 3)
        bt[s, :m] = pg.to(torch.int32)
        i += m
    return kc.to(dev), vc.to(dev), bt.to(dev)


def _q_view(c, dev):
    """q as a strided view into a wider QKV row whose K / V columns are NaN."""
    W = (c.Hq + 2 * c.Hkv) * c.D
    qkv = torch.full((c.T, W), NAN, dtype=torch.bfloat16)
    qkv[:, :c.Hq * c.D] = c.q.reshape(c.T, -1)
    return qkv.to(dev)[:, :c.Hq * c.D].view(c.T, c.Hq, c.D)


def _out_slice(c, dev, flat=False):
    shape = (c.T + 5, c.Hq * c.D) if flat else (c.T + 5, c.Hq, c.D)
    buf = torch.full(shape, SENT, dtype=torch.bfloat16, device=dev)
    return buf, buf[2:2 + c.T]


def _sentinel_kept(buf, T):
    rest = torch.cat([buf[:2], buf[2 + T:]]).cpu()
    assert torch.equal(bits(rest), bits(torch.full_like(rest, SENT))), "rows of out outside [0, T) were written"


def launch_prefill(dev, c, gh, pad):
    """max_q_len: the largest real length, or (pad) the next multiple of 256 above it."""
    from xgserve import ops
    kc, vc, bt = build_cache(c, dev)
    mq = max(c.qlens)
    if pad:
        mq = (mq // 256 + 1) * 256
    buf, out = _out_slice(c, dev)
    r = ops.prefill_attention(_q_view(c, dev), kc, vc, bt, _i32(c.start, dev), _i32(c.lens, dev), mq, c.scale,
                              out=out, gh=gh)
    assert r.data_ptr() == out.data_ptr()
    _sentinel_kept(buf, c.T)
    return out.cpu()


def launch_decode(dev, c, splits):
    from xgserve import ops
    from xgserve.ops.attention import DecodeWorkspace
    kc, vc, bt = build_cache(c, dev)
    ws = DecodeWorkspace(c.T, c.Hq, c.D, splits, dev)
    ws.part_out.fill_(NAN)  # a split that owns no key must still publish its (empty) state
    ws.part_lse.fill_(NAN)
    buf, out = _out_slice(c, dev)
    r = ops.decode_attention(_q_view(c, dev), kc, vc, bt, _i32(c.lens, dev), c.scale, num_splits=splits,
                             workspace=ws, out=out)
    assert r.data_ptr() == out.data_ptr()
    _sentinel_kept(buf, c.T)
    return out.cpu()


def _assert_empty_rows_zero(c, got):
    for s, a, b, ctx, L in c.seqs():
        if L == 0 and b > a:
            assert got[a:b].float().abs().max().item() == 0.0, f"{c.tag}: an empty row must give exactly 0"


def run_prefill(dev, kind, shapes, Hq, Hkv, D, gh, bs, pad):
    qlens, ctxs = shapes
    build = {"stair": stair_case, "count": count_case, "rand": rand_case}[kind]
    chk = {"stair": check_close, "count": check_count, "rand": check_rand}[kind]
    c = build(qlens, ctxs, Hq, Hkv, D, bs, tag=f"prefill_{kind}")
    return chk(c, launch_prefill(dev, c, gh, pad), f" gh={gh} pad={pad}")


def decode_case(kind, lens, D, G, bs):
    """Hkv = 2. The staircase takes every length twice, the second time in reverse order, so
    that with one head per kv head (sign by row) every length meets both signs."""
    if kind == "stair":
        lens = list(lens) + list(lens)[::-1]
    qlens, ctxs = decode_shape(lens)
    build = {"stair": stair_case, "count": count_case, "rand": rand_case}[kind]
    return build(qlens, ctxs, 2 * G, 2, D, bs, tag=f"decode_{kind}")


def run_decode(dev, kind, lens, D, G, bs, splits):
    chk = {"stair": check_close, "count": check_count, "rand": check_rand}[kind]
    c = decode_case(kind, lens, D, G, bs)
    got = launch_decode(dev, c, splits)
    _assert_empty_rows_zero(c, got)
    return chk(c, got, f" splits={splits}")


# ---------------------------------------------------------------- the fused decode
def _rotate64(x, cs_rows):
    h = x.shape[-1] // 2
    cos, sin = cs_rows[:, None, :h], cs_rows[:, None, h:]
    x1, x2 = x[..., :h], x[..., h:]
    return torch.cat([x1 * cos - x2 * sin, x2 * cos + x1 * sin], dim=-1)


def qkv64(rows64, pos, cs, Hq, Hkv, D, rope):
    """rows64 [B, (Hq + 2 Hkv) D] float64 -> bf16 q [B, Hq, D], k, v [B, Hkv, D], rounded once."""
    B = rows64.shape[0]
    q = rows64[:, :Hq * D].reshape(B, Hq, D)
    k = rows64[:, Hq * D:(Hq + Hkv) * D].reshape(B, Hkv, D)
    v = rows64[:, (Hq + Hkv) * D:].reshape(B, Hkv, D)
    if rope:
        rows = cs.double()[pos.long()]
        q, k = _rotate64(q, rows), _rotate64(k, rows)
    return round_bf16(q), round_bf16(k), round_bf16(v)


class FusedCase:
    pass


def fused_case(kind, G, S, bs, lens, rope, Hkv=2, D=128):
    """kind "own": the new key's score is 200 (section 3); "rand": random partials (section 4).
    f.part [S, B, W] fp32; f.c: the decode Case that the launch must equal, with the bf16 q and
    the appended K / V rows of the float64 reference; f.ks0 / f.vs0: the cache rows before
    the call, NaN in K and V from row L - 1 on."""
    from xgserve import ops
    f = FusedCase()
    Hq = Hkv * G
    B, W = len(lens), (Hq + 2 * Hkv) * D
    g = gen("fused", kind, G, S, bs, rope)
    scale = 1.0 / math.sqrt(D)
    if kind == "own":
        k_new = torch.randn(B, Hkv, D, generator=g).double() * 1.5
        v_new = torch.randn(B, Hkv, D, generator=g).double()
        q_new = _kv_head(200.0 * k_new / (k_new.pow(2).sum(-1, keepdim=True) * scale), G)
        target = torch.cat([q_new.reshape(B, -1), k_new.reshape(B, -1), v_new.reshape(B, -1)], dim=1)
        part = torch.randn(S, B, W, generator=g) * 0.3
        part[S - 1] = (target - part[:S - 1].double().sum(0)).float()
    else:
        part = torch.randn(S, B, W, generator=g) * 0.3
    f.part, f.S, f.rope, f.lens, f.bs = part, S, rope, lens, bs
    f.pos = torch.tensor([max(0, L - 1) for L in lens], dtype=torch.int32)
    f.cs = ops.build_cos_sin(D, max(lens) + 1, 500000.0)
    q, f.k_new, f.v_new = qkv64(part.double().sum(0), f.pos, f.cs, Hq, Hkv, D, rope)
    f.ks0, f.vs0, ks, vs = [], [], [], []
    for b, L in enumerate(lens):
        cap = _pages(L, bs) * bs
        k = torch.randn(cap, Hkv, D, generator=g).bfloat16()
        v = torch.randn(cap, Hkv, D, generator=g).bfloat16()
        k[max(0, L - 1):] = NAN
        v[max(0, L - 1):] = NAN
        f.ks0.append(k)
        f.vs0.append(v)
        k, v = k.clone(), v.clone()
        if L > 0:
            k[L - 1], v[L - 1] = f.k_new[b], f.v_new[b]
        ks.append(k)
        vs.append(v)
    qlens, ctxs = decode_shape(lens)
    f.c = Case(q, ks, vs, qlens, ctxs, bs, scale, f"fused {kind} G={G} S={S} bs={bs} rope={rope}")
    if kind == "own":
        want = _kv_head(f.v_new, G).clone()
        want[[b for b, L in enumerate(lens) if L == 0]] = 0
        f.c.want = want
    else:
        f.c.ref, f.c.B = attend_case(f.c)
    return f


def fused_gap(f):
    """The smallest lead, in nats, of the appended key's score over every other key of its row."""
    c, gap = f.c, INF
    for s, a, b, ctx, L in c.seqs():
        if L < 2:
            continue
        sc = torch.einsum("hd,lhd->hl", c.q[a].double(), _kv_head(c.ks[s][:L].double(), c.G)) * c.scale
        gap = min(gap, float((sc[:, L - 1] - sc[:, :L - 1].amax(-1)).min()))
    return gap


def launch_fused(dev, f, depth, splits):
    """The HIP launch (no CPU path); checks the appended and the untouched cache rows."""
    from xgserve import ops
    from xgserve.ops.attention import DecodeWorkspace
    from xgserve.ops.linear import PendingSum
    c, bs = f.c, f.bs
    before = Case(c.q, f.ks0, f.vs0, c.qlens, c.ctxs, bs, c.scale, c.tag)
    kc, vc, bt = build_cache(before, dev)
    btc = bt.cpu()
    slots = [int(btc[b, (L - 1) // bs]) * bs + (L - 1) % bs if L > 0 else -1 for b, L in enumerate(f.lens)]
    kc0, vc0 = kc.clone(), vc.clone()
    ws = DecodeWorkspace(c.T, c.Hq, c.D, splits, dev)
    ws.part_out.fill_(NAN)
    ws.part_lse.fill_(NAN)
    buf, out = _out_slice(c, dev, flat=True)
    r = ops.decode_attention_fused(PendingSum(f.part.to(dev), f.S), f.pos.to(dev), _i32(slots, dev), f.cs.to(dev), kc,
                                   vc, bt, _i32(f.lens, dev), c.Hq, c.scale, splits, workspace=ws,
                                   apply_rope=f.rope, out=out, depth=depth)
    assert r.data_ptr() == out.data_ptr()
    _sentinel_kept(buf, c.T)
    # the appended rows within one bf16 step of the float64 reference, every other row bit for bit
    kc, vc, kc0, vc0 = (t.cpu() for t in (kc, vc, kc0, vc0))
    keep = torch.ones(kc.shape[0], bs, dtype=torch.bool)
    for b, s in enumerate(slots):
        if s < 0:
            continue
        keep[s // bs, s % bs] = False
        torch.testing.assert_close(kc[s // bs, :, s % bs].double(), f.k_new[b].double(), **ULP)
        torch.testing.assert_close(vc[s // bs, :, s % bs].double(), f.v_new[b].double(), **ULP)
    for after, b4 in ((kc, kc0), (vc, vc0)):
        assert torch.equal(bits(after).permute(0, 2, 1, 3)[keep], bits(b4).permute(0, 2, 1, 3)[keep]), \
            "a cache row that slot_mapping does not name was written"
    return out.cpu().view(c.T, c.Hq, c.D)


def run_fused(dev, kind, G, S, depth, bs, splits, rope, lens=None):
    f = fused_case(kind, G, S, bs, fused_lens(bs) if lens is None else lens, rope)
    if kind == "own":
        assert fused_gap(f) >= FUSED_GAP_MIN
    got = launch_fused(dev, f, depth, splits)
    _assert_empty_rows_zero(f.c, got)
    return (check_close if kind == "own" else check_rand)(f.c, got, f" depth={depth} splits={splits}")


# ---------------------------------------------------------------- section 4's inputs, for the emulation
def rand_cases():
    """Every distinct input of section 4 (the configurations share inputs per (Hq, Hkv, D, bs))."""
    out = []
    for Hq, Hkv, D, gh, bs in RAND_PF:
        out.append(rand_case(RAND_QLENS, RAND_CTXS, Hq, Hkv, D, bs, tag="prefill_rand"))
    for D, G, bs in RAND_DEC:
        out.append(decode_case("rand", DEC_LENS, D, G, bs))
    G, S, depth, bs, splits, rope = RAND_FUSED
    out.append(fused_case("rand", G, S, bs, fused_lens(bs), rope).c)
    return out


def emulated_rms():
    """The largest row rms ratio of the float64 emulation of the kernels' arithmetic over rand_cases()."""
    worst = 0.0
    for c in rand_cases():
        emu, _ = attend_case(c, emulate=True)
        worst = max(worst, float(rms_ratio(c, emu).max()))
    return worst
