"""Problems, float64 references, checks, the case enumeration and an fp32 emulation for the fused
decode epilogues of gemm_m64g (csrc/kernels/gemm_m64g.hip, entry gemm_m64g_ex): the RMSNorm row
scale taken from ss_in, the GG_RESID tail (ticket, slab reduce, residual add, bf16 rounding,
ss_out), the split-K SiLU tail, and the hand-off of a producer's ss_out to the next GEMM's ss_in.
tests/test_m64_epi_exact_gpu.py launches the cases; tests/test_m64_epi_refs_cpu.py builds them,
runs the emulation through the same checks and plants errors. Grids, sentinels, guarded buffers,
check_silu / check_bound, slab_sum and the rotation switches are tests/_gemm_ref.py's.

Operands. x = jx 2^-e, W = jw 2^-e' are integer grids with sum_k |jx| |jw| < 2^24 (asserted), so
the unscaled value y_s of every slab s (split s owns chunks [s nch / S, (s + 1) nch / S)) is an
exact fp32 in any chunk order, and float64 knows it exactly.

1. Row scale. ss_in[j, m] = u_m a[j, m]: a[:, m] a permutation of 1 .. ss_n, u_m = 4^-(e0 + e_m),
   e_m = (m + m // 16) % 4. Every partial sum of a row is an integer <= ss_n (ss_n + 1) / 2 < 2^24
   times u_m: fp32-exact in any order, so the three summation paths (ss_n <= 8 "small"; wide:
   M <= 16, spread over 4 WV lane groups; tall: M > 16, through LDS) must all give the same sum
   bit for bit. Every row has the same integer total, so rows m +- 1 and m +- 16 (e differs by
   1, 2 or 3 mod 4) carry a sum 4 .. 64 times larger or smaller: the scale of a neighbour is off
   by a factor >= 2 (less what eps dilutes). e0 puts sum / K of the largest rows into
   (2^-11, 2^-9], so eps = 1e-5 is between 0.5 % and 130 % of sum / K. ss_in is an interior
   slice: NaN rows before it, NaN in columns [M, stride), NaN rows from j = ss_n on.
   Reference: float64 y rsqrt(sum / K + eps), eps the fp32 the kernel is handed.
   Bound, per element, from the kernel's operations (u = 2^-24, one rounding to nearest):
     inv_k = 1 / K            <= u (0 if K is a power of two)
     t = tot * inv_k          <= u
     t + eps                  <= u; the errors so far carry over scaled by t / (t + eps) <= 1
     rsqrtf                   halves the relative error of its argument (1.5 u) and adds its own:
                              2 ulp in CUDA's table, 1 ulp in HIP's -- the larger, 2 ulp <= 4 u
     acc * sc                 <= u
   together 6.5 u |sc y_s| per slab element to first order, 7 u with room for the second-order
   terms; the check (and the in-launch tails) add the S slabs with S - 1 fp32 additions, each
   <= u times a partial sum <= sum_s |sc y_s|. So
     |got - ref| <= c(S) 2^-24 sc sum_s |y_s|,   c(S) = 7 + (S - 1).
   BF16 output: + BF16_U (|ref| + B), one rounding of the erroneous value. SiLU output:
   _gemm_ref.Problem.real_bound -- B of gate and up through |d silu / dg| <= 1.1 and
   |silu(g)| <= |g| at |g| <= SILU_MAX (the grid is scaled so |sc y| <= SILU_MAX), + SILU_RTOL.
   Builder condition (asserted by every builder with statistics, against the fp32 bound B):
   changing a row's sum by ONE unit u_m -- the least that dropping, duplicating or replacing one
   partial sum by another can do, the a[:, m] being distinct positive integers -- moves some
   output of that row by >= 8 B, and so does the sum of row m +- 1 or m +- 16. In the BF16 and
   SiLU modes one dropped sum of 128 is below the rounding of the output itself, which is why
   every (path, WV, MT) instantiation runs in PARTIAL mode too; a neighbour's sum or a missing
   eps is seen in every mode.

2. GG_RESID. x in [-4, 4], W in [-2, 2]; resid0 = bf16(t0 - y) for a drawn target t0 with
   257 <= |t0| <= V(cols) = isqrt(2^24 / cols) - 8, so that (asserted) every
   sum_s y_s + resid0 is an integer whose partial sums stay below 2^24 (exact in any order), at
   least a quarter of the new values are no bf16 and at least one is an exact tie, and per
   (row, tile) sum of squares of the rounded values < 2^24 (integers: ss_out exact in any order).
   resid must be round_bf16(exact) and ss_out[tile, m] the exact sum, bit for bit. The
   256-column tile (8 waves, nw = 2) cannot meet the last condition and round at all (256 v^2 <
   2^24 means |v| < 256, where every integer is a bf16): for that width only, V is the
   128-column one and ss_out is held to (COLS - 1) 2^-24 sum (COLS - 1 additions of positive
   terms; the squares of integers below 2^12 are exact).
   Staging threshold at S = 1: the tile goes through LDS iff 256 + M COLS 4 <= sizeof(lds0),
   lds0 = NS' SLOT (NS' = 1 for the three-slot ring, whose slots are separate arrays, else the
   ring depth), SLOT = 32 KC (MT + WV NW) bytes (m64_pipe.h: 16 MT x rows and 16 NW WV weight rows
   of 2 KC bytes). Largest staged M per (waves, kc, ring) at nw = 1 / 2, MT = 4 unless noted:
     (4, 128, 3): 127 / 95    (4, 64, 3): 63 / 47    (2, 64, 3): 94 / 63    (2, 128, 3): 190 / 127
     (8, 64, 3): 47 / 39      deep rings (MT = 1, M <= 16): always staged
   so both sides exist inside 1 .. 64 for (4, 64) at either nw, (2, 64) at nw = 2 and (8, 64);
   staged() below recomputes this from the table and the tests assert cases on both sides.
   With ss_in in the same launch ("both"): resid within
     B' = 7 u sc sum |y_s| + S u (sc sum |y_s| + |resid0|)   (the residual add is the S-th addition)
   plus one bf16 rounding; ss_out against the float64 sum of squares of the resid the kernel
   wrote, within (COLS + 1) u sum (one rounding per square, COLS - 1 additions, room for second order).

3. Split-K SiLU tail: grids scaled to |g|, |u| <= SILU_MAX; without ss_in the slab sums are exact
   and check_silu applies as it stands; with ss_in, section 1's SiLU bound.

4. Chain: launch A (GG_RESID) writes resid and ss_out [tiles, M]; launch B takes resid as x,
   ss_out as ss_in (ss_n = tiles, stride M). Targets are drawn so that N_A max|t|^2 < 2^24: the
   whole row's sum of squares is an exact integer however it is split, so the per-tile layout,
   add_partials_resid's per-1024-column layout and row_sumsq's single sum give B the same
   statistics, and B's output is held to section 1's bound against float64 of the chain.
"""
from __future__ import annotations

import functools
import math
from typing import NamedTuple

import torch

import _gemm_ref as G
from _row_ref import gen, round_bf16
from xgserve.ops import linear as L

MODE_BF16, MODE_PARTIAL, MODE_SILU, MODE_RESID = G.MODE_BF16, G.MODE_PARTIAL, G.MODE_SILU, L.MODE_RESID
MODE_NAMES = dict(G.MODE_NAMES)
MODE_NAMES[MODE_RESID] = "resid"
U = 2.0 ** -24
C0 = 7                      # per slab element (module docstring)
SS_PRE, SS_POST = 2, 2      # NaN rows around the statistics
SSN_ANY, SSN_SMALL_M = (1, 4, 5, 8, 9, 63, 64), (65, 127, 128)
SMALL_M = tuple(m for m in G.M64_M if m <= 16)
BIG_M = tuple(m for m in G.M64_M if m > 16)
RESID_S = (1, 2, 3, 4, 5, 8, 9)
SILU_S = (2, 3, 4, 5, 8, 9)
# committed floors on the number of launched cases per section
FLOORS = {"scale": 600, "resid": 430, "both": 76, "silu": 130, "chain": 16}


def c_of(S):
    return C0 + S - 1


# ---------------------------------------------------------------- geometry (from the library's table)
class Geom(NamedTuple):
    wv: int
    kc: int
    ns: int
    MT: int
    cols: int
    lds0: int


def geom(cfg, nw, M):
    wv, kc, _nt, ns, _g = L.kernels().gemm_cfgs()["m64g"][cfg]
    mt1 = 16 // (512 // kc) // wv >= 1      # m64_x_dmas(wv, kc, 1) >= 1
    mt4 = ns == 3
    MT = 1 if (mt1 and (M <= 16 or not mt4)) else 4
    slot = 32 * kc * (MT + wv * nw)
    return Geom(wv, kc, ns, MT, 16 * nw * wv, slot if ns == 3 else ns * slot)


def staged(cfg, nw, M):
    g = geom(cfg, nw, M)
    return 256 + M * g.cols * 4 <= g.lds0


def stat_path(cfg, nw, M, ss_n):
    if ss_n <= 8:
        return "small"
    return "tall" if geom(cfg, nw, M).MT > 1 and M > 16 else "wide"


def row_classes(cfg, nw):
    """The row-count classes (M <= 16, M > 16) the predicate takes for a configuration."""
    k = L.kernels()
    g = geom(cfg, nw, 1)
    return [Ms for Ms in (SMALL_M, BIG_M) if k.m64g_supports(Ms[0], g.kc, g.cols, 1, MODE_PARTIAL, nw, cfg)]


@functools.lru_cache(maxsize=None)
def accepted():
    """Every (cfg, nw, MT) the predicate takes at any M of M64_M, by brute force."""
    k = L.kernels()
    out = set()
    for cfg in range(len(k.gemm_cfgs()["m64g"])):
        for nw in (1, 2):
            for M in G.M64_M:
                g = geom(cfg, nw, M)
                if k.m64g_supports(M, g.kc, g.cols, 1, MODE_PARTIAL, nw, cfg):
                    out.add((cfg, nw, g.MT))
    return frozenset(out)


@functools.lru_cache(maxsize=None)
def accepted_paths():
    """Every (cfg, nw, MT, statistics path) that exists for an accepted M and a legal ss_n."""
    k = L.kernels()
    out = set()
    for cfg in range(len(k.gemm_cfgs()["m64g"])):
        for nw in (1, 2):
            for M in G.M64_M:
                g = geom(cfg, nw, M)
                if k.m64g_supports(M, g.kc, g.cols, 1, MODE_PARTIAL, nw, cfg):
                    for n in SSN_ANY + (SSN_SMALL_M if M <= 16 else ()):
                        out.add((cfg, nw, g.MT, stat_path(cfg, nw, M, n)))
    return frozenset(out)


# ---------------------------------------------------------------- cases
class Case(NamedTuple):
    sec: str      # scale, resid, both, silu
    cfg: int
    nw: int
    mode: int
    M: int
    N: int
    K: int
    S: int
    krot: int     # set_k_rotation(0) or the default
    ss_n: int     # 0: no statistics
    stride: int
    eps: float
    idx: int

    family = "m64g"

    @property
    def tag(self):
        return (f"m64g_ex {self.sec} cfg{self.cfg} nw{self.nw} {MODE_NAMES[self.mode]} M{self.M} N{self.N} K{self.K} "
                f"S{self.S} krot{self.krot} ss_n{self.ss_n} stride{self.stride} eps{self.eps}")

    @property
    def key(self):
        g = geom(self.cfg, self.nw, self.M)
        return (self.cfg, self.nw, g.MT)

    @property
    def path(self):
        return stat_path(self.cfg, self.nw, self.M, self.ss_n) if self.ss_n else None


def _mk(sec, cfg, nw, mode, M, tiles, nch, S, i, ss_n=0):
    k = L.kernels()
    g = geom(cfg, nw, M)
    N, K = g.cols * tiles, g.kc * nch
    stride = 0 if not ss_n else (M if i % 3 == 0 else M + 1 + i % 5)
    eps = 0.0 if (i % 2 or not ss_n) else 1e-5
    c = Case(sec, cfg, nw, mode, M, N, K, S, (i // 2) % 2, ss_n, stride, eps, i)
    # a configuration the table lists and the predicate refuses here is a finding, not a skip
    assert k.m64g_supports(M, K, N, S, mode, nw, cfg), c.tag
    return c


def _configs():
    n = len(L.kernels().gemm_cfgs()["m64g"])
    return [(cfg, nw, Ms) for cfg in range(n) for nw in (1, 2) for Ms in row_classes(cfg, nw)]


SCALE_KS = ((1, 1), (3, 1), (4, 2), (5, 2), (8, 4), (7, 3), (2, 1), (9, 5))   # (chunks, S): K a power of two and not
SCALE_KS1 = (1, 3, 2, 5, 8)
SUBSET = (5, 9, 64, 128)      # the other modes: one ss_n of the small path, the rest of the wide / tall one


@functools.lru_cache(maxsize=None)
def scale_cases():
    """Section 1: PARTIAL at every ss_n; BF16, SiLU and split-K SiLU at SUBSET."""
    out = []
    for cfg, nw, Ms in _configs():
        ssns = SSN_ANY + (SSN_SMALL_M if Ms is SMALL_M else ())
        i = 0
        for mode, split in ((MODE_PARTIAL, 0), (MODE_BF16, 0), (MODE_SILU, 0), (MODE_SILU, 1)):
            if mode == MODE_SILU and nw != 2:
                continue
            for n in ssns:
                if mode != MODE_PARTIAL and n not in SUBSET:
                    continue
                M = Ms[(i + cfg) % len(Ms)]
                if mode == MODE_PARTIAL:
                    nch, S = SCALE_KS[(i + nw) % len(SCALE_KS)]
                elif split:
                    nch, S = ((3, 2), (4, 3), (8, 2))[i % 3]
                else:
                    nch, S = SCALE_KS1[i % len(SCALE_KS1)], 1
                out.append(_mk("scale", cfg, nw, mode, M, 2 + i % 2, nch, S, i, n))
                i += 1
    return tuple(out)


@functools.lru_cache(maxsize=None)
def resid_cases():
    """Section 2: S = 1 at every M of the class, S > 1 at rotating M, uneven splits."""
    out = []
    for cfg, nw, Ms in _configs():
        i = 0
        for S in RESID_S:
            for M in (Ms if S == 1 else (Ms[(S + cfg + nw) % len(Ms)],)):
                out.append(_mk("resid", cfg, nw, MODE_RESID, M, 2 + i % 2, S + (i % 3 if S > 1 else i % 2), S, i))
                i += 1
    return tuple(out)


@functools.lru_cache(maxsize=None)
def both_cases():
    """ss_in and GG_RESID in one launch: two per (cfg, nw, class)."""
    out = []
    for j, (cfg, nw, Ms) in enumerate(_configs()):
        ssns = SSN_ANY + (SSN_SMALL_M if Ms is SMALL_M else ())
        for i in range(2):
            n = ssns[(3 * j + 5 * i + 2) % len(ssns)]
            S = (1, 2, 4, 9)[(j + i) % 4]
            out.append(_mk("both", cfg, nw, MODE_RESID, Ms[(j + 2 * i) % len(Ms)], 2 + i, S + i, S, 2 * j + i + 1, n))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def silu_cases():
    """Section 3: every cfg at nw = 2, every S of SILU_S, with and without statistics."""
    out = []
    for cfg, nw, Ms in _configs():
        if nw != 2:
            continue
        if Ms is SMALL_M and len(row_classes(cfg, nw)) == 2:
            continue   # both classes exist: the S values alternate between them below
        i = 0
        for S in SILU_S:
            for with_ss in (0, 1):
                cls = row_classes(cfg, nw)
                Mc = cls[(i // 2 + with_ss) % len(cls)]
                M = Mc[(i + cfg) % len(Mc)]
                n = 0 if not with_ss else (4, 9, 64)[i // 2 % 3]
                out.append(_mk("silu", cfg, nw, MODE_SILU, M, 2 + i % 2, S + i % 3, S, i // 2 if with_ss else i, n))
                i += 1
    return tuple(out)


ALL_SECTIONS = {"scale": scale_cases, "resid": resid_cases, "both": both_cases, "silu": silu_cases}


# ---------------------------------------------------------------- problems
def eps64(eps):
    return float(torch.tensor(eps, dtype=torch.float32).double())


def scale64(sums, div, eps):
    return 1.0 / torch.sqrt(sums / div + eps64(eps))


def make_stats(c, g):
    """(ssbuf [SS_PRE + ss_n + SS_POST, stride] fp32 with NaN guards, row sums, row units), float64."""
    n, M = c.ss_n, c.M
    a = torch.stack([torch.randperm(n, generator=g) + 1 for _ in range(M)], 1).double()   # [n, M]
    A = n * (n + 1) / 2
    e0 = math.ceil((math.log2(A / c.K) + 9) / 2)
    e = torch.tensor([(m + m // 16) % 4 for m in range(M)]) + e0
    unit = 4.0 ** -e.double()
    vals = a * unit[None, :]
    assert A < G.EXACT and torch.equal(vals.float().double(), vals)
    buf = torch.full((SS_PRE + n + SS_POST, c.stride), G.NAN, dtype=torch.float32)
    buf[SS_PRE:SS_PRE + n, :M] = vals.float()
    return buf, vals.sum(0), unit


class EpiProblem:
    pass


def _visible(p, c, sums, unit):
    """The builder condition of section 1 (module docstring)."""
    Yabs = p.ys.sum(0).abs()

    def moved(sc2):
        return (((sc2 - p.sc).abs()[:, None] * Yabs) >= 8 * p.B).any(1)

    for sgn in (1.0, -1.0):
        s2 = sums + sgn * unit
        ok = s2 > 0
        m = moved(scale64(torch.where(ok, s2, sums), c.K, c.eps))
        assert bool((m | ~ok).all()), (c.tag, "one unit of a partial sum is invisible")
    for d in (1, -1, 16, -16):
        idx = torch.arange(c.M) + d
        valid = (idx >= 0) & (idx < c.M)
        if bool(valid.any()):
            m = moved(scale64(sums[idx.clamp(0, c.M - 1)], c.K, c.eps))
            assert bool(m[valid].all()), (c.tag, f"row m{d:+d}'s statistics are invisible")


def resid_vmax(cols):
    return math.isqrt(G.EXACT // min(cols, 128)) - 8


@functools.lru_cache(maxsize=16)
def problem(c: Case):
    p = EpiProblem()
    M, N, K, S = c.M, c.N, c.K, c.S
    gm = geom(c.cfg, c.nw, M)
    g = gen("m64-epi", *c)
    resid = c.mode == MODE_RESID
    if resid:
        pair, jx, jw = "r", G._ints(g, (M, K), -4, 4), G._ints(g, (N, K), -2, 2)
    else:
        pair = G.PAIRS[(c.idx + c.cfg) % 3]
        jx, jw = G._pair(pair, g, M, N, K)
    assert float((jx.abs() @ jw.abs().t()).max()) < G.EXACT
    ys = torch.stack([jx[:, lo * gm.kc:hi * gm.kc] @ jw[:, lo * gm.kc:hi * gm.kc].t()
                      for lo, hi in G.split_ranges(K // gm.kc, S)])
    p.sc = torch.ones(M, dtype=torch.float64)
    p.ssbuf = None
    if c.ss_n:
        p.ssbuf, sums, unit = make_stats(c, g)
        p.sc = scale64(sums, K, c.eps)
    ex = 0
    if c.mode == MODE_SILU:
        top = float((p.sc[:, None] * ys.sum(0)).abs().max())
        ex = max(0, math.ceil(math.log2(max(top, 1.0) / G.SILU_MAX)))
    ys = ys * 2.0 ** -ex
    sx, sw = (2.0 ** -ex, 1.0) if pair != "b" else (1.0, 2.0 ** -ex)
    p.x, p.w, p.ys = G._to_bf16(jx * sx), G._to_bf16(jw * sw), ys
    p.note = pair
    Y = p.sc[:, None] * ys.sum(0)
    absY = p.sc[:, None] * ys.abs().sum(0)
    p.B = c_of(S) * U * absY if c.ss_n else None
    if c.ss_n:
        _visible(p, c, sums, unit)
    if c.mode == MODE_PARTIAL:
        p.ref, p.lim = Y, p.B
    elif c.mode == MODE_BF16:
        p.ref, p.lim = Y, p.B + G.BF16_U * (Y.abs() + p.B)
    elif c.mode == MODE_SILU:
        assert float(Y.abs().max()) <= G.SILU_MAX
        gp = G.Problem("real", p.x, Y, w=p.w, bound=p.B if c.ss_n else torch.zeros_like(Y))
        p.ref = gp.silu_ref()[0]
        p.lim = gp.real_bound(MODE_SILU) if c.ss_n else p.ref.abs() * G.SILU_RTOL
    else:
        V = resid_vmax(gm.cols)
        tiles = N // gm.cols
        for attempt in range(16):
            mag = torch.randint(257, V + 1, (M, N), generator=g).double()
            t0 = mag * (2 * torch.randint(0, 2, (M, N), generator=g) - 1)
            p.resid0 = round_bf16(t0 - Y)
            t = Y + p.resid0.double()
            if c.ss_n or (G.bf16_rounding_stats(t)[0] >= 0.25 and G.bf16_rounding_stats(t)[1] >= 1):
                break
        if c.ss_n:
            B2 = C0 * U * absY + S * U * (absY + p.resid0.double().abs())
            p.ref, p.lim = t, B2 + G.BF16_U * (t.abs() + B2)
        else:
            assert torch.equal(t, t.round()) and float((ys.abs().sum(0) + p.resid0.double().abs()).max()) < G.EXACT
            share, ties = G.bf16_rounding_stats(t)
            assert share >= 0.25 and ties >= 1, (c.tag, share, ties)
            p.want_resid = round_bf16(t)
            sq = (p.want_resid.double() ** 2).view(M, tiles, gm.cols).sum(-1).t().contiguous()   # [tiles, M]
            p.ss_exact = gm.cols <= 128
            assert float(sq.max()) < G.EXACT or not p.ss_exact, (c.tag, float(sq.max()))
            assert float(p.want_resid.double().abs().max()) < 2 ** 12   # (squares exact)
            p.want_ss = sq
    return p


# ---------------------------------------------------------------- buffers, operands, expectations
class Buffers:
    """Fresh sentinel-filled outputs of one launch (CPU or GPU)."""

    def __init__(self, c, p, dev):
        self.flats = {}
        M, N, S = c.M, c.N, c.S
        gm = geom(c.cfg, c.nw, M)
        self.tiles = N // gm.cols
        self.part = self.out = self.resid = self.ss_out = None
        if c.mode in (MODE_PARTIAL, MODE_RESID) or (c.mode == MODE_SILU and S > 1):
            self.part = self._mk("part", (S, M, N), torch.float32, dev)
        if c.mode in (MODE_BF16, MODE_SILU):
            self.out = self._mk("out", (M, N // 2 if c.mode == MODE_SILU else N), torch.bfloat16, dev)
        if c.mode == MODE_RESID:
            self.resid = self._mk("resid", (M, N), torch.bfloat16, dev, pad=max(G.PAD, 2 * N))  # two rows behind M
            self.resid.copy_(p.resid0.to(dev))
            self.ss_out = self._mk("ss_out", (self.tiles, M), torch.float32, dev)
        self.counters = torch.zeros(self.tiles + 8, dtype=torch.int32, device=dev)
        self.uses_counters = c.mode == MODE_RESID or (c.mode == MODE_SILU and S > 1)

    def _mk(self, name, shape, dtype, dev, pad=G.PAD):
        flat, view = G.guarded(shape, dtype, dev, pad)
        self.flats[name] = (flat, math.prod(shape), pad)
        return view

    @property
    def primary(self):
        return "resid" if self.resid is not None else ("out" if self.out is not None else "part")

    def check_guards(self, tag):
        for name, (flat, n, pad) in self.flats.items():
            assert G.guards_intact(flat, n, pad), f"{tag}: wrote outside {name}"
        assert not bool(self.counters.any()), f"{tag}: a ticket was left at {self.counters.tolist()}"

    def same_as(self, other, tag):
        for name, (flat, _n, _pad) in self.flats.items():
            if name == "part" and self.resid is not None and self.part.shape[0] == 1:
                continue   # (one split: a staged tile never touches its slab, scratch either way)
            assert torch.equal(flat, other.flats[name][0]), f"{tag}: two launches differ in {name}"


class Operands:
    def __init__(self, c, p, dev):
        self.x, self.w = G.with_tail(p.x, dev), G.with_tail(p.w, dev)
        self.ss = None if p.ssbuf is None else p.ssbuf.to(dev)
        self.ss_ptr = 0 if self.ss is None else self.ss[SS_PRE:].data_ptr()


class Want:
    def __init__(self, c, p, dev):
        self.c = c
        for name in ("ref", "lim", "want_resid", "want_ss"):
            if getattr(p, name, None) is not None:
                setattr(self, name, getattr(p, name).to(dev))
        self.exact = not c.ss_n
        self.ss_exact = getattr(p, "ss_exact", False)

    def check(self, b: Buffers, tag):
        """Every check of the case's mode on one launch's buffers; returns the share of a bound used."""
        c = self.c
        b.check_guards(tag)
        if c.mode == MODE_PARTIAL:
            return G.check_bound(G.slab_sum(b.part), self.ref, self.lim, tag)
        if c.mode == MODE_BF16:
            return G.check_bound(b.out, self.ref, self.lim, tag)
        if c.mode == MODE_SILU:
            if b.part is not None:
                assert not bool((G.ibits(b.part) == G.SENT32).any()), f"{tag}: a slab element was never written"
            return G.check_silu(b.out, self.ref, tag) if self.exact else G.check_bound(b.out, self.ref, self.lim, tag)
        cols = c.N // b.tiles
        if self.exact:
            G.check_bf16(b.resid, self.want_resid, tag + " resid")
            if self.ss_exact:
                G.check_partial(b.ss_out[None], self.want_ss.float(), tag + " ss_out")
                return 0.0
            return G.check_bound(b.ss_out, self.want_ss, (cols - 1) * U * self.want_ss, tag + " ss_out")
        used = G.check_bound(b.resid, self.ref, self.lim, tag + " resid")
        sq = (b.resid.double() ** 2).view(c.M, b.tiles, cols).sum(-1).t()
        return max(used, G.check_bound(b.ss_out, sq, (cols + 1) * U * sq, tag + " ss_out"))


def native_launch(k, c, ops, b, st):
    def ptr(t):
        return 0 if t is None else t.data_ptr()

    k.gemm_m64g_ex(ops.x.data_ptr(), c.M, c.K, ops.w.data_ptr(), c.N, ptr(b.part), ptr(b.out), c.S, c.mode, c.nw, c.cfg,
                   ops.ss_ptr, c.ss_n, c.stride, c.eps, ptr(b.resid), ptr(b.ss_out),
                   b.counters.data_ptr() if b.uses_counters else 0, st)


def run_case(c, p, dev, launch):
    """Two launches of `c` into fresh buffers: the checks, the guards, zero tickets, bit-identical
    results. launch(c, p, ops, buffers). Returns the share of a bound used."""
    ops, want = Operands(c, p, dev), Want(c, p, dev)
    first, used = None, 0.0
    for rep in range(2):
        b = Buffers(c, p, dev)
        launch(c, p, ops, b)
        used = want.check(b, f"{c.tag} [{p.note}] launch {rep}")
        if first is None:
            first = b
        else:
            b.same_as(first, c.tag)
    return used


# ---------------------------------------------------------------- fp32 emulation (CPU)
SCALE_PLANTS = ("row+1", "row+16", "drop", "dup_last", "stride_m", "extra_j", "mean_n", "no_eps")
TAIL_PLANTS = ("slab_missing", "slab_twice", "resid_each", "ss_unrounded", "ss_mt")
BUFFER_PLANTS = ("ticket", "outside")


def ordered_sum(vals, path, wv):
    """The kernel's three summation orders over vals [J, M], fp32."""
    J, M = vals.shape

    def seq(rows):
        acc = torch.zeros(M)
        for r in rows:
            acc = acc + vals[r]
        return acc

    if path == "small":      # lane group g sums j = g, g + 4; xor butterflies over the groups
        v = [seq(range(g, J, 4)) for g in range(4)]
        return (v[0] + v[1]) + (v[2] + v[3])
    if path == "wide":       # wave w, group g sums j = 4 w + g + 4 WV q; butterflies, then the waves in order
        per = []
        for w in range(wv):
            v = [seq(range(4 * w + g, J, 4 * wv)) for g in range(4)]
            per.append((v[0] + v[1]) + (v[2] + v[3]))
        return seq_list(per)
    return seq_list([seq(range(w, J, wv)) for w in range(wv)])   # tall: wave w sums j = w + WV q


def seq_list(items):
    acc = torch.zeros_like(items[0])
    for it in items:
        acc = acc + it
    return acc


def emu_scale(c, p, gm, plant=None):
    M, n = c.M, c.ss_n
    stride = M if plant == "stride_m" else c.stride
    flat = p.ssbuf[SS_PRE:].reshape(-1)
    rows = torch.arange(M)
    if plant in ("row+1", "row+16"):
        rows = (rows + int(plant[4:])).clamp(max=M - 1)
    J = n + (1 if plant == "extra_j" else 0)
    vals = flat[torch.arange(J)[:, None] * stride + rows[None, :]]
    if plant == "drop":
        vals = torch.cat([vals[:n // 2], vals[n // 2 + 1:]])
    if plant == "dup_last":
        vals = torch.cat([vals, vals[-1:]])
    tot = ordered_sum(vals, c.path, gm.wv)
    inv = torch.tensor(1.0) / torch.tensor(float(c.N if plant == "mean_n" else c.K))
    t = tot * inv
    if plant != "no_eps":
        t = t + torch.tensor(c.eps, dtype=torch.float32)
    return torch.rsqrt(t)


def emu_resid_tail(c, p, slabs, b, plant=None):
    M, S = c.M, c.S
    cols = c.N // b.tiles
    r0 = p.resid0.float()
    use = list(range(S))
    if plant == "slab_missing":
        use = use[:-1]
    if plant == "slab_twice":
        use.append(S - 1)
    if plant == "resid_each":
        acc = r0
        for s in use:
            acc = (acc + slabs[s]).bfloat16().float()
    else:
        acc = torch.zeros(M, c.N)
        for s in use:
            acc = acc + slabs[s]
        acc = acc + r0
    new = acc.bfloat16()
    src = acc if plant == "ss_unrounded" else new.float()
    q = (src * src).view(M, b.tiles, cols // 4, 4)
    v = ((q[..., 0] + q[..., 1]) + q[..., 2]) + q[..., 3]          # one lane's four columns
    o, lane = cols // 8, torch.arange(cols // 4)
    while o > 0:                                                    # xor butterfly over the row's lanes
        v = v + v[..., lane ^ o]
        o >>= 1
    ss = v[..., 0]                                                  # [M, tiles]
    b.resid.copy_(new)
    if plant == "ss_mt":
        b.ss_out.view(-1).copy_(ss.reshape(-1))
    else:
        b.ss_out.copy_(ss.t())


def emulate(c, p, ops, b, order=0, plant=None):
    """The kernel's arithmetic in plain fp32 PyTorch, written into `b` like a launch: chunks and splits
    as _gemm_ref.emulate (chunk order permuted by seed `order`), the statistics in the path's
    order, the scale per slab, the tails' reduce orders."""
    gm = geom(c.cfg, c.nw, c.M)
    slabs = G.emulate(G.Problem("grid", p.x, p.ys.sum(0), w=p.w), MODE_PARTIAL, c.S, gm.kc, order)
    sc = None
    if c.ss_n:
        sc = emu_scale(c, p, gm, plant)
        if plant != "scale_after_gate":
            slabs = slabs * sc[None, :, None]
    if c.mode == MODE_PARTIAL:
        b.part.copy_(slabs)
    elif c.mode == MODE_BF16:
        b.out.copy_(slabs[0].bfloat16())
    elif c.mode == MODE_SILU:
        use = list(range(c.S))
        if c.S > 1:
            b.part.copy_(slabs)
            if plant == "slab_missing":
                use = use[:-1]
            if plant == "slab_twice":
                use.append(c.S - 1)
        acc = torch.zeros(c.M, c.N)
        for s in use:
            acc = acc + slabs[s]
        v = acc.view(c.M, c.N // 32, 2, 16)
        gt, up = v[:, :, 0], v[:, :, 1]
        o = gt / (1.0 + torch.exp(-gt)) * up
        if plant == "scale_after_gate":
            o = o * sc[:, None, None]
        b.out.copy_(o.reshape(c.M, c.N // 2).bfloat16())
    else:
        b.part.copy_(slabs)
        emu_resid_tail(c, p, slabs, b, plant)
    if plant == "ticket":
        b.counters[b.tiles - 1] = 1
    if plant == "outside":
        flat, n, pad = b.flats[b.primary]
        flat[pad + n] = 0       # the first element of row M


def applies(plant, c):
    """Whether a planted error changes what the kernel of case `c` would compute."""
    if plant in ("row+1", "row+16"):
        return c.ss_n > 0 and c.M > 1
    if plant == "stride_m":
        return c.ss_n > 1 and c.stride > c.M
    if plant == "mean_n":
        return c.ss_n > 0 and c.N != c.K
    if plant == "no_eps":
        return c.ss_n > 0 and c.eps > 0
    if plant == "drop":
        return c.ss_n > 1 and c.mode == MODE_PARTIAL     # (module docstring: one sum of many hides in a bf16)
    if plant == "dup_last":
        return c.ss_n > 0 and c.mode == MODE_PARTIAL
    if plant == "extra_j":
        return c.ss_n > 0
    if plant == "scale_after_gate":
        return c.ss_n > 0 and c.mode == MODE_SILU
    if plant in ("slab_missing", "slab_twice"):
        return c.mode == MODE_RESID or (c.mode == MODE_SILU and c.S > 1)
    if plant == "resid_each":
        return c.mode == MODE_RESID and c.S > 1 and not c.ss_n
    if plant == "ss_unrounded":
        return c.mode == MODE_RESID and not c.ss_n
    if plant == "ss_mt":
        return c.mode == MODE_RESID and c.M > 1
    if plant == "ticket":
        return c.mode == MODE_RESID or (c.mode == MODE_SILU and c.S > 1)
    return plant == "outside"


ALL_PLANTS = SCALE_PLANTS + ("scale_after_gate",) + TAIL_PLANTS + BUFFER_PLANTS


# ---------------------------------------------------------------- 4. producer -> consumer chain
class Chain(NamedTuple):
    cfgA: int
    nwA: int
    SA: int
    nchA: int
    ss_n: int     # A's column tiles
    M: int
    cfgB: int
    nwB: int
    SB: int
    modeB: int
    eps: float
    idx: int

    @property
    def tag(self):
        return (f"chain A cfg{self.cfgA} nw{self.nwA} S{self.SA} tiles{self.ss_n} M{self.M} -> B cfg{self.cfgB} "
                f"nw{self.nwB} S{self.SB} {MODE_NAMES[self.modeB]} eps{self.eps}")


# (producer cfg, nw, S, chunks, tiles, M, consumer cfg, nw, S, mode): ss_n on both sides of 8, up to 64 at
# M > 16, 65 .. 128 at M <= 16; every producer WV in {2, 4, 8} meets consumers of another WV
_CHAINS = (
    (4, 1, 1, 2, 4, 33, 0, 1, 1, MODE_PARTIAL), (4, 1, 3, 3, 12, 64, 7, 2, 1, MODE_SILU),
    (5, 1, 2, 2, 64, 17, 1, 2, 1, MODE_BF16), (10, 1, 1, 1, 128, 16, 9, 1, 4, MODE_PARTIAL),
    (6, 1, 2, 2, 96, 1, 3, 2, 3, MODE_SILU),
    (0, 1, 2, 2, 5, 49, 4, 1, 1, MODE_BF16), (2, 1, 1, 1, 9, 31, 7, 1, 3, MODE_PARTIAL),
    (1, 1, 4, 5, 63, 48, 5, 2, 2, MODE_SILU), (9, 1, 2, 2, 127, 15, 10, 2, 1, MODE_BF16),
    (3, 1, 1, 2, 65, 16, 4, 1, 5, MODE_PARTIAL),
    (7, 1, 2, 3, 7, 63, 4, 2, 2, MODE_PARTIAL), (7, 1, 1, 1, 9, 32, 0, 2, 1, MODE_SILU),
    (7, 1, 3, 3, 64, 47, 6, 1, 1, MODE_BF16), (7, 1, 2, 2, 100, 15, 10, 2, 2, MODE_PARTIAL),
    # N_A a multiple of 1024: also fed from add_partials_resid's and row_sumsq's layouts
    (0, 2, 2, 2, 16, 33, 5, 1, 2, MODE_PARTIAL), (7, 2, 1, 2, 8, 16, 1, 1, 3, MODE_PARTIAL),
)


@functools.lru_cache(maxsize=None)
def chain_cases():
    return tuple(Chain(*row, (0.0, 1e-5)[i % 2], i) for i, row in enumerate(_CHAINS))


@functools.lru_cache(maxsize=4)
def chain_problem(ch: Chain):
    """(case A, problem A, case B, problem B): B's x is A's exact new residual, B's statistics the
    exact sums of its squares (which every layout must deliver)."""
    k = L.kernels()
    gA, gB = geom(ch.cfgA, ch.nwA, ch.M), geom(ch.cfgB, ch.nwB, ch.M)
    assert gA.wv != gB.wv
    M, NA, KA = ch.M, ch.ss_n * gA.cols, ch.nchA * gA.kc
    KB, NB = NA, 2 * gB.cols
    g = gen("m64-chain", *ch)
    cA = Case("chain", ch.cfgA, ch.nwA, MODE_RESID, M, NA, KA, ch.SA, ch.idx % 2, 0, 0, 0.0, ch.idx)
    cB = Case("chain", ch.cfgB, ch.nwB, ch.modeB, M, NB, KB, ch.SB, (ch.idx // 2) % 2, ch.ss_n, M, ch.eps, ch.idx)
    assert k.m64g_supports(M, KA, NA, ch.SA, MODE_RESID, ch.nwA, ch.cfgA), ch.tag
    assert k.m64g_supports(M, KB, NB, ch.SB, ch.modeB, ch.nwB, ch.cfgB), ch.tag
    # A
    pA = EpiProblem()
    jx, jw = G._ints(g, (M, KA), -4, 4), G._ints(g, (NA, KA), -2, 2)
    pA.ys = torch.stack([jx[:, lo * gA.kc:hi * gA.kc] @ jw[:, lo * gA.kc:hi * gA.kc].t()
                         for lo, hi in G.split_ranges(ch.nchA, ch.SA)])
    Y = pA.ys.sum(0)
    V = min(255, math.isqrt((G.EXACT - 1) // NA) - 4)
    t0 = torch.randint(-V, V + 1, (M, NA), generator=g).double()
    pA.resid0 = round_bf16(t0 - Y)
    t = Y + pA.resid0.double()
    assert float((pA.ys.abs().sum(0) + pA.resid0.double().abs()).max()) < G.EXACT
    pA.x, pA.w, pA.sc, pA.ssbuf, pA.note = G._to_bf16(jx), G._to_bf16(jw), torch.ones(M, dtype=torch.float64), None, "chain A"
    pA.want_resid = round_bf16(t)
    r1 = pA.want_resid.double()
    pA.want_ss = (r1 ** 2).view(M, ch.ss_n, gA.cols).sum(-1).t().contiguous()
    pA.ss_exact = True
    sums = (r1 ** 2).sum(1)
    assert float(sums.max()) < G.EXACT       # the whole row: exact however it is split
    # B
    pB = EpiProblem()
    jwB = G._ints(g, (NB, KB), -1, 1)
    assert float((r1.abs() @ jwB.abs().t()).max()) < G.EXACT
    ys = torch.stack([r1[:, lo * gB.kc:hi * gB.kc] @ jwB[:, lo * gB.kc:hi * gB.kc].t()
                      for lo, hi in G.split_ranges(KB // gB.kc, ch.SB)])
    pB.sc = scale64(sums, KB, ch.eps)
    ex = 0
    if ch.modeB == MODE_SILU:
        top = float((pB.sc[:, None] * ys.sum(0)).abs().max())
        ex = max(0, math.ceil(math.log2(max(top, 1.0) / G.SILU_MAX)))
    ys = ys * 2.0 ** -ex
    pB.x, pB.w, pB.ys, pB.note = pA.want_resid, G._to_bf16(jwB * 2.0 ** -ex), ys, "chain B"
    # the statistics in the producer's layout, for the emulation (the GPU run reads A's own ss_out)
    pB.ssbuf = torch.full((SS_PRE + ch.ss_n + SS_POST, M), G.NAN, dtype=torch.float32)
    pB.ssbuf[SS_PRE:SS_PRE + ch.ss_n] = pA.want_ss.float()
    Yb = pB.sc[:, None] * ys.sum(0)
    pB.B = c_of(ch.SB) * U * pB.sc[:, None] * ys.abs().sum(0)
    if ch.modeB == MODE_PARTIAL:
        pB.ref, pB.lim = Yb, pB.B
    elif ch.modeB == MODE_BF16:
        pB.ref, pB.lim = Yb, pB.B + G.BF16_U * (Yb.abs() + pB.B)
    else:
        gp = G.Problem("real", pB.x, Yb, w=pB.w, bound=pB.B)
        pB.ref, pB.lim = gp.silu_ref()[0], gp.real_bound(MODE_SILU)
    return cA, pA, cB, pB
