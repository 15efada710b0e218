"""Inputs, float64 references, checks and the case enumeration of the GEMM tests that can see
ONE wrong element: skinny_gemm (stream and slab variant), gemm_m64g, gemm_w8, gemm_mw, gemm_pf
and gemm_pf_grouped, every entry point called directly through _native.kernels().

tests/test_gemm_exact_gpu.py runs the HIP kernels through run_case / run_grouped below;
tests/test_gemm_refs_cpu.py builds every committed problem (the builders assert their own
exactness conditions), runs a plain fp32 emulation of the kernels' arithmetic through the
same checks, and plants ten kinds of wrong answers that the checks must refuse.

  1. grid: x = jx * 2^-ex, w = jw * 2^-ew with small integers jx, jw. The builder checks
     that sum_k |jx[m,k]| |jw[n,k]| < 2^24 for every (m, n): every bf16 product is then an
     integer below 2^24 in units of 2^-(ex+ew), and so is every partial sum of any subset in
     any order, so fp32 accumulation (any chunk order, split, K rotation, MFMA-internal
     rounding) is exact and equals float64. Three operand pairs: "a" both in [-4, 4]; "b" x
     odd with |x| <= 255 (all 8 significand bits) and w in {-1, 0, 1}; "c" the converse.
     PARTIAL: the fp32 sum of the slabs in slab order equals the reference bit for bit.
     BF16: the output is the one round-to-nearest-even of the exact value. Pair "a" is not
     used here: its sums stay mostly below 2^8, where every integer is a bf16 and nothing
     is rounded; the builder asserts that a quarter of the outputs need rounding and that one
     is an exact tie. SILU: scaled so that max |gate|, |up| <= 16; per element
     |got - ref| <= |ref| (2^-8 + 2^-16 + 2^-24): one bf16 rounding (8 significand bits: half an
     ulp is at most 2^-8 of the value) plus room for the fp32 __expf, divide and multiply (about
     1e-6 at |g| <= 16); no atol, g = 0 or u = 0 gives 0.
  2. one-hot: every x row is a unit vector e_k(m) and w holds random full-mantissa bf16 values
     (or the converse), so out[m, n] = w[n, k(m)] whatever w holds. The hot positions cover the
     first and last k and both sides of every chunk, split and int4-group boundary. For gemm_w8
     the probed codes cover all 254 non-NaN E4M3 codes, all 256 int8 codes, and all 16 nibbles
     in all 8 positions of the packed word.
  3. quantized grid: hand-built codes (int8 -127..127, int4 -8..7, E4M3 values j / 2 with
     |j| <= 16) and power-of-two scales 2^-(r % 7), r random, that differ between neighbouring
     rows (int4: and groups), so a neighbour's scale changes the answer by a factor >= 2 and
     the result stays exact. int4 with x pair "b": the kernel's per-group acc_group =
     sum x (136 + q) is bounded by 255 * 143 * 128 < 2^23 and sum_x by 255 * 128, so both and
     136 * sum_x are exact integers; the builder checks them and the scaled total (it narrows
     the scale range until the total fits 2^24 units of the smallest scale).
  4. real: unit-normal x, 0.02-scaled w, real quantization scales. Per element
     |acc - ref| <= (K + 2) 2^-23 sum_k |x w| (worst case of fp32 accumulation in any order
     and rounding mode; + 1 for the scale multiply of fp8 / int8, and the int4 form below),
     plus one bf16 rounding for the bf16 and SiLU epilogues. Deliberately not tight.

Guards of every launch: x, w (q, scale) are the leading rows of larger allocations whose tail
is NaN (codes: the largest code); part / out are interior slices of sentinel-filled buffers
and everything outside [S, M, N] / [M, cols] must keep the sentinel bit for bit; every case
launches twice into fresh buffers and the two results must be bit-identical.
"""
from __future__ import annotations

import functools
import math
from typing import NamedTuple

import torch

from _row_ref import gen, round_bf16
from xgserve import tune
from xgserve.ops import linear as L

MODE_BF16, MODE_PARTIAL, MODE_SILU = L.MODE_BF16, L.MODE_PARTIAL, L.MODE_SILU
FP8, INT8, INT4 = L.WQ_FP8, L.WQ_INT8, L.WQ_INT4
GROUP = L.WQ_GROUP
MODE_NAMES = {MODE_BF16: "bf16", MODE_PARTIAL: "partial", MODE_SILU: "silu"}
NAN = float("nan")
SENT32, SENT16 = 0x7FC12345, 0x7FC5  # NaN payloads no kernel produces
PAD = 256          # sentinel elements on each side of part / out
TAIL = 8           # poisoned rows behind every operand
TAIL_CODE = {FP8: 0x7E, INT8: 0x7F, INT4: 0xFF}  # 448, 127, (+7, +7)
EXACT = 2 ** 24
# One bf16 rounding: bf16 has 8 significand bits, so a round to nearest moves v by at most half an
# ulp = 2^(e-8) <= 2^-8 |v| at 2^e <= |v| (tests/test_gemm_refs_cpu.py: the plain fp32 formula,
# rounded once, uses 0.99 of it; 2^-9 is the half ulp of a 9-bit significand and a correct path
# exceeds it on a quarter of the elements). Room for the fp32 epilogue (__expf, the divide and the
# multiply at |g| <= 16, about 1e-6 together): 2^-16, and 2^-24 for the product of the two.
BF16_U = 2.0 ** -8
SILU_RTOL = BF16_U + 2.0 ** -16 + 2.0 ** -24
SILU_MAX = 16.0
PAIRS = ("a", "b", "c")

# committed floors on the number of launched cases per family (tests assert len(cases) >= floor)
FLOORS = {"skinny": 280, "m64g": 700, "w8": 300, "mw": 250, "pf": 300, "pf_grouped": 24}


# ---------------------------------------------------------------- cases
class Launch(NamedTuple):
    family: str
    cfg: int      # skinny: 0 the streaming kernel, 1 the slab kernel
    mode: int
    nw: int
    fmt: int
    M: int
    N: int
    K: int
    S: int
    krot: int     # m64g / mw: set_k_rotation(0) or the default; pf: set_pf_krot
    chunk: int    # k per chunk of this configuration
    idx: int      # position within its (cfg, mode, nw, fmt) combination

    @property
    def combo(self):
        return (self.cfg, self.mode, self.nw, self.fmt)

    @property
    def tag(self):
        return (f"{self.family} cfg{self.cfg} {MODE_NAMES[self.mode]} nw{self.nw} fmt{self.fmt} M{self.M} N{self.N} "
                f"K{self.K} S{self.S} krot{self.krot}")


SKINNY_M = (1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128)
M64_M = (1, 15, 16, 17, 31, 32, 33, 47, 48, 49, 63, 64)
MW_M = (1, 63, 64, 65, 128, 129, 192, 193, 256, 257, 319, 320)
SKINNY_WAVES = 4


def pf_rows(bm):
    return (1, bm - 1, bm, bm + 1, 2 * bm + 17, 9 * bm - 5)


def skinny_stage(M):
    """k per stage of the streaming kernel's four waves (KS x 32 per wave; KS = 1 at M > 64)."""
    return SKINNY_WAVES * (32 if M > 64 else 64)


def ks_list(chunk, depth, uneven):
    """(K, S): 1-5 chunks per split, the ring depth + 2, a steady state of 33, each at S = 1, 2;
    S = K / chunk (every split owns one chunk); uneven splits where the family takes them."""
    per = sorted({1, 2, 3, 4, 5, depth + 2, 33})
    out = [(c * S * chunk, S) for c in per for S in (1, 2)]
    out += [(n * chunk, n) for n in (3, 5)]
    if uneven:
        out += [(5 * chunk, 2), (7 * chunk, 3)]
    return out


def _cover(Ms, Ns, KSs, ok, salt):
    """A covering selection of (M, N, K, S): every (K, S), every M and every N appears in at
    least one case that `ok` takes, if any case takes it."""
    picked, seen = [], set()

    def add(c):
        if c is not None and c not in seen:
            seen.add(c)
            picked.append(c)

    def first(cands):
        return next((c for c in cands if ok(*c)), None)

    nM, nN, nK = len(Ms), len(Ns), len(KSs)
    for j, (K, S) in enumerate(KSs):
        add(first((Ms[(5 * j + salt + t) % nM], Ns[(j + u) % nN], K, S) for t in range(nM) for u in range(nN)))
    for i, M in enumerate(Ms):
        if not any(c[0] == M for c in picked):
            add(first((M, Ns[(i + u) % nN], *KSs[(7 * i + salt + t) % nK]) for t in range(nK) for u in range(nN)))
    for i, N in enumerate(Ns):
        if not any(c[1] == N for c in picked):
            add(first((Ms[(i + t) % nM], N, *KSs[(i + v) % nK]) for v in range(nK) for t in range(nM)))
    return picked


def _combo_cases(family, cfg, mode, nw, fmt, Ms, Ns, KSs, ok, chunk):
    sel = _cover(Ms, Ns, KSs, ok, salt=3 * cfg + nw + mode)
    return [Launch(family, cfg, mode, nw, fmt, M, N, K, S, (i // 2) % 2, chunk, i) for i, (M, N, K, S) in enumerate(sel)]


@functools.lru_cache(maxsize=None)
def family_cases(family):
    """Every launched case of a family: cfg x mode x nw x fmt from the library's tables, kept
    iff the library's no-launch predicate takes it."""
    k = L.kernels()
    t = k.gemm_cfgs()
    out = []
    modes = (MODE_BF16, MODE_PARTIAL, MODE_SILU)
    if family == "skinny":
        # no table and no predicate: the shapes are built from the kernel's own units (32-column
        # workgroups, the stage above, skinny_slab_kmax) and every one of them must launch
        for mode in modes:
            def ok(M, N, K, S, mode=mode):
                return mode == MODE_PARTIAL or S == 1
            for M in SKINNY_M:  # the stage depends on M: one covering selection per row count
                st = skinny_stage(M)
                sel = _cover((M,), (32, 96), ks_list(st, 2, False), ok, salt=M + mode)
                # two (K, S) of every three keep the sweep short; every M keeps 1, 2, 33 stages
                sel = [c for i, c in enumerate(sel) if (i + M) % 3 != 2 or c[2] // c[3] // st in (1, 33)]
                out += [Launch(family, 0, mode, 0, 0, M_, N, K, S, 0, st, i) for i, (M_, N, K, S) in enumerate(sel)]
        for mode in (MODE_BF16, MODE_PARTIAL):
            i = 0
            for M in (17, 31, 32, 33, 63, 64):
                kmax = k.skinny_slab_kmax(M)
                for N, S in ((64, 1), (192, 2), (64, 3)):
                    if mode == MODE_PARTIAL or S == 1:
                        out.append(Launch(family, 1, mode, 0, 0, M, N, S * kmax, S, 0, 32, i))
                        i += 1
    elif family == "m64g":
        for cfg, (wv, kc, _nt, ns, _g) in enumerate(t["m64g"]):
            for nw in (1, 2):
                for mode in modes:
                    def ok(M, N, K, S, mode=mode, nw=nw, cfg=cfg):
                        # (the split-K SiLU tail is tests/test_partials_gpu.py's)
                        return k.m64g_supports(M, K, N, S, mode, nw, cfg) and (mode != MODE_SILU or S == 1)
                    cols = 16 * nw * wv
                    out += _combo_cases(family, cfg, mode, nw, 0, M64_M, (cols, 3 * cols), ks_list(kc, ns, True), ok, kc)
    elif family == "w8":
        for cfg, (nw, wv, kc) in enumerate(t["w8"]):
            for fmt in (FP8, INT8, INT4):
                for mode in (MODE_PARTIAL, MODE_SILU):
                    def ok(M, N, K, S, mode=mode, cfg=cfg, fmt=fmt):
                        return k.w8_supports(M, K, N, S, mode, cfg, fmt)
                    cols = 16 * nw * wv
                    out += _combo_cases(family, cfg, mode, 0, fmt, M64_M, (cols, 3 * cols), ks_list(kc, 3, False), ok, kc)
    elif family == "mw":
        for cfg, (cols, d, _nt) in enumerate(t["mw"]):
            for mode in modes:
                def ok(M, N, K, S, mode=mode, cfg=cfg):
                    return k.mw_supports(M, K, N, S, mode, cfg)
                out += _combo_cases(family, cfg, mode, 0, 0, MW_M, (cols, 3 * cols), ks_list(64, d, True), ok, 64)
    elif family == "pf":
        for cfg, (bm, _mtp, _lag, _g) in enumerate(t["pf"]):
            for mode in modes:
                def ok(M, N, K, S, mode=mode, cfg=cfg):
                    return k.pf_supports(M, K, N, S, mode, cfg)
                out += _combo_cases(family, cfg, mode, 0, 0, pf_rows(bm), (256, 768), ks_list(64, 2, True), ok, 64)
    else:
        raise KeyError(family)
    return tuple(out)


def accepted_combos(family):
    """Every (cfg, mode, nw, fmt) that the family's predicate takes at ANY listed shape."""
    return {c.combo for c in family_cases(family)} | _accepted_anywhere(family)


@functools.lru_cache(maxsize=None)
def _accepted_anywhere(family):
    """The same set, found by brute force over the listed shapes (not through _cover)."""
    k = L.kernels()
    t = k.gemm_cfgs()
    got = set()
    modes = (MODE_BF16, MODE_PARTIAL, MODE_SILU)
    if family == "m64g":
        for cfg, (wv, kc, _nt, ns, _g) in enumerate(t["m64g"]):
            for nw in (1, 2):
                for mode in modes:
                    if any(k.m64g_supports(M, K, N, S, mode, nw, cfg) and (mode != MODE_SILU or S == 1)
                           for M in M64_M for N in (16 * nw * wv, 48 * nw * wv) for K, S in ks_list(kc, ns, True)):
                        got.add((cfg, mode, nw, 0))
    elif family == "w8":
        for cfg, (nw, wv, kc) in enumerate(t["w8"]):
            for fmt in (FP8, INT8, INT4):
                for mode in modes:
                    if any(k.w8_supports(M, K, N, S, mode, cfg, fmt)
                           for M in M64_M for N in (16 * nw * wv, 48 * nw * wv) for K, S in ks_list(kc, 3, False)):
                        got.add((cfg, mode, 0, fmt))
    elif family == "mw":
        for cfg, (cols, d, _nt) in enumerate(t["mw"]):
            for mode in modes:
                if any(k.mw_supports(M, K, N, S, mode, cfg)
                       for M in MW_M for N in (cols, 3 * cols) for K, S in ks_list(64, d, True)):
                    got.add((cfg, mode, 0, 0))
    elif family == "pf":
        for cfg, (bm, _mtp, _lag, _g) in enumerate(t["pf"]):
            for mode in modes:
                if any(k.pf_supports(M, K, N, S, mode, cfg)
                       for M in pf_rows(bm) for N in (256, 768) for K, S in ks_list(64, 2, True)):
                    got.add((cfg, mode, 0, 0))
    return frozenset(got)


def onehot_cases(family):
    """The cases that also run section 2: one in four of every combination, short K (the hot
    positions are two per chunk boundary) -- always including the combination's first. gemm_w8 runs
    its codes through the fp32 partials only (the mode is a run-time argument of one kernel, and the
    smallest E4M3 codes times the scales leave the range where the SiLU bound has no atol)."""
    if family == "skinny":  # (k steps of 32 inside a stage: short K; every slab case of S <= 2)
        return [c for c in family_cases(family) if c.K <= 2048 and (c.idx % 4 == 0 or c.cfg == 1)]
    return [c for c in family_cases(family) if c.K // c.chunk <= 12 and (c.idx % 4 == 0 or c.S == c.K // c.chunk)
            and (family != "w8" or (c.mode == MODE_PARTIAL and c.M >= 15))]  # (a round probes M positions)


# ---------------------------------------------------------------- problems
class Problem:
    """CPU operands of one (section, M, N, K) and the exact float64 product y [M, N]."""

    def __init__(self, kind, x, y, w=None, q=None, scale=None, fmt=None, bound=None, note=""):
        self.kind, self.x, self.w, self.q, self.scale, self.fmt, self.y, self.bound = kind, x, w, q, scale, fmt, y, bound
        self.note = note
        self.M, self.K = x.shape
        self.N = y.shape[1]
        self.exact = kind != "real"

    # what each mode must produce
    def want_partial(self):
        w32 = self.y.float()
        assert torch.equal(w32.double(), self.y), "the exact value is not an fp32"
        return w32

    def want_bf16(self):
        return round_bf16(self.y)

    def silu_ref(self, y=None):
        y = self.y if y is None else y
        v = y.view(y.shape[0], self.N // 32, 2, 16)
        g, u = v[:, :, 0], v[:, :, 1]
        return (g / (1.0 + torch.exp(-g)) * u).reshape(y.shape[0], self.N // 2), g, u

    def real_bound(self, mode):
        """Section 4's per-element bound for `mode` (float64 [M, cols])."""
        B = self.bound
        if mode == MODE_PARTIAL:
            return B
        if mode == MODE_BF16:
            return B + BF16_U * (self.y.abs() + B)
        ref, g, u = self.silu_ref()
        v = B.view(self.M, self.N // 32, 2, 16)
        Bg, Bu = v[:, :, 0], v[:, :, 1]
        # |d silu / dg| <= 1.1 and |silu(g)| <= |g|: first order in each operand, the cross term, the fp32
        # epilogue (2^-16 of the value, as in section 1) and one bf16 rounding of the erroneous value
        e = 1.1 * Bg * (u.abs() + Bu) + (g.abs() + Bg) * Bu
        e = e.reshape(self.M, self.N // 2)
        return e + SILU_RTOL * (ref.abs() + e)


def _ints(g, shape, lo, hi):
    return torch.randint(lo, hi + 1, shape, generator=g).double()


def _odd255(g, shape):
    return (2 * torch.randint(0, 128, shape, generator=g) + 1).double() * (2 * torch.randint(0, 2, shape, generator=g) - 1)


def _pair(pair, g, M, N, K):
    if pair == "a":
        return _ints(g, (M, K), -4, 4), _ints(g, (N, K), -4, 4)
    if pair == "b":
        return _odd255(g, (M, K)), _ints(g, (N, K), -1, 1)
    return _ints(g, (M, K), -1, 1), _odd255(g, (N, K))


def _to_bf16(v64):
    b = v64.float().bfloat16()
    assert torch.equal(b.double(), v64), "grid value is not a bf16"
    return b


def bf16_rounding_stats(y):
    """(share of y that is not a bf16, number of exact ties) -- y float64."""
    b = y.contiguous().view(torch.int64)
    drop = 52 - 7
    rem = b & ((1 << drop) - 1)
    nz = y != 0
    return float(((rem != 0) & nz).double().mean()), int(((rem == (1 << (drop - 1))) & nz).sum())


@functools.lru_cache(maxsize=256)
def grid_problem(pair, M, N, K, mode):
    """Section 1. The same integers serve PARTIAL and BF16; SILU scales them to |g|, |u| <= 16."""
    for attempt in range(64):  # BF16: redrawn until the rounding is exercised (few outputs, wide ulps)
        g = gen("gemm-grid", pair, M, N, K, attempt)
        jx, jw = _pair(pair, g, M, N, K)
        y = jx @ jw.t()  # exact: integers below 2^24
        if mode != MODE_BF16 or (bf16_rounding_stats(y)[0] >= 0.25 and bf16_rounding_stats(y)[1] >= 1):
            break
    units = jx.abs() @ jw.abs().t()
    assert float(units.max()) < EXACT, (pair, M, N, K, float(units.max()))
    ex = 0
    if mode == MODE_SILU:
        ex = max(0, math.ceil(math.log2(max(float(y.abs().max()), 1.0) / SILU_MAX)))
        y = y * 2.0 ** -ex
        assert float(y.abs().max()) <= SILU_MAX
    if mode == MODE_BF16:
        share, ties = bf16_rounding_stats(y)
        assert share >= 0.25 and ties >= 1, (pair, M, N, K, share, ties)
    # the power of two goes on the operand with the small integers
    sx, sw = (2.0 ** -ex, 1.0) if pair != "b" else (1.0, 2.0 ** -ex)
    return Problem("grid", _to_bf16(jx * sx), y, w=_to_bf16(jw * sw), note=pair)


def grid_pair(c: Launch):
    """The operand pair of a case: a rotation; BF16 takes "b" and "c" only (module docstring)."""
    return ("b", "c")[c.idx % 2] if c.mode == MODE_BF16 else PAIRS[(c.idx + c.cfg) % 3]


def rand_bf16(g, shape):
    """Random sign, random 7-bit mantissa, exponents 2^-8 .. 2^3: |v| < 16, normal, finite."""
    man = torch.randint(0, 128, shape, generator=g)
    exp = torch.randint(119, 131, shape, generator=g)
    sgn = torch.randint(0, 2, shape, generator=g)
    b = ((sgn << 15) | (exp << 7) | man).to(torch.int32)
    b = torch.where(b >= 32768, b - 65536, b).to(torch.int16)
    return b.view(torch.bfloat16)


def hot_positions(c: Launch):
    """The k every one-hot case must probe: first, last, both sides of every chunk boundary
    (split boundaries are chunk boundaries: even splits of whole chunks, or the uneven
    s * nch / S ranges), of every int4 group boundary, and for gemm_w8 the first and last 8 k
    (every position of a packed int4 word)."""
    K = c.K
    pos = {0, K - 1}
    step = 32 if c.family == "skinny" else c.chunk  # skinny: every MFMA k step (waves split a stage by 64 / 32)
    for b in range(step, K, step):
        pos |= {b - 1, b}
    if c.family == "w8":
        for b in range(GROUP, K, GROUP):
            pos |= {b - 1, b}
        pos |= set(range(8)) | set(range(K - 8, K))
    return tuple(sorted(pos))


def onehot_rounds(c: Launch, side):
    n = len(hot_positions(c))
    rows = c.M if side == "x" else c.N
    r = -(-n // rows)
    return r if (side == "w" or c.family == "w8") else min(r, 3)


@functools.lru_cache(maxsize=64)
def onehot_problem(c: Launch, side, rnd):
    """Section 2 (bf16 weights): side "x": x rows e_k(m), w random; side "w": the converse."""
    pos = hot_positions(c)
    g = gen("gemm-onehot", side, rnd, c.M, c.N, c.K)
    M, N, K = c.M, c.N, c.K

    def hot(i):
        # every run of len(pos) rows covers every position; the shift per run keeps the pattern from
        # repeating with a tile (two column tiles with equal hot k would hide their swap)
        return pos[(i + 3 * (i // len(pos))) % len(pos)]

    if side == "x":
        km = torch.tensor([hot(rnd * M + m) for m in range(M)])
        x = torch.zeros(M, K, dtype=torch.bfloat16)
        x[torch.arange(M), km] = 1.0
        w = rand_bf16(g, (N, K))
        y = w[:, km].double().t().contiguous()
    else:
        kn = torch.tensor([hot(rnd * N + n) for n in range(N)])
        w = torch.zeros(N, K, dtype=torch.bfloat16)
        w[torch.arange(N), kn] = 1.0
        x = rand_bf16(g, (M, K))
        y = x[:, kn].double().contiguous()
    p = Problem("onehot", x, y, w=w, note=side)
    p.probed = set(km.tolist()) if side == "x" else set(kn.tolist())
    return p


# ---------------------------------------------------------------- quantized weights
FP8_GRID = tuple(j / 2 for j in range(-16, 17))
MAXCODE = {FP8: 16, INT8: 127, INT4: 8}   # in units of the code grid (fp8: halves)


def pack_int4(codes):
    """int codes -8..7 [N, K] -> packed uint8 [N, K / 2]: offset binary u = q + 8, a 32-bit word
    holds 8 consecutive k, element 2j at bits 4j and element 2j + 1 at bits 16 + 4j."""
    N, K = codes.shape
    u = (codes.to(torch.int64) + 8).view(N, K // 8, 4, 2)
    word = torch.zeros(N, K // 8, dtype=torch.int64)
    for j in range(4):
        word |= u[:, :, j, 0] << (4 * j)
        word |= u[:, :, j, 1] << (16 + 4 * j)
    by = torch.stack([(word >> (8 * i)) & 255 for i in range(4)], dim=-1)  # little endian
    return by.to(torch.uint8).view(N, K // 2).contiguous()


def encode(vals, fmt):
    """Code VALUES (fp8: multiples of 1/2 up to 8 in magnitude, or any E4M3 value; int8 / int4:
    integers) -> the uint8 codes the kernel reads."""
    if fmt == FP8:
        q = vals.float().to(torch.float8_e4m3fn)
        assert torch.equal(q.float().double(), vals.double())
        return q.view(torch.uint8).contiguous()
    if fmt == INT8:
        return vals.to(torch.int8).view(torch.uint8).contiguous()
    return pack_int4(vals)


def decode64(q, fmt):
    """uint8 codes -> float64 code values [N, K] (the package's dequantizer at scale 1)."""
    N = q.shape[0]
    G = q.shape[1] * 2 // GROUP if fmt == INT4 else 0
    one = torch.ones(G, N) if fmt == INT4 else torch.ones(N)
    return L.dequantize_weight(q, one, fmt).double()


def scale_matrix(scale, fmt, K):
    """[N, K] float64 of the scale that applies to each weight element."""
    if fmt == INT4:
        return scale.double().t().repeat_interleave(GROUP, dim=1)
    return scale.double()[:, None].expand(-1, K)


def pow2_scales(g, fmt, N, K, smod):
    """2^-e with e in 0 .. smod - 1 a random walk of non-zero steps along the rows (int4: the sum of
    one walk along the rows and one along the groups), so neighbours always differ."""
    def walk(n):
        return torch.cumsum(torch.randint(1, smod, (n,), generator=g), 0)

    e = walk(N) % smod if fmt != INT4 else (walk(N)[None, :] + walk(K // GROUP)[:, None]) % smod
    return (2.0 ** -e.double()).float().contiguous()


def quant_x_kinds(fmt, K):
    """x pair "b" (odd, |x| <= 255) wherever the WORST case 255 * max|code| * K fits 2^24 (fp8 / int8:
    the accumulator holds sum x q before the scale); int4 always (per group, see the builder)."""
    return ("a", "b") if fmt == INT4 or 255 * MAXCODE[fmt] * K < EXACT else ("a",)


@functools.lru_cache(maxsize=256)
def quant_problem(fmt, xkind, M, N, K, mode):
    """Section 3."""
    g = gen("gemm-quant", fmt, xkind, M, N, K)
    jx = _ints(g, (M, K), -4, 4) if xkind == "a" else _odd255(g, (M, K))
    if fmt == FP8:
        codes = _ints(g, (N, K), -16, 16) / 2
    elif fmt == INT8:
        codes = _ints(g, (N, K), -127, 127)
    else:
        codes = _ints(g, (N, K), -8, 7)
    ax, ac = jx.abs(), codes.abs()
    if fmt != INT4:
        assert float((ax @ ac.t()).max()) * (2 if fmt == FP8 else 1) < EXACT  # the kernel's accumulator
    else:
        # the kernel's per-group acc_group = sum x (136 + q), sum_x, and 136 sum_x: exact integers
        for k0 in range(0, K, GROUP):
            sx = ax[:, k0:k0 + GROUP].sum(1)
            assert float((ax[:, k0:k0 + GROUP] @ (136 + codes[:, k0:k0 + GROUP]).abs().t()).max()) < EXACT
            assert 136 * float(sx.max()) < EXACT
    for smod in (7, 4, 2):
        scale = pow2_scales(gen("gemm-scale", fmt, N, K, smod), fmt, N, K, smod)
        sm = scale_matrix(scale, fmt, K)
        # every partial sum of the scaled products, in units of the smallest scale
        total = float((ax @ (ac * sm).t()).max()) / float(sm.min()) * (2 if fmt == FP8 else 1)
        if total < EXACT:
            break
    assert total < EXACT, (fmt, xkind, M, N, K, total)
    y = jx @ (codes * sm).t()
    ex = 0
    if mode == MODE_SILU:
        ex = max(0, math.ceil(math.log2(max(float(y.abs().max()), 1.0) / SILU_MAX)))
        y = y * 2.0 ** -ex
    q = encode(codes, fmt)
    assert torch.equal(decode64(q, fmt), codes)
    p = Problem("quant", _to_bf16(jx * 2.0 ** -ex), y, q=q, scale=scale, fmt=fmt, note=f"{xkind} smod{smod}")
    p.codes, p.smod = codes, smod
    return p


def quant_xkind(c: Launch):
    kinds = quant_x_kinds(c.fmt, c.K)
    return kinds[(c.idx + c.cfg) % len(kinds)]


def all_codes(fmt):
    if fmt == FP8:
        return [b for b in range(256) if b & 0x7F != 0x7F]   # 254: 0x7F / 0xFF are the NaNs
    return list(range(256)) if fmt == INT8 else list(range(16))


@functools.lru_cache(maxsize=64)
def codes_problem(c: Launch, rnd):
    """Section 2 for gemm_w8: x rows e_k(m) (value 1), so out[m, n] = decode(q[n, k(m)]) * scale;
    the codes at the probed k walk through every code of the format (int4: every nibble at every
    probed k, and the probed k include all 8 positions of a packed word)."""
    fmt, M, N, K = c.fmt, c.M, c.N, c.K
    pos = hot_positions(c)
    g = gen("gemm-codes", fmt, rnd, M, N, K)
    table = all_codes(fmt)
    km = torch.tensor([pos[(rnd * M + m) % len(pos)] for m in range(M)])
    x = torch.zeros(M, K, dtype=torch.bfloat16)
    x[torch.arange(M), km] = 1.0
    nn = torch.arange(N)
    if fmt == INT4:
        u = torch.randint(0, 16, (N, K), generator=g)
        for i, kk in enumerate(pos):
            u[:, kk] = (nn + 5 * i) % 16
        q = pack_int4(u - 8)
        probed = {(kk % 8, int(v)) for kk in set(km.tolist()) for v in u[:, kk].tolist()}
    else:
        raw = torch.tensor(table)[torch.randint(0, len(table), (N, K), generator=g)]
        for i, kk in enumerate(pos):
            raw[:, kk] = torch.tensor(table)[(nn + N * i) % len(table)]
        q = raw.to(torch.uint8).contiguous()
        probed = {int(v) for kk in set(km.tolist()) for v in raw[:, kk].tolist()}
    scale = pow2_scales(gen("gemm-scale", fmt, N, K, 7), fmt, N, K, 7)
    vals = decode64(q, fmt) * scale_matrix(scale, fmt, K)
    y = vals[:, km].t().contiguous()
    p = Problem("onehot", x, y, q=q, scale=scale, fmt=fmt, note="codes")
    p.probed = probed
    return p


def codes_rounds(c: Launch):
    return -(-len(hot_positions(c)) // c.M)


# ---------------------------------------------------------------- real-valued inputs
@functools.lru_cache(maxsize=32)
def real_problem(M, N, K, fmt=None):
    """Section 4: unit-normal x, 0.02-scaled w (quantized with the package's quantizer: real
    scales). bound = the fp32 accumulation's worst case, per element."""
    g = gen("gemm-real", M, N, K, fmt)
    x = torch.randn(M, K, generator=g).bfloat16()
    w = (torch.randn(N, K, generator=g) * 0.02).bfloat16()
    u = 2.0 ** -23
    if fmt is None:
        y = x.double() @ w.double().t()
        return Problem("real", x, y, w=w, bound=(K + 2) * u * (x.double().abs() @ w.double().abs().t()))
    q, scale = L.quantize_weight(w, fmt)
    codes, sm = decode64(q, fmt), scale_matrix(scale, fmt, K)
    y = x.double() @ (codes * sm).t()
    ax = x.double().abs()
    if fmt != INT4:
        bound = (K + 3) * u * (ax @ (codes * sm).abs().t())  # + the scale multiply
    else:
        # per group: acc_group and sum_x carry (128 + 2) u of sum |x| (136 + q) and of 136 sum |x| (the
        # cancelling terms), times the scale; the outer sum over G groups adds (G + 2) u of the terms
        inner = ax @ (((136 + codes).abs() + 136) * sm).t()
        bound = (GROUP + 2) * u * inner + (K // GROUP + 2) * u * (ax @ (codes * sm).abs().t() + (GROUP + 2) * u * inner)
    return Problem("real", x, y, q=q, scale=scale, fmt=fmt, bound=bound)


REAL_SHAPES = {  # family -> [(Launch fields without idx)]: one or two shapes, every mode the cfg takes
    "skinny": [("skinny", 0, 0, 0, 16, 96, 1024, 2), ("skinny", 1, 0, 0, 33, 64, 2048, 2), ("skinny", 0, 0, 0, 128, 32, 512, 1)],
    "m64g": [("m64g", 3, 2, 0, 64, 384, 1024, 3), ("m64g", 9, 2, 0, 16, 384, 1024, 2)],
    "w8": [("w8", 0, 0, FP8, 48, 384, 1024, 2), ("w8", 1, 0, INT8, 33, 192, 1024, 2), ("w8", 3, 0, INT4, 16, 192, 1024, 2)],
    "mw": [("mw", 1, 0, 0, 193, 384, 1024, 3), ("mw", 6, 0, 0, 129, 256, 512, 2)],
    "pf": [("pf", 2, 0, 0, 273, 768, 1024, 3), ("pf", 6, 0, 0, 300, 256, 512, 2)],
}


def real_cases(family):
    out = []
    for fam, cfg, nw, fmt, M, N, K, S in REAL_SHAPES[family]:
        chunk = 64
        for mode in (MODE_BF16, MODE_PARTIAL, MODE_SILU):
            if fam == "w8" and mode == MODE_BF16:
                continue
            if fam == "skinny" and cfg == 1 and mode == MODE_SILU:
                continue
            out.append(Launch(fam, cfg, mode, nw, fmt, M, N, K, S if mode == MODE_PARTIAL else 1, 1, chunk, len(out)))
    return out


# ---------------------------------------------------------------- checks (CPU or GPU tensors)
def ibits(t):
    return t.contiguous().view({2: torch.int16, 4: torch.int32}[t.element_size()])


def slab_sum(part):
    acc = part[0].clone()
    for s in range(1, part.shape[0]):
        acc += part[s]
    return acc


def check_partial(part, want32, tag=""):
    """No slab element keeps the sentinel; the fp32 slab-order sum equals the exact value."""
    assert not bool((ibits(part) == SENT32).any()), f"{tag}: a slab element was never written"
    got = slab_sum(part)
    if not torch.equal(got, want32):
        bad = (got != want32) | torch.isnan(got)
        i = bad.nonzero()[0].tolist()
        raise AssertionError(f"{tag}: {int(bad.sum())} of {bad.numel()} sums differ from the exact value, first at "
                             f"{i}: {float(got[tuple(i)])} vs {float(want32[tuple(i)])}")


def check_bf16(out, want, tag=""):
    """The one round-to-nearest-even of the exact value (+0 and -0 compare equal)."""
    assert not bool((ibits(out) == SENT16).any()), f"{tag}: an output element was never written"
    if not torch.equal(out, want):
        bad = (out != want) | torch.isnan(out)
        i = bad.nonzero()[0].tolist()
        raise AssertionError(f"{tag}: {int(bad.sum())} of {bad.numel()} outputs are not the rounded exact value, first "
                             f"at {i}: {float(out[tuple(i)])} vs {float(want[tuple(i)])}")


def share_used(got, ref64, lim64):
    d = (got.double() - ref64).abs()
    return float(torch.where(d == 0, torch.zeros_like(d), d / lim64.clamp_min(1e-300)).max())


def check_bound(got, ref64, lim64, tag=""):
    """|got - ref| <= lim per element (NaN fails); returns the largest share of the bound used."""
    assert not bool((ibits(got) == (SENT16 if got.element_size() == 2 else SENT32)).any()), f"{tag}: never written"
    d = (got.double() - ref64).abs()
    ok = d <= lim64
    if not bool(ok.all()):
        i = (~ok).nonzero()[0].tolist()
        raise AssertionError(f"{tag}: {int((~ok).sum())} of {ok.numel()} elements miss the bound, first at {i}: "
                             f"{float(got[tuple(i)])} vs {float(ref64[tuple(i)])}, bound {float(lim64[tuple(i)])}")
    return share_used(got, ref64, lim64)


def check_silu(out, ref64, tag=""):
    return check_bound(out, ref64, ref64.abs() * SILU_RTOL, tag)


class Want:
    """A problem's expectations for one mode, on a device, made once per (problem, mode)."""

    def __init__(self, p: Problem, mode, dev):
        self.mode, self.exact = mode, p.exact
        if p.exact:
            if mode == MODE_PARTIAL:
                self.want = p.want_partial().to(dev)
            elif mode == MODE_BF16:
                self.want = p.want_bf16().to(dev)
            else:
                self.ref = p.silu_ref()[0].to(dev)
        else:
            self.ref = (p.silu_ref()[0] if mode == MODE_SILU else p.y).to(dev)
            self.lim = p.real_bound(mode).to(dev)

    def check(self, res, tag):
        """res: part [S, M, N] or out [M, cols]; returns the share of a bound used (0 if exact)."""
        if not self.exact:
            return check_bound(slab_sum(res) if self.mode == MODE_PARTIAL else res, self.ref, self.lim, tag)
        if self.mode == MODE_PARTIAL:
            check_partial(res, self.want, tag)
        elif self.mode == MODE_BF16:
            check_bf16(res, self.want, tag)
        else:
            return check_silu(res, self.ref, tag)
        return 0.0


# ---------------------------------------------------------------- guarded buffers
def guarded(shape, dtype, dev, pad=PAD):
    """(whole sentinel-filled buffer, its interior view of `shape`); `pad` sentinels on each side."""
    n = math.prod(shape)
    it, sent = (torch.int32, SENT32) if dtype == torch.float32 else (torch.int16, SENT16)
    flat = torch.full((n + 2 * pad,), sent, dtype=it, device=dev)
    return flat, flat[pad:pad + n].view(dtype).view(shape)


def guards_intact(flat, n, pad=PAD):
    sent = SENT32 if flat.dtype == torch.int32 else SENT16
    return bool((flat[:pad] == sent).all()) and bool((flat[pad + n:] == sent).all())


def with_tail(t, dev, code=None):
    """t as the leading rows of a larger allocation whose tail rows are NaN (uint8: `code`)."""
    tail = torch.full((TAIL,) + tuple(t.shape[1:]), NAN if code is None else code, dtype=t.dtype)
    buf = torch.cat([t, tail]).to(dev)
    return buf[:t.shape[0]]


class DeviceOperands:
    def __init__(self, p: Problem, dev):
        self.x = with_tail(p.x, dev)
        if p.q is None:
            self.w, self.scale = with_tail(p.w, dev), None
        else:
            self.w = with_tail(p.q, dev, TAIL_CODE[p.fmt])
            if p.fmt == INT4:
                self.scale = with_tail(p.scale, dev)       # [G, N]: NaN groups behind the last
            else:
                self.scale = with_tail(p.scale[:, None], dev)  # [N, 1] rows -> N floats + NaN
        assert self.x.is_contiguous() and self.w.is_contiguous()


def out_shape(c: Launch):
    if c.mode == MODE_PARTIAL:
        return (c.S, c.M, c.N), torch.float32
    return (c.M, c.N // 2 if c.mode == MODE_SILU else c.N), torch.bfloat16


def native_launch(k, c: Launch, ops: DeviceOperands, res, st):
    part = res.data_ptr() if c.mode == MODE_PARTIAL else 0
    out = 0 if c.mode == MODE_PARTIAL else res.data_ptr()
    x, w = ops.x.data_ptr(), ops.w.data_ptr()
    if c.family == "skinny":
        k.skinny_gemm(x, c.M, c.K, w, c.N, part, out, c.S, c.mode, st)
    elif c.family == "m64g":
        k.gemm_m64g(x, c.M, c.K, w, c.N, part, out, c.S, c.mode, c.nw, c.cfg, st)
    elif c.family == "w8":
        k.gemm_w8(x, c.M, c.K, w, ops.scale.data_ptr(), c.N, part, out, c.S, c.mode, c.cfg, st, c.fmt)
    elif c.family == "mw":
        k.gemm_mw(x, c.M, c.K, w, c.N, part, out, c.S, c.mode, c.cfg, st)
    else:
        k.gemm_pf(x, c.M, c.K, w, c.N, part, out, c.S, c.mode, c.cfg, st)


def set_rotation(k, c: Launch):
    if c.family in ("m64g", "mw"):
        k.set_k_rotation(tune.get_int("krot", 1) if c.krot else 0)
    elif c.family == "pf":
        k.set_pf_krot(c.krot)


def restore_rotation(k):
    k.set_k_rotation(tune.get_int("krot", 1))
    k.set_pf_krot(0)


def run_case(k, c: Launch, p: Problem, dev, st, cache=None):
    """Two launches of `c` on `p` into fresh guarded buffers: the mode's check, the guards, and
    bit-identical results. Returns the share of a bound used."""
    assert (p.M, p.N, p.K) == (c.M, c.N, c.K)
    key = (id(p), c.mode)
    if cache is not None and key in cache:
        ops, want, _ = cache[key]
    else:
        ops, want = DeviceOperands(p, dev), Want(p, c.mode, dev)
        if cache is not None:
            if len(cache) > 64:
                cache.clear()
            cache[key] = (ops, want, p)  # (p: its id stays its own while the entry lives)
    set_rotation(k, c)
    shape, dtype = out_shape(c)
    n = math.prod(shape)
    first, used = None, 0.0
    for rep in range(2):
        flat, res = guarded(shape, dtype, dev)
        native_launch(k, c, ops, res, st)
        used = want.check(res, f"{c.tag} [{p.kind} {p.note}] launch {rep}")
        assert guards_intact(flat, n), f"{c.tag}: wrote outside its output"
        if first is None:
            first = flat
        else:
            assert torch.equal(first, flat), f"{c.tag}: two launches differ"
    return used


# ---------------------------------------------------------------- gemm_pf_grouped
GROUPED_E = 4
GROUPED_PAD_TILES = 2   # capacity past offs[E]: never written


class GroupedLayout:
    """A moe_align layout built by hand: expert-sorted rows, every segment padded to 64; one
    empty expert, segments shorter than, equal to and longer than the tile height BM."""

    def __init__(self, bm, g):
        self.real = (40, 0, bm, 2 * bm + 70)
        self.T = sum(self.real)
        src = torch.randperm(self.T, generator=g).tolist()
        offs, rows = [0], []
        for n in self.real:
            seg = -(-n // 64) * 64
            rows += src[:n] + [-1] * (seg - n)
            src = src[n:]
            offs.append(offs[-1] + seg)
        self.end = offs[-1]
        self.P = self.end + 64 * GROUPED_PAD_TILES
        rows += [-1] * (self.P - self.end)
        self.rows = torch.tensor(rows, dtype=torch.int32)
        self.offs = torch.tensor(offs, dtype=torch.int32)
        self.real_idx = (self.rows >= 0).nonzero()[:, 0]
        self.expert_of = torch.zeros(self.P, dtype=torch.long)
        for e in range(GROUPED_E):
            self.expert_of[offs[e]:offs[e + 1]] = e


class GroupedProblem:
    """Grid inputs (pair by expert) and the float64 reference per expert, real rows only."""

    def __init__(self, bm, N, K, mode, pair):
        g = gen("gemm-grouped", bm, N, K, pair)
        lay = self.lay = GroupedLayout(bm, g)
        self.N, self.K, self.mode = N, K, mode
        jx, jw = _pair(pair, g, lay.T, GROUPED_E * N, K)
        jw = jw.view(GROUPED_E, N, K)
        real = lay.rows >= 0
        src = lay.rows[real].long()
        eo = lay.expert_of[real]
        y = torch.zeros(lay.T, N, dtype=torch.float64)  # in padded-row order of the real rows
        for e in range(GROUPED_E):
            sel = eo == e
            if bool(sel.any()):
                assert float((jx[src[sel]].abs() @ jw[e].abs().t()).max()) < EXACT
                y[sel] = jx[src[sel]] @ jw[e].t()
        ex = 0
        if mode == MODE_SILU:
            ex = max(0, math.ceil(math.log2(max(float(y.abs().max()), 1.0) / SILU_MAX)))
            y = y * 2.0 ** -ex
        sx, sw = (2.0 ** -ex, 1.0) if pair != "b" else (1.0, 2.0 ** -ex)
        self.x = _to_bf16(jx * sx)                                   # [T, K]: the gathered form
        self.xp = _to_bf16(_pair(pair, g, lay.P, 1, K)[0] * sx)      # [P, K]: already sorted; pads finite
        self.xp[real] = self.x[src]
        self.w = _to_bf16(jw * sw)
        self.p = Problem("grid", self.x[:1], y, w=self.w[0], note=f"grouped {pair}")  # (y and the mode's wants)
        self.p.M = lay.T


def grouped_cases():
    """(cfg, mode, S, gathered, N, K): every grouped cfg x mode x S x rows form the predicate takes."""
    k = L.kernels()
    out = []
    for cfg, (bm, _mtp, _lag, grouped) in enumerate(k.gemm_cfgs()["pf"]):
        if not grouped:
            continue
        lay = GroupedLayout(bm, gen("probe"))
        i = 0
        for mode in (MODE_BF16, MODE_PARTIAL, MODE_SILU):
            for S in (1, 2):
                for gathered in (True, False):
                    N, K = ((256, 320), (768, 128), (256, 192))[i % 3]
                    if k.pf_grouped_supports(GROUPED_E, lay.P, K, N, lay.T, S, mode, cfg):
                        out.append((cfg, mode, S, gathered, N, K))
                        i += 1
    return out


def run_grouped(k, case, dev, st):
    cfg, mode, S, gathered, N, K = case
    bm = k.gemm_cfgs()["pf"][cfg][0]
    gp = GroupedProblem(bm, N, K, mode, PAIRS[(cfg + S + int(gathered)) % 3])
    lay = gp.lay
    tag = f"pf_grouped cfg{cfg} {MODE_NAMES[mode]} S{S} gathered{gathered} N{N} K{K}"
    x = with_tail(gp.x if gathered else gp.xp, dev)
    w = with_tail(gp.w.view(GROUPED_E * N, K), dev)
    rows, offs = lay.rows.to(dev), lay.offs.to(dev)
    want = Want(gp.p, mode, dev)
    ridx = lay.real_idx.to(dev)
    cols = N // 2 if mode == MODE_SILU else N
    shape, dtype = ((S, lay.P, N), torch.float32) if mode == MODE_PARTIAL else ((lay.P, cols), torch.bfloat16)
    sent = SENT32 if mode == MODE_PARTIAL else SENT16
    first = None
    k.set_pf_krot(0)
    for rep in range(2):
        flat, res = guarded(shape, dtype, dev)
        k.gemm_pf_grouped(x.data_ptr(), rows.data_ptr() if gathered else 0, offs.data_ptr(), GROUPED_E, lay.P, K,
                          w.data_ptr(), N, lay.T, res.data_ptr() if mode == MODE_PARTIAL else 0,
                          0 if mode == MODE_PARTIAL else res.data_ptr(), S, mode, cfg, st)
        want.check(res.index_select(-2, ridx), f"{tag} launch {rep}")
        assert guards_intact(flat, math.prod(shape)), f"{tag}: wrote outside its output"
        assert bool((ibits(res[..., lay.end:, :]) == sent).all()), f"{tag}: wrote a capacity row past offs[E]"
        if first is None:
            first = flat
        else:
            assert torch.equal(first, flat), f"{tag}: two launches differ"


# ---------------------------------------------------------------- fp32 emulation (CPU)
def split_ranges(nch, S):
    return [(s * nch // S, (s + 1) * nch // S) for s in range(S)]


def emulate(p: Problem, mode, S, chunk, order=0, plant=None):
    """The kernels' arithmetic in plain fp32 PyTorch: K in chunks of `chunk`, S contiguous split
    ranges, the chunks of a split in a permuted order (seed `order`), fp32 accumulation chunk by
    chunk; int4: per 128-k group acc_group - 136 sum_x, scaled; fp8 / int8: the row scale on the
    accumulator. Epilogue: slabs, one bf16 rounding, or g / (1 + exp(-g)) * u rounded once.
    plant: a planted error inside the accumulation ("drop_chunk", "stale_chunk", "scale_row",
    "scale_group", "swap_nibbles"); the others are planted on the result (plant_on_result)."""
    M, K, N = p.M, p.K, p.N
    x = p.x.float()
    nch = K // chunk
    rng = torch.Generator().manual_seed(order)
    if p.q is None:
        wv, sm = p.w.float(), None
    else:
        codes = decode64(p.q, p.fmt)
        scale = p.scale.clone()
        if plant == "swap_nibbles":
            codes = codes.clone()
            n0, k0 = next((n, kk) for n in range(N) for kk in range(0, K, 2)
                          if codes[n, kk] != codes[n, kk + 1] and bool((x[:, kk] != x[:, kk + 1]).any()))
            codes[n0, k0], codes[n0, k0 + 1] = codes[n0, k0 + 1].clone(), codes[n0, k0].clone()
        if plant == "scale_row":
            scale[..., 0] = scale[..., 1]            # row 1's scale used for row 0
        if plant == "scale_group":
            scale[1, :] = scale[0, :]                # group 0's scale used for group 1
        wv = (codes + 136).float() if p.fmt == INT4 else codes.float()
        sm = scale_matrix(scale, p.fmt, K).float()
    slabs = []
    for s, (lo, hi) in enumerate(split_ranges(nch, S)):
        acc = torch.zeros(M, N)
        order_s = [lo + int(i) for i in torch.randperm(hi - lo, generator=rng)] if order else list(range(lo, hi))
        assert p.fmt != INT4 or chunk % GROUP == 0  # (whole groups per chunk: any chunk order keeps them)
        for c in order_s:
            src = c
            if plant == "drop_chunk" and s == 0 and c == lo + (1 if hi - lo > 1 else 0):
                continue
            if plant == "stale_chunk" and s == 0 and c == lo + 2:
                src = lo
            ks = slice(src * chunk, (src + 1) * chunk)
            if p.fmt == INT4:
                for k0 in range(ks.start, ks.stop, GROUP):
                    kg = slice(k0, k0 + GROUP)
                    accg = x[:, kg] @ wv[:, kg].t()
                    sx = x[:, kg].sum(1, keepdim=True)
                    acc += sm[:, k0][None, :] * (accg - 136.0 * sx)
            else:
                acc += x[:, ks] @ wv[:, ks].t()
        if sm is not None and p.fmt != INT4:
            acc = acc * sm[:, 0][None, :]
        slabs.append(acc)
    if mode == MODE_PARTIAL:
        return torch.stack(slabs)
    acc = slab_sum(torch.stack(slabs))
    if plant == "swap_gate_up":
        acc[:, 0:32] = torch.cat([acc[:, 16:32], acc[:, 0:16]], dim=1)
    if mode == MODE_BF16:
        return acc.bfloat16()
    v = acc.view(M, N // 32, 2, 16)
    g, u = v[:, :, 0], v[:, :, 1]
    return (g / (1.0 + torch.exp(-g)) * u).reshape(M, N // 2).bfloat16()


def plant_on_result(res, plant, mode, tile, ref64=None):
    """A planted error on a finished result (part [S, M, N] or out [M, cols])."""
    res = res.clone()
    t = tile // 2 if mode == MODE_SILU else tile
    if plant == "swap_col_tiles":
        a, b = res[..., 0:t].clone(), res[..., t:2 * t].clone()
        res[..., 0:t], res[..., t:2 * t] = b, a
    elif plant == "dup_row":
        res[..., -2, :] = res[..., -1, :]
    elif plant == "ulp":
        # one bf16 ulp, away from the reference, on the element of the last row that sits lowest in its
        # binade (an ulp is 2^-7 of the binade's floor: at least 2^-8 / 0.95 of such a value)
        flat = res[int(res[:, -1].abs().amax(1).argmax())] if mode == MODE_PARTIAL else res
        a = flat[-1].double().abs()
        frac = torch.where(a > 0, a / 2.0 ** torch.floor(torch.log2(a.clamp_min(1e-300))), torch.full_like(a, 9.0))
        j = int(frac.argmin())
        v = float(flat[-1, j])
        ulp = 2.0 ** (math.floor(math.log2(abs(v))) - 7)
        r = v if ref64 is None else float(ref64[-1, j])
        flat[-1, j] = v + (ulp if v >= r else -ulp)
    else:
        raise KeyError(plant)
    return res
