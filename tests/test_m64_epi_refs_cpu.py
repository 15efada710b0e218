"""CPU checks of tests/_m64_epi_ref.py, the helpers of tests/test_m64_epi_exact_gpu.py: (1) every
committed problem builds -- the builders assert their exactness conditions, the rounding and tie
shares, the SiLU range and that one unit of one partial sum or a neighbour's statistics moves an
output by 8 bounds; the enumeration launches every (cfg, nw, MT, statistics path) the predicate
takes and both sides of every staging threshold; (2) a plain fp32 emulation of the kernel's
arithmetic (chunk and split order, the three statistic summation orders, the scale per slab, the
tails' reduce orders) meets every check with a share of each bound below 1 (`pytest -s` prints
them); (3) the checks refuse every planted error on every section it applies to. Nothing is
launched: the enumeration uses the library's no-launch predicate."""
import functools

import pytest
import torch

import _gemm_ref as G
import _m64_epi_ref as E

SECTIONS = ("scale", "resid", "both", "silu")


def _cpu(order=0, plant=None):
    return functools.partial(E.emulate, order=order, plant=plant)


# ------------------------------------------------------------------ (1) every committed problem
@pytest.mark.parametrize("sec", SECTIONS)
def test_every_problem_builds(sec):
    cases = E.ALL_SECTIONS[sec]()
    assert len(cases) >= E.FLOORS[sec]
    for c in cases:
        p = E.problem(c)
        assert p.x.shape == (c.M, c.K) and p.w.shape == (c.N, c.K) and p.ys.shape == (c.S, c.M, c.N)
        if c.ss_n:
            assert c.stride >= c.M and bool(torch.isnan(p.ssbuf[:E.SS_PRE]).all())
            assert bool(torch.isnan(p.ssbuf[E.SS_PRE + c.ss_n:]).all()) and bool(torch.isnan(p.ssbuf[:, c.M:]).all())
    print(f"{sec}: {len(cases)} problems")


def test_enumeration_covers_what_the_predicate_takes():
    scale, resid, both, silu = (E.ALL_SECTIONS[s]() for s in SECTIONS)
    assert {c.key for c in scale} == {c.key for c in resid} == {c.key for c in both} == set(E.accepted())
    assert {c.key for c in silu} == {key for key in E.accepted() if key[1] == 2}
    for mode, split in ((E.MODE_PARTIAL, None), (E.MODE_BF16, False), (E.MODE_SILU, False), (E.MODE_SILU, True)):
        mine = [c for c in scale if c.mode == mode and split in (None, c.S > 1)]
        want = {key for key in E.accepted_paths() if mode != E.MODE_SILU or key[1] == 2}
        assert {c.key + (c.path,) for c in mine} == want, (mode, split)
    part = [c for c in scale if c.mode == E.MODE_PARTIAL]
    for cfg, nw, Ms in E._configs():
        ssns = {c.ss_n for c in part if (c.cfg, c.nw) == (cfg, nw) and (c.M <= 16) == (Ms is E.SMALL_M)}
        assert ssns == set(E.SSN_ANY + (E.SSN_SMALL_M if Ms is E.SMALL_M else ())), (cfg, nw)
    assert {c.krot for c in scale} == {0, 1} and {c.eps for c in scale} == {0.0, 1e-5}
    assert any(c.stride == c.M for c in scale) and any(c.stride > c.M for c in scale)
    assert any(c.K & (c.K - 1) == 0 for c in scale) and any(c.K & (c.K - 1) for c in scale)
    # GG_RESID: every S at every (cfg, nw); S = 1 at every M; both sides of the staging threshold
    for cfg, nw, Ms in E._configs():
        mine = [c for c in resid if (c.cfg, c.nw) == (cfg, nw) and (c.M <= 16) == (Ms is E.SMALL_M)]
        assert {c.S for c in mine} == set(E.RESID_S) and {c.M for c in mine if c.S == 1} == set(Ms)
    for cfg in {c.cfg for c in resid}:
        for nw in (1, 2):
            Ms = [c.M for c in resid if (c.cfg, c.nw, c.S) == (cfg, nw, 1)]
            sides = {E.staged(cfg, nw, M) for M in Ms}
            inside = {E.staged(cfg, nw, M) for M in range(1, 65) if G.L.kernels().m64g_supports(
                M, E.geom(cfg, nw, M).kc, E.geom(cfg, nw, M).cols, 1, E.MODE_PARTIAL, nw, cfg)}
            assert sides == inside, (cfg, nw, sides, inside)
    thresholds = {(cfg, nw) for cfg, nw, _ in E._configs() if not E.staged(cfg, nw, 64) and E.geom(cfg, nw, 64).MT == 4}
    assert len(thresholds) >= 4        # (4, 64) at nw 1 and 2, (2, 64) at nw 2, (8, 64): module docstring
    assert {(c.cfg, c.S) for c in silu} == {(cfg, S) for cfg in {c.cfg for c in scale} for S in E.SILU_S}
    assert {(c.cfg, c.S, c.ss_n > 0) for c in silu} == {(c.cfg, c.S, w) for c in silu for w in (False, True)}


def test_chain_cases():
    chains = E.chain_cases()
    assert len(chains) >= E.FLOORS["chain"]
    seen = set()
    for ch in chains:
        cA, pA, cB, pB = E.chain_problem(ch)
        seen.add((E.geom(ch.cfgA, ch.nwA, ch.M).wv, E.geom(ch.cfgB, ch.nwB, ch.M).wv))
        assert ch.ss_n <= (128 if ch.M <= 16 else 64)
    assert {a for a, _ in seen} == {2, 4, 8} and all(a != b for a, b in seen)
    ns = [(ch.ss_n, ch.M) for ch in chains]
    assert any(n < 8 for n, _ in ns) and any(8 < n <= 64 and M > 16 for n, M in ns) and any(n == 64 and M > 16 for n, M in ns)
    assert any(65 <= n <= 128 and M <= 16 for n, M in ns)
    assert sum(1 for ch in chains if ch.ss_n * E.geom(ch.cfgA, ch.nwA, ch.M).cols % 1024 == 0) >= 2


# ------------------------------------------------------------------ (2) the fp32 emulation meets every check
def _sample(sec, every):
    return [c for i, c in enumerate(E.ALL_SECTIONS[sec]()) if i % every == 0]


@pytest.mark.parametrize("sec,every", [("scale", 6), ("resid", 6), ("both", 3), ("silu", 4)])
def test_emulation_meets_the_checks(sec, every):
    worst, n = {}, 0
    for c in _sample(sec, every):
        kind = E.MODE_NAMES[c.mode] + (" split" if c.mode == E.MODE_SILU and c.S > 1 else "")
        for order in (0, 1):
            worst[kind] = max(worst.get(kind, 0.0), E.run_case(c, E.problem(c), "cpu", _cpu(order)))
            n += 1
    shares = ", ".join(f"{kind} {v:.3f}" for kind, v in sorted(worst.items()))
    print(f"{sec}: {n} emulated cases x 2 launches; largest share of a bound used: {shares}")
    assert n >= 20 and max(worst.values()) < 1.0


def test_emulated_chain():
    worst = 0.0
    for ch in E.chain_cases()[::3]:
        cA, pA, cB, pB = E.chain_problem(ch)
        assert E.run_case(cA, pA, "cpu", _cpu()) == 0.0
        worst = max(worst, E.run_case(cB, pB, "cpu", _cpu(1)))
    print(f"chain: largest share of the bound used: {worst:.3f}")
    assert worst < 1.0


# ------------------------------------------------------------------ (3) detection
def _pick(sec):
    """Cases of a section that together let every plant apply: tall / wide / small statistics,
    stride > M, eps > 0, N != K, S > 1, M > 16 and M in 2 .. 16."""
    cases = E.ALL_SECTIONS[sec]()
    out = []
    for want in ("tall", "wide", "small", None):
        for mode in (E.MODE_PARTIAL, E.MODE_BF16, E.MODE_SILU, E.MODE_RESID):
            for split in (False, True):
                hit = next((c for c in cases if c.path == want and c.mode == mode and (c.S > 1) == split and c.M > 1
                            and (not c.ss_n or (c.stride > c.M and c.eps > 0 and c.ss_n > 1)) and c.N != c.K), None)
                if hit is not None:
                    out.append(hit)
    return out


@pytest.mark.parametrize("sec", SECTIONS)
def test_planted_errors_are_refused(sec):
    picked = _pick(sec)
    assert picked
    refused = {}
    for c in picked:
        p = E.problem(c)
        E.run_case(c, p, "cpu", _cpu(1))                      # unplanted
        for plant in E.ALL_PLANTS:
            if not E.applies(plant, c):
                continue
            with pytest.raises(AssertionError):
                E.run_case(c, p, "cpu", _cpu(0, plant))
                print(f"NOT refused: {plant} at {c.tag}")
            refused[plant] = refused.get(plant, 0) + 1
    want = {pl for pl in E.ALL_PLANTS if any(E.applies(pl, c) for c in E.ALL_SECTIONS[sec]())}
    assert set(refused) == want, (sec, sorted(want - set(refused)))
    print(f"{sec}: {sum(refused.values())} planted errors refused over {len(picked)} cases: "
          + ", ".join(f"{k} x{v}" for k, v in sorted(refused.items())))


def test_planted_chain_errors_are_refused():
    """The hand-off: ss_out stored [m, tile] by the producer, or read with another stride / one tile
    too many by the consumer."""
    ch = next(ch for ch in E.chain_cases() if ch.M > 16 and ch.ss_n > 8 and ch.modeB == E.MODE_PARTIAL)
    cA, pA, cB, pB = E.chain_problem(ch)
    with pytest.raises(AssertionError):
        E.run_case(cA, pA, "cpu", _cpu(0, "ss_mt"))
    for plant in ("row+1", "row+16", "drop", "dup_last", "extra_j", "mean_n"):
        with pytest.raises(AssertionError):
            E.run_case(cB, pB, "cpu", _cpu(0, plant))
            print(f"NOT refused: {plant} at {ch.tag}")
    # the statistics transposed on the consumer's side
    bad = E.EpiProblem()
    bad.__dict__.update(pB.__dict__)
    bad.ssbuf = pB.ssbuf.clone()
    n = ch.ss_n
    bad.ssbuf[E.SS_PRE:E.SS_PRE + n] = pB.ssbuf[E.SS_PRE:E.SS_PRE + n].t().reshape(n, ch.M)
    with pytest.raises(AssertionError):
        E.run_case(cB, bad, "cpu", _cpu())
