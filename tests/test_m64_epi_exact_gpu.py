"""gemm_m64g's fused decode epilogues through gemm_m64g_ex, called directly (no planner, no
fallback), at every (cfg, nw, MT) the library's predicate takes: the RMSNorm row scale from ss_in
on all three statistics paths, the GG_RESID tail (bit-exact residual and ss_out) on both sides of
the LDS-staging threshold, ss_in and GG_RESID in one launch, the split-K SiLU tail, and the
producer -> consumer hand-off of ss_out, also from add_partials_resid's and row_sumsq's layouts.

tests/test_fused_decode_gpu.py and tests/test_partials_gpu.py check these paths by one Frobenius
norm at the planner's configurations, or bit-exactly at two (nw, cfg) against the kernel's own
slabs. Here x and W are exact integer grids, the statistics are exact in any summation order and
differ by powers of 4 between neighbouring rows, the residual is built so that the rounded sum and
its squares are known exactly, and every bound is derived per element from the kernel's operations
(tests/_m64_epi_ref.py's docstring; tests/test_m64_epi_refs_cpu.py holds an fp32 emulation to the
same checks and plants errors). Every launch writes interior slices of sentinel-filled buffers,
reads statistics surrounded by NaN, runs twice into fresh buffers with bit-identical results and
must leave its tickets zero; K rotation off and at its default, restored afterwards.
"""
import time

import pytest
import torch

import _gemm_ref as G
import _m64_epi_ref as E
from xgserve.ops import _native
from xgserve.ops import linear as L
from xgserve.ops._native import stream_ptr

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module")
def k():
    kern = _native.kernels()  # fail loudly: the HIP library must be the one that runs
    yield kern
    G.restore_rotation(kern)


def _launch(k):
    st = stream_ptr()

    def go(c, p, ops, b):
        G.set_rotation(k, c)
        E.native_launch(k, c, ops, b, st)

    return go


def _sweep(k, cases, what):
    t0, worst = time.perf_counter(), {}
    go = _launch(k)
    for c in cases:
        kind = E.MODE_NAMES[c.mode] + (" split" if c.mode == E.MODE_SILU and c.S > 1 else "")
        worst[kind] = max(worst.get(kind, 0.0), E.run_case(c, E.problem(c), DEV, go))
    torch.cuda.synchronize()
    shares = ", ".join(f"{kind} {v:.3f}" for kind, v in sorted(worst.items()))
    print(f"{what}: {len(cases)} cases x 2 launches in {time.perf_counter() - t0:.1f} s; largest share of a bound used: {shares}")


# ---------------------------------------------------------------- 1. row scale
@pytest.mark.parametrize("kind", ["partial", "bf16", "silu", "silu split"])
def test_row_scale(k, kind):
    cases = E.scale_cases()
    assert len(cases) >= E.FLOORS["scale"]
    assert {c.key for c in cases} == set(E.accepted())
    mode = {"partial": E.MODE_PARTIAL, "bf16": E.MODE_BF16}.get(kind, E.MODE_SILU)
    mine = [c for c in cases if c.mode == mode and (mode != E.MODE_SILU or (c.S > 1) == (kind == "silu split"))]
    want = {key for key in E.accepted_paths() if mode != E.MODE_SILU or key[1] == 2}
    assert {c.key + (c.path,) for c in mine} == want     # every path at every WV and MT it is instantiated for
    _sweep(k, mine, f"row scale, {kind}")


# ---------------------------------------------------------------- 2. GG_RESID tail
@pytest.mark.parametrize("nw", [1, 2])
def test_resid_tail(k, nw):
    cases = E.resid_cases()
    assert len(cases) >= E.FLOORS["resid"]
    assert {c.key for c in cases} == set(E.accepted())
    mine = [c for c in cases if c.nw == nw]
    for cfg in {c.cfg for c in mine}:
        one = [c.M for c in mine if c.cfg == cfg and c.S == 1]
        assert {c.S for c in mine if c.cfg == cfg} == set(E.RESID_S)
        inside = {E.staged(cfg, nw, M) for M in range(1, 65) if k.m64g_supports(
            M, E.geom(cfg, nw, M).kc, E.geom(cfg, nw, M).cols, 1, E.MODE_PARTIAL, nw, cfg)}
        assert {E.staged(cfg, nw, M) for M in one} == inside, (cfg, nw)   # both sides of the staging threshold
    _sweep(k, mine, f"GG_RESID nw{nw}")


def test_row_scale_and_resid_in_one_launch(k):
    cases = E.both_cases()
    assert len(cases) >= E.FLOORS["both"] and {c.key for c in cases} == set(E.accepted())
    _sweep(k, cases, "ss_in + GG_RESID")


# ---------------------------------------------------------------- 3. split-K SiLU tail
def test_split_silu_tail(k):
    cases = E.silu_cases()
    assert len(cases) >= E.FLOORS["silu"]
    assert {c.key for c in cases} == {key for key in E.accepted() if key[1] == 2}
    assert {(c.cfg, c.S, c.ss_n > 0) for c in cases} == {(cfg, S, w) for cfg in {c.cfg for c in cases}
                                                         for S in E.SILU_S for w in (False, True)}
    _sweep(k, cases, "split-K SiLU tail")


# ---------------------------------------------------------------- 4. producer -> consumer chain
def _consumer(k, cB, pB, x, ss_ptr, ss_n, want, st, tag):
    """Launch B on statistics at ss_ptr ([ss_n, M]); returns (share of the bound, its buffers)."""
    ops = E.Operands(cB, pB, DEV)
    ops.x, ops.ss, ops.ss_ptr = x, None, ss_ptr
    c = cB._replace(ss_n=ss_n)
    b = E.Buffers(c, pB, DEV)
    G.set_rotation(k, c)
    E.native_launch(k, c, ops, b, st)
    return want.check(b, tag), b


def test_chain(k):
    chains = E.chain_cases()
    assert len(chains) >= E.FLOORS["chain"]
    st, worst, t0, layouts = stream_ptr(), 0.0, time.perf_counter(), 0
    for ch in chains:
        cA, pA, cB, pB = E.chain_problem(ch)
        opsA, wantA, wantB = E.Operands(cA, pA, DEV), E.Want(cA, pA, DEV), E.Want(cB, pB, DEV)
        first = None
        for rep in range(2):
            bA = E.Buffers(cA, pA, DEV)
            G.set_rotation(k, cA)
            E.native_launch(k, cA, opsA, bA, st)
            wantA.check(bA, f"{ch.tag} A launch {rep}")
            # B reads A's own outputs in place: the residual as x, ss_out as ss_in with stride M
            used, bB = _consumer(k, cB, pB, bA.resid, bA.ss_out.data_ptr(), ch.ss_n, wantB, st, f"{ch.tag} B launch {rep}")
            worst = max(worst, used)
            bA.check_guards(f"{ch.tag} A after B")
            if first is None:
                first = bB
            else:
                bB.same_as(first, ch.tag)
        if cA.N % 1024:
            continue
        # the same residual add through the wide kernel (statistics per 1024 columns) and row_sumsq (one sum)
        layouts += 1
        fp, part = G.guarded((cA.S, cA.M, cA.N), torch.float32, DEV)
        k.gemm_m64g(opsA.x.data_ptr(), cA.M, cA.K, opsA.w.data_ptr(), cA.N, part.data_ptr(), 0, cA.S, E.MODE_PARTIAL,
                    cA.nw, cA.cfg, st)
        fr, resid = G.guarded((cA.M, cA.N), torch.bfloat16, DEV, 2 * cA.N)
        resid.copy_(pA.resid0.to(DEV))
        chunks = cA.N // 1024
        f2, ss2 = G.guarded((chunks, cA.M), torch.float32, DEV)
        k.add_partials_resid(part.data_ptr(), cA.S, cA.M, resid.data_ptr(), ss2.data_ptr(), cA.N, st)
        G.check_bf16(resid, wantA.want_resid, f"{ch.tag} add_partials_resid")
        assert G.guards_intact(fr, resid.numel(), 2 * cA.N) and G.guards_intact(f2, ss2.numel()) and G.guards_intact(fp, part.numel())
        f3, ss3 = G.guarded((1, cA.M), torch.float32, DEV)
        k.row_sumsq(resid.data_ptr(), cA.M, cA.N, ss3.data_ptr(), st)
        assert G.guards_intact(f3, ss3.numel())
        assert torch.equal(ss2.sum(0), ss3[0]) and torch.equal(ss3[0], bA.ss_out.sum(0)), ch.tag   # (exact in any order)
        for name, ss, n in (("per 1024 columns", ss2, chunks), ("one sum", ss3, 1)):
            used, b = _consumer(k, cB, pB, resid, ss.data_ptr(), n, wantB, st, f"{ch.tag} B on {name}")
            worst = max(worst, used)
            b.same_as(first, f"{ch.tag} B on {name}")   # exact sums: the same scale on any statistics path
    torch.cuda.synchronize()
    assert layouts >= 2
    print(f"chain: {len(chains)} chains x 2 launches (+ {layouts} through the other two layouts) in "
          f"{time.perf_counter() - t0:.1f} s; largest share of the bound used: {worst:.3f}")


# ---------------------------------------------------------------- 5. refusals and wrappers
def test_refusals_leave_the_outputs_untouched(k):
    """Every refused call raises and writes nothing. The operands are real, in-bounds device buffers
    of the stated shapes, so a missing check fails this test and does not fault the card."""
    st = stream_ptr()
    cfg, nw, S = 0, 2, 2
    g = E.geom(cfg, nw, 17)
    N, K = 2 * g.cols, 4 * g.kc
    x = torch.zeros(64, K, dtype=torch.bfloat16, device=DEV)
    w = torch.zeros(N, K, dtype=torch.bfloat16, device=DEV)
    ss = torch.ones(140, 64, dtype=torch.float32, device=DEV)[4:]   # (rows in front of it too)

    def call(M=17, mode=E.MODE_PARTIAL, S=S, ss_n=4, stride=64, part=True, out=True, resid=True, ss_out=True,
             counters=True, plain=False, with_ss=True):
        fp, vp = G.guarded((S, 64, N), torch.float32, DEV)
        fo, vo = G.guarded((64, N), torch.bfloat16, DEV)
        fr, vr = G.guarded((64, N), torch.bfloat16, DEV)
        fs, vs = G.guarded((N // g.cols, 64), torch.float32, DEV)
        cnt = torch.zeros(64, dtype=torch.int32, device=DEV)
        with pytest.raises(Exception):
            if plain:
                k.gemm_m64g(x.data_ptr(), M, K, w.data_ptr(), N, vp.data_ptr(), vo.data_ptr(), S, mode, nw, cfg, st)
            else:
                k.gemm_m64g_ex(x.data_ptr(), M, K, w.data_ptr(), N, vp.data_ptr() if part else 0,
                               vo.data_ptr() if out else 0, S, mode, nw, cfg, ss.data_ptr() if with_ss else 0, ss_n, stride,
                               1e-5, vr.data_ptr() if resid else 0, vs.data_ptr() if ss_out else 0,
                               cnt.data_ptr() if counters else 0, st)
            pytest.fail("a refused call was launched")
        torch.cuda.synchronize()
        for f in (fp, fo, fr, fs):
            sent = G.SENT32 if f.dtype == torch.int32 else G.SENT16
            assert bool((f == sent).all())
        assert not bool(cnt.any())

    call(ss_n=0)
    call(ss_n=129, M=16)
    call(ss_n=65, M=17)
    call(ss_n=65, M=16, stride=15)          # ss_stride < M
    call(stride=16)                         # ss_stride < M at M = 17
    call(mode=E.MODE_SILU, part=False, with_ss=False)
    call(mode=E.MODE_SILU, counters=False, with_ss=False)
    for missing in ("resid", "ss_out", "counters"):
        call(mode=E.MODE_RESID, with_ss=False, **{missing: False})
    call(mode=E.MODE_RESID, plain=True)
    # and the same operands are accepted when nothing is wrong (the refusals above are not an accident)
    fp, vp = G.guarded((S, 17, N), torch.float32, DEV)
    k.gemm_m64g_ex(x.data_ptr(), 17, K, w.data_ptr(), N, vp.data_ptr(), 0, S, E.MODE_PARTIAL, nw, cfg, ss.data_ptr(), 64,
                   64, 1e-5, 0, 0, 0, st)
    assert not bool(vp.any()) and G.guards_intact(fp, vp.numel())


def test_wrappers_give_the_native_results(k):
    """m64_linear(stats=RowStats(...)) with stride > M, and m64_resid_linear(plan=...), against the
    native results of the same case, bit for bit."""
    go = _launch(k)
    n = 0
    for mode in (E.MODE_PARTIAL, E.MODE_BF16, E.MODE_SILU):
        c = next(c for c in E.scale_cases() if c.mode == mode and c.stride > c.M and c.ss_n > 8 and c.eps > 0)
        p = E.problem(c)
        ops, b = E.Operands(c, p, DEV), E.Buffers(c, p, DEV)
        go(c, p, ops, b)
        E.Want(c, p, DEV).check(b, c.tag)
        stats = L.RowStats(ops.ss[E.SS_PRE:], c.ss_n, c.stride)
        got = L.m64_linear(ops.x, ops.w, mode, c.S, c.nw, cfg=c.cfg, stats=stats, eps=c.eps)
        if mode == E.MODE_PARTIAL:
            assert got.part.shape == b.part.shape and torch.equal(G.ibits(got.part), G.ibits(b.part)), c.tag
        else:
            assert torch.equal(G.ibits(got), G.ibits(b.out)), c.tag
        n += 1
    # GG_RESID in the launch (small slabs) and through add_partials_resid (large ones)
    for M, S, cfg, nw in ((33, 2, 0, 1), (64, 4, 1, 2)):
        g = E.geom(cfg, nw, M)
        c = E.Case("resid", cfg, nw, E.MODE_RESID, M, 1024, 5 * g.kc, S, 1, 0, 0, 0.0, n)
        p = E.problem(c)
        inlaunch = S * M * g.cols * 4 <= L.RESID_INLAUNCH_MAX_BYTES
        ops, b = E.Operands(c, p, DEV), E.Buffers(c, p, DEV)
        go(c, p, ops, b)
        want = E.Want(c, p, DEV)
        want.check(b, c.tag)
        ws = L.ResidWorkspace(2, M, c.N, DEV)
        resid = p.resid0.to(DEV)
        stats = L.m64_resid_linear(ops.x, ops.w, resid, ws, 1, 1e-5, plan=(nw, S, cfg))
        assert torch.equal(G.ibits(resid), G.ibits(b.resid)), c.tag
        if inlaunch:
            assert (stats.n, stats.stride) == (b.tiles, M)
            assert torch.equal(stats.ss[:b.tiles * M].view(b.tiles, M), b.ss_out), c.tag
        else:
            assert (stats.n, stats.stride) == (c.N // 1024, M)
            ref = (want.want_resid.double() ** 2).view(M, stats.n, 1024).sum(-1).t()   # (1023 fp32 additions)
            G.check_bound(stats.ss[:stats.n * M].view(stats.n, M), ref, 1024 * E.U * ref, c.tag)
        assert not bool(ws.counters.any())
        n += 1
    assert n == 5
