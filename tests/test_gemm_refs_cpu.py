"""CPU checks of tests/_gemm_ref.py, the helpers of tests/test_gemm_exact_gpu.py: (1) every
committed case builds -- the builders assert their own exactness conditions, the BF16 rounding
conditions, the SiLU range and the coverage of hot positions and codes; (2) a plain fp32
emulation of the kernels' arithmetic (chunk by chunk, permuted chunk orders, even and uneven
splits) reproduces the float64 reference exactly on the grid, one-hot and quantized sections and
meets the bounds of the SiLU and real-valued sections (`pytest -s` prints the share of each
bound used); (3) the checks refuse ten planted errors, for every section that claims to detect
them. Nothing is launched: the case enumeration uses the library's no-launch predicates."""
import pytest
import torch

import _gemm_ref as G

FAMILIES = ("skinny", "m64g", "w8", "mw", "pf")


def _problem(c, section="grid"):
    if section == "grid":
        return G.grid_problem(G.grid_pair(c), c.M, c.N, c.K, c.mode)
    return G.quant_problem(c.fmt, G.quant_xkind(c), c.M, c.N, c.K, c.mode)


# ------------------------------------------------------------------ (1) exactness of every committed case
@pytest.mark.parametrize("family", FAMILIES)
def test_every_case_builds_and_is_covered(family):
    cases = G.family_cases(family)
    assert len(cases) >= G.FLOORS[family]
    if family != "skinny":
        assert {c.combo for c in cases} == set(G._accepted_anywhere(family))
    n = 0
    for c in cases:
        p = _problem(c, "quant" if family == "w8" else "grid")
        assert (p.M, p.N, p.K) == (c.M, c.N, c.K)
        if c.mode == G.MODE_SILU:
            assert float(p.y.abs().max()) <= G.SILU_MAX
        n += 1
    for c in G.onehot_cases(family):
        pos = set(G.hot_positions(c))
        assert {0, c.K - 1} <= pos and all({b - 1, b} <= pos for b in range(c.chunk, c.K, c.chunk))
        if family == "w8":
            probed = set()
            for r in range(G.codes_rounds(c)):
                probed |= G.codes_problem(c, r).probed
            want = ({(i, v) for i in range(8) for v in range(16)} if c.fmt == G.INT4 else set(G.all_codes(c.fmt)))
            assert probed == want, (c.tag, len(probed), len(want))
        else:
            hit = set()
            for r in range(G.onehot_rounds(c, "w")):
                hit |= G.onehot_problem(c, "w", r).probed
            assert hit == pos, c.tag
    assert len(G.all_codes(G.FP8)) == 254 and len(G.all_codes(G.INT8)) == 256
    print(f"{family}: {n} cases, {len(G.onehot_cases(family))} with one-hot inputs")


def test_quantized_cases_use_the_wide_x_and_differing_scales():
    kinds, smods = set(), set()
    for c in G.family_cases("w8"):
        p = _problem(c, "quant")
        kinds.add((c.fmt, G.quant_xkind(c)))
        smods.add(p.smod)
        s = p.scale
        assert bool((s[..., 1:] != s[..., :-1]).all()), c.tag           # neighbouring rows
        if c.fmt == G.INT4 and s.shape[0] > 1:
            assert bool((s[1:] != s[:-1]).all()), c.tag                 # neighbouring groups
    assert {(G.INT4, "b"), (G.INT8, "b"), (G.FP8, "b")} <= kinds and 7 in smods


def test_int4_packing_is_the_packages():
    g = G.gen("pack")
    codes = torch.randint(-8, 8, (48, 256), generator=g)
    q = G.pack_int4(codes)
    assert torch.equal(G.L.dequantize_int4(q, torch.ones(2, 48)), codes.float())
    codes[:, ::128] = 7   # every group's largest magnitude is 7: the package's quantizer returns these codes
    q2, s2 = G.L.quantize_int4(codes.clamp_min(-7).float() * 0.5)
    assert torch.equal(q2, G.pack_int4(codes.clamp_min(-7))) and bool((s2 == 0.5).all())


def test_grouped_cases():
    cases = G.grouped_cases()
    assert len(cases) >= G.FLOORS["pf_grouped"]
    k = G.L.kernels()
    grouped = {cfg for cfg, row in enumerate(k.gemm_cfgs()["pf"]) if row[3]}
    assert {c[0] for c in cases} == grouped
    for cfg in grouped:
        mine = [c for c in cases if c[0] == cfg]
        assert {c[1] for c in mine} == {G.MODE_BF16, G.MODE_PARTIAL, G.MODE_SILU}
        assert {(c[2], c[3]) for c in mine if c[1] == G.MODE_PARTIAL} == {(1, True), (1, False), (2, True), (2, False)}
        bm = k.gemm_cfgs()["pf"][cfg][0]
        lay = G.GroupedLayout(bm, G.gen("t"))
        seg = [int(lay.offs[e + 1] - lay.offs[e]) for e in range(G.GROUPED_E)]
        assert 0 in seg and any(0 < s < bm for s in seg) and any(s > bm for s in seg) and bm in lay.real
        assert lay.P > lay.end
    gp = G.GroupedProblem(192, 256, 128, G.MODE_SILU, "b")
    assert float(gp.p.y.abs().max()) <= G.SILU_MAX


# ------------------------------------------------------------------ (2) the fp32 emulation meets every check
def _emulated(family):
    """One case in five of a family (every combination's first), M capped for the CPU."""
    return [c for c in G.family_cases(family) if c.idx % 5 == 0 and c.M * c.N * c.K <= 1 << 26]


@pytest.mark.parametrize("family", FAMILIES)
def test_emulation_meets_the_checks(family):
    worst = 0.0
    n = 0
    for c in _emulated(family):
        secs = [_problem(c, "quant" if family == "w8" else "grid")]
        if c in G.onehot_cases(family):
            if family == "w8":
                secs.append(G.codes_problem(c, 0))
            else:
                secs += [G.onehot_problem(c, "x", 0), G.onehot_problem(c, "w", 0)]
        for p in secs:
            want = G.Want(p, c.mode, "cpu")
            for order in (0, 1, 2):
                S = c.S if order < 2 else 1
                if c.mode != G.MODE_PARTIAL:
                    S = 1
                got = G.emulate(p, c.mode, S, c.chunk, order)
                worst = max(worst, want.check(got, f"{c.tag} {p.kind} order {order}"))
                n += 1
    assert n > 20
    print(f"{family}: {n} emulated launches; largest share of the SiLU bound used: {worst:.3f}")
    assert worst <= 1.0


@pytest.mark.parametrize("family", FAMILIES)
def test_emulation_meets_the_real_bounds(family):
    for c in G.real_cases(family):
        p = G.real_problem(c.M, c.N, c.K, c.fmt if family == "w8" else None)
        want = G.Want(p, c.mode, "cpu")
        for order in (0, 3):
            used = want.check(G.emulate(p, c.mode, c.S, 128, order), c.tag)
            print(f"{c.tag}: share of the bound used {used:.4f}")
            assert used <= 1.0


# ------------------------------------------------------------------ (3) detection
def _refused(want, res, what):
    with pytest.raises(AssertionError):
        want.check(res, what)
    return 1


@pytest.mark.parametrize("mode", [G.MODE_PARTIAL, G.MODE_BF16, G.MODE_SILU])
@pytest.mark.parametrize("section", ["grid", "onehot", "real"])
def test_planted_errors_are_refused(section, mode):
    M, N, K, chunk, tile, S = 33, 192, 512, 64, 64, (2 if mode == G.MODE_PARTIAL else 1)
    c = G.Launch("m64g", 2, mode, 1, 0, M, N, K, S, 0, chunk, 0)
    if section == "grid":
        ps = [G.grid_problem(pair, M, N, K, mode) for pair in (("b", "c") if mode == G.MODE_BF16 else G.PAIRS)]
    elif section == "onehot":
        ps = [G.onehot_problem(c, "x", 0), G.onehot_problem(c, "w", 0)]
    else:
        ps = [G.real_problem(M, N, K)]
    plants = ["drop_chunk", "stale_chunk", "swap_col_tiles", "dup_row"]
    if mode == G.MODE_SILU and section != "onehot":
        plants.append("swap_gate_up")
    if section != "real":
        plants.append("ulp")   # (the real-valued bound is loose by design: sections 1-3 carry this one)
    n = 0
    for p in ps:
        want = G.Want(p, mode, "cpu")
        good = G.emulate(p, mode, S, chunk, 1)
        want.check(good, "unplanted")
        for plant in plants:
            if plant in ("drop_chunk", "stale_chunk", "swap_gate_up"):
                bad = G.emulate(p, mode, S, chunk, 0, plant=plant)
            else:
                ref = p.silu_ref()[0] if mode == G.MODE_SILU else p.y
                bad = G.plant_on_result(good, plant, mode, tile, ref)
            n += _refused(want, bad, f"{section} {p.note} {plant}")
    print(f"{section} {G.MODE_NAMES[mode]}: {n} planted errors refused ({', '.join(plants)})")


@pytest.mark.parametrize("mode", [G.MODE_PARTIAL, G.MODE_SILU])
@pytest.mark.parametrize("fmt", [G.FP8, G.INT8, G.INT4])
def test_planted_quantization_errors_are_refused(fmt, mode):
    M, N, K, chunk, S = 17, 128, 1024, 128, (2 if mode == G.MODE_PARTIAL else 1)
    plants = ["scale_row", "drop_chunk", "stale_chunk", "ulp"] + (["scale_group", "swap_nibbles"] if fmt == G.INT4 else [])
    n = 0
    for xkind in G.quant_x_kinds(fmt, K):
        p = G.quant_problem(fmt, xkind, M, N, K, mode)
        want = G.Want(p, mode, "cpu")
        good = G.emulate(p, mode, S, chunk, 1)
        want.check(good, "unplanted")
        for plant in plants:
            if plant == "ulp":
                bad = G.plant_on_result(good, plant, mode, 64, p.silu_ref()[0] if mode == G.MODE_SILU else p.y)
            else:
                bad = G.emulate(p, mode, S, chunk, 0, plant=plant)
            n += _refused(want, bad, f"fmt {fmt} x {xkind} {plant}")
    print(f"quant fmt {fmt} {G.MODE_NAMES[mode]}: {n} planted errors refused ({', '.join(plants)})")


def test_codes_section_refuses_a_wrong_widening():
    """One code decoded as its neighbour (fp8 / int8), one nibble read from the next position."""
    for fmt in (G.FP8, G.INT8, G.INT4):
        c = G.Launch("w8", 1, G.MODE_PARTIAL, 0, fmt, 16, 64, 256, 1, 0, 128, 0)
        p = G.codes_problem(c, 0)
        want = G.Want(p, G.MODE_PARTIAL, "cpu")
        want.check(G.emulate(p, G.MODE_PARTIAL, 1, 128, 0), "unplanted")
        q = p.q.clone()
        kk = G.hot_positions(c)[0]
        q[3, kk // 2 if fmt == G.INT4 else kk] ^= 1
        bad = G.Problem("onehot", p.x, p.y, q=q, scale=p.scale, fmt=fmt)
        _refused(want, G.emulate(bad, G.MODE_PARTIAL, 1, 128, 0), f"fmt {fmt}")


def test_a_write_outside_the_output_is_seen():
    for dtype in (torch.float32, torch.bfloat16):
        flat, res = G.guarded((2, 5, 32), dtype, "cpu")
        res.fill_(1.0)
        assert G.guards_intact(flat, res.numel())
        for at in (G.PAD - 1, G.PAD + res.numel()):
            f2 = flat.clone()
            f2[at] = 0
            assert not G.guards_intact(f2, res.numel())
    # and an element the kernel never wrote, inside the output
    flat, res = G.guarded((1, 4, 32), torch.float32, "cpu")
    res[:, :3].fill_(0.0)
    with pytest.raises(AssertionError):
        G.check_partial(res, torch.zeros(4, 32))
    print("sentinel: an overwritten guard element and an unwritten output element are refused")
