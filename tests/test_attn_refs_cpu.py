"""The inputs, bounds and checks of tests/test_attn_exact_gpu.py, checked without a GPU.

  * The package's fp32 CPU paths (ops.prefill_attention and ops.decode_attention on CPU
    tensors) run on the staircase, counted-key and random inputs and must meet every bound.
    `pytest -s` prints the largest share of each bound that they use.
  * The counted-key precondition and the lead of the fused decode's appended key hold for
    the committed seeds.
  * Five wrong references (the diagonal key not seen, key lim + 1 seen, keys 64..127
    dropped, V[70] read as V[71], the last 16 visible keys dropped) are refused: by the
    staircase on exactly the (row, head) pairs whose winning V row they change, by the
    counted keys on exactly the rows whose set of keys they change, by the random check on
    every sequence with such a row, and by its rms limit at (ctx 1000, qlen 5).
  * RMS_EMU / RMS_LIMIT of tests/_attn_ref.py are re-derived from the float64 emulation.
  * The suite's older atol = rtol = 2e-2 accepts the first two wrong references at ctx 1000:
    the reason these files exist.
"""
import pytest
import torch

import _attn_ref as A
from _row_ref import round_bf16

DEV = "cpu"
WORST = {}
# the distinct inputs of the GPU module's prefill configurations (the CPU path has no gh)
PF_INPUTS = [(8, 2, 128), (8, 1, 128), (8, 2, 64)]


def note(res):
    for name, v in res.items():
        WORST[name] = max(WORST.get(name, 0.0), v)


# ---------------------------------------------------------------- the fp32 CPU paths meet every bound
@pytest.mark.parametrize("kind", ["stair", "count"])
@pytest.mark.parametrize("bs", A.PF_BS)
@pytest.mark.parametrize("Hq,Hkv,D", PF_INPUTS)
def test_prefill_fp32_path(Hq, Hkv, D, bs, kind):
    note(A.run_prefill(DEV, kind, A.prefill_shapes(), Hq, Hkv, D, 0, bs, False))


@pytest.mark.parametrize("kind", ["stair", "count"])
def test_prefill_fp32_path_ks2_shapes_and_page_size_64(kind):
    note(A.run_prefill(DEV, kind, A.PF_KS2, 8, 2, 128, 0, 16, True))
    note(A.run_prefill(DEV, kind, A.prefill_shapes(), 8, 2, 128, 0, 64, False))
    note(A.run_prefill(DEV, kind, A.prefill_shapes(long_only=True), 8, 2, 128, 0, 48, True))


@pytest.mark.parametrize("kind", ["stair", "count"])
@pytest.mark.parametrize("bs", A.PF_BS)
@pytest.mark.parametrize("D,G", A.DG)
def test_decode_fp32_path(D, G, bs, kind):
    note(A.run_decode(DEV, kind, A.DEC_LENS, D, G, bs, 1))


def test_random_fp32_path():
    for Hq, Hkv, D, gh, bs in A.RAND_PF:
        note(A.run_prefill(DEV, "rand", (A.RAND_QLENS, A.RAND_CTXS), Hq, Hkv, D, gh, bs, False))
    for D, G, bs in A.RAND_DEC:
        note(A.run_decode(DEV, "rand", A.DEC_LENS, D, G, bs, 1))


def _fused_on_cpu(f):
    """decode_attention_fused has no CPU path: the fp32 decode path on the reference's appended cache."""
    got = A.launch_decode(DEV, f.c, 1)
    A._assert_empty_rows_zero(f.c, got)
    return got


@pytest.mark.parametrize("G,S,depth,bs,splits,rope", A.FUSED_CASES)
def test_fused_own_row_inputs(G, S, depth, bs, splits, rope):
    """The appended key leads every other key by FUSED_GAP_MIN nats, the stale rows are NaN
    in K and V, and the fp32 path returns the new V row."""
    f = A.fused_case("own", G, S, bs, A.fused_lens(bs), rope)
    gap = A.fused_gap(f)
    print(f"fused own-row G={G} S={S} bs={bs} rope={rope}: smallest lead {gap:.1f} nats")
    assert gap >= A.FUSED_GAP_MIN
    for b, L in enumerate(f.lens):
        assert bool(torch.isnan(f.ks0[b][max(0, L - 1):].float()).all()) and bool(torch.isnan(f.vs0[b][max(0, L - 1):].float()).all())
    note(A.check_close(f.c, _fused_on_cpu(f)))


def test_fused_random_inputs():
    G, S, depth, bs, splits, rope = A.RAND_FUSED
    f = A.fused_case("rand", G, S, bs, A.fused_lens(bs), rope)
    note(A.check_rand(f.c, _fused_on_cpu(f)))


# ---------------------------------------------------------------- preconditions for the committed seeds
def _count_inputs():
    for Hq, Hkv, D in PF_INPUTS:
        for bs in A.PF_BS:
            yield A.count_case(*A.prefill_shapes(), Hq, Hkv, D, bs, tag="prefill_count")
    yield A.count_case(*A.PF_KS2, 8, 2, 128, 16, tag="prefill_count")
    yield A.count_case(*A.prefill_shapes(), 8, 2, 128, 64, tag="prefill_count")
    for D, G in A.DG:
        for bs in A.PF_BS:
            yield A.decode_case("count", A.DEC_LENS, D, G, bs)
            yield A.decode_case("count", A.DEC_LENS_LONG, D, G, bs)
    for Hq, Hkv, D in PF_INPUTS:
        for bs in A.PF_BS:
            yield A.count_case(*A.prefill_shapes(long_only=True), Hq, Hkv, D, bs, tag="prefill_count")


def test_counted_keys_precondition():
    for c in _count_inputs():
        assert A.count_precondition(c), c.tag


def test_shapes_are_what_the_launcher_needs():
    qlens, ctxs = A.prefill_shapes()
    assert len(qlens) == 116 and qlens.count(0) == 2 and 0 not in (qlens[0], qlens[-1])
    assert len(qlens) * -(-max(qlens) // 128) * 8 // 2 >= 512       # gh = 0 -> KS = 1
    assert len(A.PF_KS2[0]) == len(A.PF_KS2[1]) and len(A.PF_KS2[0]) * -(-max(A.PF_KS2[0]) // 128) * 8 // 2 < 512
    assert {c % 64 for c in A.RAND_CTXS} >= {0, 1, 63}
    assert len(A.FUSED_CASES) == 18
    assert {x[:2] for x in A.FUSED_CASES} == {(G, S) for G in (1, 2, 4, 8) for S in (2, 5, 9)}


# ---------------------------------------------------------------- the rms limit
def test_rms_limit_is_three_times_the_emulation():
    emu = A.emulated_rms()
    print(f"float64 emulation of the kernels' arithmetic: largest row rms ratio {emu:.6e} = {emu * 256:.3f} * 2^-8")
    assert emu == pytest.approx(A.RMS_EMU, rel=1e-6)
    assert A.RMS_LIMIT == 3 * A.RMS_EMU


# ---------------------------------------------------------------- wrong references are refused
def _wrong_out(c, name):
    return round_bf16(A.attend_case(c, wrong=name)[0])


def _stair_and_count_inputs():
    return [(A.stair_case(*A.prefill_shapes(), 8, 2, 128, 16, tag="prefill_stair"),
             A.count_case(*A.prefill_shapes(), 8, 2, 128, 16, tag="prefill_count")),
            (A.stair_case(*A.prefill_shapes(), 8, 2, 64, 48, tag="prefill_stair"),
             A.count_case(*A.prefill_shapes(), 8, 2, 64, 48, tag="prefill_count")),
            (A.decode_case("stair", A.DEC_LENS, 128, 4, 16), A.decode_case("count", A.DEC_LENS, 128, 4, 16)),
            (A.decode_case("stair", A.DEC_LENS, 64, 1, 48), A.decode_case("count", A.DEC_LENS, 64, 1, 48))]


@pytest.mark.parametrize("name", A.WRONG)
def test_wrong_reference_refused_by_staircase_and_counted_keys(name):
    n_stair = n_count = 0
    for st, ct in _stair_and_count_inputs():
        bad, _ = A.close_bad(st, _wrong_out(st, name))
        hit = A.touched_stair(st, name)
        assert torch.equal(bad, hit), f"{st.tag}: {name}: refused {int(bad.sum())}, winning row changed on {int(hit.sum())}"
        n_stair += int(hit.sum())
        bad, _ = A.count_bad(ct, _wrong_out(ct, name))
        hit = A.touched(ct, name)[:, None].expand_as(bad)
        assert torch.equal(bad, hit), f"{ct.tag}: {name}: refused {int(bad.sum())}, key set changed on {int(hit.sum())}"
        n_count += int(hit.sum())
    assert n_stair > 0 and n_count > 0


def _rand_inputs():
    return [A.rand_case(A.RAND_QLENS, A.RAND_CTXS, 8, 2, 128, 16, tag="prefill_rand"),
            A.rand_case(A.RAND_QLENS, A.RAND_CTXS, 8, 2, 64, 16, tag="prefill_rand"),
            A.decode_case("rand", A.DEC_LENS, 128, 4, 16), A.decode_case("rand", A.DEC_LENS, 64, 1, 48)]


@pytest.mark.parametrize("name", A.WRONG)
def test_wrong_reference_refused_by_random_check(name):
    for c in _rand_inputs():
        got = _wrong_out(c, name)
        right = round_bf16(c.ref)
        assert not bool(A.elem_bad(c, right)[0].any()) and not bool(A.rms_bad(c, right)[0].any())
        bad = A.elem_bad(c, got)[0] | A.rms_bad(c, got)[0]
        hit = A.touched(c, name)
        for s, a, b, ctx, L in c.seqs():
            if bool(hit[a:b].any()):
                assert bool(bad[a:b].any()), f"{c.tag}: {name} accepted on sequence {s} (qlen {b - a}, ctx {ctx})"
            else:
                assert not bool(bad[a:b].any())
    c = _rand_inputs()[0]
    s = list(zip(c.qlens, c.ctxs)).index((5, 1000))
    a, b = c.start[s], c.start[s + 1]
    r = A.rms_ratio(c, _wrong_out(c, name))[a:b]
    print(f"{name} at (ctx 1000, qlen 5): largest row rms ratio {float(r.max()) * 256:.2f} * 2^-8, "
          f"limit {A.RMS_LIMIT * 256:.2f} * 2^-8")
    assert float(r.max()) > A.RMS_LIMIT


@pytest.mark.parametrize("name", ["no_diag", "one_past"])
def test_old_tolerance_accepts_one_wrong_key_at_ctx_1000(name):
    """Why these files exist: atol = rtol = 2e-2 against the reference, the check of the older
    attention tests, passes a mask that is off by one key at (ctx 1000, qlen 5): on every
    (row, head) pair for the unseen diagonal, on 9 in 10 of the pairs for the key past the
    limit (to one head of this seed that key is worth 4 % of the row). The rms limit refuses
    the sequence either way (test_wrong_reference_refused_by_random_check)."""
    c = _rand_inputs()[0]
    s = list(zip(c.qlens, c.ctxs)).index((5, 1000))
    a, b = c.start[s], c.start[s + 1]
    hit = A.touched(c, name)[a:b]
    got, ref = _wrong_out(c, name), round_bf16(c.ref)
    old_ok = ((got.float() - ref.float()).abs() <= 2e-2 + 2e-2 * ref.float().abs()).all(-1)[a:b][hit]
    new_bad = A.rms_bad(c, got)[0][a:b][hit]
    print(f"{name}: atol = rtol = 2e-2 accepts {int(old_ok.sum())} of {old_ok.numel()} touched (row, head) pairs, "
          f"the rms limit refuses {int(new_bad.sum())}")
    assert old_ok.numel() >= 32 and bool(new_bad.any())
    assert int(old_ok.sum()) >= (old_ok.numel() if name == "no_diag" else 0.9 * old_ok.numel())


def test_zz_report_worst_share_of_each_bound():
    """Not a check of its own: prints what the fp32 paths used of each bound (pytest -s)."""
    for name in sorted(WORST):
        print(f"fp32 CPU path, largest share of bound {name}: {WORST[name]:.3g}")
    assert all(v <= 1.0 for v in WORST.values())
