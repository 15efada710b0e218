"""CPU self-test of tests/_model_ref.py, the helper behind tests/test_model_regimes_gpu.py.

Tolerance rule. For a model and a token sequence the bound on rel(logits, reference64) is
    bound = 2 * rel(emulate(...), reference64(...))            on the same inputs,
the error that bf16 storage alone forces on the chain, times 2 for what the emulation leaves
out (the kernels' fp32 summation order, their bf16 P.V product). It is computed where it is used,
never copied from what a kernel gave. Discrimination: every planted error must move emulate() by
at least 4 * bound, or a test that holds the kernels to `bound` could not see that bug.

Measured here (tiny registry models after trained_like(seed 11), 40-token sequence; run with -s
to print them again):

    model              emulate rel  bound     smallest plant displacement / bound
    llama-tiny         9.7e-3       1.9e-2    22 x  (rope_q_shift; the norm plants 29-75 x)
    llama-tiny-scaled  9.5e-3       1.9e-2    13 x  (post_norm)
    mixtral-tiny       1.1e-2       2.2e-2    30 x  (final_norm; moe_post_folded 31 x)
    gpt2-tiny          3.6e-3       7.3e-3    4.1 x (ln_b; kv_page 6 x, the linear biases 15-73 x)
    quantized, against reference64(quant): llama-tiny / llama-tiny-scaled
    fp8   emulate rel 1.0e-2 / 7.2e-3, bound 2.1e-2 / 1.4e-2 (format's own error 9.6e-2 / 1.3e-1)
    int8  emulate rel 1.3e-2 / 7.0e-3, bound 2.6e-2 / 1.4e-2 (2.7e-2 / 1.9e-2)
    int4  emulate rel 9.0e-3 / 7.2e-3, bound 1.8e-2 / 1.4e-2 (7.8e-1 / 3.0e-1)
    every norm, fold, RoPE and KV-page plant at least 4 x bound in all six (asserted)

At the GPU module's own shape (llama3-8b, 2 layers, 40 tokens, float64 on the CPU): emulate rel
1.4e-2, bound 2.7e-2, input_norm 38 x, post_norm 28 x, final_norm 13 x, norm_twice 52 x,
rope_q_shift 17 x, kv_page 36 x. The
kernels' own worst rel per regime is recorded in tests/test_model_regimes_gpu.py.
"""
from dataclasses import replace

import pytest
import torch

from _model_ref import (NORM_PLANTS, Snapshot, check_rope_tables, emulate, gap, plants_for, reference64, rel,
                        rope_inv_freq64, trained_like)
from xgserve.models import build_model, get_config

LLAMA3_SCALING = {"rope_type": "llama3", "factor": 32.0, "low_freq_factor": 1.0, "high_freq_factor": 4.0,
                  "original_max_position_embeddings": 8192}
TOKENS = [1] + [(37 * i + 11) % 500 + 3 for i in range(39)]   # 40 tokens: more than two KV pages
SHORT = TOKENS[:19]


def _cfg(name):
    if name == "llama-tiny-scaled":  # the llama3.2-1b traits: scaled RoPE, tied head
        return replace(get_config("llama-tiny"), name=name, rope_scaling=dict(LLAMA3_SCALING), tie_embeddings=True)
    return get_config(name)


MODELS = ("llama-tiny", "llama-tiny-scaled", "mixtral-tiny", "gpt2-tiny")
# Weight scale of the tiny llama / mixtral models: random_init's 0.02 at H = 4096 gives q, k and
# v a standard deviation of 0.02 * sqrt(4096) = 1.28 and attention scores that tell positions
# apart; at H = 256 the same 0.02 gives near-uniform attention that no RoPE or KV-page error can
# move. 0.02 * sqrt(4096 / 256) = 0.08 restores the 8B shape's gain per projection.
STD = {"llama-tiny": 0.08, "llama-tiny-scaled": 0.08, "mixtral-tiny": 0.08, "gpt2-tiny": 0.02}
_cache = {}


def _trained(name, dtype):
    m = build_model(_cfg(name), device="cpu", dtype=dtype, seed=4)
    m.random_init(4, std=STD[name])
    return trained_like(m, seed=11)


def _family(name):
    """(cfg, snapshot of the trained-like checkpoint, reference64 and emulate logits of TOKENS)."""
    if name not in _cache:
        cfg = _cfg(name)
        snap = Snapshot(_trained(name, torch.bfloat16))
        _cache[name] = (cfg, snap, reference64(snap, cfg, TOKENS), emulate(snap, cfg, TOKENS))
    return _cache[name]


def test_rope_table_matches_build_cos_sin():
    diffs = check_rope_tables()
    assert {"llama3-8b", "llama3.2-1b", "mixtral-8x7b"} <= set(diffs)
    # the scaling really acts on the 1B table: its lowest frequency is slowed by the full factor
    cfg = get_config("llama3.2-1b")
    plain = rope_inv_freq64(cfg.head_dim, cfg.rope_theta, None)
    scaled = rope_inv_freq64(cfg.head_dim, cfg.rope_theta, cfg.rope_scaling)
    assert scaled[0] == plain[0] and scaled[-1] == pytest.approx(plain[-1] / 32.0, rel=1e-12)
    assert any(p / 32.0 < s < p for p, s in zip(plain, scaled))  # and the band between is interpolated


@pytest.mark.parametrize("name", MODELS)
def test_reference64_agrees_with_the_model_reference(name):
    """reference64 shares no code with xgserve/models/reference.py (fp32, the model's RoPE
    table); the two must still describe the same function."""
    from xgserve.models.reference import reference_logits
    cfg, snap, ref, _ = _family(name)
    m = _trained(name, torch.float32)
    with torch.no_grad():  # the snapshot's values (bf16-exact), unfolded, in fp32
        for n, p in m.named_parameters():
            p.copy_(snap[n].float())
    other = reference_logits(m, TOKENS)[-1]
    assert rel(other, ref) < 1e-4, rel(other, ref)


@pytest.mark.parametrize("name", MODELS)
def test_every_plant_moves_the_emulation_by_four_bounds(name):
    cfg, snap, ref, emu = _family(name)
    e = rel(emu, ref)
    bound = 2 * e
    print(f"\n{name}: emulate rel {e:.3e}  bound {bound:.3e}  gap {gap(emu, ref):.3e}")
    assert 0 < e < 0.05, e   # bf16 storage noise, not a different function
    worst = None
    for plant in plants_for(cfg):
        d = rel(emulate(snap, cfg, TOKENS, plant=plant), emu)
        print(f"  {plant:20s} displacement {d:.3e} = {d / bound:7.1f} x bound")
        worst = d if worst is None else min(worst, d)
        assert d >= 4 * bound, (plant, d, bound)
        # and the reference sees it as an error of the same size
        assert rel(emulate(snap, cfg, TOKENS, plant=plant), ref) >= 3 * bound, plant
    print(f"  smallest displacement / bound: {worst / bound:.1f}")


@pytest.mark.parametrize("name", ("llama-tiny", "llama-tiny-scaled"))
@pytest.mark.parametrize("kind", ("fp8", "int8", "int4"))
def test_quantized_bounds_still_discriminate(name, kind):
    """A quantized regime is held to the function its quantized checkpoint defines:
    reference64(quant=kind) reads what the codes stand for, as the kernels and emulate(quant=kind)
    do, so the bound is again twice the bf16 storage error and every plant clears 4 x bound.
    (Against the unquantized reference the format's own rounding -- 3 to 14 % for int8 / fp8,
    30 to 80 % for int4 on these random weights -- would be the bound, and would hide them.)"""
    cfg, snap, ref, _ = _family(name)
    refq = reference64(snap, cfg, TOKENS, quant=kind)
    emu = emulate(snap, cfg, TOKENS, quant=kind)
    e = rel(emu, refq)
    bound = 2 * e
    print(f"\n{name} {kind}: emulate rel {e:.3e}  bound {bound:.3e}  format's own error {rel(refq, ref):.3e}")
    assert 0 < e < 0.05, e
    assert rel(refq, ref) > e   # the quantization is really in the reference
    for plant in NORM_PLANTS + ("post_into_qkv", "input_into_gate_up", "rope_q_shift", "kv_page"):
        d = rel(emulate(snap, cfg, TOKENS, plant=plant, quant=kind), emu)
        print(f"  {plant:20s} displacement {d:.3e} = {d / bound:7.1f} x bound")
        assert d >= 4 * bound, (plant, d, bound)


@pytest.mark.parametrize("name", ("llama-tiny", "mixtral-tiny"))
def test_random_init_hides_the_norm_plants(name):
    """Why the regime tests exist: under random_init every norm weight is exactly 1, and the
    four norm plants change nothing at all."""
    cfg = _cfg(name)
    snap = Snapshot(build_model(cfg, device="cpu", dtype=torch.bfloat16, seed=4))
    emu = emulate(snap, cfg, SHORT)
    for plant in NORM_PLANTS:
        assert torch.equal(emulate(snap, cfg, SHORT, plant=plant), emu), plant


def test_gpt2_random_init_hides_the_bias_plants():
    cfg = _cfg("gpt2-tiny")
    snap = Snapshot(build_model(cfg, device="cpu", dtype=torch.bfloat16, seed=4))
    emu = emulate(snap, cfg, SHORT)
    for plant in ("qkv_b", "o_b", "fc_b", "proj_b", "ln_b", "final_norm"):
        assert torch.equal(emulate(snap, cfg, SHORT, plant=plant), emu), plant


def test_trained_like_plants_outliers_and_survives_folding():
    cfg = _cfg("llama-tiny")
    m = trained_like(build_model(cfg, device="cpu", dtype=torch.float32, seed=4), seed=11)
    v = m.layers[0].input_norm
    assert int((v.abs() > 3).sum()) >= 1 and int((v.abs() < 0.15).sum()) >= 1 and int((v < 0).sum()) >= 1
    assert not m.norms_folded
    m.fold_norms()
    assert bool((m.layers[0].input_norm == 1).all()) and not bool((m.norm == 1).all())
    moe = trained_like(build_model(_cfg("mixtral-tiny"), device="cpu", dtype=torch.float32, seed=4), seed=11)
    want = moe.layers[1].post_norm.clone()
    moe.fold_norms()
    assert torch.equal(moe.layers[1].post_norm, want) and bool((moe.layers[1].input_norm == 1).all())


def test_routed_forwards_and_admissible_routings():
    """routed(): under the reference's own routing it is reference64 / emulate and the slack is
    0; a swap of the second choice for the third at the token nearest a tie changes the
    function and is judged by that token's own gap; choosing the worst expert is refused."""
    from _model_ref import _forward, _same, routed
    cfg, snap, ref, emu = _family("mixtral-tiny")
    zr = []
    _forward(snap, cfg, TOKENS, _same, None, trace=zr)
    k = cfg.experts_per_token
    own = [z.topk(k, -1).indices for z in zr]
    slack, allowed, r0, e0 = routed(snap, cfg, TOKENS, own)
    assert slack == 0 and allowed > 0 and torch.equal(r0, ref)
    assert rel(e0, r0) < 0.03   # no routing jump left in the emulation's error
    third = [z.topk(k + 1, -1).indices for z in zr]
    gaps = zr[0].topk(k + 1, -1).values
    t = int((gaps[:, k - 1] - gaps[:, k]).argmin())      # the token nearest a tie in layer 0
    swapped = [o.clone() for o in own]
    swapped[0][t, k - 1] = third[0][t, k]
    slack, allowed, r1, _ = routed(snap, cfg, TOKENS, swapped)
    print(f"\n  nearest tie: slack {slack:.3e} allowed {allowed:.3e} moves the logits by {rel(r1, ref):.3e}")
    assert not torch.equal(r1, ref)   # the routing is part of the function
    if slack > allowed:               # refused: then for the one place that differs, by its own gap
        assert slack == pytest.approx(float(gaps[t, k - 1] - gaps[t, k]), rel=1e-9)
    worst = [o.clone() for o in own]
    worst[0][:, k - 1] = zr[0].argmin(-1)
    slack, allowed, _, _ = routed(snap, cfg, TOKENS, worst)
    assert slack > allowed


def test_quant_last_mixes_the_two_weight_sets():
    """quant_last = n: the last n tokens on the quantized weights, the others on the bf16 ones."""
    cfg, snap, ref, _ = _family("llama-tiny")
    full = reference64(snap, cfg, SHORT, quant="int4")
    assert torch.equal(reference64(snap, cfg, SHORT, quant="int4", quant_last=len(SHORT)), full)
    assert rel(reference64(snap, cfg, SHORT, quant="int4", quant_last=0), reference64(snap, cfg, SHORT)) < 1e-12
    one = reference64(snap, cfg, SHORT, quant="int4", quant_last=1)
    assert rel(one, full) > 0.05 and rel(one, reference64(snap, cfg, SHORT)) > 0.05
