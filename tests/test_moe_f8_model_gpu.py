"""fp8 expert activations end to end (quantize_weights("fp8", ea8=True), EngineConfig.fp8_expert_activations): a
400-token prompt step (800 token-expert pairs) of mixtral-tiny with its experts on moe_gemm_f8, against the fp32
reference of the unquantized model and next to the bf16 path on the dequantized fp8 expert weights. Every
model's qkv / o hold fp8-representable values, so the quantized decode steps after the prompt and the reference
compute one function outside the experts. The step and the engine are test_f8_model_gpu.py's."""
import pytest
import torch

from _model_ref import rel
from test_f8_model_gpu import DEV, T, _engine, _last_logits
from xgserve.ops.linear import WQ_FP8, dequantize_weight, quantize_weight

pytestmark = pytest.mark.gpu


def _model(**quant):
    from xgserve.models import build_model, get_config
    m = build_model(get_config("mixtral-tiny"), device=DEV, seed=5)
    with torch.no_grad():
        for w in [w for l in m.layers for w in (l.qkv, l.o)]:
            w.copy_(dequantize_weight(*quantize_weight(w, WQ_FP8), WQ_FP8).to(w.dtype))
    assert not quant or m.quantize_weights("fp8", **quant)
    return m


def _decode_logits(m, ea8):
    """Logits of a 160-row pure decode step (320 pairs) with the layers' switch at `ea8`, after the same fill
    (one 320-token prompt step) with the switch off."""
    from xgserve.engine import EngineConfig, LLMEngine, SamplingParams
    eng = LLMEngine(EngineConfig(model=m.cfg.name, device=DEV, num_blocks=256, max_num_seqs=160, use_graphs=False,
                                 max_num_batched_tokens=2048, max_model_len=64), model=m)
    eng.runner.capture_logits = True
    for i in range(160):
        eng.add_request(str(i), [1, 5 + i], SamplingParams(max_tokens=4, temperature=0.0, ignore_eos=True))
    for on in (False, ea8):
        for l in m.layers:
            l.ea8 = on
        eng.step()
    c = eng.stats_counters
    assert (c["steps"], c["decode_steps"], eng.runner.last_logits.shape[0]) == (2, 1, 160)
    return eng.runner.last_logits


def test_prompt_step_on_moe_f8_follows_the_reference():
    """rel(F) <= 2 rel(D), the bound and the reasoning of tests/test_f8_model_gpu.py: D's error is the fp8
    expert-weight error on the bf16 path; E4M3 activations carry the same 3-bit mantissa, independent errors of
    equal size combine to about sqrt(2) of it, and the rest is room for per-row against per-channel scales."""
    from xgserve.engine import SamplingParams
    from xgserve.models.reference import reference_logits
    prompt = [1] + [3 + (7 * i) % 500 for i in range(T - 1)]
    R, W, D, F = _model(), _model(ea8=False), _model(), _model(ea8=True)
    assert all(l.ea8 for l in F.layers) and not any(l.ea8 for l in W.layers)
    for kind, kw in (("int8", {}), ("fp8", {"quantized_only": True})):
        with pytest.raises(ValueError):
            _model().quantize_weights(kind, ea8=True, **kw)
    ref, plain = reference_logits(R, prompt)[-1].float(), _last_logits(R, prompt)
    # without the switch the step reads the bf16 experts on the kernels of an unquantized model, bit for bit
    assert torch.equal(_last_logits(W, prompt), plain)
    # ... and a pure decode step keeps its kernels with the switch on, however many pairs it has
    assert torch.equal(_decode_logits(F, False), _decode_logits(F, True)) and all(l.ea8 for l in F.layers)
    with torch.no_grad():
        for ld, lw in zip(D.layers, W.layers):
            for n, e in ((n, e) for n in ("w13", "w2") for e in range(lw.w8[n][0].shape[0])):
                q, s, fmt = lw.w8[n]
                getattr(ld, n)[e].copy_(dequantize_weight(q[e], s[e], fmt).to(torch.bfloat16))
    rd, rf = rel(_last_logits(D, prompt), ref), rel(_last_logits(F, prompt), ref)
    print(f"rel to the fp32 reference: bf16 {rel(plain, ref):.5f}, dequantized fp8 experts {rd:.5f}, moe_gemm_f8 {rf:.5f}")
    assert 0 < rf <= 2 * rd, (rf, rd)
    # greedy tokens of the engine: each within 0.15 in logit of the reference's best, over D's weights
    eng = _engine(F, fp8_expert_activations=True)
    assert (eng.stats()["expert_activation_dtype"], eng.stats()["activation_dtype"]) == ("fp8", "bf16")
    assert _engine(W).stats()["expert_activation_dtype"] == "bf16"
    gen = eng.generate([prompt], SamplingParams(max_tokens=8, temperature=0.0, ignore_eos=True))[0]
    rows = reference_logits(D, prompt + gen[:-1]).float()[T - 1:]
    gaps = [float(r.max() - r[tok]) for r, tok in zip(rows, gen)]
    print(f"worst reference-logit gap of a greedy token {max(gaps):.4f}")
    assert len(gen) == 8 and max(gaps) < 0.15, gaps
