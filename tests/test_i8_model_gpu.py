"""int8 activations end to end (quantize_weights(..., ai8=True), EngineConfig.int8_activations): a
400-token prompt step of a quantized-only llama-tiny on gemm_i8 against the fp32 reference of the
unquantized model, next to the same step on the dequantize + library GEMM path."""
import pytest
import torch

from _model_ref import rel
from test_f8_model_gpu import DEV, T, _engine, _last_logits
from xgserve.ops import _native

pytestmark = pytest.mark.gpu


def _model(**quant):
    from xgserve.models import build_model, get_config
    m = build_model(get_config("llama-tiny"), device=DEV, seed=5)
    assert not quant or m.quantize_weights("int8", quantized_only=True, **quant)
    return m


def test_prompt_step_on_i8_follows_the_reference():
    """rel(I) <= 2 rel(D): D's error is the int8 weight error on the dequantize path; per-token int8
    activations add an independent error of about the same size (a fp32 CPU emulation of this step
    gives 1.45-1.52 at three seeds), and bf16 noise common to both paths only lowers the ratio."""
    from xgserve.engine import SamplingParams
    from xgserve.models.reference import reference_logits
    from xgserve.ops.linear import dequantize_weight
    _native.kernels()
    prompt = [1] + [3 + (7 * i) % 500 for i in range(T - 1)]
    R, D, I = _model(), _model(ai8=False), _model(ai8=True)
    assert all(l.dispatch.select(T, 0)[:4] == ("dq",) * 4 for l in D.layers)
    assert all(tuple(l.dispatch.select(T, 0)) == ("i8",) * 4 + ("from_partials",) for l in I.layers)
    with pytest.raises(ValueError):
        _model().quantize_weights("fp8", ai8=True)
    ref = reference_logits(R, prompt)[-1].float()
    rd, ri = rel(_last_logits(D, prompt), ref), rel(_last_logits(I, prompt), ref)
    print(f"rel to the fp32 reference of the bf16 model: dequantize + library {rd:.5f}, gemm_i8 {ri:.5f}")
    assert 0 < ri <= 2 * rd, (ri, rd)
    # greedy tokens of the engine: each within 0.15 in logit of the reference's best, over D's dequantized weights
    eng = _engine(I, int8_activations=True)
    assert eng.stats()["activation_dtype"] == "int8" and _engine(D).stats()["activation_dtype"] == "bf16"
    gen = eng.generate([prompt], SamplingParams(max_tokens=8, temperature=0.0, ignore_eos=True))[0]
    with torch.no_grad():
        for lr, ld in zip(R.layers, D.layers):
            for n, q in ld.w8.items():
                getattr(lr, n).copy_(dequantize_weight(*q).to(torch.bfloat16))
    rows = reference_logits(R, prompt + gen[:-1]).float()[T - 1:]
    gaps = [float(r.max() - r[tok]) for r, tok in zip(rows, gen)]
    print(f"worst reference-logit gap of a greedy token {max(gaps):.4f}")
    assert len(gen) == 8 and max(gaps) < 0.15, gaps
