"""int8 activations on an int4 model end to end: a 400-token prompt step of a quantized-only llama-tiny on
gemm_i4 against the fp32 reference of the unquantized model, next to the dequantize + library GEMM path."""
import pytest
import torch

from _model_ref import rel
from test_f8_model_gpu import DEV, T, _engine, _last_logits

pytestmark = pytest.mark.gpu


def _model(**quant):
    from xgserve.models import build_model, get_config
    m = build_model(get_config("llama-tiny"), device=DEV, seed=5)
    assert not quant or m.quantize_weights("int4", quantized_only=True, **quant)
    return m


def test_prompt_step_on_i4_follows_the_reference():
    """rel(I4) <= 1.34 rel(D). A fp32 CPU emulation of this step gives rel(D) / rel(I4) of 0.21408 /
    0.21515, 0.25277 / 0.25214 and 0.25769 / 0.26231 at seeds 5, 6, 7 (ratios 1.005, 0.998, 1.018); the
    worst times the margin the int8 test allows itself (its 1.52 became 2) is 1.34."""
    from xgserve.engine import SamplingParams
    from xgserve.models.reference import reference_logits
    from xgserve.ops.linear import dequantize_weight
    prompt = [1] + [3 + (7 * i) % 500 for i in range(T - 1)]
    R, D, I = _model(), _model(ai8=False), _model(ai8=True)
    assert all(d.dispatch.select(T, 0)[:4] == ("dq",) * 4 and i.dispatch.select(T, 0)[:4] == ("i4",) * 4 for d, i in zip(D.layers, I.layers))
    ref = reference_logits(R, prompt)[-1].float()
    rd, ri = rel(_last_logits(D, prompt), ref), rel(_last_logits(I, prompt), ref)
    assert 0 < ri <= 1.34 * rd, (ri, rd)   # rel to the fp32 reference; below: greedy tokens within 0.15 of its best logit
    eng = _engine(I, int8_activations=True)
    assert eng.stats()["activation_dtype"] == "int8"
    gen = eng.generate([prompt], SamplingParams(max_tokens=8, temperature=0.0, ignore_eos=True))[0]
    with torch.no_grad():
        for lr, ld in zip(R.layers, D.layers):
            for n, q in ld.w8.items():
                getattr(lr, n).copy_(dequantize_weight(*q).to(torch.bfloat16))
    rows = reference_logits(R, prompt + gen[:-1]).float()[T - 1:]
    gaps = [float(r.max() - r[tok]) for r, tok in zip(rows, gen)]
    assert len(gen) == 8 and max(gaps) < 0.15, gaps
