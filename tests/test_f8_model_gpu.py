"""fp8 activations end to end (quantize_weights(..., a8=True), EngineConfig.fp8_activations): a
400-token prompt step of a quantized-only llama-tiny on gemm_f8 against the fp32 reference of the
unquantized model, next to the same step on today's dequantize + library GEMM path."""
import numpy as np
import pytest
import torch

from _model_ref import rel
from xgserve.ops import _native

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
T = 400


def _model(**quant):
    from xgserve.models import build_model, get_config
    m = build_model(get_config("llama-tiny"), device=DEV, seed=5)
    assert not quant or m.quantize_weights("fp8", quantized_only=True, **quant)
    return m


def _engine(m, **kw):
    from xgserve.engine import EngineConfig, LLMEngine
    return LLMEngine(EngineConfig(model=m.cfg.name, device=DEV, num_blocks=256, max_num_seqs=4,
                                  max_num_batched_tokens=2048, max_model_len=512, graph_batch_sizes=[1], **kw), model=m)


def _last_logits(m, prompt):
    """One prompt step through the model's own forward (the runner's plan, by hand)."""
    from xgserve.engine import SamplingParams
    from xgserve.models.base import AttnMeta
    eng = _engine(m, use_graphs=False)
    eng.add_request("a", prompt, SamplingParams(max_tokens=1, temperature=0.0, ignore_eos=True))
    plan = eng.sched.schedule()
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(DEV)  # noqa: E731
    meta = AttnMeta(num_tokens=int(plan["num_tokens"]), num_decodes=0, positions=t(plan["positions"]),
                    slot_mapping=t(plan["slot_mapping"]), pre_block_tables=t(plan["block_tables"]).view(1, -1),
                    pre_qsl=t(plan["query_start_loc"]), pre_seq_lens=t(plan["seq_lens"]),
                    pre_max_q=int(plan["q_lens"].max()))
    assert meta.num_tokens == T
    h = m(t(plan["input_ids"]), meta, eng.runner.kv_caches)
    return m.compute_logits(h[-1:]).float()[0]


def test_prompt_step_on_f8_follows_the_reference():
    """rel(F) <= 2 rel(D): D's error is the fp8 weight error on today's path; E4M3 activations
    carry the same 3-bit mantissa, independent errors of equal size combine to about sqrt(2) of it,
    and the rest of the factor is room for per-row against per-channel scale granularity."""
    from xgserve.engine import SamplingParams
    from xgserve.models.reference import reference_logits
    _native.kernels()
    prompt = [1] + [3 + (7 * i) % 500 for i in range(T - 1)]
    R, D, F = _model(), _model(a8=False), _model(a8=True)
    assert all(l.dispatch.select(T, 0)[:4] == ("dq",) * 4 for l in D.layers)
    assert all(tuple(l.dispatch.select(T, 0)) == ("f8",) * 4 + ("from_partials",) for l in F.layers)
    with pytest.raises(ValueError):
        _model().quantize_weights("int8", a8=True)
    ref = reference_logits(R, prompt)[-1].float()
    rd, rf = rel(_last_logits(D, prompt), ref), rel(_last_logits(F, prompt), ref)
    print(f"rel to the fp32 reference of the bf16 model: dequantize + library {rd:.5f}, gemm_f8 {rf:.5f}")
    assert 0 < rf <= 2 * rd, (rf, rd)
    # greedy tokens of the engine: each within 0.15 in logit of the reference's best, over D's dequantized weights
    eng = _engine(F, fp8_activations=True)
    assert eng.stats()["activation_dtype"] == "fp8" and _engine(D).stats()["activation_dtype"] == "bf16"
    gen = eng.generate([prompt], SamplingParams(max_tokens=8, temperature=0.0, ignore_eos=True))[0]
    from xgserve.ops.linear import dequantize_weight
    with torch.no_grad():
        for lr, ld in zip(R.layers, D.layers):
            for n, q in ld.w8.items():
                getattr(lr, n).copy_(dequantize_weight(*q).to(torch.bfloat16))
    rows = reference_logits(R, prompt + gen[:-1]).float()[T - 1:]
    gaps = [float(r.max() - r[tok]) for r, tok in zip(rows, gen)]
    print(f"worst reference-logit gap of a greedy token {max(gaps):.4f}")
    assert len(gen) == 8 and max(gaps) < 0.15, gaps
