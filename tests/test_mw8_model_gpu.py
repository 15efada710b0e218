"""Quantized-only models (llama-tiny in every format, a 2-layer Llama-3-8B in int4) whose 65..320-row
steps run on gemm_mw8 (quantize_weights(..., mw8=True)): 96-row mixed steps (decode rows + a prompt
chunk) against the fp32 reference over the dequantized weights, at the bound
tests/test_quantized_only_gpu.py holds its "dq" steps to -- and the "dq" form (mw8=False) at the
same bound in the same test."""
from dataclasses import replace

import pytest
import torch

from xgserve.models import llama as ll
from xgserve.ops import _native
from xgserve.ops.linear import MODE_PARTIAL, MODE_SILU, WQ_FORMATS, dequantize_weight, mw8_plan, quantize_weight

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAMES = ("qkv", "o", "gate_up", "down")
BUDGET = 96


def _model(name, kind, quantize, mw8=False):
    from xgserve.models import build_model, get_config
    cfg = get_config(name)
    m = build_model(cfg if cfg.num_layers <= 2 else replace(cfg, num_layers=2, name=f"{name}-2l-mw8"), device=DEV, seed=5)
    fmt = WQ_FORMATS[kind]
    with torch.no_grad():   # quantizing these weights again loses (nearly) nothing
        for layer in m.layers:
            for n in NAMES:
                w = getattr(layer, n)
                w.copy_(dequantize_weight(*quantize_weight(w, fmt), fmt).to(w.dtype))
    if quantize:
        assert m.quantize_weights(kind, quantized_only=True, mw8=mw8)
    return m


def test_every_projection_of_llama_tiny_has_a_plan():
    from xgserve.models import get_config
    shapes = ll.LayerDispatch.for_layer(get_config("llama-tiny"), 1, on_gpu=True).shapes
    assert set(shapes) == set(NAMES) and shapes["gate_up"][2] == MODE_SILU and shapes["down"][2] == MODE_PARTIAL
    assert all(mw8_plan(T, *s, fmt) is not None for s in shapes.values() for fmt in WQ_FORMATS.values()
               for T in (65, BUDGET, 320))


@pytest.mark.parametrize("name,kind", [("llama-tiny", "fp8"), ("llama-tiny", "int8"), ("llama-tiny", "int4"),
                                       ("llama3-8b", "int4")])
def test_mixed_steps_match_reference(name, kind, monkeypatch):
    from xgserve.engine import EngineConfig, LLMEngine, SamplingParams
    from xgserve.models.reference import reference_logits
    _native.kernels()
    ref_model = _model(name, kind, quantize=False)
    rows = []
    real = ll.mw8_linear
    monkeypatch.setattr(ll, "mw8_linear", lambda x, *a, **kw: (rows.append(x.shape[0]), real(x, *a, **kw))[1])
    prompts = [[1] + list(range(10 + 3 * i, 30 + 3 * i)) for i in range(24)] + [[1] + list(range(40, 400))]
    for mw8 in (True, False):
        m = _model(name, kind, quantize=True, mw8=mw8)
        want = ("mw8",) * 4 if mw8 else ("dq",) * 4
        assert all(l.dispatch.select(T, 8)[:4] == want for l in m.layers for T in (65, BUDGET, 320))
        eng = LLMEngine(EngineConfig(model=m.cfg.name, device=DEV, num_blocks=256, max_num_seqs=32,
                                     max_num_batched_tokens=BUDGET, max_model_len=512, graph_batch_sizes=[1, 2]),
                        model=m)
        del rows[:]
        outs = eng.generate(prompts, SamplingParams(max_tokens=8, temperature=0.0, ignore_eos=True))
        # the step's dispatch: every projection of full mixed steps ran on gemm_mw8 (or never, mw8 off)
        assert (rows.count(BUDGET) >= 4 * len(m.layers)) if mw8 else not rows, rows
        worst = 0.0
        for p, gen in zip(prompts, outs):
            ref = reference_logits(ref_model, p + gen[:-1]).float()
            for i, tok in enumerate(gen):
                row = ref[len(p) - 1 + i]
                gap = float(row.max() - row[tok])
                worst = max(worst, gap)
                assert gap < 0.15, (mw8, i, tok, int(row.argmax()), gap)
        print(f"{name} {kind} mw8={mw8}: worst reference-logit gap of a greedy token {worst:.4f}; gemm_mw8 rows {sorted(set(rows))}")
        del eng, m


def test_captured_decode_graph_runs_mw8(monkeypatch):
    """80 sequences decode as replays of a captured 96-row graph whose projections were recorded on
    gemm_mw8: the same reference bound, and the same tokens as the eager engine."""
    from xgserve.engine import EngineConfig, LLMEngine, SamplingParams
    from xgserve.models.reference import reference_logits
    ref_model = _model("llama-tiny", "int4", quantize=False)
    m = _model("llama-tiny", "int4", quantize=True, mw8=True)
    rows = []
    real = ll.mw8_linear
    monkeypatch.setattr(ll, "mw8_linear", lambda x, *a, **kw: (rows.append(x.shape[0]), real(x, *a, **kw))[1])
    prompts = [[1] + list(range(10 + 3 * i, 22 + 3 * i)) for i in range(80)]
    sp = SamplingParams(max_tokens=8, temperature=0.0, ignore_eos=True)
    outs = {}
    for graphs in (True, False):
        eng = LLMEngine(EngineConfig(model=m.cfg.name, device=DEV, num_blocks=512, max_num_seqs=96, use_graphs=graphs,
                                     max_num_batched_tokens=2048, max_model_len=256, graph_batch_sizes=[96]), model=m)
        assert (96 in rows) == graphs   # recorded while the graph was warmed and captured
        del rows[:]
        outs[graphs] = eng.generate(prompts, sp)
        # decode steps of 80 rows: replays (no Python call of the wrapper), or eager calls of 80 rows
        assert (80 in rows) == (not graphs) and 96 not in rows, sorted(set(rows))
        del rows[:], eng
    assert outs[True] == outs[False]
    for p, gen in zip(prompts, outs[True]):
        ref = reference_logits(ref_model, p + gen[:-1]).float()
        for i, tok in enumerate(gen):
            row = ref[len(p) - 1 + i]
            assert float(row.max() - row[tok]) < 0.15, (i, tok, int(row.argmax()))
