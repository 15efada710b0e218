"""Quantized-only serving on the MI355X (LlamaForCausalLM.quantize_weights(kind,
quantized_only=True)): the bf16 projection weights really leave HBM, the engine's
prompt steps (dequantize into the shared scratch + library GEMM) and decode steps
(gemm_w8) follow the fp32 reference, and the freed bytes reach the KV pool."""
import gc
from dataclasses import replace

import pytest
import torch

from xgserve.ops import _native
from xgserve.ops.linear import WQ_FORMATS, WQ_GROUP, WQ_INT4, dequantize_weight, quantize_weight

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
KINDS = ["int8", "int4", "fp8"]
NAMES = ("qkv", "o", "gate_up", "down")
MIB = 1 << 20


@pytest.fixture(autouse=True, scope="module")
def _k():
    _native.kernels()  # fail loudly: the HIP library must be the one that runs
    torch.manual_seed(0)


def _cfg(kind):
    from xgserve.models import get_config
    return replace(get_config("llama3-8b"), num_layers=2, name=f"llama3-8b-2l-qonly-{kind}")


def _free():
    gc.collect()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def _allocated():
    _free()
    return torch.cuda.memory_allocated()


def _build(kind, quantized_only, requantized=False, quantize=True):
    """The 2-layer model, seed 5. requantized: the projection weights replaced by their
    dequantized values first, so quantizing them again loses (nearly) nothing."""
    from xgserve.models import build_model
    fmt = WQ_FORMATS[kind]
    if quantize and not requantized:  # the public way in
        m = build_model(_cfg(kind), device=DEV, seed=5, weight_dtype=kind, quantized_only=quantized_only)
        assert m.weight_dtype == kind
        return m
    m = build_model(_cfg(kind), device=DEV, seed=5)
    if requantized:
        with torch.no_grad():
            for layer in m.layers:
                for n in NAMES:
                    w = getattr(layer, n)
                    w.copy_(dequantize_weight(*quantize_weight(w, fmt), fmt).to(w.dtype))
    if quantize:
        assert m.quantize_weights(kind, quantized_only=quantized_only) and m.weight_dtype == kind
    return m


def _projection_shapes(cfg):
    D, H, F = cfg.head_dim, cfg.hidden_size, cfg.intermediate_size
    return [((cfg.num_heads + 2 * cfg.num_kv_heads) * D, H), (H, cfg.num_heads * D), (2 * F, H), (H, F)]


@pytest.mark.parametrize("kind", KINDS)
def test_footprint(kind):
    cfg = _cfg(kind)
    fmt = WQ_FORMATS[kind]
    shapes = _projection_shapes(cfg)
    a0 = _allocated()
    res = _build(kind, quantized_only=False)
    a_res = _allocated() - a0
    assert res.scratch_bytes() == 0 and not res.quantized_only
    n_tensors = len(list(res.parameters())) + 2 * len(NAMES) * cfg.num_layers + 16  # + scratch, RoPE table, workspaces
    bf16_proj = 2 * cfg.num_layers * sum(n * k for n, k in shapes)
    assert res.weight_bytes() == sum(p.numel() * 2 for p in res.parameters()) + sum(
        q.numel() + 4 * s.numel() for l in res.layers for q, s, _ in l.w8.values())
    del res
    a1 = _allocated()
    m = _build(kind, quantized_only=True)
    a_q = _allocated() - a1
    # the formula: embedding, LM head and norms at 2 B per element; each projection at its quantized size
    H, V = cfg.hidden_size, cfg.vocab_size
    want = 2 * (V * H + (0 if m.lm_head is None else m.lm_head.numel()) + H + cfg.num_layers * 2 * H)
    for n, k in shapes:
        per = n * k // 2 + 4 * (k // WQ_GROUP) * n if fmt == WQ_INT4 else n * k + 4 * n
        want += cfg.num_layers * per
    assert m.weight_bytes() == want
    assert m.scratch_bytes() == 2 * max(n * k for n, k in shapes)
    assert m.quantized_only and all(not hasattr(l, n) for l in m.layers for n in NAMES)
    assert all(l.released[n] == s for l in m.layers for n, s in zip(NAMES, shapes))
    print(f"{kind}: allocated resident {a_res / MIB:.1f} MiB, quantized-only {a_q / MIB:.1f} MiB, "
          f"released bf16 {bf16_proj / MIB:.1f} MiB, scratch {m.scratch_bytes() / MIB:.1f} MiB, "
          f"weight_bytes {m.weight_bytes() / MIB:.1f} MiB")
    # 2 MiB per tensor: the caching allocator's large-block rounding
    assert a_res - a_q >= bf16_proj - m.scratch_bytes() - 2 * MIB * n_tensors
    from xgserve.models import save_checkpoint
    with pytest.raises(ValueError):
        save_checkpoint(m, "/nonexistent/never-written")


def _check_against_reference(ref_model, eng, prompts):
    from xgserve.engine import SamplingParams
    from xgserve.models.reference import reference_logits
    outs = eng.generate(prompts, SamplingParams(max_tokens=8, temperature=0.0, ignore_eos=True))
    worst = 0.0
    for p, gen in zip(prompts, outs):
        assert len(gen) == 8
        ref = reference_logits(ref_model, p + gen[:-1]).float()
        for i, tok in enumerate(gen):
            row = ref[len(p) - 1 + i]
            gap = float(row.max() - row[tok])
            worst = max(worst, gap)
            assert gap < 0.15, (i, tok, int(row.argmax()), gap)
    return worst


@pytest.mark.parametrize("kind", KINDS)
def test_engine_matches_reference(kind):
    """Every greedy token of the quantized-only engine is (within 0.15 in logit) an
    argmax of the fp32 reference over the same weights, held by a second, resident
    model: one prompt step of several hundred rows (budget 2048), then chunked prompt
    steps of 65..256 rows mixed with decode rows (budget 256); decode graphs on."""
    from xgserve.engine import EngineConfig, LLMEngine
    ref_model = _build(kind, quantized_only=False, requantized=True, quantize=False)
    m = _build(kind, quantized_only=True, requantized=True)
    assert all(l.dispatch.select(T, 0)[:4] == ("dq",) * 4 for l in m.layers for T in (65, 256, 725))
    prompts = [[128000] + list(range(200 + 7 * i, 260 + 11 * i)) for i in range(3)]
    prompts += [[128000] + list(range(900 + 3 * i, 930 + 3 * i)) for i in range(17)]  # 20 rows: the MT=4 kernel
    for budget in (2048, 256):
        eng = LLMEngine(EngineConfig(model=m.cfg.name, device=DEV, num_blocks=512, max_num_seqs=32,
                                     max_num_batched_tokens=budget, max_model_len=1024,
                                     graph_batch_sizes=[1, 2, 4, 8]), model=m)
        st = eng.stats()
        assert st["weight_bytes"] == m.weight_bytes() and st["scratch_bytes"] == m.scratch_bytes()
        assert st["weight_dtype"] == kind
        worst = _check_against_reference(ref_model, eng, prompts)
        print(f"{kind} budget {budget}: worst reference-logit gap of a greedy token {worst:.4f}")
        del eng
        _free()


def test_auto_num_blocks_gets_the_freed_bytes():
    from xgserve.engine import EngineConfig, LLMEngine
    kind = "int4"
    blocks = []
    for quantized_only in (False, True):
        _free()
        m = _build(kind, quantized_only=quantized_only)
        eng = LLMEngine(EngineConfig(model=m.cfg.name, device=DEV, num_blocks=None, max_num_seqs=8,
                                     max_num_batched_tokens=256, max_model_len=256, graph_batch_sizes=[1],
                                     gpu_memory_utilization=0.3), model=m)
        assert eng.model.quantized_only is quantized_only
        blocks.append(eng.num_blocks)
        del eng, m
    _free()
    print(f"auto num_blocks: resident {blocks[0]}, quantized-only {blocks[1]}")
    assert blocks[1] >= blocks[0]
