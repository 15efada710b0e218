#!/usr/bin/env python3
"""Prefill attention (K5) throughput on one MI355X: one sequence of L new tokens
(no cached prefix) over the paged KV cache, causal, for L in --lens, Llama-3-8B
(32 q / 8 kv heads) and Llama-3-70B (64 / 8) head layouts, every GQA head-group
width `gh` (query heads per workgroup). TFLOP/s counts the causal work:
4 * Hq * D * L (L + 1) / 2. Also --ttft: end-to-end batch-1 TTFT of one
--ttft-len-token prompt through the engine (random-init Llama-3-8B, bf16, or
--quantization fp8|int8|int4 with or without --quantized-only; --ttft-only skips the
attention sweep), followed by the tok/s of --batch prompts of --batch-prompt-len
tokens generating --batch-out tokens each (prompt steps and decode steps together)."""
import argparse
import json
import math
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from xgserve import ops  # noqa: E402
from xgserve.ops._native import kernels  # noqa: E402


def bench_attn(L, Hq, Hkv, D, gh, iters=20, bs=16):
    n_pages = (L + bs - 1) // bs
    kc = (torch.randn(n_pages, Hkv, bs, D, device="cuda") * 0.5).bfloat16()
    vc = torch.randn(n_pages, Hkv, bs, D, device="cuda").bfloat16()
    bt = torch.randperm(n_pages, device="cuda", dtype=torch.int32)[None, :].contiguous()
    q = torch.randn(L, Hq, D, device="cuda").bfloat16()
    qsl = torch.tensor([0, L], dtype=torch.int32, device="cuda")
    sl = torch.tensor([L], dtype=torch.int32, device="cuda")
    out = torch.empty_like(q)
    fn = lambda: ops.prefill_attention(q, kc, vc, bt, qsl, sl, L, 1.0 / math.sqrt(D), out=out, gh=gh)  # noqa: E731
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    us = s.elapsed_time(e) / iters * 1000.0
    flops = 4.0 * Hq * D * L * (L + 1) / 2
    return us, flops / us / 1e6


def ttft(L, quantization=None, quantized_only=False, batch=0, batch_prompt_len=512, batch_out=64, default_graphs=False,
         fp8_activations=False, int8_activations=False, model="llama3-8b", fp8_expert_activations=False):
    from xgserve.engine import EngineConfig, LLMEngine, SamplingParams
    wdt = quantization if quantization in ("fp8", "int8", "int4") else None
    # default_graphs: the engine's own decode graph sizes (up to max_num_seqs; above 64 rows too)
    bs = None if default_graphs else sorted({1, *(b for b in (2, 4, 8, 16, 32, 64) if b <= batch)})
    eng = LLMEngine(EngineConfig(model=model, max_num_seqs=max(4, batch), max_num_batched_tokens=max(8192, L),
                                 max_model_len=max(L, batch_prompt_len + batch_out) + 16, graph_batch_sizes=bs,
                                 weight_dtype=wdt, quantized_only=quantized_only,
                                 fp8_activations=fp8_activations, int8_activations=int8_activations,
                                 fp8_expert_activations=fp8_expert_activations))
    res = []
    for it in range(4):
        prompt = torch.randint(10, min(128000, eng.mcfg.vocab_size), (L,)).tolist()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        eng.add_request(f"t{it}", prompt, SamplingParams(max_tokens=1, temperature=0.0, ignore_eos=True))
        done = False
        while not done:
            for o in eng.step():
                if o.new_token_ids:
                    done = True
        res.append(1000 * (time.perf_counter() - t0))
        eng.clear_prefix_cache()
    extra = dict(eng.stats())
    extra = {k: extra[k] for k in ("weight_bytes", "scratch_bytes", "weight_dtype", "kv_blocks_total")}
    if batch > 0:
        sp = SamplingParams(max_tokens=batch_out, temperature=0.0, ignore_eos=True)
        for it in range(2):  # the second run is the measured one
            prompts = [torch.randint(10, min(128000, eng.mcfg.vocab_size), (batch_prompt_len,)).tolist() for _ in range(batch)]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            outs = eng.generate(prompts, sp)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            eng.clear_prefix_cache()
        extra.update(batch=batch, batch_prompt_len=batch_prompt_len, batch_out=batch_out,
                     batch_s=round(dt, 4), output_tok_s=round(sum(len(o) for o in outs) / dt, 1))
    return res, extra


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lens", type=int, nargs="*", default=[512, 2048, 8192])
    ap.add_argument("--gh", type=int, nargs="+", default=[0, 4, -44, -84, -82, -1284, -1282, -1281])
    ap.add_argument("--ttft-len", type=int, default=8000)
    ap.add_argument("--no-ttft", action="store_true")
    ap.add_argument("--ttft-only", action="store_true", help="skip the attention sweep")
    ap.add_argument("--quantization", default="bf16", choices=["bf16", "fp8", "int8", "int4"])
    ap.add_argument("--quantized-only", action="store_true",
                    help="release the bf16 projection weights (prompt steps dequantize into a scratch)")
    ap.add_argument("--batch", type=int, default=0, help="also time this many prompts generating together")
    ap.add_argument("--batch-prompt-len", type=int, default=512)
    ap.add_argument("--batch-out", type=int, default=64)
    ap.add_argument("--default-graphs", action="store_true",
                    help="capture the engine's default decode graph sizes instead of 1..64 (batches above 64 replay graphs)")
    ap.add_argument("--fp8-activations", action="store_true",
                    help="with --quantization fp8: prompt steps above 320 rows on gemm_f8 (activations quantized per token)")
    ap.add_argument("--fp8-activations-pair", action="store_true",
                    help="with --quantization fp8: the TTFT without and then with fp8 activations, in this one call")
    ap.add_argument("--int8-activations", action="store_true",
                    help="with --quantization int8 / int4: prompt steps above 320 rows on gemm_i8 / gemm_i4 (activations quantized per token)")
    ap.add_argument("--int8-activations-pair", action="store_true",
                    help="with --quantization int8 / int4: the TTFT without and then with int8 activations, in this one call")
    ap.add_argument("--model", default="llama3-8b", help="the TTFT runs' model (mixtral-8x7b for the expert pair)")
    ap.add_argument("--fp8-expert-activations-pair", action="store_true",
                    help="with --quantization fp8 --model mixtral-8x7b: the TTFT without and then with fp8 expert "
                         "activations (moe_gemm_f8), in this one call")
    a = ap.parse_args()
    kernels()
    for name, Hq, Hkv in (("llama3-8b", 32, 8), ("llama3-70b", 64, 8)):
        for L in ([] if a.ttft_only else a.lens):
            for gh in a.gh:
                us, tf = bench_attn(L, Hq, Hkv, 128, gh)
                print(json.dumps({"op": "prefill_attention", "heads": name, "L": L, "gh": gh, "us": round(us, 1),
                                  "TFLOP/s": round(tf, 1)}), flush=True)
    runs = ([(False, False, False), (False, False, True)] if a.fp8_expert_activations_pair else
            [(False, False, False), (True, False, False)] if a.fp8_activations_pair else
            [(False, False, False), (False, True, False)] if a.int8_activations_pair else
            [(a.fp8_activations, a.int8_activations, False)])
    for a8, ai8, ea8 in ([] if a.no_ttft else runs):
        r, extra = ttft(a.ttft_len, a.quantization, a.quantized_only, a.batch, a.batch_prompt_len, a.batch_out,
                        a.default_graphs, a8, ai8, a.model, ea8)
        torch.cuda.empty_cache()
        print(json.dumps({"op": "ttft_batch1", "model": a.model, "prompt_len": a.ttft_len,
                          "quantization": a.quantization, "quantized_only": a.quantized_only, "fp8_activations": a8,
                          "int8_activations": ai8, "fp8_expert_activations": ea8,
                          "ttft_ms": [round(x, 2) for x in r], "ttft_ms_best_of_last3": round(min(r[1:]), 2),
                          **extra}), flush=True)


if __name__ == "__main__":
    main()
