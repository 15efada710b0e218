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


def ttft(L, quantization=None, quantized_only=False, batch=0, batch_prompt_len=512, batch_out=64):
    from xgserve.engine import EngineConfig, LLMEngine, SamplingParams
    wdt = quantization if quantization in ("fp8", "int8", "int4") else None
    bs = sorted({1, *(b for b in (2, 4, 8, 16, 32, 64) if b <= batch)})
    eng = LLMEngine(EngineConfig(model="llama3-8b", max_num_seqs=max(4, batch), max_num_batched_tokens=max(8192, L),
                                 max_model_len=max(L, batch_prompt_len + batch_out) + 16, graph_batch_sizes=bs,
                                 weight_dtype=wdt, quantized_only=quantized_only))
    res = []
    for it in range(4):
        prompt = torch.randint(10, 128000, (L,)).tolist()
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
            prompts = [torch.randint(10, 128000, (batch_prompt_len,)).tolist() for _ in range(batch)]
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
    a = ap.parse_args()
    kernels()
    for name, Hq, Hkv in (("llama3-8b", 32, 8), ("llama3-70b", 64, 8)):
        for L in ([] if a.ttft_only else a.lens):
            for gh in a.gh:
                us, tf = bench_attn(L, Hq, Hkv, 128, gh)
                print(json.dumps({"op": "prefill_attention", "heads": name, "L": L, "gh": gh, "us": round(us, 1),
                                  "TFLOP/s": round(tf, 1)}), flush=True)
    if not a.no_ttft:
        r, extra = ttft(a.ttft_len, a.quantization, a.quantized_only, a.batch, a.batch_prompt_len, a.batch_out)
        print(json.dumps({"op": "ttft_batch1", "model": "llama3-8b", "prompt_len": a.ttft_len,
                          "quantization": a.quantization, "quantized_only": a.quantized_only,
                          "ttft_ms": [round(x, 2) for x in r], "ttft_ms_best_of_last3": round(min(r[1:]), 2),
                          **extra}), flush=True)


if __name__ == "__main__":
    main()
