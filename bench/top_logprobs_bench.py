#!/usr/bin/env python3
"""Cost of top_logprobs on one MI355X.

Kernel part: ops.top_logprobs at B x 128256 logits, B in {1, 8, 64}, bf16 and fp32,
K in {5, 20}, against ops.argmax_logprob on the same rows -- the project's one-pass floor
for the same bytes. Device time per call from a HIP graph of calls that rotate over
several buffer sets (as many as give a footprint above the 256 MB last-level cache, at
most MAX_SETS), so that a call finds as little as possible of its input in a cache; the
footprint is printed with every line. Bytes: the logits, read once.

Engine part (--engine): wall time per decode step of `rows` rows with no row asking, one
row asking and all rows asking for 20 alternatives, each case `--repeats` times in turn,
so the spread of a case is seen next to the differences between cases. --cases none runs
on a tree that has no top_logprobs at all (the parent commit's).

Prints one JSON line per measurement."""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from xgserve import ops  # noqa: E402

DEV = "cuda:0"
MAX_SETS = 128
L3_BYTES = 256 << 20


def timeit(fn, iters=20, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters * 1000.0  # us


def graphed(fns):
    """device time per call: the calls captured in one HIP graph (no host launch cost)"""
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        for f in fns[:2]:
            f()
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            for f in fns:
                f()
    torch.cuda.synchronize()
    return timeit(g.replay) / len(fns)


def kernels(V, batches):
    for dtype, name, esz in ((torch.bfloat16, "bf16", 2), (torch.float32, "fp32", 4)):
        for B in batches:
            row_bytes = B * V * esz
            sets = int(min(MAX_SETS, max(4, -(-2 * L3_BYTES // row_bytes))))
            big = torch.empty(sets * B, V, dtype=dtype, device=DEV)
            for k in range(sets):  # filled set by set: no fp32 temporary of the whole footprint
                big[k * B:(k + 1) * B] = (torch.randn(B, V, device=DEV) * 3).to(dtype)
            xs = [big[k * B:(k + 1) * B] for k in range(sets)]
            temps = torch.full((B,), 0.8, device=DEV)
            tok = torch.empty(B, dtype=torch.int32, device=DEV)
            lp = torch.empty(B, dtype=torch.float32, device=DEV)
            base = graphed([lambda k=k: ops.argmax_logprob(xs[k], tok, lp) for k in range(sets)])
            common = {"B": B, "V": V, "dtype": name, "sets": sets, "footprint_MB": round(sets * row_bytes / 2**20, 1)}
            print(json.dumps({"op": "argmax_logprob", **common, "us": round(base, 2),
                              "GBps": round(row_bytes / base / 1e3, 1)}), flush=True)
            for K in (5, 20):
                ids = torch.empty(B, K, dtype=torch.int32, device=DEV)
                lps = torch.empty(B, K, dtype=torch.float32, device=DEV)
                us = graphed([lambda k=k: ops.top_logprobs(xs[k], temps, K, None, ids, lps) for k in range(sets)])
                print(json.dumps({"op": "top_logprobs", "K": K, **common, "us": round(us, 2),
                                  "GBps": round(row_bytes / us / 1e3, 1), "ratio_to_argmax": round(us / base, 2)}),
                      flush=True)
            del big, xs


def engine(model_name, layers, rows, steps, repeats, cases):
    from dataclasses import replace
    from xgserve.engine import EngineConfig, LLMEngine, SamplingParams
    from xgserve.models import build_model, get_config
    cfg = get_config(model_name)
    if layers:
        cfg = replace(cfg, num_layers=layers, name=f"{model_name}-{layers}l")
    model = build_model(cfg, device=DEV, seed=0)
    eng = LLMEngine(EngineConfig(model=cfg.name, device=DEV, max_num_seqs=rows, max_num_batched_tokens=8192,
                                 max_model_len=2048, graph_batch_sizes=[rows], num_blocks=rows * 64 + 64), model=model)
    asking = {"none": lambda i: 0, "one": lambda i: 20 if i == 0 else 0, "all": lambda i: 20}
    for rep in range(repeats):
        for label in cases:
            for i in range(rows):
                k = asking[label](i)
                kw = {"top_logprobs": k} if k else {}
                eng.add_request(f"{label}-{rep}-{i}", [1] + list(range(1000 + i, 1128 + i)),
                                SamplingParams(max_tokens=steps + 16, temperature=0.0, ignore_eos=True, **kw))
            for _ in range(12):  # prompts + warm steps
                eng.step()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                eng.step()
            torch.cuda.synchronize()
            ms = (time.perf_counter() - t0) / steps * 1e3
            while eng.has_work():
                eng.step()
            print(json.dumps({"op": f"engine decode step ({label} asking)", "model": cfg.name, "rows": rows,
                              "repeat": rep, "ms_per_step": round(ms, 4), "steps": steps}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--vocab", type=int, default=128256)
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 8, 64])
    ap.add_argument("--no-kernels", action="store_true")
    ap.add_argument("--engine", action="store_true", help="time the engine's decode step: no / one / all rows asking")
    ap.add_argument("--cases", nargs="+", default=["none", "one", "all"], choices=["none", "one", "all"])
    ap.add_argument("--model", default="llama3-8b")
    ap.add_argument("--layers", type=int, default=0, help="truncate the model to this many layers (0: all)")
    ap.add_argument("--rows", type=int, default=64)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=3)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("top_logprobs_bench: needs a GPU")
    if not a.no_kernels:
        kernels(a.vocab, a.batches)
    if a.engine:
        engine(a.model, a.layers, a.rows, a.steps, a.repeats, a.cases)


if __name__ == "__main__":
    main()
