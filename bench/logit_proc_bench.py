#!/usr/bin/env python3
"""Cost of the logit processors on one MI355X.

Kernel part: process_logits + logit_state_update at 64 x 128256 bf16 logits with every
row penalised (tracked slot, all three penalties, 16 bias entries; with and without
min_p), and the two samplers on the bf16 logits and on the fp32 scratch. Device time per
call from a HIP graph of several calls that rotate over SETS buffer sets, so that a call
finds as little as possible of its inputs in the 256 MB last-level cache.
Bytes: what the pass must move -- logits 2 B + state cell 2 B + scratch 4 B per logit,
and the min_p pass reads the scratch again (4 B; its writes are the masked tokens only).

Engine part (--engine): wall time per decode step of 64 rows, all plain against all
penalised, same model.

Prints one JSON line per measurement."""
import argparse
import json
import math
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from xgserve import ops  # noqa: E402

DEV = "cuda:0"
SETS = 4


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
        for f in fns:
            f()
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            for f in fns:
                f()
    torch.cuda.synchronize()
    return timeit(g.replay) / len(fns)


def kernels(rows, V):
    rng = np.random.default_rng(0)
    nb = ops.LOGIT_BIAS_MAX
    state = ops.logit_state_alloc(rows, V, DEV)
    resets = []
    for s in range(rows):  # a 512-token prompt and 256 generated tokens per slot
        ids, cells = ops.logit_state_cells(rng.integers(0, V, 512), rng.integers(0, V, 256))
        resets.append((s, ids, cells))
    packed, nres, total = ops.pack_state_resets(resets)
    ops.logit_state_reset(state, torch.from_numpy(packed).to(DEV), nres, total)
    pi = np.zeros((3, rows), np.int32)
    pi[0] = np.arange(rows)
    pi[1] = np.arange(rows) * nb
    pi[2] = 16
    pf = np.zeros((4, rows), np.float32)
    pf[0], pf[1], pf[2] = 1.2, 0.5, 0.5
    bias_ids = torch.from_numpy(rng.integers(0, V, rows * nb).astype(np.int32)).to(DEV)
    bias_vals = torch.from_numpy(rng.uniform(-5, 5, rows * nb).astype(np.float32)).to(DEV)
    temps = torch.full((rows,), 0.8, device=DEV)
    top_ps = torch.ones(rows, device=DEV)
    top_ks = torch.zeros(rows, dtype=torch.int32, device=DEV)
    seeds = torch.arange(rows, dtype=torch.int64, device=DEV)
    logits = [(torch.randn(rows, V, device=DEV) * 3).to(torch.bfloat16) for _ in range(SETS)]
    outs = [ops.process_scratch(rows, V, DEV) for _ in range(SETS)]
    toks = torch.from_numpy(rng.integers(0, V, rows).astype(np.int32)).to(DEV)
    res = []

    def emit(op, us, nbytes=None, **kw):
        r = {"op": op, "rows": rows, "V": V, "us": round(us, 2), **kw}
        if nbytes:
            r["GBps"] = round(nbytes / us / 1e3, 1)
        print(json.dumps(r), flush=True)
        res.append(r)

    for name, lm, bpl in (("penalties+bias", -math.inf, 8), ("penalties+bias+min_p", math.log(0.05), 12)):
        pf[3] = lm
        d_pi, d_pf = torch.from_numpy(pi).to(DEV), torch.from_numpy(pf.copy()).to(DEV)

        def step(k, d_pi=d_pi, d_pf=d_pf):
            ops.process_logits(logits[k], outs[k], state, d_pi, d_pf, temps, bias_ids, bias_vals)
            ops.logit_state_update(state, d_pi[0], toks, rows)

        us = graphed([lambda k=k % SETS: step(k) for k in range(2 * SETS)])
        emit(f"process_logits({name})+logit_state_update", us, rows * V * bpl, bytes_per_logit=bpl)
    plain_pi = pi.copy()
    plain_pi[0], plain_pi[2] = -1, 0
    plain_pf = np.zeros((4, rows), np.float32)
    plain_pf[0], plain_pf[3] = 1.0, -math.inf
    d_pi, d_pf = torch.from_numpy(plain_pi).to(DEV), torch.from_numpy(plain_pf).to(DEV)
    us = graphed([lambda k=k % SETS: ops.process_logits(logits[k], outs[k], state, d_pi, d_pf, temps) for k in
                  range(2 * SETS)])
    emit("process_logits(plain rows: bf16 -> fp32 only)", us, rows * V * 6, bytes_per_logit=6)
    for label, src, bpl in (("bf16", logits, 2), ("fp32 scratch", outs, 4)):
        us = graphed([lambda k=k % SETS: ops.argmax_logprob(src[k]) for k in range(2 * SETS)])
        emit(f"argmax_logprob({label})", us, rows * V * bpl)
        us = graphed([lambda k=k % SETS: ops.sample_tokens(src[k], temps, top_ps, top_ks, seeds) for k in
                      range(2 * SETS)])
        emit(f"sample_tokens(T=0.8, {label})", us, rows * V * bpl)
        tp = torch.full((rows,), 0.9, device=DEV)
        us = graphed([lambda k=k % SETS: ops.sample_tokens(src[k], temps, tp, top_ks, seeds) for k in range(2 * SETS)])
        emit(f"sample_tokens(T=0.8, top_p=0.9, {label})", us)
    return res


def engine(model_name, layers, rows, steps):
    from dataclasses import replace
    from xgserve.engine import EngineConfig, LLMEngine, SamplingParams
    from xgserve.models import build_model, get_config
    cfg = get_config(model_name)
    if layers:
        cfg = replace(cfg, num_layers=layers, name=f"{model_name}-{layers}l")
    model = build_model(cfg, device=DEV, seed=0)
    eng = LLMEngine(EngineConfig(model=cfg.name, device=DEV, max_num_seqs=rows, max_num_batched_tokens=8192,
                                 max_model_len=2048, graph_batch_sizes=[rows], num_blocks=rows * 64 + 64), model=model)
    pen = dict(repetition_penalty=1.2, frequency_penalty=0.5, presence_penalty=0.5,
               logit_bias={100 + i: 1.0 for i in range(16)})
    for label, kw in (("plain", {}), ("penalised", pen), ("plain", {}), ("penalised", pen)):
        for i in range(rows):
            eng.add_request(f"{label}-{i}-{time.monotonic_ns()}", [1] + list(range(1000 + i, 1128 + i)),
                            SamplingParams(max_tokens=steps + 16, temperature=0.0, ignore_eos=True, **kw))
        for _ in range(12):  # prompts + graph capture at first need + warm steps
            eng.step()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            eng.step()
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) / steps * 1e3
        while eng.has_work():
            eng.step()
        print(json.dumps({"op": f"engine decode step ({label})", "model": cfg.name, "rows": rows,
                          "ms_per_step": round(ms, 4), "steps": steps}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=64)
    ap.add_argument("--vocab", type=int, default=128256)
    ap.add_argument("--engine", action="store_true", help="also time the engine's decode step, plain vs penalised")
    ap.add_argument("--model", default="llama3-8b")
    ap.add_argument("--layers", type=int, default=0, help="truncate the model to this many layers (0: all)")
    ap.add_argument("--steps", type=int, default=60)
    a = ap.parse_args()
    kernels(a.rows, a.vocab)
    if a.engine:
        engine(a.model, a.layers, a.rows, a.steps)


if __name__ == "__main__":
    main()
