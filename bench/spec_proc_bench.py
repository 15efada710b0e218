#!/usr/bin/env python3
"""Cost of processed speculation on one MI355X.

Kernel part: process_logits with per-row extra history over 64 verify blocks of k + 1 = 4
rows (256 rows x 128256 bf16 logits; every block on a tracked slot with all three
penalties and 16 bias entries; row i of a block takes the block's first i draft tokens,
lists of length 0..3) against the plain process_logits on the same 256 rows, and
logit_state_add over 64 x 4 entries. Device time per call from a HIP graph of several
calls that rotate over SETS buffer sets (bench/logit_proc_bench.py), so that a call finds
as little as possible of its inputs in the 256 MB last-level cache. Bytes: logits 2 B +
state cell 2 B + scratch 4 B per logit.

Engine part (--engine): a self-draft run of greedy requests with and without penalties,
spec.processors on: stats()["speculative"]["speedup_factor"] and the acceptance rate.

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
from logit_proc_bench import DEV, SETS, graphed  # noqa: E402


def kernels(blocks, k, V):
    rng = np.random.default_rng(0)
    nb, rows = ops.LOGIT_BIAS_MAX, blocks * (k + 1)
    state = ops.logit_state_alloc(blocks, V, DEV)
    resets = []
    for s in range(blocks):  # a 512-token prompt and 256 generated tokens per slot
        ids, cells = ops.logit_state_cells(rng.integers(0, V, 512), rng.integers(0, V, 256))
        resets.append((s, ids, cells))
    packed, nres, total = ops.pack_state_resets(resets)
    ops.logit_state_reset(state, torch.from_numpy(packed).to(DEV), nres, total)
    slot = np.repeat(np.arange(blocks), k + 1)
    pi = np.zeros((3, rows), np.int32)
    pi[0], pi[1], pi[2] = slot, slot * nb, 16
    pf = np.zeros((4, rows), np.float32)
    pf[0], pf[1], pf[2], pf[3] = 1.2, 0.5, 0.5, -math.inf
    hp = np.zeros((2, rows), np.int32)
    hp[0], hp[1] = slot * k, np.tile(np.arange(k + 1), blocks)
    hist = rng.integers(0, V, blocks * k).astype(np.int32)
    ops.check_hist_pos(hp, len(hist), rows)
    d = lambda a: torch.from_numpy(a).to(DEV)  # noqa: E731
    d_pi, d_pf, d_hp, d_hist = d(pi), d(pf), d(hp), d(hist)
    bias_ids = d(rng.integers(0, V, blocks * nb).astype(np.int32))
    bias_vals = d(rng.uniform(-5, 5, blocks * nb).astype(np.float32))
    temps = torch.zeros(rows, device=DEV)
    logits = [(torch.randn(rows, V, device=DEV) * 3).to(torch.bfloat16) for _ in range(SETS)]
    outs = [ops.process_scratch(rows, V, DEV) for _ in range(SETS)]

    def emit(op, us, nbytes=None, **kw):
        r = {"op": op, "rows": rows, "V": V, "us": round(us, 2), **kw}
        if nbytes:
            r["GBps"] = round(nbytes / us / 1e3, 1)
        print(json.dumps(r), flush=True)

    us0 = graphed([lambda j=j % SETS: ops.process_logits(logits[j], outs[j], state, d_pi, d_pf, temps, bias_ids,
                                                         bias_vals) for j in range(2 * SETS)])
    emit("process_logits(penalties+bias), plain kernel", us0, rows * V * 8, bytes_per_logit=8)
    us1 = graphed([lambda j=j % SETS: ops.process_logits(logits[j], outs[j], state, d_pi, d_pf, temps, bias_ids,
                                                         bias_vals, hist_ids=d_hist, hist_pos=d_hp)
                   for j in range(2 * SETS)])
    emit(f"process_logits(penalties+bias), history kernel, lists of 0..{k}", us1, rows * V * 8, bytes_per_logit=8,
         over_plain=round(us1 / us0, 4))
    n = blocks * (k + 1)
    a_slots = d(np.repeat(np.arange(blocks), k + 1).astype(np.int32))
    a_toks = d(rng.integers(0, V, n).astype(np.int32))
    us = graphed([lambda: ops.logit_state_add(state, a_slots, a_toks, n) for _ in range(2 * SETS)])
    emit(f"logit_state_add({blocks} x {k + 1} entries)", us)


def engine(model_name, layers, rows, tokens, k):
    from dataclasses import replace
    from xgserve.engine import EngineConfig, LLMEngine, SamplingParams
    from xgserve.models import build_model, get_config
    cfg = get_config(model_name)
    if layers:
        cfg = replace(cfg, num_layers=layers, name=f"{model_name}-{layers}l")
    model = build_model(cfg, device=DEV, seed=0)
    pen = dict(repetition_penalty=1.2, frequency_penalty=0.5, presence_penalty=0.5,
               logit_bias={100 + i: 1.0 for i in range(16)})
    for label, kw in (("plain", {}), ("penalised", pen)):
        eng = LLMEngine(EngineConfig(model=cfg.name, device=DEV, max_num_seqs=rows, max_num_batched_tokens=8192,
                                     max_model_len=2048, graph_batch_sizes=[rows], num_blocks=rows * 64 + 64,
                                     draft_model=model, num_speculative_tokens=k, spec_processors=True), model=model)
        for i in range(rows):
            eng.add_request(f"{label}-{i}", [1] + list(range(1000 + i, 1128 + i)),
                            SamplingParams(max_tokens=tokens, temperature=0.0, ignore_eos=True, **kw))
        t0 = time.perf_counter()
        steps = 0
        while eng.has_work():
            eng.step()
            steps += 1
        torch.cuda.synchronize()
        wall = time.perf_counter() - t0
        # the plain decode step of the same rows and processors: sampled requests, which this
        # engine (spec_sampled off) decodes one token per step
        for i in range(rows):
            eng.add_request(f"{label}-plain-{i}", [1] + list(range(1000 + i, 1128 + i)),
                            SamplingParams(max_tokens=32, temperature=0.8, seed=i, ignore_eos=True, **kw))
        while eng.has_work():
            eng.step()
        torch.cuda.synchronize()
        st = eng.stats()["speculative"]
        print(json.dumps({"op": f"self-draft engine run ({label})", "model": cfg.name, "rows": rows, "k": k,
                          "tokens_per_request": tokens, "steps": steps, "wall_s": round(wall, 3),
                          "acceptance_rate": round(st["acceptance_rate"], 4), "speedup_factor": st["speedup_factor"],
                          "spec_step_ms": st["spec_step_ms"], "plain_decode_step_ms": st["plain_decode_step_ms"],
                          "processed_draft_tokens_proposed": st["processed_draft_tokens_proposed"]}), flush=True)
        del eng


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=64)
    ap.add_argument("--k", type=int, default=3)
    ap.add_argument("--vocab", type=int, default=128256)
    ap.add_argument("--engine", action="store_true", help="also a self-draft engine run, plain vs penalised")
    ap.add_argument("--model", default="llama3-8b")
    ap.add_argument("--layers", type=int, default=0, help="truncate the model to this many layers (0: all)")
    ap.add_argument("--rows", type=int, default=8)
    ap.add_argument("--tokens", type=int, default=64)
    a = ap.parse_args()
    kernels(a.blocks, a.k, a.vocab)
    if a.engine:
        engine(a.model, a.layers, a.rows, a.tokens, a.k)


if __name__ == "__main__":
    main()
