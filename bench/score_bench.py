#!/usr/bin/env python3
"""Prompt scoring on one MI355X: ops.score_rows (lm_head_score.hip, no logits buffer) against the
pieces that existed before it -- lm_head_linear, then top_logprobs(n = 1), then a gather of the
target's logit and the row's log-sum-exp -- at the 8B LM head (V = 128,256, K = 4,096) and
M = 128, 512, 2,048 rows.

Per case: device time per call (events around `--iters` calls after a warm-up, `--repeats` times, the
median and the range printed) and the peak of extra device memory one call allocates (outputs and
temporaries; the operands are not counted). The weight (1.05 GB) is four times the 256 MB last-level
cache, so every call streams it from HBM. Prints one JSON line per measurement."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from xgserve import ops  # noqa: E402
from xgserve.ops.linear import lm_head_linear  # noqa: E402

DEV = "cuda:0"


def unfused(h, w, V, targets, temps):
    logits = lm_head_linear(h, w)[:, :V]
    ids, lps = ops.top_logprobs(logits, temps, 1)
    z_t = logits.gather(1, targets.clamp(min=0).long()[:, None])[:, 0].float()
    # top_logprobs gives max - lse; the target's logprob needs the lse itself
    lse = logits.gather(1, ids.long())[:, 0].float() - lps[:, 0]
    return torch.where(targets >= 0, z_t - lse, torch.zeros_like(z_t)), ids[:, 0], lps[:, 0]


def measure(fn, iters, repeats):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    extra = torch.cuda.max_memory_allocated() - base
    us = []
    for _ in range(repeats):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(iters):
            fn()
        e.record()
        torch.cuda.synchronize()
        us.append(s.elapsed_time(e) / iters * 1e3)
    return statistics.median(us), min(us), max(us), extra


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--vocab", type=int, default=128256)
    ap.add_argument("--hidden", type=int, default=4096)
    ap.add_argument("--rows", type=int, nargs="+", default=[128, 512, 2048])
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("score_bench: needs a GPU")
    V, K = a.vocab, a.hidden
    g = torch.Generator(device=DEV).manual_seed(0)
    w = (torch.randn(V, K, device=DEV, generator=g) * 0.02).bfloat16()
    for M in a.rows:
        h = torch.randn(M, K, device=DEV, generator=g).bfloat16()
        targets = torch.randint(0, V, (M,), device=DEV, generator=g, dtype=torch.int32)
        temps = torch.zeros(M, device=DEV)
        got, want = ops.score_rows(h, w, V, targets), unfused(h, w, V, targets, temps)
        agree = {"lp_max_diff": float((got[0] - want[0]).abs().max()),  # the unfused path rounds logits to bf16
                 "best_id_equal": float((got[1] == want[1]).float().mean())}
        for name, fn in (("score_rows", lambda: ops.score_rows(h, w, V, targets)),
                         ("lm_head_linear+top_logprobs+gather", lambda: unfused(h, w, V, targets, temps))):
            med, lo, hi, extra = measure(fn, a.iters, a.repeats)
            print(json.dumps({"op": name, "M": M, "V": V, "K": K, "us": round(med, 1), "us_min": round(lo, 1),
                              "us_max": round(hi, 1), "TFLOPs": round(2.0 * M * V * K / med / 1e6, 1),
                              "extra_MB": round(extra / 2**20, 2), **agree}), flush=True)


if __name__ == "__main__":
    main()
