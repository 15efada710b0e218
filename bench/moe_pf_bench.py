#!/usr/bin/env python3
"""Prompt-sized expert GEMMs of a Mixtral 8x7B layer: the grouped gemm_m64g path vs
gemm_pf's grouped form (xgserve/ops/moe.py fused_moe), whole fused_moe calls timed
with events, random routing of T tokens (top-2 of 8). One JSON line per (T, path).
--format fp8: gemm_pf's grouped form (the baseline) vs moe_gemm_f8 on the fp8 expert copies
(fused_moe(wq=..., expert_a8=True): both row quantizers and both grouped launches are inside
the timed call), alternated over --rounds rounds; each line carries the median and the spread."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from xgserve import ops  # noqa: E402
from xgserve.ops import linear as L  # noqa: E402
from xgserve.ops import moe as MOE  # noqa: E402


def timed(fn, iters):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters * 1000


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--T", type=int, nargs="+", default=None, help="tokens (default 575 1024; fp8: 256 575 2048 8000)")
    ap.add_argument("--E", type=int, default=8)
    ap.add_argument("--H", type=int, default=4096)
    ap.add_argument("--F", type=int, default=14336)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--cfg", type=int, nargs="*", default=[], help="gemm_pf tiles to force (6 / 7 / 8)")
    ap.add_argument("--format", choices=["bf16", "fp8"], default="bf16")
    ap.add_argument("--rounds", type=int, default=3, help="fp8: alternations of the two paths")
    ap.add_argument("--f8-plans", type=int, nargs="*", default=[], metavar="CFG S",
                    help="fp8: also time these (cfg, w2 splits) pairs in place of moe_f8_plan's, e.g. 0 1 1 2")
    a = ap.parse_args()
    dev = "cuda"
    E, H, F = a.E, a.H, a.F
    fp8 = a.format == "fp8"
    w13 = (torch.randn(E, 2 * F, H, device=dev) * 0.02).bfloat16()
    w2 = (torch.randn(E, H, F, device=dev) * 0.02).bfloat16()
    wq = L.quantize_expert_stack(w13, L.WQ_FP8) + L.quantize_expert_stack(w2, L.WQ_FP8) + (L.WQ_FP8,) if fp8 else None
    for T in a.T or ([256, 575, 2048, 8000] if fp8 else [575, 1024]):
        x = torch.randn(T, H, device=dev).bfloat16()
        w, ids = ops.moe_topk_softmax(torch.randn(T, E, device=dev), 2)
        rows_max = int(torch.bincount(ids.flatten().long(), minlength=E).max())
        if fp8:
            rule = MOE.moe_f8_plan
            plans = [None] + [tuple(a.f8_plans[i:i + 2]) for i in range(0, len(a.f8_plans), 2)]
            # path -> (the plan rule in force while it is timed, the call); the rule is swapped outside
            # the timed region, as the bf16 form below forces its tiles
            pf, f8 = (lambda: ops.fused_moe(x, w13, w2, w, ids)), (lambda: ops.fused_moe(x, w13, w2, w, ids, wq=wq, expert_a8=True))
            paths = {"pf": (rule, pf)}
            for p in plans:
                paths["f8" if p is None else f"f8_c{p[0]}_S{p[1]}"] = (
                    rule if p is None else (lambda *_, p=p, **__: (p[0], p[0], p[1])), f8)
            ref = pf().float()
            err = float((f8().float() - ref).norm() / ref.norm())
            us = {n: [] for n in paths}
            for rnd in range(a.rounds + 1):   # round 0 warms every path up
                for n, (plan_of, fn) in paths.items():
                    MOE.moe_f8_plan = plan_of
                    t = timed(fn, a.iters if rnd else 3)
                    MOE.moe_f8_plan = rule
                    if rnd:
                        us[n].append(t)
            for n, v in us.items():
                print(json.dumps({"op": "fused_moe", "T": T, "pairs": 2 * T, "path": n, "us": round(statistics.median(v), 1),
                                  "us_min": round(min(v), 1), "us_max": round(max(v), 1),
                                  "plan": list(rule(2 * T, E, H, F)) if n == "f8" else None,
                                  "rel_l2_to_pf": round(err, 5) if n == "f8" else None, "expert_rows_max": rows_max}),
                      flush=True)
            continue
        variants = [("m64g", False, None)] + [("pf", True, None)] + [(f"pf_c{c}", True, c) for c in a.cfg]
        for name, on, cfg in variants:
            MOE.MOE_PF = on
            keep = MOE._moe_pf_cfg
            if cfg is not None:
                MOE._moe_pf_cfg = lambda pairs, E_, c=cfg: c
            timed(lambda: ops.fused_moe(x, w13, w2, w, ids), 3)
            us = timed(lambda: ops.fused_moe(x, w13, w2, w, ids), a.iters)
            MOE._moe_pf_cfg = keep
            print(json.dumps({"op": "fused_moe", "T": T, "path": name, "us": round(us, 1), "expert_rows_max": rows_max}),
                  flush=True)


if __name__ == "__main__":
    main()
