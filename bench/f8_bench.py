"""gemm_f8 (fp8 activations x fp8 weights on the FP8 matrix instructions) beside the two paths it
replaces, at the 8B and 70B projection shapes in their engine modes: cold weights, graph-timed with
gemm_bench.graph_us, the three candidates alternating within one call:

  f8        f8_linear (row quantizer + gemm_f8 on its default plan); "quant" is the quantizer alone
  dq+lib    dequantize_into + F.linear (+ silu_and_mul for gate_up): today's quantized-only prompt step
  bf16      pf_linear on its plan: today's resident prompt step

One JSON line per (shape, M, op): us and achieved TFLOP/s from 2 M N K.
--format int8: the same table for gemm_i8 (int8 weights, per-token int8 activations, INT8 matrix
instructions) beside dequantize + library of the int8 weight and the same bf16 gemm_pf.
--format int4: the same for gemm_i4 (packed int4 weights with 128-k group scales, per-token int8
activations in the kernel's k order).
  python bench/f8_bench.py [--format fp8|int8|int4] [--shapes qkv o gate_up down ...] [--M 384 576 1024 2048 8192]"""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gemm_bench import SHAPES, graph_us  # noqa: E402
from xgserve import ops  # noqa: E402
from xgserve.ops import linear as L  # noqa: E402
from xgserve.ops._native import kernels  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="+", default=["qkv", "o", "gate_up", "down", "qkv70", "o70", "gate_up70", "down70"])
    ap.add_argument("--M", type=int, nargs="+", default=[384, 576, 1024, 2048, 8192])
    ap.add_argument("--format", choices=["fp8", "int8", "int4"], default="fp8")
    a = ap.parse_args()
    kernels()
    fam, fmt, quantize, dequantize, plan_of, linear, quant_rows = {
        "fp8": ("f8", L.WQ_FP8, L.quantize_fp8, L.dequantize_fp8, L.f8_plan, L.f8_linear, L.quant_rows_fp8),
        "int8": ("i8", L.WQ_INT8, L.quantize_int8, L.dequantize_int8, L.i8_plan, L.i8_linear, L.quant_rows_int8),
        "int4": ("i4", L.WQ_INT4, L.quantize_int4, L.dequantize_int4, L.i4_plan, L.i4_linear, L.quant_rows_int8_i4)}[a.format]
    for name in a.shapes:
        N, K = SHAPES[name]
        mode = L.MODE_SILU if name.startswith("gate_up") else L.MODE_PARTIAL
        copies = max(2, min(6, (1 << 30) // (N * K * 2) + 1))
        ws = [(torch.randn(N, K, device="cuda") * 0.02).bfloat16() for _ in range(copies)]
        qs = [quantize(w) for w in ws]
        wd = dequantize(*qs[0])
        scratch = torch.empty(N * K, dtype=torch.bfloat16, device="cuda")
        for M in a.M:
            x = torch.randn(M, K, device="cuda").bfloat16()
            y = x.float() @ wd.t()
            if mode == L.MODE_SILU:
                g, u = L.deinterleave_gate_up(y.t().contiguous())
                y = F.silu(g.t()) * u.t()
            plan = plan_of(M, N, K, mode, L.cu_count())
            got = linear(x, *qs[0], mode)
            got = got.part.sum(0) if mode == L.MODE_PARTIAL else got.float()
            err = float((got - y).norm() / y.norm())
            assert err < 0.1, (name, M, err)   # (E4M3 activations: a few percent; int8: about one)

            def dq(q, sc):
                o = F.linear(x, L.dequantize_into(q, sc, fmt, out=scratch))
                return ops.silu_and_mul(o, interleave16=True) if mode == L.MODE_SILU else o
            fns = {fam: [lambda q=q, sc=sc: linear(x, q, sc, mode) for q, sc in qs],
                   "quant": [lambda: quant_rows(x) for _ in qs],
                   "dq+lib": [lambda q=q, sc=sc: dq(q, sc) for q, sc in qs],
                   "bf16": [lambda w=w: L.pf_linear(x, w, mode) for w in ws]}
            for op, (us, spread) in graph_us(fns).items():
                print(json.dumps({"shape": name, "M": M, "op": op, "us": round(us, 2), "spread": round(spread, 3),
                                  "TFLOP/s": None if op == "quant" else round(2 * M * N * K / us / 1e6, 1),
                                  f"{fam}_plan": list(plan), f"{fam}_rel_err": round(err, 4)}), flush=True)
        del ws, qs, scratch
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
