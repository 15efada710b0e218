"""Time ops.spec_verify_sample on a verify step's worth of sampled blocks against what the
step's sampler alone costs on the same target rows.

  64 blocks, k = 4, V = 128256, bf16: 320 target rows + 256 draft rows.
  A: ops.spec_verify_sample (three launches + one small H2D of the block descriptors)
  B: ops.sample_tokens on the 320 target rows (what a verify step spends sampling anyway)
With --top-p / --top-k every block is truncated: the draft draws with them, A runs the six
launches of the truncated form and B samples with them too.

Device events around windows of `--iters` back-to-back calls, after a warm-up of every
shape; the two are alternated window by window inside one process and the median and the
spread over `--windows` windows are printed as one JSON line. Bytes read are computed from
the shapes: the stats pass reads every row once, the draw pass every target row and the
draft rows of the residual positions once more (from L2 / MALL where they still sit).
Needs a GPU: there is no fallback.
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from xgserve import ops  # noqa: E402
from xgserve.ops import _native  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=64)
    ap.add_argument("--k", type=int, default=4)
    ap.add_argument("--vocab", type=int, default=128256)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--top-p", type=float, default=1.0)
    ap.add_argument("--top-k", type=int, default=0)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("spec_sample_bench: needs a GPU")
    _native.kernels()
    dev = "cuda"
    nb, k, V = a.blocks, a.k, a.vocab
    Lp, Lq = nb * (k + 1), nb * k
    g = torch.Generator().manual_seed(0)
    p = (torch.randn(Lp, V, generator=g) * 3).to(torch.bfloat16).to(dev)
    rows = np.concatenate([np.arange(j * (k + 1), j * (k + 1) + k) for j in range(nb)])
    q = (p[torch.from_numpy(rows).to(dev)].float() + torch.randn(Lq, V, generator=g).to(dev) * 0.3).to(torch.bfloat16)
    ks = np.full(nb, k, np.int64)
    temps = np.full(nb, 0.8, np.float32)
    seeds = np.arange(1, Lp + 1, dtype=np.int64) * 7919
    p_row0, q_row0 = np.arange(nb) * (k + 1), np.arange(nb) * k
    qt = torch.from_numpy(np.repeat(temps, k)).to(dev)
    trunc = a.top_p < 1.0 or a.top_k > 0
    tkw = dict(top_ps=np.full(nb, a.top_p, np.float32), top_ks=np.full(nb, a.top_k, np.int32)) if trunc else {}

    def rows_of(n):  # per-row top_p / top_k tensors for ops.sample_tokens
        if not trunc:
            return None, None
        return (torch.full((n,), a.top_p, dtype=torch.float32, device=dev),
                torch.full((n,), a.top_k, dtype=torch.int32, device=dev))

    draft, _ = ops.sample_tokens(q, qt, *rows_of(Lq), torch.from_numpy(seeds[:Lq].copy()).to(dev), step=0)
    draft = draft.contiguous()
    pt = torch.from_numpy(np.repeat(temps, k + 1)).to(dev)
    pseeds = torch.from_numpy(seeds).to(dev)

    def run_a():
        return ops.spec_verify_sample(p, q, draft, p_row0, q_row0, q_row0, ks, temps, seeds, **tkw)

    def run_b():
        return ops.sample_tokens(p, pt, *rows_of(Lp), pseeds, step=0)

    for _ in range(a.warmup):
        run_a()
        run_b()
    torch.cuda.synchronize()
    acc = run_a()[2]
    torch.cuda.synchronize()
    mean_acc = float(acc.float().mean())

    def window(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.iters):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / a.iters

    ta, tb = [], []
    for _ in range(a.windows):
        ta.append(window(run_a))
        tb.append(window(run_b))
    esz = p.element_size()
    read = (Lp + Lq) * V * esz + (Lp + Lq) * V * esz  # stats pass + draw pass
    res = {"bench": "spec_verify_sample", "blocks": nb, "k": k, "vocab": V, "dtype": "bf16",
           "top_p": a.top_p, "top_k": a.top_k,
           "spec_verify_ms_median": round(statistics.median(ta), 4), "spec_verify_ms_min": round(min(ta), 4),
           "spec_verify_ms_max": round(max(ta), 4),
           "sample_tokens_ms_median": round(statistics.median(tb), 4), "sample_tokens_ms_min": round(min(tb), 4),
           "sample_tokens_ms_max": round(max(tb), 4),
           "bytes_read": read, "read_GBps_at_median": round(read / statistics.median(ta) / 1e6, 1),
           "mean_accepted": round(mean_acc, 3), "iters": a.iters, "windows": a.windows}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
