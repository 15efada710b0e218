"""Prompt scoring: log-probability of a given token, best token and its log-probability per
hidden row, without a logits buffer (csrc/kernels/lm_head_score.hip)."""
from __future__ import annotations

import torch

from ._native import kernels, stream_ptr, use_native


def score_tile():
    """(BM, BN) of the kernel's tile: rows and vocabulary columns per workgroup."""
    return tuple(kernels().lm_head_score_tile())


def score_rows_ref(h: torch.Tensor, w: torch.Tensor, V: int, targets: torch.Tensor):
    """fp32 log_softmax reference of score_rows (CPU runs, the fp32 GPT-2)."""
    lsm = torch.log_softmax(torch.nn.functional.linear(h.float(), w[:V].float()), dim=-1)
    best_lp, best_id = lsm.max(dim=-1)
    t = targets.long()
    has = (t >= 0) & (t < V)
    lp = lsm.gather(1, t.clamp(0, V - 1).unsqueeze(1)).squeeze(1)
    return torch.where(has, lp, torch.zeros_like(lp)), best_id.to(torch.int32), best_lp


def _dma_ready(t: torch.Tensor) -> torch.Tensor:
    """The kernel's LDS-DMA reads 16 B at a time: unit column stride, a row stride that is a multiple
    of 8 elements and a 16-B aligned base. Anything else is copied."""
    if t.stride(1) == 1 and t.stride(0) % 8 == 0 and t.data_ptr() % 16 == 0:
        return t
    return t.contiguous() if not t.is_contiguous() else t.clone()


def score_rows(h: torch.Tensor, w: torch.Tensor, V: int, targets: torch.Tensor):
    """h [M, K] (final-norm output), LM-head weight w [>= V, K], targets int32 [M] (-1 or any value
    outside [0, V): no target) -> (lp fp32 [M], best_id int32 [M], best_lp fp32 [M]) of the raw
    (temperature 1) distribution over v < V: lp = z[t] - logsumexp(z), 0 for a row with no target;
    best_id = argmax z (lowest index of a tie); best_lp = max z - logsumexp(z)."""
    M, K = h.shape
    if V < 1 or V > w.shape[0] or w.shape[1] != K or targets.shape != (M,):
        raise ValueError(f"score_rows: h {tuple(h.shape)}, w {tuple(w.shape)}, V {V}, targets {tuple(targets.shape)}")
    if not use_native(h) or h.dtype != torch.bfloat16 or w.dtype != torch.bfloat16:
        return score_rows_ref(h, w, V, targets)
    h, w = _dma_ready(h), _dma_ready(w)
    k = kernels()
    targets = targets.to(device=h.device, dtype=torch.int32).contiguous()
    lp = torch.empty(M, dtype=torch.float32, device=h.device)
    best_id = torch.empty(M, dtype=torch.int32, device=h.device)
    best_lp = torch.empty(M, dtype=torch.float32, device=h.device)
    ws = torch.empty(k.lm_head_score_ws_floats(M, V), dtype=torch.float32, device=h.device)
    k.lm_head_score(h.data_ptr(), h.stride(0), M, K, w.data_ptr(), w.stride(0), V, targets.data_ptr(), ws.data_ptr(),
                    lp.data_ptr(), best_id.data_ptr(), best_lp.data_ptr(), stream_ptr())
    return lp, best_id, best_lp
