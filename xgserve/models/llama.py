"""Llama-3 (8B / 70B / 3.2-1B) and Mixtral-8x7B decoders on the paged-KV engine.

Tensor parallelism (Megatron layout, one process per GPU, RCCL/xGMI):
  * fused QKV and gate_up projections are column-parallel (heads / FFN split),
  * o_proj and down_proj are row-parallel followed by one all-reduce each,
  * the LM head is vocab-parallel (logits all-gathered), the embedding is
    replicated (2 GB for 70B -- negligible in 288 GB of HBM).
Expert parallelism (Mixtral): EP == TP group, rank r owns experts
[r*E/tp, (r+1)*E/tp). Two exchange forms, chosen per step by moe_comm "auto" (the
default: allreduce for decode-sized steps on the custom IPC all-reduce, all_to_all
for prefill-sized ones) or forced with "alltoall" / "allreduce":
  * "alltoall" (prefill steps under "auto"; BASELINE config 5): each rank routes its
    token slice, packs (token, choice) rows for the expert owners with the HIP
    ep_plan / ep_scatter kernels (count-exact splits on eager prefill steps,
    fixed capacity under graph capture), runs its local experts as one grouped
    GEMM, returns rows with a second all_to_all, combines them with ep_combine
    and all-gathers the slices;
  * "allreduce": every rank runs its local experts on all tokens and one
    all-reduce sums the partial outputs.
Per layer the hot path is one chain (LlamaLayer.forward): add + RMSNorm -> QKV GEMM
-> RoPE + KV append + paged decode / varlen prefill attention -> O GEMM (-> AR) ->
add + RMSNorm -> gate_up GEMM with the SiLU gate -> down GEMM (-> AR). LayerDispatch
picks each projection's GEMM kernel from the step size: gemm_w8 (quantized copies)
or gemm_m64g up to 64 tokens (skinny_gemm up to 16 where gemm_m64g has no small-M
plan), gemm_mw up to 320, gemm_pf inside its measured windows, else the library.
A quantized-only model (quantize_weights(kind, quantized_only=True)) has no bf16
projection weights: above 64 tokens each projection is dequantized (dequant.hip)
into one shared bf16 scratch that the library GEMM reads, except that its steps of
65..320 tokens run the projections that have a gemm_mw8 plan on the codes themselves
("mw8": models quantized with mw8=True, as the engine does; a resident model too, where
MW8_RESIDENT lists a measured shape).
The HIP GEMMs hand split-K partials to their consumer (the attention prologue or
add + RMSNorm) and gate inside gate_up; the library GEMMs are followed by rope_cache
and silu_and_mul launches. Pure-decode steps of dense and MoE models normally take
the fused decode layer instead (forward_fused, below).
"""
from __future__ import annotations

import functools
import os
from typing import List, NamedTuple, Optional, Tuple

import torch
import torch.nn as nn
import torch.nn.functional as F

from .. import ops, tune
from ..parallel import comm
from ..parallel.state import get_state
from ..ops import linear as linear_mod
from ..ops.linear import (MODE_BF16, MODE_PARTIAL, MODE_SILU, MW_MAX_M, W8_MAX_M, W8_MIN_ELEMS, PendingSum,
                          ResidWorkspace, RowStats, dequantize_into, lm_head_linear, m64_ar_resid_linear,
                          m64_linear, m64_plan, m64_resid_linear,
                          f8_linear, f8_plan, i4_linear, i4_plan, i8_linear, i8_plan, mw8_linear, mw8_plan, mw_linear, mw_plan, pf_linear, pf_plan,
                          quantize_expert_stack, quantize_fp8, quantize_weight, skinny_linear, splitk_linear, splitk_prefill_ok, w8_linear,
                          w8_plan, WQ_FORMATS)
from ..ops.moe import MOE_PREFILL_PAIRS, moe_f8_plan, moe_w8_plan
from .base import AttnMeta, PagedAttention, init_weight, kv_head_range, local_heads, shard
from .config import ModelConfig



FAST_M_SMALL = 16   # tokens per step on the streaming skinny GEMM (shapes without a small-M gemm_m64g plan)
FAST_M_SLAB = 64    # tokens per step on gemm_m64g (and on gemm_w8)
# Fused decode layer (dense Llama, TP=1, pure-decode steps of <= 64 tokens): the
# RMSNorms become GEMM epilogue row scales (norm weights folded into W), the
# residual adds + norm statistics run inside the O / down GEMM launches and the
# QKV reduce + RoPE + KV append inside the attention prologue: 4 GEMM launches +
# 1 attention launch per layer instead of 9. Under TP the O / down GEMMs emit
# split-K partials and ONE custom all-reduce launch per projection reduces them,
# sums across ranks over xGMI, adds the residual and writes the next norm's
# statistics (comm.tp_allreduce_resid): 6 launches + attention per layer instead
# of 11. XGS_TUNE fused_decode=0 restores the unfused chain (A/B measurements, tests).
FUSED_DECODE = tune.get_bool("fused_decode", True)
# 64 < T <= this many tokens (the mixed step: decode rows + one bounded prefill chunk)
# run every projection on gemm_mw (csrc/kernels/gemm_mw.hip): weight-stream-bound
# MFMA GEMMs whose split-K partials go to the consumers, SiLU-gate in gate_up.
# 0 = hipBLASLt for every step above 64 tokens.
MW_MAX_TOKENS = min(MW_MAX_M, tune.get_int("mw_max_tokens", MW_MAX_M))
# The same steps of a quantized model can read the fp8 / int8 / int4 codes on gemm_mw8
# (csrc/kernels/gemm_mw8.hip) when the model was quantized with mw8=True (the engine's
# default; quantize_weights' own default keeps the earlier steps), on TP = 1, in eager
# steps and captured decode graphs (the runner's mixed-step graphs keep their families),
# per projection, where mw8_plan has a plan at every row bucket and profiles/mw8.md measured it ahead of the path it replaces at every bucket:
#   quantized-only (dequant_w8 + library GEMM): 1.2-4.4x ahead at every measured shape,
#     format and bucket, so every projection with a plan takes it;
#   resident (bf16 gemm_mw): only (shape, format) pairs that ran ahead at every bucket by more
#     than the spread of their rows, in two runs: the Llama-3-70B projections in fp8 (9-30 %
#     ahead on 256-column tiles, spreads up to 8 %). fp8 at the 8B shapes is within +-10 %,
#     int8 ahead at some 70B buckets only, int4 10-30 % behind everywhere: those keep gemm_mw.
# XGS_TUNE mw8=0 restores the earlier choice everywhere.
MW8 = tune.get_bool("mw8", True)
MW8_BUCKET_ENDS = (W8_MAX_M + 1, 128, 129, 192, 193, 256, 257, MW_MAX_M)  # both ends of every plan bucket
# (N, K, fmt) of the projections of a resident model that take gemm_mw8
MW8_RESIDENT = frozenset((N, K, linear_mod.WQ_FP8) for N, K in ((10240, 8192), (8192, 8192), (57344, 8192),
                                                                (8192, 28672)))
# Prompt-sized mixed steps on TP = 1: each projection takes gemm_pf
# (csrc/kernels/gemm_pf.hip) for the step sizes where it measured faster than the
# tuned library GEMM (profiles/r6/r6p_pf_vs_library.md, cold weights, the engine's
# library forms) -- QKV / O / down as split-K partials into their consumers, gate_up
# with the SiLU gate in its epilogue:
#   gate_up 448-576 rows: 4-5 % ahead of the library's GEMM + SiLU-gate pair at 448 / 512
#     rows, 22 % at 575 -- its tile-quantisation cliff (GEMM 103 us at 512 rows, 135 at
#     575), where two 288-row tiles cover the step; within +-1 % or behind elsewhere;
#   down 513-576 rows: 5-11 % ahead of the library's split-4 GEMM in isolation at every
#     measured size from 320 to 576 rows, but its 8 fp32 slabs (vs the library's 4) cost
#     the consumer more than that below 513: 447-row steps (--prompt-len 384) ran 11,603
#     vs 11,694 tok/s with down on pf (r6p_pf_vs_library.md);
#   QKV / O: never -- pf's isolated lead is smaller than the fp32 partial slabs it adds
#     to their consumers (r5: -0.5 % end to end with every projection on pf).
# XGS_TUNE pf: "1" = these windows, "0" = library everywhere, or a comma list of
# projections to allow; pf_windows overrides the table ("gate_up:513-576/down:321-576").
PF_WINDOWS_DEFAULT = "gate_up:448-576/down:513-576"


def _parse_pf_windows(spec: str):
    out = {"qkv": (), "o": (), "gate_up": (), "down": ()}
    for item in filter(None, (t.strip() for t in spec.split("/"))):
        name, rng = item.split(":")
        assert name in out, f"XGS_TUNE pf_windows: {name!r}"
        out[name] = tuple(tuple(int(v) for v in r.split("-")) for r in rng.split("+"))
    return out


_pf_spec = tune.get_str("pf", "1")
PF_SET = frozenset() if _pf_spec in ("0", "") else frozenset(
    ("qkv,o,gate_up,down" if _pf_spec == "1" else _pf_spec).replace("+", ",").split(","))
assert PF_SET <= {"qkv", "o", "gate_up", "down"}, f"XGS_TUNE pf: {sorted(PF_SET)}"
PF_WINDOWS = {k: (v if k in PF_SET else ())
              for k, v in _parse_pf_windows(tune.get_str("pf_windows", PF_WINDOWS_DEFAULT)).items()}
PF_MAX_M = max([hi for ws in PF_WINDOWS.values() for _, hi in ws] or [0])


def pf_projections(T: int) -> frozenset:
    """The projections that run on gemm_pf at a T-token step."""
    return frozenset(k for k, ws in PF_WINDOWS.items() if any(lo <= T <= hi for lo, hi in ws))


# TP > 1 prefill-sized steps: the row-parallel all-reduces are pipelined over this
# many token chunks and overlapped with the next chunk's GEMMs (RCCL stream); a
# 2k-token 8B step moves 16 MiB per all-reduce -- ~100 us on 7 xGMI links, a
# GEMM-sized share of the layer. XGS_TUNE tp_overlap_chunks=1 disables it.
TP_OVERLAP_CHUNKS = tune.get_int("tp_overlap_chunks", 2)
TP_OVERLAP_MIN_TOKENS = tune.get_int("tp_overlap_min_tokens", 256)
# EP all_to_all: steps with at least this many (token, choice) pairs (and not under
# graph capture) exchange exact per-destination counts first and send only real rows
EP_EXACT_MIN_PAIRS = tune.get_int("ep_exact_min_pairs", 256)
# moe_comm "auto": steps of at most this many tokens use the allreduce form when the
# custom IPC all-reduce can take the [T, H] message
EP_AR_MAX_TOKENS = 64


PROJECTIONS = ("qkv", "o", "gate_up", "down")


class Step(NamedTuple):
    """The GEMM kernel family of each projection at one step -- "w8", "skinny", "m64",
    "mw", "mw8", "pf", "f8", "i8", "i4" (HIP: QKV / O / down as split-K partials into their consumers, the SiLU
    gate inside gate_up), "lib" (library GEMM, bf16 out) or "dq" (the quantized weight
    dequantized into the model's scratch, then the library GEMM) -- and the attention entry:
    "fused_decode" / "from_partials" for QKV partials, "rope" for a QKV tensor. MoE
    layers run their experts (LlamaLayer.mlp) in place of gate_up / down."""
    qkv: str
    o: str
    gate_up: str
    down: str
    attn: str


def _uniform(family: str, attn: str = "from_partials") -> Step:
    return Step(family, family, family, family, attn)


SKINNY, M64, M64_FUSED_QKV, MW, LIB = (_uniform("skinny"), _uniform("m64"), _uniform("m64", "fused_decode"),
                                       _uniform("mw"), _uniform("lib", "rope"))


@functools.lru_cache(maxsize=None)  # (eager prompt steps ask once per layer; T <= PF_MAX_M bounds it)
def _pf_step(T: int) -> Step:
    """gemm_pf for the projections whose measured window holds T, the library for the rest."""
    use_pf = pf_projections(T)
    if not use_pf:
        return LIB
    return Step(*("pf" if n in use_pf else "lib" for n in PROJECTIONS), "from_partials" if "qkv" in use_pf else "rope")


class LayerDispatch:
    """Which kernels a layer of these dimensions runs at a (T tokens, num_decodes)
    step of the unfused chain. Pure: built from the local projection shapes
    (qkv [Nqkv, H], o [H, HqD], gate_up [2 Fl, H], down [H, Fl]; MoE layers have no
    Fl), the TP degree and whether the layer is on a GPU; no tensors, no device
    calls. m64_plan has a plan at 16 < M <= 64 for every shape that passes `fast_ok`
    (tests/test_layer_dispatch.py pins it), so such a layer has no library arm below
    65 tokens."""

    def __init__(self, Nqkv: int, H: int, HqD: int, Fl: int, moe: bool, tp: int, on_gpu: bool, attn_fq_ok: bool):
        self.attn_fq_ok = attn_fq_ok    # the decode attention kernel's fused-QKV form fits the head layout
        self.quantized: Optional[Step] = None
        self.dequantized: Optional[Step] = None  # T > W8_MAX_M of a model without its bf16 weights
        self.mw8: Optional[Step] = None          # W8_MAX_M < T <= MW_MAX_TOKENS with a projection on gemm_mw8
        self.f8: tuple = ()                      # projections that run T > MW_MAX_TOKENS on gemm_f8 (a8)
        self.i8: tuple = ()                      # ... on gemm_i8 (ai8)
        self.i4: tuple = ()                      # ... on gemm_i4 (aw4: int8 activations on int4 copies)
        self.on_gpu, self.tp = on_gpu, tp
        self.fast_ok = on_gpu and H % 256 == 0 and HqD % 256 == 0 and Nqkv % 64 == 0 and (moe or Fl % 256 == 0)
        shapes = ((Nqkv, H, MODE_PARTIAL), (H, HqD, MODE_PARTIAL))
        if not moe:
            shapes += ((2 * Fl, H, MODE_SILU), (H, Fl, MODE_PARTIAL))
        self.shapes = dict(zip(PROJECTIONS, shapes))
        # M <= 16 on gemm_m64g too, when every projection has a measured small-M plan
        self.m64_small_ok = self.fast_ok and all(m64_plan(1, n, k, mode) is not None for n, k, mode in shapes)
        # 64 < M <= MW_MAX_TOKENS: gemm_mw for every projection (MoE layers: the attention
        # projections; the experts stay on the grouped gemm_m64g)
        self.mw_ok = self.fast_ok and MW_MAX_TOKENS > FAST_M_SLAB and all(
            mw_plan(MW_MAX_TOKENS, n, k, mode) is not None and mw_plan(FAST_M_SLAB + 1, n, k, mode) is not None
            for n, k, mode in shapes)
        # T > MW_MAX_TOKENS on TP = 1: gemm_pf inside PF_WINDOWS
        self.pf_ok = self.fast_ok and PF_MAX_M > 0 and tp == 1 and all(
            pf_plan(PF_MAX_M, n, k, mode) is not None for n, k, mode in shapes)

    @classmethod
    def for_layer(cls, cfg: ModelConfig, tp: int, on_gpu: bool) -> "LayerDispatch":
        Hq, Hkv = local_heads(cfg, tp)
        D, moe = cfg.head_dim, cfg.arch == "mixtral"
        # the decode attention kernel's fused-QKV form: D = 128, GQA groups of 1/2/4/8
        attn_fq_ok = on_gpu and D == 128 and Hq % Hkv == 0 and Hq // Hkv in (1, 2, 4, 8)
        return cls((Hq + 2 * Hkv) * D, cfg.hidden_size, Hq * D, 0 if moe else cfg.intermediate_size // tp, moe, tp,
                   on_gpu, attn_fq_ok)

    def set_quantized(self, names, resident: bool = True, fmt: Optional[int] = None, a8: bool = False,
                      a8_fmt: Optional[int] = None, ai8: bool = False, ai8_fmt: Optional[int] = None,
                      aw4: bool = False, aw4_fmt: Optional[int] = None) -> None:
        """The projections in `names` have fp8 / int8 / int4 copies (gemm_w8, T <= W8_MAX_M);
        the others run their bf16 weight on gemm_m64g there. resident=False: the bf16
        weights of `names` are gone, so every larger step dequantizes them into the
        model's scratch for the library GEMM ("dq") -- no bf16 HIP GEMM family is ever
        chosen for them. fmt (WQ_*, the format of the copies; TP = 1 only): steps
        of W8_MAX_M < T <= MW_MAX_TOKENS run each projection of `names` that has a gemm_mw8
        plan at every row bucket and was measured ahead there (a resident model:
        MW8_RESIDENT) on its codes ("mw8"); the other projections keep that step's family of
        today. Without fmt, or when no projection qualifies, nothing changes.
        a8 (fp8 activations; a8_fmt = the format of the copies, taken from fmt when that is given):
        on a GPU, TP = 1, a dense layer and fp8 copies, steps of T > MW_MAX_TOKENS (not the
        mixed-step graph bodies) run each projection of `names` that has an f8_plan on gemm_f8
        ("f8": rows quantized to E4M3 per token, then the FP8 matrix instructions on the codes);
        the others keep that step's family of today. Otherwise a8 changes nothing.
        ai8 / ai8_fmt (int8 activations): the same for int8 copies, i8_plan and gemm_i8 ("i8": rows
        quantized to int8 per token, then the INT8 matrix instructions). a8 stays fp8 only.
        aw4 / aw4_fmt (int8 activations on int4 weights): the same for int4 copies, i4_plan and
        gemm_i4 ("i4": rows quantized to int8 per token in the kernel's k order, then the INT8 matrix
        instructions on the widened int4 codes, one group scale per K tile). ai8 stays int8 only."""
        a8_fmt = fmt if a8_fmt is None else a8_fmt
        ai8_fmt = fmt if ai8_fmt is None else ai8_fmt
        aw4_fmt = fmt if aw4_fmt is None else aw4_fmt
        self.f8 = self.i8 = self.i4 = ()
        if aw4 and aw4_fmt == linear_mod.WQ_INT4 and self.on_gpu and self.tp == 1 and "gate_up" in self.shapes:
            self.i4 = tuple(n for n in PROJECTIONS if n in names
                            and i4_plan(MW_MAX_TOKENS + 1, *self.shapes[n]) is not None)
        if ai8 and ai8_fmt == linear_mod.WQ_INT8 and self.on_gpu and self.tp == 1 and "gate_up" in self.shapes:
            self.i8 = tuple(n for n in PROJECTIONS if n in names
                            and i8_plan(MW_MAX_TOKENS + 1, *self.shapes[n]) is not None)
        if a8 and a8_fmt == linear_mod.WQ_FP8 and self.on_gpu and self.tp == 1 and "gate_up" in self.shapes:
            self.f8 = tuple(n for n in PROJECTIONS if n in names
                            and f8_plan(MW_MAX_TOKENS + 1, *self.shapes[n]) is not None)
        self.quantized = Step(*("w8" if n in names else "m64" for n in PROJECTIONS), "from_partials")
        self.dequantized = None if resident else Step(*("dq" if n in names else "lib" for n in PROJECTIONS), "rope")
        self.mw8 = None
        if fmt is None or not (MW8 and self.on_gpu and self.tp == 1 and MW_MAX_TOKENS > W8_MAX_M):
            return
        today = self.select(W8_MAX_M + 1, 0)  # (the same step up to MW_MAX_TOKENS: MW, LIB or dequantized)
        fam = []
        for n in PROJECTIONS:
            N, K, mode = self.shapes.get(n, (0, 0, 0))
            take = (N, K, fmt) in MW8_RESIDENT if resident else True
            ok = (n in names and n in self.shapes and take
                  and all(mw8_plan(T, N, K, mode, fmt) is not None for T in MW8_BUCKET_ENDS if T <= MW_MAX_TOKENS))
            fam.append("mw8" if ok else getattr(today, n))
        if "mw8" in fam:
            self.mw8 = Step(*fam, "from_partials" if fam[0] in ("mw8", "mw") else "rope")

    def select(self, T: int, num_decodes: int, mixed_graph: bool = False) -> Step:
        """mixed_graph: a body of the runner's mixed-step graphs (AttnMeta.mixed_graph), which keep
        the families they had: no "mw8", no "f8" / "i8" / "i4". Decode graphs and eager steps take them."""
        today = self._select(T, num_decodes, mixed_graph)
        if T <= MW_MAX_TOKENS or mixed_graph:
            return today
        for a8, on8 in (("f8", self.f8), ("i8", self.i8), ("i4", self.i4)):  # (the copies have one format)
            if on8:
                fam = [a8 if n in on8 else getattr(today, n) for n in PROJECTIONS]
                return Step(*fam, "from_partials" if fam[0] in (a8, "pf") else "rope")
        return today

    def _select(self, T: int, num_decodes: int, mixed_graph: bool) -> Step:
        if self.quantized is not None and T <= W8_MAX_M:
            return self.quantized
        if self.mw8 is not None and T <= MW_MAX_TOKENS and not mixed_graph:
            return self.mw8
        if self.dequantized is not None:
            return self.dequantized
        if self.fast_ok and T <= FAST_M_SLAB:
            if T <= FAST_M_SMALL and not self.m64_small_ok:
                return SKINNY
            # pure-decode steps reduce the QKV partials + RoPE + KV append in the attention prologue
            return M64_FUSED_QKV if (T == num_decodes and self.attn_fq_ok) else M64
        if self.mw_ok and T <= MW_MAX_TOKENS:
            return MW
        return _pf_step(T) if (self.pf_ok and T <= PF_MAX_M) else LIB


@torch.no_grad()
def _fold_norm(w: torch.Tensor, norm: torch.Tensor) -> None:
    """W[:, k] *= norm[k] (one bf16 rounding), norm <- 1: rmsnorm(x, g) @ W^T ==
    rmsnorm(x, 1) @ (W diag(g))^T exactly in real arithmetic."""
    if bool((norm == 1).all()):
        return
    w.copy_((w.float() * norm.float()[None, :]).to(w.dtype))
    norm.fill_(1.0)


def _p(t: torch.Tensor) -> nn.Parameter:
    return nn.Parameter(t, requires_grad=False)


class LlamaLayer(nn.Module):
    def __init__(self, cfg: ModelConfig, tp: int, rank: int, device, dtype):
        super().__init__()
        self.cfg = cfg
        self.tp, self.rank = tp, rank
        Hq, Hkv = local_heads(cfg, tp)
        D, H = cfg.head_dim, cfg.hidden_size
        self.Hq, self.Hkv = Hq, Hkv
        z = lambda *s: torch.empty(*s, device=device, dtype=dtype)  # noqa: E731
        self.input_norm = _p(torch.ones(H, device=device, dtype=dtype))
        self.post_norm = _p(torch.ones(H, device=device, dtype=dtype))
        self.qkv = _p(z((Hq + 2 * Hkv) * D, H))
        self.o = _p(z(H, Hq * D))
        self.moe = cfg.arch == "mixtral"
        if self.moe:
            E = cfg.num_experts
            if E % tp:
                raise ValueError(f"{E} experts not divisible by ep={tp}")
            self.E_local = E // tp
            self.expert_offset = rank * self.E_local
            self.router = _p(z(E, H))
            self.w13 = _p(z(self.E_local, 2 * cfg.intermediate_size, H))
            self.w2 = _p(z(self.E_local, H, cfg.intermediate_size))
        else:
            Fl = cfg.intermediate_size // tp
            self.gate_up = _p(z(2 * Fl, H))
            self.down = _p(z(H, Fl))
        self.attn = PagedAttention(Hq, Hkv, D)
        self.moe_comm = "auto"
        self.w8 = None  # fp8 / int8 / int4 weight copies for decode (LlamaForCausalLM.quantize_weights)
        self.ea8 = False  # MoE: steps above MOE_PREFILL_PAIRS pairs run the experts on fp8 codes (quantize_weights ea8)
        # quantized_only: the model's bf16 scratch that "dq" steps dequantize one projection
        # into, and the [N, K] of each projection whose bf16 weight was released
        self.dq_scratch: Optional[torch.Tensor] = None
        self.released: dict = {}
        # the GEMM kernel of each projection and the attention entry, per step size
        self.dispatch = d = LayerDispatch.for_layer(cfg, tp, torch.device(device).type == "cuda")
        self.fast_ok, self.m64_small_ok, self.mw_ok, self.pf_ok, self.attn_fq_ok = (
            d.fast_ok, d.m64_small_ok, d.mw_ok, d.pf_ok, d.attn_fq_ok)

    def _ar(self, x):
        """Row-parallel output -> all-reduced tensor. TP = 1: as it is -- a PendingSum
        goes on to its consumer's prologue. (Keyed on the layer's own TP degree: a TP=1
        draft model may live in a TP>1 process.)"""
        if self.tp == 1:
            return x
        return comm.tp_all_reduce(x.materialize() if isinstance(x, PendingSum) else x)

    def _gemm(self, family: str, x: torch.Tensor, name: str, mode: int):
        """Projection `name` of x on the kernel family a Step names (a missing kernel or
        plan raises in the wrapper: no family stands in for another)."""
        if family == "w8":
            q = self.w8[name]
            return w8_linear(x, q[0], q[1], mode, fmt=q[2])
        if family == "mw8":
            q = self.w8[name]
            return mw8_linear(x, q[0], q[1], mode, fmt=q[2])
        if family == "f8":
            q = self.w8[name]
            return f8_linear(x, q[0], q[1], mode)
        if family == "i8":
            q = self.w8[name]
            return i8_linear(x, q[0], q[1], mode)
        if family == "i4":
            q = self.w8[name]
            return i4_linear(x, q[0], q[1], mode)
        if family == "dq":
            # One scratch for every projection of every layer: the whole step runs on one
            # stream, so the GEMM that reads the scratch is enqueued before the next
            # projection's dequantization overwrites it, and the scratch is dead once that
            # GEMM is enqueued. Its address never changes, so captured steps replay it.
            q = self.w8[name]
            return F.linear(x, dequantize_into(q[0], q[1], q[2], out=self.dq_scratch))
        w = getattr(self, name)  # (a released bf16 weight raises here: no family stands in for "dq")
        if family == "lib":  # (the eager, host-bound steps first)
            return F.linear(x, w)
        if family == "pf":
            return pf_linear(x, w, mode)
        if family == "m64":
            return m64_linear(x, w, mode)
        if family == "mw":
            return mw_linear(x, w, mode)
        assert family == "skinny", family
        return skinny_linear(x, w, None, mode)

    # ------------------------------------------------------------------ MoE
    def _moe_allreduce(self, h: torch.Tensor, codes: bool = False, ea8: bool = False) -> torch.Tensor:
        w, ids = ops.moe_route(h, self.router, self.cfg.experts_per_token)
        # codes: the step reads the experts' quantized copies on moe_gemm_w8; ea8: a step above
        # MOE_PREFILL_PAIRS pairs reads them on moe_gemm_f8 (smaller ones keep their kernels of today)
        ea8 = ea8 and ids.numel() > MOE_PREFILL_PAIRS
        wq = self.w8["w13"][:2] + self.w8["w2"] if codes or ea8 else None
        out = ops.fused_moe(h, self.w13, self.w2, w, ids, self.expert_offset,
                              experts_total=self.router.shape[0], wq=wq, expert_a8=ea8)
        return self._ar(out)

    def _moe_alltoall(self, h: torch.Tensor) -> torch.Tensor:
        """Expert-parallel MoE with an all_to_all dispatch on the replicated [T, H]
        input: this rank's token slice goes through `_moe_alltoall_rows`, and an
        all_gather rebuilds the replicated output. (Prefill-sized steps take the
        sequence-parallel form instead, `forward_sp`, which never gathers it.)"""
        T = h.shape[0]
        per = (T + self.tp - 1) // self.tp
        lo, hi = min(T, self.rank * per), min(T, (self.rank + 1) * per)
        out_slice = self._moe_alltoall_rows(h[lo:hi], T, per)
        return comm.tp_all_gather_rows(out_slice)[:T].contiguous()

    def _moe_alltoall_rows(self, hs: torch.Tensor, T: int, per: int) -> torch.Tensor:
        """The all_to_all MoE on this rank's rows hs [Ts <= per, H] of a T-token step
        (rank r owns tokens [r * per, r * per + Ts)) -> [per, H], rows >= Ts zero.
        ep_plan/ep_scatter (HIP) pack each (token, choice) row for the rank that owns
        the expert, the owners run their experts as one grouped GEMM (send_eid = -1
        rows are skipped by the align), the rows travel back and ep_combine (HIP)
        applies the routing weights.
        Split policy: count-exact (packed layout, splits exchanged first: one host
        sync per layer) for eager steps of >= EP_EXACT_MIN_PAIRS pairs; fixed
        capacity (per * k rows per destination, no host sync) otherwise, which is
        what a captured decode graph needs."""
        tp = self.tp
        Ts, H = hs.shape
        k = self.cfg.experts_per_token
        cap = per * k
        if Ts > 0:
            w, ids = ops.moe_route(hs, self.router, k)
        else:
            w = torch.empty(0, k, dtype=torch.float32, device=hs.device)
            ids = torch.empty(0, k, dtype=torch.int32, device=hs.device)
        capturing = hs.is_cuda and torch.cuda.is_current_stream_capturing()
        packed = not capturing and T * k >= EP_EXACT_MIN_PAIRS
        slot, send_eid, counts = ops.ep_plan(ids, self.E_local, tp, cap, packed)
        rows = Ts * k if packed else tp * cap
        send = ops.ep_scatter(hs, k, slot, rows)
        if packed:
            recv_counts = comm.tp_exchange_counts(counts)
            send_splits, recv_splits = counts.tolist(), recv_counts.tolist()
        else:
            send_splits = recv_splits = [cap] * tp
        recv = comm.tp_all_to_all(send, send_splits, recv_splits)
        recv_eid = comm.tp_all_to_all(send_eid.view(-1, 1), send_splits, recv_splits).view(-1, 1)
        ones = torch.ones(recv.shape[0], 1, dtype=torch.float32, device=hs.device)
        y = ops.fused_moe(recv, self.w13, self.w2, ones, recv_eid, 0)    # unused slots (eid -1) -> 0 rows
        back = comm.tp_all_to_all(y, recv_splits, send_splits)            # rows in this rank's send order
        out_slice = torch.zeros(per, H, dtype=hs.dtype, device=hs.device)
        ops.ep_combine(back, slot, w, out_slice)
        return out_slice

    def forward_sp(self, x: torch.Tensor, residual: Optional[torch.Tensor], meta: AttnMeta,
                   kv: Tuple[torch.Tensor, torch.Tensor], cos_sin: torch.Tensor, T: int, per: int):
        """Sequence-parallel TP + EP layer (MoE layers on the all_to_all exchange): the
        residual stream stays token-sliced, [per, H] per rank (rank r holds tokens
        [r * per, r * per + per), zero-padded). The head-parallel attention reads
        the all-gathered normed input; its row-parallel output is reduce-scattered
        (half the bytes of the all-reduce) straight into this rank's rows, whose
        post-attention norm feeds the expert dispatch, and the combined expert output
        stays sliced. Per layer: all_gather(h) + reduce_scatter(o) + 2 all_to_all,
        against all_reduce(o) + 2 all_to_all + all_gather(out) in the replicated form
        (VERDICT r2 #8)."""
        eps = self.cfg.norm_eps
        Ts = max(0, min(T, (self.rank + 1) * per) - self.rank * per)
        if residual is None:
            residual = x
            hs = ops.rmsnorm(x, self.input_norm, eps)
        else:
            hs, residual = ops.fused_add_rmsnorm(x, residual, self.input_norm, eps)
        h = comm.tp_all_gather_rows(hs)[:T]
        a = self.attn(F.linear(h, self.qkv), meta, kv, cos_sin)
        o = F.linear(a, self.o)
        if o.shape[0] < self.tp * per:
            o = torch.cat([o, o.new_zeros(self.tp * per - o.shape[0], o.shape[1])])
        hs, residual = ops.fused_add_rmsnorm(comm.tp_reduce_scatter_rows(o), residual, self.post_norm, eps)
        return self._moe_alltoall_rows(hs[:Ts], T, per), residual

    def _moe_use_alltoall(self, h: torch.Tensor) -> bool:
        """Exchange choice for a TP > 1 MoE layer. "auto" (default): the activations
        are replicated after the head-parallel attention, so the allreduce form needs
        no dispatch at all -- each rank runs its experts on the tokens routed to them
        and one all-reduce sums the partial outputs. For decode-sized steps that
        all-reduce is ONE launch of the custom IPC kernel (~latency of one xGMI hop),
        where the all_to_all form costs three RCCL all_to_alls + an all_gather of tiny
        messages per layer; prefill-sized steps take the all_to_all, which moves only
        the routed rows (count-exact) instead of the whole [T, H] partial."""
        if self.moe_comm == "alltoall":
            return True
        if self.moe_comm == "allreduce":
            return False
        if get_state().tp_size == 1:  # a simulated TP shard (bench --tp-shard): collectives are local
            return False
        ar = comm.custom_allreduce()
        # the partial output is a fresh contiguous [T, H] bf16 tensor like h
        return not (h.shape[0] <= EP_AR_MAX_TOKENS and ar is not None and ar.can_run(h.contiguous()))

    def mlp(self, h: torch.Tensor, codes: bool = False, ea8: bool = False) -> torch.Tensor:
        """The experts of a MoE layer (a dense layer's MLP is the tail of `forward`).
        codes: the quantized step of a quantized model (TP = 1) -- the experts run on their
        fp8 / int8 / int4 copies. ea8: fp8 expert activations (TP = 1) -- a prompt-sized step
        runs them on the fp8 copies and per-token E4M3 activations."""
        if self.tp > 1 and self._moe_use_alltoall(h):
            return self._moe_alltoall(h)
        return self._moe_allreduce(h, codes, ea8)

    def forward(self, x, residual: Optional[torch.Tensor], meta: AttnMeta,
                kv: Tuple[torch.Tensor, torch.Tensor], cos_sin: torch.Tensor):
        eps = self.cfg.norm_eps
        if residual is None:
            residual = x
            h = ops.rmsnorm(x, self.input_norm, eps)
        else:
            h, residual = ops.fused_add_rmsnorm(x, residual, self.input_norm, eps)
        T = meta.num_tokens
        step = self.dispatch.select(T, meta.num_decodes, mixed_graph=meta.mixed_graph)
        qkv = self._gemm(step.qkv, h, "qkv", MODE_PARTIAL)
        if step.attn == "fused_decode":
            a = self.attn.fused_decode(qkv, meta, kv, cos_sin)
        elif step.attn == "from_partials":
            a = self.attn.from_partials(qkv, meta, kv, cos_sin)
        else:
            a = self.attn(qkv, meta, kv, cos_sin)
        if (self.tp > 1 and step is LIB and not self.moe and T >= TP_OVERLAP_MIN_TOKENS
                and TP_OVERLAP_CHUNKS > 1):
            return self._forward_tp_overlap(a, residual)
        o = self._ar(self._gemm(step.o, a, "o", MODE_PARTIAL))
        h, residual = ops.fused_add_rmsnorm(o, residual, self.post_norm, eps)
        if self.moe:
            # the experts switch to their codes where the attention projections do
            # ea8: prompt steps only -- a pure decode step keeps its kernels however many rows it has
            # (129 sequences are already 258 pairs), and the runner's mixed-step graph bodies keep
            # their families, as for "f8"
            return self.mlp(h, codes=step is self.dispatch.quantized and "w13" in (self.w8 or {}),
                            ea8=self.ea8 and meta.num_decodes < T and not meta.mixed_graph), residual
        if step.gate_up in ("lib", "dq"):  # bf16 gate|up rows out of the library GEMM
            act = ops.silu_and_mul(self._gemm(step.gate_up, h, "gate_up", MODE_BF16), interleave16=True)
        else:
            act = self._gemm(step.gate_up, h, "gate_up", MODE_SILU)
        if step.down == "lib" and self.tp == 1 and splitk_prefill_ok(act, self.down):
            # one K-split library GEMM, reduced by the next add + norm
            return splitk_linear(act, self.down, linear_mod.SPLITK_PREFILL_S), residual
        return self._ar(self._gemm(step.down, act, "down", MODE_PARTIAL)), residual

    def _forward_tp_overlap(self, a: torch.Tensor, residual: torch.Tensor):
        """Row-parallel half of a TP layer for prefill-sized steps, pipelined over
        token chunks so every all-reduce runs (on RCCL's stream) under the GEMMs of
        the following chunk: O GEMM(c) -> AR(c) async; then per chunk: wait AR(c)
        -> add + post-norm -> gate_up -> SiLU-gate -> down(c) -> AR(c) async. Only
        the last chunk's down all-reduce is exposed. Everything after attention is
        per-token, so the chunked result equals the unchunked one exactly."""
        T, H = residual.shape
        eps = self.cfg.norm_eps
        n = TP_OVERLAP_CHUNKS
        step = (T + n - 1) // n
        if step > 64:
            step = (step + 63) // 64 * 64  # GEMM-friendly row blocks
        bounds = [(lo, min(T, lo + step)) for lo in range(0, T, step)]
        o = torch.empty(T, H, dtype=a.dtype, device=a.device)
        works = []
        for lo, hi in bounds:
            torch.mm(a[lo:hi], self.o.t(), out=o[lo:hi])
            works.append(comm.tp_all_reduce_async(o[lo:hi]))
        d = torch.empty(T, H, dtype=a.dtype, device=a.device)
        dworks = []
        for (lo, hi), w in zip(bounds, works):
            w.wait()
            hc, _ = ops.fused_add_rmsnorm(o[lo:hi], residual[lo:hi], self.post_norm, eps)
            act = ops.silu_and_mul(F.linear(hc, self.gate_up), interleave16=True)
            torch.mm(act, self.down.t(), out=d[lo:hi])
            dworks.append(comm.tp_all_reduce_async(d[lo:hi]))
        for w in dworks:
            w.wait()
        return d, residual

    def forward_fused(self, resid: torch.Tensor, stats: RowStats, meta: AttnMeta,
                      kv: Tuple[torch.Tensor, torch.Tensor], cos_sin: torch.Tensor, ws: ResidWorkspace,
                      site: int) -> RowStats:
        """Fused decode layer: QKV GEMM (input norm as a row scale) -> attention (QKV
        reduce + RoPE + KV append in its prologue) -> O GEMM (+ residual, + post-norm
        statistics) -> gate_up GEMM (post-norm row scale, SiLU-gate) -> down GEMM
        (+ residual, + next statistics). `resid` (bf16 [T, H]) is updated in place;
        returns the statistics of the new residual for the next layer."""
        eps = self.cfg.norm_eps
        pqkv = m64_linear(resid, self.qkv, MODE_PARTIAL, stats=stats, eps=eps)
        a = self.attn.fused_decode(pqkv, meta, kv, cos_sin)
        if self.moe:
            return self._fused_moe_tail(a, resid, ws, site)
        if self.tp > 1:
            return self._fused_tp_tail(a, resid, ws, site)
        st = m64_resid_linear(a, self.o, resid, ws, site, eps)
        act = m64_linear(resid, self.gate_up, MODE_SILU, stats=st, eps=eps)
        return m64_resid_linear(act, self.down, resid, ws, site + 1, eps)

    def _fused_moe_tail(self, a, resid: torch.Tensor, ws: ResidWorkspace, site: int) -> RowStats:
        """MoE half of the fused decode layer: O GEMM (+ residual; under TP the custom
        all-reduce with the residual) -> router with the post-attention RMSNorm in its
        prologue (writes the normalised rows for the experts) -> align -> grouped w13
        (SiLU-gate) -> grouped w2 -> combine + residual + next-norm statistics (under
        TP: this rank's experts' partial through the residual all-reduce -- the
        activations are replicated, so no dispatch). 7 launches instead of 9."""
        T, H = resid.shape
        eps = self.cfg.norm_eps
        if self.tp > 1:
            po = m64_linear(a, self.o, MODE_PARTIAL)
            comm.tp_allreduce_resid(po.part, resid, ws.ss[site], self.tp)
        else:
            m64_resid_linear(a, self.o, resid, ws, site, eps)  # its statistics go unused: the router renorms
        # one token (batch 1): the router launch also writes the expert layout
        hn, w, ids, layout = ops.moe_route_norm(resid, self.post_norm, eps, self.router, self.cfg.experts_per_token,
                                                align=(self.E_local, self.expert_offset))
        ss = ws.ss[site + 1]
        if self.tp > 1:
            part = ops.fused_moe(hn, self.w13, self.w2, w, ids, self.expert_offset, out_f32=True, layout=layout,
                                 experts_total=self.router.shape[0])
            comm.tp_allreduce_resid(part.unsqueeze(0), resid, ss, self.tp)
        else:
            return RowStats(ss, ops.fused_moe(hn, self.w13, self.w2, w, ids, self.expert_offset, resid=resid, ss=ss,
                                              layout=layout, counters=ws.counters[site + 1]), T)
        return RowStats(ss, H // 1024, T)

    def _fused_tp_tail(self, a: torch.Tensor, resid: torch.Tensor, ws: ResidWorkspace, site: int) -> RowStats:
        """Row-parallel half of the fused decode layer under TP: O GEMM partials ->
        all-reduce + residual + statistics (one launch) -> gate_up (norm row scale,
        SiLU-gate) -> down GEMM partials -> all-reduce + residual + statistics."""
        T, H = resid.shape
        eps = self.cfg.norm_eps
        ar = comm.gemm_ar_args(self.tp, T, H, resid.device)
        if ar is not None:
            # the all-reduce inside the O / down launches (gemm_m64g GG_AR): 2 launches fewer
            st = m64_ar_resid_linear(a, self.o, resid, ws, site, ar)
            act = m64_linear(resid, self.gate_up, MODE_SILU, stats=st, eps=eps)
            return m64_ar_resid_linear(act, self.down, resid, ws, site + 1, ar)
        po = m64_linear(a, self.o, MODE_PARTIAL)
        comm.tp_allreduce_resid(po.part, resid, ws.ss[site], self.tp)
        st = RowStats(ws.ss[site], H // 1024, T)
        act = m64_linear(resid, self.gate_up, MODE_SILU, stats=st, eps=eps)
        pd = m64_linear(act, self.down, MODE_PARTIAL)
        comm.tp_allreduce_resid(pd.part, resid, ws.ss[site + 1], self.tp)
        return RowStats(ws.ss[site + 1], H // 1024, T)


class LlamaForCausalLM(nn.Module):
    def __init__(self, cfg: ModelConfig, device="cpu", dtype=torch.bfloat16, tp: Optional[int] = None,
                 rank: Optional[int] = None):
        super().__init__()
        st = get_state()
        self.cfg = cfg
        self.tp = st.tp_size if tp is None else tp
        self.rank = st.tp_rank if rank is None else rank
        self.device = torch.device(device)
        self.dtype = dtype
        H, V = cfg.hidden_size, cfg.vocab_size
        self.V_pad = (V + self.tp - 1) // self.tp * self.tp
        self.embed = _p(torch.empty(V, H, device=device, dtype=dtype))
        self.layers = nn.ModuleList([LlamaLayer(cfg, self.tp, self.rank, device, dtype)
                                     for _ in range(cfg.num_layers)])
        self.norm = _p(torch.ones(H, device=device, dtype=dtype))
        self.lm_head = None if (cfg.tie_embeddings and self.tp == 1) else \
            _p(torch.empty(self.V_pad // self.tp, H, device=device, dtype=dtype))
        self.cos_sin = ops.build_cos_sin(cfg.head_dim, cfg.max_position, cfg.rope_theta, cfg.rope_scaling,
                                         device=device)
        self.num_kv_heads_local = self.layers[0].Hkv
        l0 = self.layers[0]
        self.norms_folded = False
        self.weight_dtype = "bf16"
        self.quantized_only = False     # quantize_weights(kind, quantized_only=True): no bf16 projections
        self._dq_scratch: Optional[torch.Tensor] = None
        self._fused_ok = l0.fast_ok and l0.attn_fq_ok and H % 1024 == 0 and H // 1024 <= 8
        self._fused_small_ok = self._fused_ok and l0.m64_small_ok
        # every layer on gemm_mw for 64 < T <= MW_MAX_TOKENS (the runner's mixed-step graphs)
        self._mw_ok = self.device.type == "cuda" and all(l.mw_ok for l in self.layers)
        self._fused_ws = ResidWorkspace(2 * cfg.num_layers + 1, FAST_M_SLAB, H, device) if self._fused_ok else None

    @torch.no_grad()
    def fold_norms(self):
        """Fold every RMSNorm weight into the input columns of the projection that
        consumes it and reset the norm to 1, so the decode GEMMs can apply the norm
        as a per-row epilogue scale of the raw residual stream. Exact in real
        arithmetic: every other path (prefill, TP, the fp32 reference) computes the
        same function. MoE post-attention norms stay (router and experts read them)."""
        for l in self.layers:
            _fold_norm(l.qkv, l.input_norm)
            if not l.moe:
                _fold_norm(l.gate_up, l.post_norm)
        self.norms_folded = True

    @torch.no_grad()
    def quantize_fp8(self) -> bool:
        return self.quantize_weights("fp8")

    @torch.no_grad()
    def quantize_weights(self, kind: str = "fp8", quantized_only: bool = False, mw8: bool = False,
                         a8: bool = False, ai8: bool = False, ea8: bool = False) -> bool:
        """Weight-only quantization for decode batches <= 64 (Req 10.3): per dense
        layer, copies of the QKV / O / gate_up / down weights (unfolded:
        build_model keeps the RMSNorm weights in the norms of a quantized model)
        as fp8 (E4M3, per-channel scale), int8 (per-channel scale) or int4 (per
        128-k group scales), run by gemm_w8. mw8=True (what the engine passes,
        EngineConfig.mw8): steps of 65..MW_MAX_TOKENS rows on TP = 1 (not the runner's
        mixed-step graphs) read the
        same codes on gemm_mw8, per projection, where mw8_plan has a plan at every
        row bucket (checked here, once) and it was measured ahead (a resident model:
        MW8_RESIDENT); a model without such a projection, and mw8=False, behave as
        before.
        Larger steps keep the bf16 weights (MFMA-bound there); the fused bf16
        decode layer is disabled. Returns False (and changes nothing) when a shape has no gemm_w8
        plan.

        A MoE model (Mixtral) on TP = 1: QKV / O as above, and per layer quantized copies of
        the expert stacks w13 / w2 (linear.quantize_expert_stack, counted by weight_bytes).
        Steps of at most 64 tokens -- where LayerDispatch.select returns the quantized step
        -- run the experts on the codes (moe_gemm_w8 through fused_moe(wq=...)); larger
        steps read the resident bf16 experts as before. Returns False for a MoE model
        under TP / EP, with quantized_only (the bf16 experts cannot be released: prompt
        steps read them), or whose expert shapes have no moe_w8_plan.

        quantized_only: the model is served from the quantized weights alone. Layer
        by layer, once a layer's copies exist the bf16 storage of its quantized
        projections is released (peak: the bf16 model plus about one layer), and
        steps above 64 rows that are not gemm_mw8's dequantize one projection at a
        time into one model-wide bf16 scratch of the largest projection that the
        library GEMM reads (LayerDispatch "dq"). The freed bytes go back to the device, where the
        engine's KV-pool sizing finds them.

        a8 (EngineConfig.fp8_activations; fp8, TP = 1, dense models on a GPU -- anything else
        raises): prompt steps above MW_MAX_TOKENS rows quantize their activations per token to
        E4M3 and run each projection that has an f8_plan on the FP8 matrix instructions
        (gemm_f8), for resident and quantized-only models alike. Outputs then differ from the
        weight-only model's. Smaller steps stay weight-only.
        ai8 (EngineConfig.int8_activations): the same for int8 models -- per-token int8 codes,
        i8_plan, the INT8 matrix instructions (gemm_i8) -- and for int4 models: the same codes
        against the packed int4 weights, i4_plan, gemm_i4 (one int32 sum per 128-k scale group).
        ea8 (EngineConfig.fp8_expert_activations; fp8, TP = 1, Mixtral on a GPU, not
        quantized_only, expert shapes with a moe_f8_plan -- anything else raises): steps above
        MOE_PREFILL_PAIRS token-expert pairs (not the mixed-step graph bodies) quantize the
        experts' input and the gated activation per token to E4M3 and run both expert GEMMs on
        the fp8 expert copies (moe_gemm_f8). Outputs then differ from the weight-only model's.
        QKV / O, smaller steps and every decode step stay as they are."""
        fmt = WQ_FORMATS[kind]
        l0 = self.layers[0]
        moe = any(l.moe for l in self.layers)
        if ea8:
            why = [t for c, t in ((kind != "fp8", f"fp8 weights, not {kind}"), (self.tp != 1, "TP = 1"),
                                  (not moe, "Mixtral (a dense model takes a8)"), (self.device.type != "cuda", "a GPU"),
                                  (quantized_only, "the resident bf16 experts (not quantized_only)")) if c]
            if not why and moe_f8_plan(MOE_PREFILL_PAIRS + 1, l0.w13.shape[0], l0.w13.shape[2], l0.w13.shape[1] // 2) is None:
                why = [f"expert shapes that moe_gemm_f8 takes, not H={l0.w13.shape[2]} F={l0.w13.shape[1] // 2}"]
            if why:
                raise ValueError("fp8 expert activations (ea8) need " + ", ".join(why))
        for on, key, need in ((a8, "a8", ("fp8",)), (ai8, "ai8", ("int8", "int4"))):
            if on:
                why = [t for c, t in ((kind not in need, f"{' or '.join(need)} weights, not {kind}"), (self.tp != 1, "TP = 1"),
                                      (moe, "a dense model, not Mixtral"), (self.device.type != "cuda", "a GPU")) if c]
                if why:
                    raise ValueError(f"{need[0]} activations ({key}) need " + ", ".join(why))
        if self.device.type != "cuda" or (moe and (self.tp != 1 or quantized_only)):
            return False
        if moe:  # the experts at both ends of every row body and at the largest quantized step
            E, F2, H = l0.w13.shape
            k = self.cfg.experts_per_token
            if any(moe_w8_plan(p, E, H, F2 // 2, fmt) is None for p in (1, 16, 17, W8_MAX_M * k)):
                return False
        names = ("qkv", "o") if moe else ("qkv", "o", "gate_up", "down")
        for n in names:
            w = getattr(l0, n)
            mode = MODE_SILU if n == "gate_up" else MODE_PARTIAL
            if any(w8_plan(m, w.shape[0], w.shape[1], mode, fmt) is None for m in (1, W8_MAX_M)):
                return False
        def use_q(n):  # small projections stay bf16 where gemm_m64g has a plan
            w = getattr(l0, n)
            mode = MODE_SILU if n == "gate_up" else MODE_PARTIAL
            return w.numel() >= W8_MIN_ELEMS or not (l0.m64_small_ok and
                                                     m64_plan(1, w.shape[0], w.shape[1], mode) is not None)
        chosen = [n for n in names if use_q(n)]
        for l in self.layers:
            l.w8 = {n: quantize_weight(getattr(l, n), fmt) + (fmt,) for n in chosen}
            if l.moe:  # expert copies beside the resident bf16 experts (which larger steps read)
                l.w8.update({n: quantize_expert_stack(getattr(l, n), fmt) + (fmt,) for n in ("w13", "w2")})
                l.ea8 = ea8
            l.dispatch.set_quantized(chosen, resident=not quantized_only, fmt=fmt if mw8 else None, a8=a8, a8_fmt=fmt,
                                     ai8=ai8, ai8_fmt=fmt, aw4=ai8, aw4_fmt=fmt)
            if quantized_only:
                for n in chosen:
                    l.released[n] = tuple(getattr(l, n).shape)
                    delattr(l, n)  # the parameter and its bf16 storage
        self._fused_ok = self._fused_small_ok = False
        self.weight_dtype = kind
        if quantized_only:
            self.quantized_only = True
            self._mw_ok = False  # (the runner's mixed-step graphs: library-sized, not gemm_mw)
            self._dq_scratch = torch.empty(max(N * K for l in self.layers for N, K in l.released.values()),
                                           dtype=torch.bfloat16, device=self.device)
            for l in self.layers:
                l.dq_scratch = self._dq_scratch
            torch.cuda.empty_cache()  # the released weights leave the allocator's cache too
        return True

    def weight_bytes(self) -> int:
        """Bytes of the weights resident on this rank: every parameter and every quantized
        copy (codes and scales), without the dequantization scratch."""
        n = sum(p.numel() * p.element_size() for p in self.parameters())
        for l in self.layers:
            for q, s, _ in (l.w8 or {}).values():
                n += q.numel() * q.element_size() + s.numel() * s.element_size()
        return n

    def scratch_bytes(self) -> int:
        """Bytes of the bf16 scratch of a quantized-only model (0 otherwise)."""
        s = self._dq_scratch
        return 0 if s is None else s.numel() * s.element_size()

    def fused_decode_ok(self, meta: AttnMeta) -> bool:
        T = meta.num_tokens
        if not (FUSED_DECODE and self._fused_ok and self.norms_folded) or T != meta.num_decodes or not 0 < T <= 64:
            return False
        l0 = self.layers[0]
        if l0.moe and self.tp > 1 and l0.moe_comm == "alltoall":  # the fused MoE tail is the allreduce form
            return False
        if self.tp > 1 and not comm.resid_allreduce_ok(T, self.cfg.hidden_size):
            return False
        return T > FAST_M_SMALL or self._fused_small_ok

    def _forward_fused(self, input_ids: torch.Tensor, meta: AttnMeta,
                       kv_caches: List[Tuple[torch.Tensor, torch.Tensor]]) -> torch.Tensor:
        ws = self._fused_ws
        resid = ops.embed_gather(input_ids, self.embed, ws.ss[0])  # gather + first norm statistic, one launch
        st = RowStats(ws.ss[0], 1, meta.num_tokens)
        for i, layer in enumerate(self.layers):
            st = layer.forward_fused(resid, st, meta, kv_caches[i], self.cos_sin, ws, 2 * i + 1)
        return ops.rmsnorm(resid, self.norm, self.cfg.norm_eps)

    def set_moe_comm(self, mode: str):
        for l in self.layers:
            l.moe_comm = mode

    # ------------------------------------------------------------------ init
    @torch.no_grad()
    def random_init(self, seed: int = 0, std: float = 0.02):
        g = torch.Generator(device=self.device).manual_seed(seed + 1000 * self.rank) \
            if self.device.type == "cuda" else torch.Generator().manual_seed(seed + 1000 * self.rank)
        for name, p in self.named_parameters():
            if "norm" in name:
                p.fill_(1.0)
            else:
                p.normal_(0.0, std, generator=g)
        # replicated parameters must agree across TP ranks
        ge = torch.Generator(device=self.device).manual_seed(seed) if self.device.type == "cuda" \
            else torch.Generator().manual_seed(seed)
        self.embed.normal_(0.0, std, generator=ge)
        for l in self.layers:
            if l.moe:
                l.router.normal_(0.0, std, generator=ge)

    # ------------------------------------------------------------------ forward
    def forward(self, input_ids: torch.Tensor, meta: AttnMeta,
                kv_caches: List[Tuple[torch.Tensor, torch.Tensor]]) -> torch.Tensor:
        if self.fused_decode_ok(meta):
            return self._forward_fused(input_ids, meta, kv_caches)
        x = ops.embed_gather(input_ids, self.embed) if input_ids.dtype == torch.int32 else \
            F.embedding(input_ids, self.embed)
        residual = None
        l0 = self.layers[0]
        if self.tp > 1 and l0.moe and l0._moe_use_alltoall(x):
            return self._forward_sp(x, meta, kv_caches)
        for i, layer in enumerate(self.layers):
            x, residual = layer(x, residual, meta, kv_caches[i], self.cos_sin)
        if residual is None:
            return ops.rmsnorm(x, self.norm, self.cfg.norm_eps)
        h, _ = ops.fused_add_rmsnorm(x, residual, self.norm, self.cfg.norm_eps)
        return h

    def _forward_sp(self, x: torch.Tensor, meta: AttnMeta, kv_caches) -> torch.Tensor:
        """Every layer in the sequence-parallel form (LlamaLayer.forward_sp): the
        residual stream stays token-sliced from the embedding to the final norm,
        whose rows are gathered once for the LM head."""
        T, H = x.shape
        per = (T + self.tp - 1) // self.tp
        lo = min(T, self.rank * per)
        xs = x.new_zeros(per, H)
        xs[:min(T, lo + per) - lo] = x[lo:lo + per]
        residual = None
        for i, layer in enumerate(self.layers):
            xs, residual = layer.forward_sp(xs, residual, meta, kv_caches[i], self.cos_sin, T, per)
        hs, _ = ops.fused_add_rmsnorm(xs, residual, self.norm, self.cfg.norm_eps)
        return comm.tp_all_gather_rows(hs)[:T]

    def lm_head_weight(self) -> torch.Tensor:
        """[>= vocab_size, H] (TP = 1): what ops.score_rows reads"""
        return self.embed if self.lm_head is None else self.lm_head

    def compute_logits(self, h: torch.Tensor) -> torch.Tensor:
        w = self.embed if self.lm_head is None else self.lm_head
        logits = lm_head_linear(h, w)
        if self.tp > 1:
            logits = comm.tp_all_gather_lastdim(logits)
        return logits[:, :self.cfg.vocab_size]

    def hidden_size(self) -> int:
        return self.cfg.hidden_size
