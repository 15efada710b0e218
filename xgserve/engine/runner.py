"""Model runner: step plan -> device metadata -> forward -> logits -> sampled tokens.

* The paged KV cache is one zero-initialised HBM tensor [L, 2, NB, Hkv, bs, D]
  (zero-init: stale pages can never inject NaN into masked lanes), sized from
  the free HBM left after the weights (gpu_memory_utilization of 288 GB).
* All per-step int32 metadata of an eager step is packed into ONE pinned host
  buffer and moved with ONE async H2D copy.
* Pure-decode steps replay a HIP graph captured per padded batch size; the
  graph covers embedding -> all layers -> LM head -> sampling, so a decode step
  is one graph launch + one small H2D + one D2H. Padding rows use slot -1
  (no KV write) and seq_len 0 (no attention work).
* Mixed steps of the stall-free schedule -- the decode rows plus ONE prompt
  chunk of at most `mixed_chunk` tokens (the scheduler's decode_prefill_cap) --
  replay a graph too, captured per (padded decode rows, chunk): the eager
  forward of such a step costs more host time than its ~5 ms of GPU work. The
  chunk's rows are padded to the chunk size (slot -1, outside every sequence);
  its last row's logits follow the decode rows', so the sampled tokens come out
  in the plan's sample order.
"""
from __future__ import annotations

import contextlib
import gc
import logging
import math
import os
import time
from dataclasses import dataclass
from typing import Dict, List, Optional, Tuple

import numpy as np
import torch

from .. import tune
from .. import ops
from ..models.base import AttnMeta
from ..ops.attention import DecodeWorkspace
from ..parallel import comm
from .staging import StagingRing, pinned as _pinned

# eager (prompt) steps leave their sampled tokens on the device for a looked-ahead successor
ASYNC_MIXED = True
# host wait for a step's results: poll the event (default; XGS_TUNE spin_wait=0: a
# blocking synchronize) for at most 50 ms before blocking (profiles/r2_spin_wait.md)
SPIN_WAIT = tune.get_bool("spin_wait", True)
SPIN_MAX_S = 0.050

log = logging.getLogger("xgserve.runner")


@dataclass
class SpecVerifyRows:
    """The sampled verify blocks of a step (ops.spec_verify_sample), host arrays per block:
    first logits row of the step (in sample order), first row of the draft's kept logits,
    draft tokens (ks[j] each, concatenated), temperature; one seed per position; top_ps /
    top_ks per block (None: no block is truncated)."""
    p_row0: np.ndarray
    q_row0: np.ndarray
    ks: np.ndarray
    temps: np.ndarray
    seeds: np.ndarray
    draft: np.ndarray
    q_logits: torch.Tensor
    top_ps: Optional[np.ndarray] = None
    top_ks: Optional[np.ndarray] = None


@dataclass
class SamplingRows:
    """Per-row sampling parameters (host numpy arrays), aligned with logits rows."""
    temps: np.ndarray
    top_ps: np.ndarray
    top_ks: np.ndarray
    seeds: np.ndarray  # int64, already mixed with the step counter
    # logit processors (ops.process_logits); None: every row is plain and the step
    # enqueues exactly what it did before they existed
    slots: Optional[np.ndarray] = None      # int32 state-table slot per row, -1: no history
    bias_lens: Optional[np.ndarray] = None  # int32 logit_bias entries per row (at slot * LOGIT_BIAS_MAX)
    pens: Optional[np.ndarray] = None       # float32 [4, rows]: repetition | frequency | presence | ln(min_p)
    # slots bound since the last processed step, reset ahead of this one on every rank:
    # [(slot, unique ids, cells, bias ids, bias values)]
    resets: Optional[list] = None
    # per-row extra history (speculation: a verify block's rows, a draft step's rows): an
    # int32 token list and int32 [2, rows] = offset | length (<= LOGIT_HIST_MAX) into it;
    # None: the step enqueues the processors without it
    hist_ids: Optional[np.ndarray] = None
    hist_pos: Optional[np.ndarray] = None
    # the slots of the in-step logit_state_update where they differ from `slots` (-1 for
    # the rows of a verify block, whose emitted tokens are committed after acceptance)
    upd_slots: Optional[np.ndarray] = None
    # top-N alternatives (ops.top_logprobs): int32 entries asked per row, None: no row asked
    # and the step enqueues nothing for them
    topn: Optional[np.ndarray] = None
    # speculative sampling: after the step's sampler ran over every row, these blocks' rows
    # are overwritten by the rejection-sampling verification; None: nothing is enqueued
    spec: Optional[SpecVerifyRows] = None

    @property
    def all_greedy(self) -> bool:
        return bool((self.temps <= 0).all())

    @property
    def processed(self) -> bool:
        return self.pens is not None


@dataclass(slots=True)
class TopRecord:
    """A step's top-N request: the asking rows, K, the step's sampled rows; ids / lps are the
    host results of a CPU step (None: they arrive in the step's output set, OutputSet.tops)."""
    ask: np.ndarray
    K: int
    S: int
    ids: Optional[np.ndarray]
    lps: Optional[np.ndarray]


@dataclass(slots=True)
class SpecRecord:
    """A step's sampled verify blocks: their count; acc is accepted[j] of a CPU step (None:
    it arrives in the step's output set, OutputSet.acc)."""
    nb: int
    acc: Optional[np.ndarray]


@dataclass(slots=True)
class StepHandle:
    """What launch() returns and wait() takes."""
    n: int = 0                              # sampled rows
    hidden: Optional[torch.Tensor] = None
    ready: Optional[tuple] = None           # the host result of a CPU or empty step: nothing to wait for
    out: Optional[int] = None               # the output set the step's D2H copies write into
    event: Optional[object] = None          # recorded behind those copies
    in_gout: bool = False                   # tokens | logprobs in the set's gout (one copy), else in toks / lps
    on_device: bool = False                 # the sampled tokens also stay in g_out_tok (launched_as_graph)
    follower_event: Optional[object] = None  # a step of a TP follower: no D2H, an event of this step only
    top: Optional[TopRecord] = None
    spec: Optional[SpecRecord] = None


class OutputSet:
    """One of the two sets of pinned D2H targets. A step writes into the set it acquired
    (StepHandle.out) and records one event behind all its copies; wait() waits on that
    event, and the set comes round again only after that step was waited on."""
    __slots__ = ("toks", "lps", "gout", "tops", "tins", "acc")

    def __init__(self, nt: int, OB: int):
        self.toks = _pinned(nt, torch.int32)        # an eager step's sampled tokens
        self.lps = _pinned(nt, torch.float32)       # ... and their logprobs
        self.gout = _pinned(2 * OB, torch.int32)    # a graph step's tokens | logprobs (g_out)
        self.tops = self.tins = None                # top-N results and inputs (_top_init)
        self.acc = None                             # accepted[j] of the sampled verify blocks (_spec_launch)


def stage_decode_inputs(plan: dict, n: int, bs: int, B: int, W: int, src: Optional[np.ndarray], hi: np.ndarray) -> None:
    """Host staging of a decode-graph step (ModelRunner._execute_graph): the plan's n rows
    padded to the bucket bs in the sections ids | positions | slots | seq lens | src (B
    each) of the int32 buffer `hi` (padding: id 0, position 0, slot -1, seq len 0, src -1),
    then the first bs block-table rows of width W (the plan's bt_width columns of its n
    rows are written; the sequence lengths bound what the graph reads)."""
    hi[0:n] = plan["input_ids"]
    hi[n:bs] = 0
    hi[B:B + n] = plan["positions"]
    hi[B + n:B + bs] = 0
    hi[2 * B:2 * B + n] = plan["slot_mapping"]
    hi[2 * B + n:2 * B + bs] = -1
    hi[3 * B:3 * B + n] = plan["seq_lens"]
    hi[3 * B + n:3 * B + bs] = 0
    hi[4 * B:4 * B + bs] = -1
    if src is not None:
        hi[4 * B:4 * B + n] = src
    w = int(plan["bt_width"])
    bt = hi[5 * B:5 * B + bs * W].reshape(bs, W)
    bt[:n, :w] = plan["block_tables"].reshape(n, w)


def stage_mixed_inputs(plan: dict, Nd: int, nb: int, B: int, C: int, W: int, src: Optional[np.ndarray],
                       sec: tuple, hi: np.ndarray, hl: np.ndarray) -> None:
    """Host staging of a mixed-graph step (ModelRunner._execute_mixed): the plan's Nd
    decode rows go to rows [0, Nd) and its prompt chunk's q rows to [B, B + q) of the
    static ids / positions / slot buffers (padding: id 0, position 0, slot -1); seq
    lens [0, Nd) + the chunk's at B; the chunk's query_start_loc [0, q]; block-table
    rows likewise; lidx = the logits rows in sample order (decode rows, then the
    chunk's last row). sec: the section offsets of the int32 buffer `hi`."""
    T = int(plan["num_tokens"])
    q = T - Nd
    o = sec
    for k, arr, pad in ((0, plan["input_ids"], 0), (1, plan["positions"], 0), (2, plan["slot_mapping"], -1)):
        base = o[k]
        hi[base:base + Nd] = arr[:Nd]
        hi[base + Nd:base + nb] = pad
        hi[base + B:base + B + q] = arr[Nd:T]
        hi[base + B + q:base + B + C] = pad
    sl = plan["seq_lens"]
    hi[o[3]:o[3] + Nd] = sl[:Nd]
    hi[o[3] + Nd:o[3] + nb] = 0
    hi[o[3] + B] = sl[Nd]
    hi[o[4]:o[4] + nb] = -1
    if src is not None:
        hi[o[4]:o[4] + src.shape[0]] = src
    hi[o[5]] = 0
    hi[o[5] + 1] = q
    w = int(plan["bt_width"])
    bt = hi[o[6]:o[6] + (B + 1) * W].reshape(B + 1, W)
    pbt = plan["block_tables"].reshape(Nd + 1, w)
    bt[:Nd, :w] = pbt[:Nd]
    bt[B, :w] = pbt[Nd]
    hl[:Nd] = np.arange(Nd)
    hl[Nd] = nb + q - 1
    hl[Nd + 1:nb + 1] = 0


class ModelRunner:
    DECODE_SPLIT_WGS = 512
    # the first launches run under the generous peer-wait limit too (first-call RCCL
    # communicator setup of a subgroup, first-seen library GEMM shapes)
    WARM_LAUNCHES = 32

    def __init__(self, model, *, block_size: int, num_blocks: int, max_num_seqs: int,
                 max_num_batched_tokens: int, max_model_len: int, use_graphs: bool = True,
                 graph_batch_sizes: Optional[List[int]] = None, is_driver: bool = True,
                 mixed_chunk: int = 0):
        self.model = model
        self.cfg = model.cfg
        self.device = model.device
        self.dtype = model.dtype
        self.bs = block_size
        self.num_blocks = num_blocks
        self.max_num_seqs = max_num_seqs
        self.max_tokens = max_num_batched_tokens
        self.max_model_len = max_model_len
        self.max_blocks_per_seq = (max_model_len + block_size - 1) // block_size + 1
        self.is_driver = is_driver
        self.capture_logits = False  # tests: keep the last eager step's logits
        self.last_logits = None
        cfg = self.cfg
        self.Hkv = model.num_kv_heads_local
        self.kv = torch.zeros(cfg.num_layers, 2, num_blocks, self.Hkv, block_size, cfg.head_dim,
                              dtype=self.dtype, device=self.device)
        self.kv_caches = [(self.kv[i, 0], self.kv[i, 1]) for i in range(cfg.num_layers)]
        self.is_cuda = self.device.type == "cuda"
        Hq_local = cfg.num_heads // model.tp
        self.max_splits = tune.get_int("decode_max_splits", 16)
        self.workspace = DecodeWorkspace(max(max_num_seqs, 1), Hq_local, cfg.head_dim, self.max_splits,
                                         self.device) if self.is_cuda else None
        # pinned staging for eager steps
        cap = 8 * max_num_batched_tokens + 4 * max_num_seqs * (self.max_blocks_per_seq + 4) + 64
        # two pinned host staging buffers + device twins: a step may return
        # before its async H2D copy ran, so the next step must not overwrite the
        # same host buffer until that copy's event has completed
        self.stage_ring = StagingRing({"ints": (cap, torch.int32)}, self.is_cuda, units=1)
        self.d_stages = [torch.empty(cap, dtype=torch.int32, device=self.device) for _ in range(2)]
        # top-N alternatives: nothing of this exists until a step asks (_top_init)
        self.t_out = None             # static device buffer: ids [n, K] | logprobs [n, K] of the asking rows
        self.top_result = None        # per sampled row of the step wait() last returned: [(id, lp)] or None
        # speculative sampling: accepted[j] of the step's sampled verify blocks, riding the
        # step's output set and event like the top-N results (nothing exists until a step asks)
        self.spec_result = None       # int32 per sampled block of the step wait() last returned, or None
        self.sampler_logits = None    # what the last step's sampler read, in sample order
        self.keep_sampler_logits = False  # eager steps too (a speculating draft): holds the tensor a step longer
        # eager-step sampling rows (units: rows): temperatures | top-p, top-k, seeds, and the
        # processor rows [3, n] / [4, n] of a processed step
        self.es_ring = StagingRing({"f": (2, torch.float32), "k": (1, torch.int32), "s": (1, torch.int64),
                                    "pi": (3, torch.int32), "pf": (4, torch.float32),
                                    # extra history: offset | length | update slot, and the token list
                                    "ph": (3, torch.int32), "hl": (ops.LOGIT_HIST_MAX, torch.int32)}, self.is_cuda)
        # XGS_TEST_SAMPLE_LOG=1 (tests): every eager sample of this rank, to check that TP
        # followers draw exactly the leader's tokens at temperature > 0
        self.sample_log = [] if os.environ.get("XGS_TEST_SAMPLE_LOG") == "1" else None
        # graphs
        self.use_graphs = use_graphs and self.is_cuda
        if graph_batch_sizes is None:
            graph_batch_sizes = [1, 2, 4, 8, 16, 24, 32, 48, 64, 96, 128, 160, 192, 256]
        self.graph_bs = sorted(b for b in graph_batch_sizes if b <= max_num_seqs)
        self.graphs: Dict[int, torch.cuda.CUDAGraph] = {}
        # mixed-step graphs: (decode bucket, chunk) -> graph; buckets of >= 16 decode rows
        # whose step stays on the gemm_mw path (decode rows + chunk <= MW_MAX_TOKENS)
        self.mixed_chunk = int(mixed_chunk) if (self.use_graphs and comm.get_state().tp_size == 1) else 0
        self.mixed_graphs: Dict[tuple, torch.cuda.CUDAGraph] = {}
        self.mixed_bs: List[int] = []
        self.mixed_replays = 0
        if self.mixed_chunk > 0:
            # decode rows + chunk run on gemm_mw when every layer has it and they fit
            # (<= MW_MAX_TOKENS rows), else on the library GEMMs (graph-capturable too): a
            # chunk of a whole prompt (e.g. 512) replays as one graph instead of an eager
            # step whose host-side launch of ~400 kernels the GPU would wait on
            from ..models.llama import MW_MAX_TOKENS
            mw = getattr(model, "_mw_ok", False) and 16 + self.mixed_chunk <= MW_MAX_TOKENS
            lim = MW_MAX_TOKENS if mw else max_num_batched_tokens
            self.mixed_bs = [b for b in self.graph_bs if b >= 16 and b + self.mixed_chunk <= lim]
            if not self.mixed_bs:
                self.mixed_chunk = 0
        self._graph_pool = None
        self._init_graph_buffers()
        # sampled tokens / logprobs D2H: two sets of pinned buffers + an event per step, so a
        # step launched before the previous one was waited on never overwrites its results
        nt = max(max_num_batched_tokens, max_num_seqs)
        self.out_sets = [OutputSet(nt, self.g_OB) for _ in range(2)]
        self.out_idx = 0              # read and flipped by _acquire_out only
        # logit processors: nothing of this exists until a request asks for one (_proc_init)
        self.g_pi = self.g_pf = None  # per-row parameters of a graph step
        self.p_state = None           # [max_num_seqs, V] prompt flag | generated count per slot (_state_init)
        self.p_bias_ids = self.p_bias_vals = None   # per-slot logit_bias lists, allocated with the table
        self.p_scratch = None         # fp32 processed logits of a graph step
        self.proc_graphs: Dict[tuple, torch.cuda.CUDAGraph] = {}        # (bucket, greedy), captured at first need
        self.proc_mixed_graphs: Dict[tuple, torch.cuda.CUDAGraph] = {}
        self.rst_ring = StagingRing({"ints": (1, torch.int32)}, self.is_cuda)  # slot resets (units: words)
        # read-only processor mode (a speculating draft): the table and bias lists are
        # proc_source's, never updated, reset or allocated here (set_proc_source)
        self.proc_source: Optional["ModelRunner"] = None
        self.g_ph = self.g_hist = None  # per-row extra history of a graph step (proc_hist runners)
        self.proc_hist = False          # processed graph steps take per-row extra history
        self.add_ring = StagingRing({"ints": (2, torch.int32)}, self.is_cuda)  # commit_tokens (units: entries)
        # custom all-reduce peer-wait limit while serving (EngineConfig.collective_timeout_s);
        # warmup, graph capture and the first WARM_LAUNCHES steps run under the warmup limit
        self.collective_timeout_s = 2.0
        self._warm_launches = self.WARM_LAUNCHES
        from ..parallel.custom_ar import CustomAllReduce
        self._set_comm_timeout(CustomAllReduce.WARMUP_TIMEOUT_S)

    # ------------------------------------------------------------------ utils
    def kv_bytes(self) -> int:
        return self.kv.numel() * self.kv.element_size()

    def decode_splits(self, bs: int) -> int:
        wgs = max(1, bs * self.Hkv)
        target = self.DECODE_SPLIT_WGS
        if 4 * wgs >= 3 * target:
            # within a quarter of the target (e.g. the 63 decode rows of a mixed step):
            # a second split would only add the combine launch
            return 1
        return int(max(1, min(self.max_splits, (target + wgs - 1) // wgs)))

    # ------------------------------------------------------------------ graph buffers
    def _init_graph_buffers(self):
        B = max(self.graph_bs) if self.graph_bs else 1
        W = self.max_blocks_per_seq
        self.g_B, self.g_W = B, W
        # int32 region: ids | pos | slots | sl | src | bt ; sampling region separate.
        # src[i] >= 0: row i's input id is the previous graph step's sampled token
        # g_out_tok[src[i]] (asynchronous scheduling), substituted inside the graph
        n = 5 * B + B * W
        self.g_int = torch.zeros(n, dtype=torch.int32, device=self.device)
        self.g_ids = self.g_int[0:B]
        self.g_pos = self.g_int[B:2 * B]
        self.g_slot = self.g_int[2 * B:3 * B]
        self.g_sl = self.g_int[3 * B:4 * B]
        self.g_src = self.g_int[4 * B:5 * B]
        self.g_bt = self.g_int[5 * B:5 * B + B * W].view(B, W)
        # sampling parameters: one row more than the widest decode graph (mixed steps)
        self.g_temp = torch.zeros(B + 1, dtype=torch.float32, device=self.device)
        self.g_topp = torch.ones(B + 1, dtype=torch.float32, device=self.device)
        self.g_topk = torch.zeros(B + 1, dtype=torch.int32, device=self.device)
        self.g_seed = torch.zeros(B + 1, dtype=torch.int64, device=self.device)
        # two sets of pinned host inputs (event-guarded): the next step's inputs can be
        # written while this step's H2D copies are still queued behind the GPU
        ring = {"ints": (n, torch.int32), "samp_f": (2 * (B + 1), torch.float32), "samp_i": (B + 1, torch.int32),
                "samp_s": (B + 1, torch.int64)}
        # sampled tokens [0, OB) and their logprobs [OB, 2 OB) in one buffer: a graph step's
        # outputs leave in ONE D2H copy (g_out[:OB + n]) instead of two; OB = B + 1 (a
        # mixed step samples its decode rows + the chunk's last row)
        OB = self.g_OB = B + 1
        self.g_out = torch.zeros(2 * OB, dtype=torch.int32, device=self.device)
        self.g_out_tok = self.g_out[:OB]
        self.g_out_lp = self.g_out[OB:].view(torch.float32)
        self.g_greedy_graph: Dict[int, bool] = {}
        # mixed-step inputs: ids | pos | slot (B + C rows each) | sl (B + 1) | src (B) |
        # qsl (2) | bt ((B + 1) x W) ; lidx (int64, B + 1)
        C = self.mixed_chunk
        if C > 0:
            R = B + C
            self.m_sec = (0, R, 2 * R, 3 * R, 3 * R + B + 1, 3 * R + 2 * B + 1, 3 * R + 2 * B + 3)
            n_m = self.m_sec[-1] + (B + 1) * W
            self.m_int = torch.zeros(n_m, dtype=torch.int32, device=self.device)
            o = self.m_sec
            self.m_ids, self.m_pos, self.m_slot = self.m_int[o[0]:o[1]], self.m_int[o[1]:o[2]], self.m_int[o[2]:o[3]]
            self.m_sl, self.m_src, self.m_qsl = self.m_int[o[3]:o[4]], self.m_int[o[4]:o[5]], self.m_int[o[5]:o[6]]
            self.m_bt = self.m_int[o[6]:].view(B + 1, W)
            self.m_lidx = torch.zeros(B + 1, dtype=torch.int64, device=self.device)
            ring.update(mints=(n_m, torch.int32), mlidx=(B + 1, torch.int64))
        self.g_ring = StagingRing(ring, self.is_cuda, units=1)

    def _decode_body(self, bs: int, greedy: bool, proc: bool = False):
        ops.subst_tokens(self.g_ids[:bs], self.g_src[:bs], self.g_out_tok)
        meta = AttnMeta(num_tokens=bs, num_decodes=bs, positions=self.g_pos[:bs], slot_mapping=self.g_slot[:bs],
                        dec_block_tables=self.g_bt[:bs], dec_seq_lens=self.g_sl[:bs],
                        num_splits=self.decode_splits(bs), workspace=self.workspace)
        h = self.model(self.g_ids[:bs], meta, self.kv_caches)
        return self._sample_rows(self.model.compute_logits(h), bs, greedy, proc)

    def _sample_rows(self, logits: torch.Tensor, rows: int, greedy: bool, proc: bool):
        """The tail of a graph body: process -> argmax or sample into g_out -> state update."""
        if proc:
            logits = ops.process_logits(logits, self.p_scratch[:rows], self.p_state, self.g_pi, self.g_pf,
                                        self.g_temp, self.p_bias_ids, self.p_bias_vals,
                                        self.g_hist if self.proc_hist else None, self.g_ph if self.proc_hist else None)
        if greedy:
            ops.argmax_logprob(logits, self.g_out_tok[:rows], self.g_out_lp[:rows])
        else:
            tok, lp = ops.sample_tokens(logits, self.g_temp[:rows], self.g_topp[:rows], self.g_topk[:rows],
                                        self.g_seed[:rows], step=0)
            self.g_out_tok[:rows].copy_(tok)
            self.g_out_lp[:rows].copy_(lp)
        if proc and self.p_state is not None and self.proc_source is None:
            ops.logit_state_update(self.p_state, self.g_pi[0], self.g_out_tok, rows)
        return logits  # what the sampler read: kept by the graph for an eager top_logprobs after a replay

    def _mixed_body(self, nb: int, greedy: bool, proc: bool = False):
        """nb decode rows (padded) + one prompt chunk of up to C rows (padded) -> the
        sampled tokens of the decode rows and the chunk's last row (g_out_tok[:nb + 1])."""
        B, C = self.g_B, self.mixed_chunk
        T = nb + C
        ops.subst_tokens(self.m_ids[:nb], self.m_src[:nb], self.g_out_tok)
        ids, pos, slot = self.m_ids[:B + C], self.m_pos[:B + C], self.m_slot[:B + C]
        # decode rows [0, nb) and the chunk [B, B + C) of the B + C row buffers, as one
        # contiguous [nb + C] view when nb == B, else gathered into place
        if nb == B:
            ids_t, pos_t, slot_t = ids, pos, slot
        else:
            ids_t = torch.cat([ids[:nb], ids[B:]])
            pos_t = torch.cat([pos[:nb], pos[B:]])
            slot_t = torch.cat([slot[:nb], slot[B:]])
        meta = AttnMeta(num_tokens=T, num_decodes=nb, positions=pos_t, slot_mapping=slot_t,
                        dec_block_tables=self.m_bt[:nb], dec_seq_lens=self.m_sl[:nb],
                        num_splits=self.decode_splits(nb), workspace=self.workspace,
                        pre_block_tables=self.m_bt[B:B + 1], pre_qsl=self.m_qsl, pre_seq_lens=self.m_sl[B:B + 1],
                        pre_max_q=C)
        h = self.model(ids_t, meta, self.kv_caches)
        logits = self.model.compute_logits(h.index_select(0, self.m_lidx[:nb + 1]))
        return self._sample_rows(logits, nb + 1, greedy, proc)

    # ------------------------------------------------------------------ logit processors
    def _proc_init(self) -> None:
        """Per-row parameter buffers and the fp32 scratch of graph steps: allocated by the
        first step that is not plain, out of the gpu_memory_utilization headroom (the KV
        pool was sized before)."""
        if self.g_pi is not None:
            return
        V = self.cfg.vocab_size
        R = self.g_OB
        # [slot | bias offset | bias length] and [repetition | frequency | presence | ln(min_p)] per row
        self.g_pi = torch.zeros(3, R, dtype=torch.int32, device=self.device)
        self.g_pi[0].fill_(-1)
        self.g_pf = torch.zeros(4, R, dtype=torch.float32, device=self.device)
        self.g_ring.add({"pi": (3 * R, torch.int32), "pf": (4 * R, torch.float32)})
        if self.proc_hist:  # [offset | length] per row, row i's list at i * LOGIT_HIST_MAX
            H = ops.LOGIT_HIST_MAX
            self.g_ph = torch.zeros(2, R, dtype=torch.int32, device=self.device)
            self.g_hist = torch.zeros(R * H, dtype=torch.int32, device=self.device)
            self.g_ring.add({"ph": (2 * R, torch.int32), "hl": (R * H, torch.int32)})
        if self.use_graphs:
            self.p_scratch = ops.process_scratch(R, V, self.device)

    def set_proc_source(self, source: "ModelRunner") -> None:
        """Read-only processor mode: this runner processes its rows against `source`'s state
        table and bias lists (same device), with per-row extra history in its graph steps.
        It never enqueues logit_state_update, never applies resets and never allocates a
        table; the table is aliased again at every launch, as the source allocates its own
        at its first request that needs one (the processed graphs are keyed on it)."""
        assert source.device == self.device and source.cfg.vocab_size == self.cfg.vocab_size
        self.proc_source = source
        self.proc_hist = True

    def _alias_proc_source(self) -> None:
        src = self.proc_source
        self.p_state, self.p_bias_ids, self.p_bias_vals = src.p_state, src.p_bias_ids, src.p_bias_vals

    def commit_tokens(self, slots: np.ndarray, toks: np.ndarray) -> None:
        """count[slot][token] += 1 for the emitted tokens of verify blocks (entries may repeat
        a slot and a pair): ops.logit_state_add on the step's stream, ahead of whatever
        reads the table next."""
        n = int(len(slots))
        if n == 0 or self.p_state is None:
            return
        h = self.add_ring.acquire(max(n, 64))["ints"]
        hn = h.numpy()
        hn[:n] = slots
        hn[n:2 * n] = toks
        d = h[:2 * n].to(self.device, non_blocking=True)
        self.add_ring.fence()
        ops.logit_state_add(self.p_state, d[:n], d[n:], n)

    def _state_init(self) -> None:
        """The state table and the per-slot bias lists: allocated by the first request
        that needs token statistics (min_p alone does not). Processed graphs captured
        before hold no table; they are keyed apart from those captured after."""
        if self.p_state is not None or self.proc_source is not None:
            return
        V, ns, nb = self.cfg.vocab_size, self.max_num_seqs, ops.LOGIT_BIAS_MAX
        self.p_state = ops.logit_state_alloc(ns, V, self.device)
        self.p_bias_ids = torch.zeros(ns * nb, dtype=torch.int32, device=self.device)
        self.p_bias_vals = torch.zeros(ns * nb, dtype=torch.float32, device=self.device)
        log.info("logit processors: state table %d x %d (%.1f MiB)", ns, V, ns * V * 2 / 2**20)

    def _apply_resets(self, resets: list) -> None:
        """Rows of the state table (and bias lists) of newly bound slots, staged through
        the reset ring; enqueued on the step's stream, so every update
        of the slot's previous owner lands before and the owner's first step after."""
        self._state_init()
        nb = ops.LOGIT_BIAS_MAX
        packed, nres, total = ops.pack_state_resets([r[:3] for r in resets])
        n = packed.size + 2 * nres * nb
        h = self.rst_ring.acquire(max(n, 1 << 16))["ints"]
        hn = h.numpy()
        hn[:packed.size] = packed
        bi = hn[packed.size:packed.size + nres * nb].reshape(nres, nb)
        bv = hn[packed.size + nres * nb:n].view(np.float32).reshape(nres, nb)
        bi[:] = 0
        bv[:] = 0.0
        for j, r in enumerate(resets):
            k = len(r[3])
            bi[j, :k] = r[3]
            bv[j, :k] = r[4]
        d = h[:n].to(self.device, non_blocking=True)
        self.rst_ring.fence()
        ops.logit_state_reset(self.p_state, d, nres, total)
        for j, r in enumerate(resets):
            if len(r[3]):
                s, o = int(r[0]), packed.size + j * nb
                self.p_bias_ids[s * nb:(s + 1) * nb].copy_(d[o:o + nb])
                self.p_bias_vals[s * nb:(s + 1) * nb].copy_(d[o + nres * nb:o + nres * nb + nb].view(torch.float32))

    @staticmethod
    def _fill_proc_rows(pi: np.ndarray, pf: np.ndarray, samp: SamplingRows, n: int, rows: int) -> None:
        """Host rows [0, n) from `samp`, padding rows [n, rows) plain (pi: [3, R], pf: [4, R])."""
        pi[0, :n] = samp.slots
        pi[1, :n] = np.maximum(samp.slots, 0) * ops.LOGIT_BIAS_MAX
        pi[2, :n] = samp.bias_lens
        pf[:, :n] = samp.pens
        pi[0, n:rows] = -1
        pi[1:, n:rows] = 0
        pf[0, n:rows] = 1.0
        pf[1:3, n:rows] = 0.0
        pf[3, n:rows] = -np.inf

    def _stage_proc(self, slot: dict, samp: SamplingRows, n: int, rows: int) -> None:
        """Per-row processor parameters of a graph step -> g_pi / g_pf (rows >= n: plain)."""
        R = self.g_OB
        hi, hf = slot["pi"], slot["pf"]
        self._fill_proc_rows(hi.numpy().reshape(3, R), hf.numpy().reshape(4, R), samp, n, rows)
        self.g_pi.view(-1).copy_(hi, non_blocking=True)
        self.g_pf.view(-1).copy_(hf, non_blocking=True)
        if self.proc_hist:
            H = ops.LOGIT_HIST_MAX
            hp, hl = slot["ph"], slot["hl"]
            ph = hp.numpy().reshape(2, R)
            ph[:] = 0
            if samp.hist_pos is not None:
                # every row's own copy of its list at row * H: the graph's list has a fixed layout
                ops.check_hist_pos(samp.hist_pos, len(samp.hist_ids), n)
                lst = hl.numpy().reshape(R, H)
                for i in range(n):
                    o, ln = int(samp.hist_pos[0, i]), int(samp.hist_pos[1, i])
                    lst[i, :ln] = samp.hist_ids[o:o + ln]
                    ph[0, i], ph[1, i] = i * H, ln
                self.g_hist[:n * H].copy_(hl[:n * H], non_blocking=True)
            self.g_ph.view(-1).copy_(hp, non_blocking=True)

    def _proc_graph(self, key: tuple, mixed: bool):
        """The processed form of a decode (mixed) graph, captured when a step first needs
        it. Steps may still be running ahead (asynchronous scheduling), so the device is
        drained first; the warm-up run and the capture see neutral inputs (padding rows,
        no tracked slot) and the static buffers get their contents back afterwards."""
        graphs = self.proc_mixed_graphs if mixed else self.proc_graphs
        n, greedy = key
        key = (n, greedy, self.p_state is not None)  # (a read-only runner: its source's table, aliased at launch)
        g = graphs.get(key)
        if g is not None:
            return g
        torch.cuda.synchronize()
        body = (lambda: self._mixed_body(n, greedy, True)) if mixed else (lambda: self._decode_body(n, greedy, True))
        keep = [self.g_int, self.g_out, self.g_pi] + ([self.m_int, self.m_lidx] if mixed else [])
        saved = [t.clone() for t in keep]
        with self._gc_held():
            self._neutral_inputs(mixed)
            self.g_pi[0].fill_(-1)
            self.g_pi[2].zero_()
            if self.g_ph is not None:
                self.g_ph.zero_()
            g = self._warm_and_capture([(key, body)], warm=1, error_mode="thread_local")[key]
        for t, c in zip(keep, saved):
            t.copy_(c)
        torch.cuda.synchronize()
        graphs[key] = g
        log.info("captured the processed %s graph %s", "mixed-step" if mixed else "decode", key)
        return g

    # ---- capture choreography shared by the start-up graphs and the processed ones
    @staticmethod
    @contextlib.contextmanager
    def _gc_held():
        """An engine that was dropped earlier is a reference cycle: its graphs and their
        pool live until the cycle collector runs. A collection in the middle of a
        capture would destroy them inside the capturing region (graph destruction and
        the pool's frees are not allowed there) and abort the process, so collect now
        and hold automatic collections off until the last capture has ended."""
        gc.collect()
        gc_was_enabled = gc.isenabled()
        gc.disable()
        try:
            yield
        finally:
            if gc_was_enabled:
                gc.enable()

    def _neutral_inputs(self, mixed: bool) -> None:
        if mixed:  # padding decode rows, an empty chunk (q = 0: no attention rows)
            self.m_int.zero_()
            self.m_slot.fill_(-1)
            self.m_src.fill_(-1)
            self.m_lidx.zero_()
        else:      # padding rows (no KV writes, no attention work)
            self.g_slot.fill_(-1)
            self.g_src.fill_(-1)
            self.g_sl.fill_(0)
            self.g_ids.fill_(0)
            self.g_pos.fill_(0)

    def _warm_and_capture(self, bodies: list, warm: int, error_mode: str = "global") -> dict:
        """bodies: [(key, fn)]. Every fn runs `warm` times on a side stream, then each is
        captured into the shared graph pool. Returns {key: graph}."""
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            for _, fn in bodies:
                for _ in range(warm):
                    fn()
        torch.cuda.current_stream().wait_stream(s)
        torch.cuda.synchronize()
        if self._graph_pool is None:
            self._graph_pool = torch.cuda.graph_pool_handle()
        out = {}
        for key, fn in bodies:
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, pool=self._graph_pool, capture_error_mode=error_mode):
                kept = fn()
            # the body's logits rows stay referenced, so no later capture of the pool reuses
            # their storage: a replay leaves them readable until the next replay
            g.xgs_logits = kept
            out[key] = g
        torch.cuda.synchronize()
        return out

    def _set_comm_timeout(self, seconds: float) -> None:
        from ..parallel.custom_ar import CustomAllReduce
        ar = comm.custom_allreduce()
        if ar is not None:
            ar.set_timeout(seconds if seconds >= CustomAllReduce.WARMUP_TIMEOUT_S else ar.serve_timeout(seconds))

    @torch.no_grad()
    def capture_graphs(self):
        if not self.use_graphs or not self.graph_bs:
            return
        with self._gc_held():
            self._capture_graphs()

    def _capture_graphs(self):
        torch.cuda.synchronize()
        self._neutral_inputs(False)
        bodies = [((bs, greedy), (lambda bs=bs, greedy=greedy: self._decode_body(bs, greedy)))
                  for bs in reversed(self.graph_bs) for greedy in (True, False)]
        self.graphs.update(self._warm_and_capture(bodies, warm=2))
        log.info("captured %d decode graphs (batch sizes %s)", len(self.graphs), self.graph_bs)
        if self.mixed_chunk > 0:
            self._capture_mixed()

    def _capture_mixed(self):
        self._neutral_inputs(True)
        bodies = [((nb, greedy), (lambda nb=nb, greedy=greedy: self._mixed_body(nb, greedy)))
                  for nb in reversed(self.mixed_bs) for greedy in (True, False)]
        self.mixed_graphs.update(self._warm_and_capture(bodies, warm=2))
        log.info("captured %d mixed-step graphs (decode rows %s + a %d-token chunk)", len(self.mixed_graphs),
                 self.mixed_bs, self.mixed_chunk)

    def _mixed_bucket(self, plan, Nd: int, ns: int, T: int) -> Optional[int]:
        """Decode bucket of a mixed-graph step, or None: Nd decode rows + exactly one
        prefill chunk of <= mixed_chunk tokens (no verify rows, no embeddings)."""
        if not self.mixed_graphs or ns != Nd + 1 or T - Nd > self.mixed_chunk or T - Nd < 1:
            return None
        if not plan["is_prefill"][Nd] or plan["is_embed"][Nd]:
            return None
        for b in self.mixed_bs:
            if b >= Nd:
                return b
        return None

    def _graph_bucket(self, n: int) -> Optional[int]:
        for b in self.graph_bs:
            if b >= n:
                return b
        return None

    # ------------------------------------------------------------------ execution
    @torch.no_grad()
    def execute(self, plan: dict, samp: Optional[SamplingRows]):
        """Run one step. Returns (tokens np[int32], logprobs np[float32], hidden or None).
        On non-driver TP ranks the returned arrays are None."""
        return self.wait(self.launch(plan, samp))

    @torch.no_grad()
    def launch(self, plan: dict, samp: Optional[SamplingRows], src: Optional[np.ndarray] = None) -> StepHandle:
        """Enqueue one step (inputs H2D, forward, sampling, tokens D2H) without
        waiting for it; `wait(handle)` returns what `execute` returns. The host
        can do other work (previous step's detokenisation, planning the next step)
        while the GPU runs. `src` (asynchronous scheduling): per decode row, the
        row of the previous GRAPH step whose sampled token is this row's input
        (-1: the plan's own id)."""
        T = int(plan["num_tokens"])
        Nd = int(plan["num_decodes"])
        ns = int(plan["num_seqs"])
        if T == 0:
            return StepHandle(ready=(None, None, None))
        if self.proc_source is not None:
            self._alias_proc_source()
        if samp is not None and samp.processed and samp.resets:
            assert self.proc_source is None, "a read-only runner applies no resets"
            self._apply_resets(samp.resets)
        if self._warm_launches:
            self._warm_launches -= 1
            if self._warm_launches == 0:
                self._set_comm_timeout(self.collective_timeout_s)
        need_hidden = bool(plan["is_embed"].any()) if ns else False
        bucket = self._graph_bucket(Nd) if (Nd == ns and T == Nd and not need_hidden) else None
        if bucket is not None and self.graphs:
            return self._execute_graph(plan, samp, Nd, bucket, src)
        if not need_hidden and self.mixed_chunk > 0:
            mb = self._mixed_bucket(plan, Nd, ns, T)
            if mb is not None:
                return self._execute_mixed(plan, samp, Nd, mb, src)
        return self._execute_eager(plan, samp, need_hidden, src)

    def launched_as_graph(self, handle: StepHandle) -> bool:
        """True if the step left its sampled tokens in g_out_tok (every graph step,
        and eager steps that qualify, _async_ok): the next step may be
        planned and launched before this one completes."""
        return handle.on_device

    @staticmethod
    def _poll_comm():
        """Queue the custom all-reduce's error-counter copy behind this step's work
        (TP): wait() then fails the step if a peer wait timed out."""
        ar = comm.custom_allreduce()
        if ar is not None:
            ar.poll_async()

    @staticmethod
    def _check_comm():
        ar = comm.custom_allreduce()
        if ar is not None:
            ar.check()

    def _acquire_out(self) -> int:
        """The output set this step's D2H copies go to; the one place that flips out_idx."""
        i = self.out_idx
        self.out_idx ^= 1
        return i

    def _record_out(self, h: StepHandle, tok: torch.Tensor, lp: torch.Tensor) -> StepHandle:
        """Tokens / logprobs D2H into the step's output set + an event."""
        self._poll_comm()
        o, n = self.out_sets[h.out], h.n
        o.toks[:n].copy_(tok[:n], non_blocking=True)
        o.lps[:n].copy_(lp[:n], non_blocking=True)
        h.event = torch.cuda.Event()
        h.event.record()
        return h

    def _follower_out(self, h: StepHandle) -> StepHandle:
        """A step of a TP follower: no D2H to wait on, so an event of THIS step -- a
        follower that queued its successor waits for this launch only
        (engine.follower_loop), not the whole stream; wait() still drains before the
        pinned inputs get rewritten."""
        self._poll_comm()
        h.follower_event = torch.cuda.Event()
        h.follower_event.record()
        return h

    @staticmethod
    def _wait_event(ev):
        """Block until `ev` completed. SPIN_WAIT: poll hipEventQuery instead of a
        blocking synchronize (whose sleeping wake-up costs ~0.1 ms per step on the host
        critical path), falling back to the blocking wait after SPIN_MAX_S."""
        if not SPIN_WAIT:
            ev.synchronize()
            return
        t_end = time.perf_counter() + SPIN_MAX_S
        while not ev.query():
            if time.perf_counter() > t_end:
                ev.synchronize()
                return

    def wait(self, handle: StepHandle):
        res = self._wait(handle)
        self.top_result = self._top_collect(handle) if handle.top is not None else None
        self.spec_result = self._spec_collect(handle) if handle.spec is not None else None
        return res

    def _wait(self, h: StepHandle):
        if h.ready is not None:
            return h.ready
        if h.follower_event is not None:
            self._wait_event(h.follower_event)  # this step only (TP follower with a successor queued)
            self._check_comm()
            return None, None, h.hidden
        self._wait_event(h.event)  # this step only: a step queued behind it keeps running
        self._check_comm()
        o, n = self.out_sets[h.out], h.n
        if h.in_gout:  # graph step: tokens and logprobs in one pinned buffer
            OB = self.g_OB
            return o.gout[:n].numpy().copy(), o.gout[OB:OB + n].view(torch.float32).numpy().copy(), h.hidden
        return o.toks[:n].numpy().copy(), o.lps[:n].numpy().copy(), h.hidden

    # ------------------------------------------------------------------ top-N alternatives
    def _top_init(self) -> None:
        if self.t_out is not None:
            return
        nt, K = max(self.max_tokens, self.max_num_seqs, self.g_OB), ops.TOPLP_MAX
        self._t_rows = nt
        self.t_out = torch.zeros(2 * nt * K, dtype=torch.int32, device=self.device)
        # per output set: results, and the inputs [asking rows | temperatures]
        for o in self.out_sets:
            o.tops = _pinned(2 * nt * K, torch.int32)
            o.tins = _pinned(2 * nt, torch.int32)

    def _top_launch(self, logits: torch.Tensor, samp: SamplingRows, h: StepHandle) -> None:
        """ops.top_logprobs over the rows of `logits` (what this step's sampler read, in
        sample order) that asked, into the static buffer, and its D2H into the pinned
        buffer of the step's output set -- queued in front of the step's token copy, so the
        event wait() waits on covers it and the pinned sets are fenced as the token buffers are."""
        S = len(samp.temps)
        ask = np.nonzero(samp.topn[:S] > 0)[0].astype(np.int32)
        na = int(ask.shape[0])
        if na == 0 or not self.is_driver:
            return
        K = int(min(ops.TOPLP_MAX, samp.topn.max()))
        if not self.is_cuda:
            rows = torch.from_numpy(ask)
            ids, lps = ops.top_logprobs(logits[:S], torch.from_numpy(np.ascontiguousarray(samp.temps, np.float32)), K,
                                        rows)
            h.top = TopRecord(ask, K, S, ids.numpy(), lps.numpy())
            return
        self._top_init()
        assert S <= self._t_rows and logits.shape[0] >= S
        out = self.out_sets[h.out]
        hin = out.tins
        a = hin.numpy()
        a[:na] = ask
        a[na:na + S].view(np.float32)[:] = samp.temps
        d = hin[:na + S].to(self.device, non_blocking=True)
        o = self.t_out
        ops.top_logprobs(logits[:S], d[na:].view(torch.float32), K, d[:na], o[:na * K],
                         o[na * K:2 * na * K].view(torch.float32))
        out.tops[:2 * na * K].copy_(o[:2 * na * K], non_blocking=True)
        h.top = TopRecord(ask, K, S, None, None)

    def _top_collect(self, h: StepHandle):
        t = h.top
        na, K, ids, lps = t.ask.shape[0], t.K, t.ids, t.lps
        if ids is None:
            host = self.out_sets[h.out].tops.numpy()
            ids = host[:na * K].reshape(na, K).copy()
            lps = host[na * K:2 * na * K].view(np.float32).reshape(na, K).copy()
        top = [None] * t.S
        for j, r in enumerate(t.ask.tolist()):
            top[r] = list(zip(ids[j].tolist(), lps[j].tolist()))
        return top

    # ------------------------------------------------------------------ speculative sampling
    def last_sampler_logits(self) -> Optional[torch.Tensor]:
        """The logits rows the last launched step's sampler read, in sample order (a graph
        step's static buffer: valid until the next replay of that graph; eager steps keep
        theirs only under keep_sampler_logits)."""
        return self.sampler_logits

    def _spec_launch(self, logits: torch.Tensor, tok: torch.Tensor, lp: torch.Tensor, sv: SpecVerifyRows,
                     h: StepHandle) -> None:
        """ops.spec_verify_sample over the step's sampled verify blocks: overwrites their
        rows of tok / lp in place; accepted[j] leaves with the step's output set (queued in
        front of the token copy, covered by the event wait() waits on)."""
        nb = len(sv.ks)
        d_off = np.concatenate([[0], np.cumsum(sv.ks)[:-1]])
        _, _, acc = ops.spec_verify_sample(logits, sv.q_logits, sv.draft, sv.p_row0, sv.q_row0, d_off, sv.ks, sv.temps,
                                           sv.seeds, out_row0=sv.p_row0, out_tok=tok, out_lp=lp,
                                           top_ps=sv.top_ps, top_ks=sv.top_ks)
        if not self.is_cuda:
            h.spec = SpecRecord(nb, acc.numpy().copy())
            return
        out = self.out_sets[h.out]
        if out.acc is None:
            for o in self.out_sets:
                o.acc = _pinned(max(self.max_num_seqs, self.max_tokens), torch.int32)
        out.acc[:nb].copy_(acc, non_blocking=True)
        h.spec = SpecRecord(nb, None)

    def _spec_collect(self, h: StepHandle):
        if h.spec.acc is not None:
            return h.spec.acc
        return self.out_sets[h.out].acc[:h.spec.nb].numpy().copy()

    # ------------------------------------------------------------------ graph steps
    def _execute_graph(self, plan, samp: Optional[SamplingRows], n: int, bs: int, src: Optional[np.ndarray]):
        B, W = self.g_B, self.g_W
        greedy = samp is None or samp.all_greedy
        proc = samp is not None and samp.processed
        if proc:
            self._proc_init()
        graph = self._proc_graph((bs, greedy), False) if proc else self.graphs[(bs, greedy)]
        slot = self.g_ring.acquire()
        h_int = slot["ints"]
        stage_decode_inputs(plan, n, bs, B, W, src, h_int.numpy())
        # ids..src (5*B) and the first bs rows of bt: one contiguous H2D copy
        self.g_int[:5 * B + bs * W].copy_(h_int[:5 * B + bs * W], non_blocking=True)
        return self._replay(graph, slot, samp, n, bs, False)

    def _execute_mixed(self, plan, samp: Optional[SamplingRows], Nd: int, nb: int, src: Optional[np.ndarray]):
        """Replay the (nb, chunk) mixed graph: Nd decode rows at [0, Nd), the prompt
        chunk's q rows at [B, B + q) of the static input buffers."""
        B, W, C = self.g_B, self.g_W, self.mixed_chunk
        greedy = samp is None or samp.all_greedy
        proc = samp is not None and samp.processed
        if proc:
            self._proc_init()
        graph = self._proc_graph((nb, greedy), True) if proc else self.mixed_graphs[(nb, greedy)]
        slot = self.g_ring.acquire()
        stage_mixed_inputs(plan, Nd, nb, B, C, W, src, self.m_sec, slot["mints"].numpy(), slot["mlidx"].numpy())
        self.m_int.copy_(slot["mints"], non_blocking=True)
        self.m_lidx[:nb + 1].copy_(slot["mlidx"][:nb + 1], non_blocking=True)
        return self._replay(graph, slot, samp, int(plan["num_sample"]), nb + 1, True)

    def _replay(self, graph, slot: dict, samp: Optional[SamplingRows], n: int, rows: int, mixed: bool) -> StepHandle:
        """The tail of a graph step, its inputs already copied from the ring slot: stage the
        sampling and processor rows (`rows`: the graph's sampled rows, n of them real),
        fence the slot, replay, then the step's outputs."""
        proc = samp is not None and samp.processed
        if proc or not (samp is None or samp.all_greedy):
            self._stage_sampling(slot, samp, n)
        if proc:
            self._stage_proc(slot, samp, n, rows)
        self.g_ring.fence()
        graph.replay()
        self.sampler_logits = graph.xgs_logits
        h = StepHandle(n=n, on_device=True)
        if self.is_driver:
            h.out = self._acquire_out()
        if samp is not None and samp.topn is not None:
            self._top_launch(graph.xgs_logits, samp, h)
        self.mixed_replays += mixed
        self._log_samples(n)
        if not self.is_driver:
            return self._follower_out(h)
        # a graph step's n sampled tokens + logprobs (g_out) leave in one D2H copy
        OB = self.g_OB
        self._poll_comm()
        self.out_sets[h.out].gout[:OB + n].copy_(self.g_out[:OB + n], non_blocking=True)
        h.in_gout = True
        h.event = torch.cuda.Event()
        h.event.record()
        return h

    def _stage_sampling(self, slot: dict, samp: SamplingRows, n: int) -> None:
        """Per-row sampling parameters of a graph step -> g_temp / g_topp / g_topk / g_seed."""
        hf, hsi, hss = slot["samp_f"], slot["samp_i"], slot["samp_s"]
        OB = self.g_OB
        f = hf.numpy()
        f[:n] = samp.temps
        f[OB:OB + n] = samp.top_ps
        hsi.numpy()[:n] = samp.top_ks
        hss.numpy()[:n] = samp.seeds
        self.g_temp[:n].copy_(hf[:n], non_blocking=True)
        self.g_topp[:n].copy_(hf[OB:OB + n], non_blocking=True)
        self.g_topk[:n].copy_(hsi[:n], non_blocking=True)
        self.g_seed[:n].copy_(hss[:n], non_blocking=True)

    # ------------------------------------------------------------------ eager steps
    def _stage_parts(self, parts):
        """The int32 arrays of an eager step -> ONE pinned host buffer -> ONE async H2D
        copy (the eager ring). Returns (device buffer, section offsets)."""
        sizes = [p.size for p in parts]
        total = sum(sizes)
        h_stage = self.stage_ring.acquire()["ints"]
        hs = h_stage.numpy()
        off = 0
        for p in parts:
            hs[off:off + p.size] = p.reshape(-1)
            off += p.size
        if self.is_cuda:
            dev = self.d_stages[self.stage_ring.slot]
            dev[:total].copy_(h_stage[:total], non_blocking=True)
            self.stage_ring.fence()
        else:
            dev = h_stage
        return dev, np.cumsum([0] + sizes)

    def _execute_eager(self, plan, samp: Optional[SamplingRows], need_hidden: bool, src: Optional[np.ndarray]):
        T = int(plan["num_tokens"])
        Nd = int(plan["num_decodes"])
        ns = int(plan["num_seqs"])
        w = int(plan["bt_width"])
        Np = ns - Nd
        li = plan["logits_indices"]
        S = li.shape[0]
        qsl = plan["query_start_loc"]
        parts = [plan["input_ids"], plan["positions"], plan["slot_mapping"],
                 plan["block_tables"], plan["seq_lens"], (qsl[Nd:] - Nd).astype(np.int32), li]
        if src is not None:  # staged with the other inputs: no blocking copy ahead of the queued step
            parts.append(np.ascontiguousarray(src, dtype=np.int32))
        dev, o = self._stage_parts(parts)
        ids = dev[o[0]:o[1]]
        pos = dev[o[1]:o[2]]
        slots = dev[o[2]:o[3]]
        bt = dev[o[3]:o[4]].view(ns, w)
        sl = dev[o[4]:o[5]]
        pre_qsl = dev[o[5]:o[6]]
        lidx = dev[o[6]:o[7]]
        if src is not None:  # decode rows first: their ids from the previous step's sampled tokens
            ops.subst_tokens(ids[:src.shape[0]], dev[o[7]:o[8]], self.g_out_tok)
        meta = AttnMeta(num_tokens=T, num_decodes=Nd, positions=pos, slot_mapping=slots,
                        dec_block_tables=bt[:Nd], dec_seq_lens=sl[:Nd],
                        num_splits=self.decode_splits(Nd) if self.is_cuda else 1, workspace=self.workspace,
                        pre_block_tables=bt[Nd:], pre_qsl=pre_qsl, pre_seq_lens=sl[Nd:],
                        pre_max_q=int(plan["q_lens"][Nd:].max()) if Np > 0 else 0)
        h = self.model(ids, meta, self.kv_caches)
        hid = h if need_hidden else None
        if S == 0:
            return StepHandle(hidden=hid, ready=(np.zeros(0, np.int32), np.zeros(0, np.float32), hid))
        logits = self.model.compute_logits(h.index_select(0, lidx.long()))
        if self.capture_logits:
            self.last_logits = logits.float().cpu()
        hd = StepHandle(n=S, hidden=hid, out=self._acquire_out() if self.is_driver else None)
        if not self.is_cuda:
            if self.is_driver:
                tok, lp = self._sample(logits, samp, hd)
                hd.ready = (tok.numpy().astype(np.int32), lp.numpy().astype(np.float32), hid)
            else:
                hd.ready = (None, None, hid)
            return hd
        # also leave the sampled tokens in g_out_tok, in sample order, so the engine can plan
        # and launch the next step before this one ends (its decode rows substitute their
        # ids from there). Asynchronous prompt steps under TP: when the leader leaves this
        # step's tokens on the device, so does every follower -- the same all-gathered
        # logits and the leader's broadcast sampling rows give the same tokens, and the
        # successor's decode rows substitute their ids from this rank's g_out_tok exactly
        # as after a graph step
        hd.on_device = self._async_ok(S, plan)
        # a processed step is sampled on every rank even when its tokens stay unused
        # there: the sampling advances that rank's token statistics
        if self.is_driver or hd.on_device or (samp is not None and samp.processed):
            tok, lp = self._sample(logits, samp, hd)
        if hd.on_device:
            self.g_out_tok[:S].copy_(tok[:S])
            self._log_samples(S)
        return self._record_out(hd, tok, lp) if self.is_driver else self._follower_out(hd)

    def _stage_eager_sampling(self, samp: SamplingRows, n: int, with_proc: bool):
        """An eager step's sampling rows (with_proc: and its processor rows) through the
        eager-sampling ring: async H2D -- a follower samples every asynchronous eager
        step, so no pageable copy or host sync on its step path. Returns the device views
        temperatures, top-p, top-k, seeds, pi [3, n], pf [4, n] (pi / pf: None without
        with_proc), ph [3, n] = history offset | length | update slot and the history token
        list (None unless the rows carry them)."""
        slot = self.es_ring.acquire(max(n, 64))
        hf, hk, hs = slot["f"], slot["k"], slot["s"]
        f = hf.numpy()
        f[:n] = samp.temps
        f[n:2 * n] = samp.top_ps
        hk.numpy()[:n] = samp.top_ks
        hs.numpy()[:n] = samp.seeds
        if with_proc:
            hpi, hpf = slot["pi"], slot["pf"]
            self._fill_proc_rows(hpi.numpy()[:3 * n].reshape(3, n), hpf.numpy()[:4 * n].reshape(4, n), samp, n, n)
        dev_f = hf[:2 * n].to(self.device, non_blocking=True).view(2, n)
        topk = hk[:n].to(self.device, non_blocking=True)
        seeds = hs[:n].to(self.device, non_blocking=True)
        d_pi = d_pf = d_ph = d_hl = None
        if with_proc:
            d_pi = hpi[:3 * n].to(self.device, non_blocking=True).view(3, n)
            d_pf = hpf[:4 * n].to(self.device, non_blocking=True).view(4, n)
            if samp.hist_pos is not None or samp.upd_slots is not None:
                # offset | length | update slot per row, and the step's token list
                nl = 0 if samp.hist_ids is None else len(samp.hist_ids)
                assert nl <= n * ops.LOGIT_HIST_MAX
                hph, hhl = slot["ph"], slot["hl"]
                ph = hph.numpy()[:3 * n].reshape(3, n)
                ph[:2] = 0
                if samp.hist_pos is not None:
                    ops.check_hist_pos(samp.hist_pos, nl, n)
                    ph[:2] = samp.hist_pos[:, :n]
                    hhl.numpy()[:nl] = samp.hist_ids
                ph[2] = samp.slots if samp.upd_slots is None else samp.upd_slots
                d_ph = hph[:3 * n].to(self.device, non_blocking=True).view(3, n)
                if samp.hist_pos is not None:
                    d_hl = hhl[:max(nl, 1)].to(self.device, non_blocking=True)[:nl]
        self.es_ring.fence()
        return dev_f[0], dev_f[1], topk, seeds, d_pi, d_pf, d_ph, d_hl

    def _sample(self, logits: torch.Tensor, samp: Optional[SamplingRows], h: StepHandle):
        """An eager step's sampling: (process_logits into an fp32 scratch ->) argmax or the
        sampler (-> logit_state_update), then the step's verify blocks and top-N rows."""
        greedy = samp is None or samp.all_greedy
        proc = samp is not None and samp.processed
        if greedy and not proc:
            tok, lp = ops.argmax_logprob(logits)
        else:
            n, V = logits.shape
            temps, top_ps, topk, seeds, d_pi, d_pf, d_ph, d_hl = self._stage_eager_sampling(samp, n, proc)
            if proc:
                hist = d_hl is not None
                logits = ops.process_logits(logits, ops.process_scratch(n, V, logits.device), self.p_state, d_pi, d_pf,
                                            temps, self.p_bias_ids, self.p_bias_vals, d_hl if hist else None,
                                            d_ph[:2].view(2, n) if hist else None)
            if greedy:
                tok, lp = ops.argmax_logprob(logits)
            else:
                gen = None if self.is_cuda else torch.Generator().manual_seed(int(samp.seeds[0]) & 0x7FFFFFFF)
                tok, lp = ops.sample_tokens(logits, temps, top_ps, topk, seeds, step=0, generator=gen)
            if proc and self.p_state is not None and self.proc_source is None:
                ops.logit_state_update(self.p_state, d_pi[0] if d_ph is None else d_ph[2], tok, n)
        if self.keep_sampler_logits:
            self.sampler_logits = logits
        if samp is not None and samp.spec is not None:
            self._spec_launch(logits, tok, lp, samp.spec, h)
        if samp is not None and samp.topn is not None:
            self._top_launch(logits, samp, h)
        return tok, lp

    def _log_samples(self, n: int) -> None:
        """(tests) the tokens of a step this rank sampled into g_out_tok -- the steps
        whose successor reads its decode ids from there on EVERY rank"""
        if self.sample_log is not None:
            self.sample_log.append(self.g_out_tok[:n].cpu().tolist())

    def _async_ok(self, S: int, plan: dict) -> bool:
        """May an eager step's successor be planned before its tokens reach the host?
        The same answer on every TP rank (it depends on the plan only)."""
        return not (not ASYNC_MIXED or not self.graphs or S > self.g_B or bool(plan["is_embed"].any())
                    or int(plan["num_sample"]) != S)
