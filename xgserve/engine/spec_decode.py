"""Speculative decoding (Req 12, requirements.md:160-170; tasks.md:340-354).

A small draft model (same vocabulary, e.g. Llama-3.2-1B for Llama-3-8B) runs on
the TP leader's GPU with its own paged KV cache and ModelRunner (HIP graphs for
its single-token steps). Each engine step:

  propose():  for every running greedy decode sequence, catch the draft's KV
              up to the sequence's tokens (one ragged step), then run k-1
              batched single-token draft steps -> k draft tokens, handed to the
              C++ scheduler (set_draft). The scheduler emits such a sequence as
              a verify row block of q_len = 1 + k.
  verify:     the target runs ONE forward over all rows (the prefill-attention
              kernel handles q_len > 1 against the paged context); the longest
              prefix of draft tokens matching the target's argmax is accepted,
              plus the target's own token at the first mismatch (so every verify
              yields >= 1 token and the output equals plain greedy decoding).

Speedup (Req 12.4, requirements.md:169) is measured, not assumed: the engine
times every step it runs with the draft (propose + verify) and every pure-decode
step without verify rows, and `stats()` reports
  speedup_factor = (tokens per sequence-step when speculating / spec step time)
                 / (1 token per sequence-step / plain decode step time)
from exponential moving averages of both (None until both kinds were seen).

Acceptance is tracked per request and globally; a request whose acceptance rate
stays below `min_acceptance_rate` (0.5, requirements.md:170) after a few
verifies stops speculating (its draft pages are freed).

Sampled requests (temperature > 0) are speculated only with `sampled=True`
(spec.sampled), those with top-p / top-k only with `truncated=True` on top of it
(spec.truncated): the draft DRAWS its tokens (its
sampler, stream 0 of the position's seed), the logits rows it drew from are kept
(the definition of q), and the verify step runs ops.spec_verify_sample over those
blocks after its sampler: draft token i is accepted with probability
min(1, p(d)/q(d)), the first rejected position emits a token of the residual
norm(max(0, p - q)), a fully accepted block a bonus token of p -- the output
follows the target's distribution whatever the draft says. With top-p / top-k the
draft draws with the request's own top_p / top_k and the verification runs on the
truncated, renormalised distributions of both models (the kept sets of the sampler),
so the output follows the truncated target distribution, which is what the plain
engine samples from. A fixed seed
reproduces on the same configuration but, unlike greedy, does not equal the
non-speculating engine's output. Otherwise sampled requests run as plain decodes
in the same batches.

Requests with logit processors (min_p, penalties, logit_bias) are speculated only with
`processors=True` (spec.processors). Row i of a verify block is processed as the
non-speculating engine would process it had the block's first i draft tokens been
emitted: its history is the slot's committed row of the state table plus those i tokens
(ops.process_logits with per-row extra history). The draft processes the rows it draws
from the same way -- the target's table, read-only, plus the tokens drafted so far this
round -- so it proposes what the processed target accepts. After the acceptance test the
block's emitted tokens are added to the table (ops.logit_state_add) before anything
reads it again. With the key on, the draft's kept rows are fp32 and a verify step with a
sampled block is run processed (plain rows with neutral parameters): the widening is
exact, so plain requests draw what they draw with the key off.

TP > 1: the draft lives only on the leader (TP=1 weights); followers execute the
verify plan broadcast with every other step.
"""
from __future__ import annotations

import logging
from dataclasses import dataclass
from typing import Dict, List, Optional

import numpy as np
import torch

from .request import RequestType
from .runner import ModelRunner, SamplingRows, SpecVerifyRows

log = logging.getLogger("xgserve.spec")

MIN_VERIFIES = 3
# sampled requests with min_p > 0: their processed rows hold -inf where min_p masked a
# token; speculated only if ops.spec_verify_sample agrees with its reference on such rows
# (tests/test_spec_proc_gpu.py), else they decode plainly, as top_p = 0 does
SAMPLED_MIN_P = True


@dataclass
class _DraftSeq:
    blocks: List[int]
    computed: int = 0        # draft KV valid for positions [0, computed)
    pending_L: int = -1      # len(tokens) at the last proposal (-1: none outstanding)
    pending_k: int = 0
    proposed: int = 0
    accepted: int = 0
    verifies: int = 0
    disabled: bool = False
    q_row0: int = -1         # sampled proposal of this round: first row of the kept draft logits
    slot: int = -1           # processed proposal of this round: the engine slot whose table row it read


class SpeculativeDecoder:
    def __init__(self, engine, draft_model: str, k: int, min_acceptance_rate: float = 0.5, sampled: bool = False,
                 truncated: bool = False, processors: bool = False):
        from ..models import build_model, get_config
        self.engine = engine
        self.k = int(k)
        self.min_acceptance_rate = min_acceptance_rate
        self.enabled = engine.is_driver
        self.sampled = bool(sampled)
        self.truncated = bool(truncated) and self.sampled  # top-p / top-k requests too
        self.proposed = 0
        self.accepted = 0
        self.sampled_proposed = 0   # the part of proposed / accepted that sampled blocks contributed
        self.sampled_accepted = 0
        self.truncated_proposed = 0  # the part of sampled_* that top-p / top-k blocks contributed
        self.truncated_accepted = 0
        self.processors = bool(processors)  # requests with logit processors too
        self.processed_proposed = 0  # the part of proposed / accepted that processed requests contributed
        self.processed_accepted = 0
        self.q_buf: Optional[torch.Tensor] = None  # [max_num_seqs * k, V] draft logits rows of sampled proposals
        self.verifies = 0
        self.seqs: Dict[int, _DraftSeq] = {}
        self.ema_spec_ms: Optional[float] = None   # step time with verify rows (propose + verify)
        self.ema_plain_ms: Optional[float] = None  # pure-decode step time without verify rows
        self.ema_tokens_per_row: Optional[float] = None  # tokens per speculated sequence-step
        if not self.enabled:
            return
        if isinstance(draft_model, str):
            dcfg = get_config(draft_model)
            self.model = build_model(dcfg, device=engine.device, dtype=engine.model.dtype, seed=engine.cfg.seed,
                                     tp=1, rank=0)
        else:  # a pre-built TP=1 model (tests, or a draft sharing memory with something else)
            self.model, dcfg = draft_model, draft_model.cfg
        if dcfg.vocab_size != engine.mcfg.vocab_size:
            raise ValueError(f"draft vocab {dcfg.vocab_size} != target vocab {engine.mcfg.vocab_size}")
        ec = engine.cfg
        if self.truncated:
            # a verify step may hold max_num_seqs truncated blocks of k draft tokens in one
            # ops.spec_verify_sample call: refuse here what that call would refuse mid-step
            from ..ops import sampling as _sp
            n = ec.max_num_seqs
            need = _sp.spec_ws_need(n * (self.k + 1), n * self.k, dcfg.vocab_size, n * (2 * self.k + 1))
            if need > _sp.SPEC_WS_CAP:
                raise ValueError(f"spec_truncated: max_num_seqs={n} with {self.k} speculative tokens needs {need} "
                                 f"bytes of verify workspace, more than the {_sp.SPEC_WS_CAP} one call may take; "
                                 f"lower max_num_seqs or num_speculative_tokens")
        bs = ec.block_size
        per_seq = (engine.max_model_len + bs - 1) // bs + 1
        nblocks = int(min(engine.num_blocks, ec.max_num_seqs * per_seq))
        self.bs = bs
        self.runner = ModelRunner(self.model, block_size=bs, num_blocks=nblocks, max_num_seqs=ec.max_num_seqs,
                                  max_num_batched_tokens=ec.max_num_batched_tokens, max_model_len=engine.max_model_len,
                                  use_graphs=ec.use_graphs, graph_batch_sizes=ec.graph_batch_sizes, is_driver=True)
        self.runner.keep_sampler_logits = self.sampled
        if self.processors:  # the draft reads the target's table and bias lists, never writes them
            self.runner.set_proc_source(engine.runner)
        self.runner.capture_graphs()
        self.free: List[int] = list(range(nblocks - 1, -1, -1))
        log.info("speculative decoding: draft=%s k=%d draft KV pages=%d", draft_model, self.k, nblocks)

    # ------------------------------------------------------------------ bookkeeping
    def _release(self, sid: int) -> None:
        ds = self.seqs.pop(sid, None)
        if ds is not None:
            self.free.extend(ds.blocks)

    def _ensure(self, ds: _DraftSeq, n_tokens: int) -> bool:
        need = (n_tokens + self.bs - 1) // self.bs - len(ds.blocks)
        if need > len(self.free):
            return False
        for _ in range(max(0, need)):
            ds.blocks.append(self.free.pop())
        return True

    EMA = 0.1

    def _ema(self, old: Optional[float], x: float) -> float:
        return x if old is None else (1 - self.EMA) * old + self.EMA * x

    def record_step(self, seconds: float, plan: dict, counts: Optional[np.ndarray]) -> None:
        """Engine hook: wall time of one step run with the draft attached."""
        ns, nd = int(plan["num_seqs"]), int(plan["num_decodes"])
        if ns == 0:
            return
        q, pre = plan["q_lens"], plan["is_prefill"]
        verify = (q > 1) & (pre == 0)
        if verify.any() and counts is not None:
            nrows = int(verify.sum())
            sidx = plan["sample_seq_index"]
            vtoks = int(sum(int(c) for j, c in enumerate(counts.tolist()) if verify[int(sidx[j])]))
            self.ema_spec_ms = self._ema(self.ema_spec_ms, 1000.0 * seconds)
            self.ema_tokens_per_row = self._ema(self.ema_tokens_per_row, vtoks / nrows)
        elif nd == ns:
            self.ema_plain_ms = self._ema(self.ema_plain_ms, 1000.0 * seconds)

    def speedup_factor(self) -> Optional[float]:
        if self.ema_spec_ms is None or self.ema_plain_ms is None or not self.ema_spec_ms:
            return None
        return self.ema_tokens_per_row * self.ema_plain_ms / self.ema_spec_ms

    def stats(self) -> dict:
        sf = self.speedup_factor()
        return {"draft_tokens_proposed": self.proposed, "draft_tokens_accepted": self.accepted,
                "acceptance_rate": self.accepted / self.proposed if self.proposed else 0.0,
                "sampled_draft_tokens_proposed": self.sampled_proposed,
                "sampled_draft_tokens_accepted": self.sampled_accepted,
                "truncated_draft_tokens_proposed": self.truncated_proposed,
                "truncated_draft_tokens_accepted": self.truncated_accepted,
                "processed_draft_tokens_proposed": self.processed_proposed,
                "processed_draft_tokens_accepted": self.processed_accepted,
                "verify_steps": self.verifies,
                "mean_tokens_per_verify": (self.accepted + self.verifies) / self.verifies if self.verifies else 0.0,
                "spec_step_ms": self.ema_spec_ms, "plain_decode_step_ms": self.ema_plain_ms,
                "speedup_factor": None if sf is None else round(sf, 4),
                "active": sum(1 for d in self.seqs.values() if not d.disabled)}

    def scratch_bytes(self) -> int:
        return 0 if self.q_buf is None else self.q_buf.numel() * self.q_buf.element_size()

    def _eligible_sampled(self, p) -> bool:
        if not (self.sampled and p.temperature > 0):
            return False
        if p.top_p >= 1.0 and p.top_k == 0:
            return True
        # top_p = 0, NaN or a negative value is served by the samplers (they keep the first
        # sub-bin) but is outside what the verify kernels take: such a request decodes plainly.
        # Decided on the float32 the kernels get: a positive double below 2^-150 is 0 there.
        with np.errstate(over="ignore"):
            return bool(self.truncated and np.float32(p.top_p) > 0 and p.top_k >= 0)

    def _is_truncated(self, top_p, top_k) -> bool:
        """What ops.spec_verify_sample treats as truncated: top_k >= V is off, as 0."""
        return bool(top_p < 1.0 or 0 < top_k < self.engine.mcfg.vocab_size)

    def _draft_samp(self, order, sampled: dict, step: int, proc: Optional[dict] = None,
                    drafts: Optional[dict] = None) -> Optional[SamplingRows]:
        """Sampling rows of a draft step, in its sample order: sampled sequences draw at
        their temperature, top_p and top_k from the seed of output token n + step, the
        engine's mix; greedy ones keep temperature 0. Processed sequences (proc: id(ds) ->
        engine slot) get their slot's parameters and, as extra history, the tokens drafted
        so far this round (drafts: id(ds) -> list). None: every row is greedy and plain."""
        from .engine import position_seeds
        has_proc = bool(proc) and any(id(ds) in proc for ds in order)
        if not has_proc and not any(id(ds) in sampled for ds in order):
            return None
        ns = len(order)
        temps, base, n = np.zeros(ns, np.float32), np.zeros(ns, np.uint64), np.zeros(ns, np.uint64)
        top_ps, top_ks = np.ones(ns, np.float32), np.zeros(ns, np.int32)
        for i, ds in enumerate(order):
            e = sampled.get(id(ds))
            if e is not None:
                temps[i], base[i], n[i], top_ps[i], top_ks[i] = e[1], e[2], e[3] + step, e[4], e[5]
        rows = SamplingRows(temps, top_ps, top_ks, position_seeds(base, n))
        if has_proc:
            eng = self.engine
            rows.slots, rows.bias_lens = np.full(ns, -1, np.int32), np.zeros(ns, np.int32)
            rows.pens = np.zeros((4, ns), np.float32)
            rows.pens[0], rows.pens[3] = 1.0, -np.inf
            hist, pos = [], np.zeros((2, ns), np.int32)
            for i, ds in enumerate(order):
                s = proc.get(id(ds))
                if s is None:
                    continue
                rows.slots[i], rows.bias_lens[i], rows.pens[:, i] = eng.slot_track[s], eng.slot_blen[s], eng.slot_pen[:, s]
                d = drafts.get(id(ds)) if drafts else None
                if d and eng.slot_track[s] >= 0:
                    pos[0, i], pos[1, i] = len(hist), len(d)
                    hist.extend(d)
            if hist:
                rows.hist_ids, rows.hist_pos = np.asarray(hist, np.int32), pos
        return rows

    def _keep_q(self, order, sampled: dict, step: int) -> None:
        """Copy the logits rows the draft sampler just read for the sampled sequences
        into their rows of q_buf (row q_row0 + step): with sample_tokens, the definition
        of q -- the verify kernel recomputes y_q from exactly these rows."""
        src = [i for i, ds in enumerate(order) if id(ds) in sampled]
        if not src:
            return
        logits = self.runner.last_sampler_logits()
        # with processors the kept rows are fp32, as processed rows are: a step's p and q
        # rows must be of one dtype (plain bf16 rows are widened here, which is exact)
        dt = torch.float32 if self.processors else logits.dtype
        if self.q_buf is None:  # lazily, at the first sampled proposal
            self.q_buf = torch.zeros(self.engine.cfg.max_num_seqs * self.k, logits.shape[1], dtype=dt,
                                     device=logits.device)
        dst = [sampled[id(order[i])][0] + step for i in src]
        dev = logits.device
        self.q_buf.index_copy_(0, torch.tensor(dst, dtype=torch.long, device=dev),
                               logits.index_select(0, torch.tensor(src, dtype=torch.long, device=dev)).to(dt))

    # ------------------------------------------------------------------ draft steps
    def _plan(self, rows) -> dict:
        """rows: (ds, tokens_slice, start_pos, want_logits) -> a runner plan dict
        (decodes first, as the runner expects)."""
        rows = sorted(rows, key=lambda r: len(r[1]) != 1)
        ns = len(rows)
        w = max(1, max(len(r[0].blocks) for r in rows))
        ids, pos, slot, ql, sl, qsl, li, bt = [], [], [], [], [], [0], [], np.zeros((ns, w), np.int32)
        nd = sum(1 for r in rows if len(r[1]) == 1)  # single-token rows lead (sorted above)
        for i, (ds, toks, p0, _) in enumerate(rows):
            q = len(toks)
            for t in range(q):
                p = p0 + t
                ids.append(toks[t])
                pos.append(p)
                slot.append(ds.blocks[p // self.bs] * self.bs + p % self.bs)
            ql.append(q)
            sl.append(p0 + q)
            bt[i, :len(ds.blocks)] = ds.blocks
            if rows[i][3]:
                li.append(qsl[-1] + q - 1)
            qsl.append(qsl[-1] + q)
        i32 = lambda a: np.asarray(a, np.int32)  # noqa: E731
        return {"num_seqs": ns, "num_decodes": nd, "num_tokens": len(ids), "num_sample": len(li),
                "max_q_len": max(ql), "bt_width": w, "input_ids": i32(ids), "positions": i32(pos),
                "slot_mapping": i32(slot), "q_lens": i32(ql), "seq_lens": i32(sl), "query_start_loc": i32(qsl),
                "block_tables": bt.reshape(-1), "logits_indices": i32(li), "is_embed": np.zeros(ns, np.uint8),
                "order": rows}

    def propose(self) -> None:
        """Called by the engine (under its lock) right before scheduling."""
        if not self.enabled or self.k <= 0:
            return
        eng = self.engine
        live = set(eng.by_seq)
        for sid in [s for s in self.seqs if s not in live]:
            self._release(sid)
        budget = self.runner.max_tokens
        rows, ready = [], []
        for sid, ds in self.seqs.items():
            ds.slot = -1
            if ds.q_row0 >= 0:
                # a sampled proposal the scheduler has not verified: its q rows are about to be
                # reused, so the draft is withdrawn (re-proposed below if still eligible)
                ds.q_row0 = -1
                eng.sched.set_draft(sid, [])
        for sid, req in eng.by_seq.items():
            if req.finished or req.kind == RequestType.Embeddings or not req.output_ids:
                continue
            if sid not in eng.last_plan_seqs:
                # not running (pre-empted, waiting to be resumed): a draft set now would ride
                # its recompute step, which is a prompt row and verifies nothing
                continue
            p = req.params
            if (p.temperature > 0 and not self._eligible_sampled(p)) or len(req.output_ids) + 1 >= p.max_tokens:
                continue
            slot = -1
            if not p.plain:
                # a processed proposal reads the slot's row of the target's table: the slot must
                # be bound to this sequence, and its row current (a pending reset: stale until
                # the next processed target step)
                slot = eng.seq_slot.get(sid, -1)
                if not self.processors or slot < 0 or eng.slot_owner[slot] != sid or slot in eng._resets:
                    continue
                if p.temperature > 0 and p.min_p > 0 and not SAMPLED_MIN_P:
                    continue
            ds = self.seqs.get(sid)
            if ds is None:
                ds = self.seqs[sid] = _DraftSeq(blocks=[])
            ds.slot = slot
            if ds.disabled:
                continue
            if ds.pending_L >= 0:  # last proposal was never verified: trust only the real tokens
                ds.computed = min(ds.computed, ds.pending_L)
                ds.pending_L = -1
            toks = req.prompt_ids + req.output_ids
            L = len(toks)
            if L + self.k > eng.max_model_len:
                continue
            if not self._ensure(ds, L + self.k):  # draft KV pool exhausted: plain decoding for this one
                self.free.extend(ds.blocks)
                ds.blocks = []
                ds.disabled = True
                continue
            new = toks[ds.computed:]
            if not new:  # cannot happen (the last token is never in the draft KV) -- be safe
                ds.computed = L - 1
                new = toks[-1:]
            if budget <= 0:
                break
            take = min(len(new), budget)
            budget -= take
            done = take == len(new)
            rows.append((ds, new[:take], ds.computed, done))
            ds.computed += take
            if done:
                ready.append((sid, ds, L))
        if not rows:
            return
        # sampled sequences of this round: id(ds) -> (first q_buf row, temperature, seed, n, top_p, top_k)
        sampled = {}
        for sid, ds, _ in ready:
            req = eng.by_seq[sid]
            if req.params.temperature > 0:
                sampled[id(ds)] = (len(sampled) * self.k, req.params.temperature, req.params.seed & ((1 << 63) - 1),
                                   len(req.output_ids), req.params.top_p, req.params.top_k)
        proc = {id(ds): ds.slot for _, ds, _ in ready if ds.slot >= 0}
        plan = self._plan(rows)
        order = [r[0] for r in plan["order"] if r[3]]
        toks, _, _ = self.runner.execute(plan, self._draft_samp(order, sampled, 0, proc))
        if not ready:
            return
        self._keep_q(order, sampled, 0)
        first = {id(ds): int(t) for ds, t in zip(order, toks)}
        drafts = {sid: [first[id(ds)]] for sid, ds, _ in ready}
        for step in range(1, self.k):
            drows = [(ds, [drafts[sid][-1]], L + step - 1, True) for sid, ds, L in ready]
            dplan = self._plan(drows)
            dorder = [r[0] for r in dplan["order"]]
            so_far = {id(ds): drafts[sid] for sid, ds, _ in ready if ds.slot >= 0}
            t2, _, _ = self.runner.execute(dplan, self._draft_samp(dorder, sampled, step, proc, so_far))
            self._keep_q(dorder, sampled, step)
            by_ds = {id(r[0]): int(t) for r, t in zip(dplan["order"], t2)}
            for sid, ds, _ in ready:
                drafts[sid].append(by_ds[id(ds)])
        for sid, ds, L in ready:
            ds.computed = L + self.k - 1
            ds.pending_L, ds.pending_k = L, self.k
            e = sampled.get(id(ds))
            ds.q_row0 = -1 if e is None else e[0]
            eng.sched.set_draft(sid, drafts[sid])

    # ------------------------------------------------------------------ verify
    def verify_execute(self, plan: dict, samp: Optional[SamplingRows]):
        """Run the target over a plan that may contain verify row blocks. Returns
        (accepted tokens concatenated per sampled sequence, logprobs, hidden, counts)."""
        sidx = plan["sample_seq_index"]
        q_lens, is_pre = plan["q_lens"], plan["is_prefill"]
        nrows = np.array([int(q_lens[s]) if (not is_pre[s] and q_lens[s] > 1) else 1 for s in sidx.tolist()],
                         dtype=np.int64)
        rsamp = None
        qsl, ids, seq_ids = plan["query_start_loc"], plan["input_ids"], plan["seq_ids"]
        sblock = {}  # index j of a sampled verify block -> its index among the step's sampled blocks
        if samp is not None:
            seeds = np.repeat(samp.seeds, nrows)
            if self.sampled and self.q_buf is not None:
                sv = self._sampled_blocks(plan, samp, nrows, seeds, sblock)
            else:
                sv = None
            rsamp = SamplingRows(np.repeat(samp.temps, nrows), np.repeat(samp.top_ps, nrows),
                                 np.repeat(samp.top_ks, nrows), seeds, spec=sv)
            if samp.topn is not None:
                rsamp.topn = np.repeat(samp.topn, nrows)
            if samp.processed or (self.processors and sv is not None):
                # (a step with a sampled block is run processed, plain rows neutral: its kept
                # q rows are fp32, and p and q must be of one dtype)
                self._processed_rows(plan, samp, rsamp, nrows)
        toks, lps, hidden = self.engine.runner.execute(plan, rsamp)
        if toks is None:
            return None, None, hidden, None
        acc = self.engine.runner.spec_result  # accepted[b] of the sampled blocks, same D2H and event as toks
        out_t, out_l, counts = [], [], []
        tops = self.engine.runner.top_result  # per verify row; sliced to the accepted positions as lps
        c_slots, c_toks = [], []  # (slot, token) of every token a tracked verify block emitted
        out_top = [] if tops is not None else None
        k = 0
        for j, s in enumerate(sidx.tolist()):
            n_r = int(nrows[j])
            if n_r == 1:
                out_t.append(int(toks[k]))
                out_l.append(float(lps[k]))
                counts.append(1)
                if tops is not None:
                    out_top.append(tops[k])
                k += 1
                continue
            draft = ids[int(qsl[s]) + 1:int(qsl[s]) + n_r]
            t = toks[k:k + n_r]
            n = 0
            sampled = samp is not None and samp.temps[j] > 0
            if j in sblock:
                # rejection sampling ran on the device: rows [0, n] hold the accepted draft
                # tokens and the residual / bonus token
                n = int(acc[sblock[j]])
            elif not sampled:
                while n < n_r - 1 and int(draft[n]) == int(t[n]):
                    n += 1
            # (a sampled block without kept draft logits takes the target's own draw of row 0)
            out_t.extend(int(x) for x in t[:n + 1])  # accepted drafts == target tokens, + the bonus token
            out_l.extend(float(x) for x in lps[k:k + n + 1])
            counts.append(n + 1)
            if tops is not None:
                out_top.extend(tops[k:k + n + 1])
            k += n_r
            self._account(int(seq_ids[s]), n_r - 1, n, sampled,
                          j in sblock and self._is_truncated(samp.top_ps[j], samp.top_ks[j]))
            if samp is not None and samp.slots is not None and samp.slots[j] >= 0:
                c_slots.extend([int(samp.slots[j])] * (n + 1))
                c_toks.extend(int(x) for x in t[:n + 1])
        if c_slots:
            # the blocks' emitted tokens become history before the next proposal or step
            self.engine.runner.commit_tokens(np.asarray(c_slots, np.int32), np.asarray(c_toks, np.int32))
        plan["_top"] = out_top
        return (np.asarray(out_t, np.int32), np.asarray(out_l, np.float32), hidden, np.asarray(counts, np.int32))

    def _processed_rows(self, plan: dict, samp: SamplingRows, rsamp: SamplingRows, nrows: np.ndarray) -> None:
        """Processor parameters of the repeated rows: every row of a block gets its
        sequence's slot, bias list and penalties; row i of a tracked block the block's first
        i draft tokens as extra history (one staged list: the blocks' drafts, concatenated).
        The in-step table update is left to single rows (q_len 1, prompts): a block's
        emitted tokens are committed after the acceptance test."""
        ns = len(nrows)
        if samp.processed:
            slots, blens, pens = samp.slots, samp.bias_lens, samp.pens
        else:
            slots, blens = np.full(ns, -1, np.int32), np.zeros(ns, np.int32)
            pens = np.zeros((4, ns), np.float32)
            pens[0], pens[3] = 1.0, -np.inf
        rsamp.slots, rsamp.bias_lens = np.repeat(slots, nrows), np.repeat(blens, nrows)
        rsamp.pens = np.repeat(pens, nrows, axis=1)
        rsamp.resets = samp.resets
        rsamp.upd_slots = np.repeat(np.where(nrows == 1, slots, -1).astype(np.int32), nrows)
        sidx, qsl, ids = plan["sample_seq_index"], plan["query_start_loc"], plan["input_ids"]
        hist, pos, r = [], np.zeros((2, int(nrows.sum())), np.int32), 0
        for j, s in enumerate(sidx.tolist()):
            n_r = int(nrows[j])
            if n_r > 1 and slots[j] >= 0:
                pos[0, r:r + n_r], pos[1, r:r + n_r] = len(hist), np.arange(n_r)
                hist.extend(int(x) for x in ids[int(qsl[s]) + 1:int(qsl[s]) + n_r])
            r += n_r
        if hist:
            rsamp.hist_ids, rsamp.hist_pos = np.asarray(hist, np.int32), pos

    def _sampled_blocks(self, plan: dict, samp: SamplingRows, nrows: np.ndarray, seeds: np.ndarray,
                        sblock: dict) -> Optional[SpecVerifyRows]:
        """The step's sampled verify blocks (proposed this round, their q rows kept):
        fills their per-position seeds (output tokens n .. n + k of the request) into
        `seeds` and their order into `sblock`."""
        from .engine import position_seeds
        sidx, seq_ids, qsl, ids = plan["sample_seq_index"], plan["seq_ids"], plan["query_start_loc"], plan["input_ids"]
        row0 = np.concatenate([[0], np.cumsum(nrows)[:-1]])
        p0, q0, ks, temps, pseeds, draft, top_ps, top_ks = [], [], [], [], [], [], [], []
        for j, s in enumerate(sidx.tolist()):
            n_r = int(nrows[j])
            if n_r == 1 or not samp.temps[j] > 0:
                continue
            sid = int(seq_ids[s])
            ds, req = self.seqs.get(sid), self.engine.by_seq.get(sid)
            if ds is None or req is None or ds.q_row0 < 0 or n_r - 1 > self.k:
                continue
            if not (samp.top_ps[j] > 0 and samp.top_ks[j] >= 0):
                continue  # never proposed (_eligible_sampled); the op would refuse the whole call
            r0 = int(row0[j])
            ps = position_seeds(np.full(n_r, req.params.seed & ((1 << 63) - 1), np.uint64),
                                len(req.output_ids) + np.arange(n_r, dtype=np.uint64))
            seeds[r0:r0 + n_r] = ps
            sblock[j] = len(ks)
            p0.append(r0)
            q0.append(ds.q_row0)
            ks.append(n_r - 1)
            temps.append(samp.temps[j])
            top_ps.append(min(float(samp.top_ps[j]), 1.0))  # above 1 is off, as 1
            top_ks.append(samp.top_ks[j])
            pseeds.append(ps)
            draft.append(ids[int(qsl[s]) + 1:int(qsl[s]) + n_r])
        if not ks:
            return None
        top_ps, top_ks = np.asarray(top_ps, np.float32), np.asarray(top_ks, np.int32)
        if not any(self._is_truncated(a, b) for a, b in zip(top_ps, top_ks)):  # the call of before
            top_ps = top_ks = None
        return SpecVerifyRows(np.asarray(p0, np.int64), np.asarray(q0, np.int64), np.asarray(ks, np.int64),
                              np.asarray(temps, np.float32), np.concatenate(pseeds),
                              np.concatenate(draft).astype(np.int32), self.q_buf, top_ps, top_ks)

    def _account(self, sid: int, proposed: int, accepted: int, sampled: bool = False,
                 truncated: bool = False) -> None:
        self.proposed += proposed
        self.accepted += accepted
        self.verifies += 1
        if sampled:
            self.sampled_proposed += proposed
            self.sampled_accepted += accepted
        if truncated:
            self.truncated_proposed += proposed
            self.truncated_accepted += accepted
        req = self.engine.by_seq.get(sid)
        if req is not None and not req.params.plain:
            self.processed_proposed += proposed
            self.processed_accepted += accepted
        ds = self.seqs.get(sid)
        if ds is None:
            return
        ds.q_row0 = -1  # verified: the q rows are free again
        if ds.pending_L >= 0:
            ds.computed = ds.pending_L + min(accepted, ds.pending_k - 1)
            ds.pending_L = -1
        ds.proposed += proposed
        ds.accepted += accepted
        ds.verifies += 1
        if ds.verifies >= MIN_VERIFIES and ds.accepted < self.min_acceptance_rate * ds.proposed:
            log.debug("seq %d: acceptance %.2f < %.2f, speculation disabled", sid, ds.accepted / ds.proposed,
                      self.min_acceptance_rate)
            self.free.extend(ds.blocks)
            ds.blocks = []
            ds.disabled = True
