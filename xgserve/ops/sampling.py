"""K9 sampling + K11 pooling helpers."""
from __future__ import annotations

import math
from typing import Optional, Tuple

import torch

from ._native import kernels, stream_ptr, use_native, ptr


def argmax_logprob_ref(logits: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    lf = logits.float()
    tok = lf.argmax(-1)
    lp = torch.log_softmax(lf, -1).gather(-1, tok[:, None])[:, 0]
    return tok.to(torch.int32), lp


_ARGMAX_WS = {}
_ARGMAX_WS_RETIRED = []
# below this a row is one workgroup's work anyway; XGS_TUNE argmax_split=0: always the
# one-workgroup-per-row kernel (A/B)
ARGMAX_SPLIT_MIN_V = 16384 if __import__("xgserve.tune", fromlist=["get_bool"]).get_bool("argmax_split", True) else 1 << 62


def _argmax_ws(device, B: int):
    """Split-row argmax scratch: per-slice partials and zeroed per-row tickets (every
    launch's last arriver re-arms its row), grown on demand, kept alive for captured graphs."""
    key = str(device)
    ws = _ARGMAX_WS.get(key)
    if ws is None or ws[1].numel() < B:
        if ws is not None:
            _ARGMAX_WS_RETIRED.append(ws)
        n = max(B, 64)
        ws = _ARGMAX_WS[key] = (torch.empty(n * kernels().argmax_ws_floats_per_row(), dtype=torch.float32,
                                            device=device),
                                torch.zeros(n, dtype=torch.int32, device=device))
    return ws


def argmax_logprob(logits: torch.Tensor, out_tok: Optional[torch.Tensor] = None,
                   out_lp: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """Greedy token + its log-probability per row of a [B, V] logits matrix. Large
    vocabularies take the split-row kernel (8 workgroups per row, last arriver merges)."""
    if not use_native(logits):
        t, lp = argmax_logprob_ref(logits)
        return t, lp
    B, V = logits.shape
    assert logits.stride(1) == 1
    if out_tok is None:
        out_tok = torch.empty(B, dtype=torch.int32, device=logits.device)
    if out_lp is None:
        out_lp = torch.empty(B, dtype=torch.float32, device=logits.device)
    ws = cnt = 0
    if V >= ARGMAX_SPLIT_MIN_V:
        w, c = _argmax_ws(logits.device, B)
        ws, cnt = w.data_ptr(), c.data_ptr()
    kernels().argmax_logprob(logits.data_ptr(), 1 if logits.dtype == torch.float32 else 0, logits.stride(0), B, V,
                             out_tok.data_ptr(), out_lp.data_ptr(), stream_ptr(), ws, cnt)
    return out_tok, out_lp


def _kept_mask(x: torch.Tensor, logp: torch.Tensor, top_p: float, top_k: int) -> torch.Tensor:
    """The CPU sampler's exact kept set of one row (x = logits / T, logp its log-softmax):
    top-k keeps x >= the k-th value, top-p the smallest prefix by sorted probability."""
    V = x.shape[0]
    keep = torch.ones(V, dtype=torch.bool, device=x.device)
    if 0 < top_k < V:
        kth = torch.topk(x, top_k).values[-1]
        keep &= x >= kth
    if top_p < 1.0:
        sp, si = torch.sort(logp.exp(), descending=True)
        c = torch.cumsum(sp, 0)
        n = int((c < top_p).sum()) + 1
        m = torch.zeros(V, dtype=torch.bool, device=x.device)
        m[si[:n]] = True
        keep &= m
    return keep


def _sample_ref(logits, temps, top_ps, top_ks, gen: Optional[torch.Generator]):
    lf = logits.float()
    B, V = lf.shape
    toks = torch.empty(B, dtype=torch.int32, device=lf.device)
    lps = torch.empty(B, dtype=torch.float32, device=lf.device)
    for i in range(B):
        t = float(temps[i])
        if t <= 0:
            toks[i] = int(lf[i].argmax())
            lps[i] = torch.log_softmax(lf[i], -1)[toks[i]]
            continue
        x = lf[i] / t
        logp = torch.log_softmax(x, -1)
        keep = _kept_mask(x, logp, float(top_ps[i]) if top_ps is not None else 1.0,
                          int(top_ks[i]) if top_ks is not None else 0)
        probs = torch.where(keep, logp.exp(), torch.zeros_like(logp))
        j = int(torch.multinomial(probs / probs.sum(), 1, generator=gen))
        toks[i] = j
        lps[i] = logp[j]
    return toks, lps


def sample_tokens(logits: torch.Tensor, temps: torch.Tensor, top_ps: Optional[torch.Tensor] = None,
                  top_ks: Optional[torch.Tensor] = None, seeds: Optional[torch.Tensor] = None, step: int = 0,
                  generator: Optional[torch.Generator] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """Per-row temperature / top-k / top-p sampling (temps <= 0 -> greedy)."""
    if not use_native(logits):
        return _sample_ref(logits, temps, top_ps, top_ks, generator)
    B, V = logits.shape
    tok = torch.empty(B, dtype=torch.int32, device=logits.device)
    lp = torch.empty(B, dtype=torch.float32, device=logits.device)
    ws = _sample_workspace(logits.device, B) if SAMPLE_SPLIT else None
    kernels().sample_tokens(logits.data_ptr(), 1 if logits.dtype == torch.float32 else 0, logits.stride(0), B, V,
                            temps.data_ptr(), ptr(top_ps), ptr(top_ks), ptr(seeds), int(step) & ((1 << 64) - 1),
                            tok.data_ptr(), lp.data_ptr(), stream_ptr(), ptr(ws),
                            0 if ws is None else ws.shape[0])
    return tok, lp


# ---------------------------------------------------------------------------
# Top-K alternatives (csrc/kernels/top_logprobs.hip)
# ---------------------------------------------------------------------------
TOPLP_MAX = 20
_TOPLP_WS = {}


def _toplp_ws(device, n: int):
    """Split-row scratch of top_logprobs: per-slice winners and zeroed per-row tickets
    (re-armed by every launch), grown on demand; earlier ones stay alive for captured graphs."""
    wss = _TOPLP_WS.setdefault((device.type, device.index), [])
    if not wss or wss[-1][1].numel() < n:
        m = max(n, 64)
        wss.append((torch.empty(m * kernels().top_logprobs_ws_words(), dtype=torch.int64, device=device),
                    torch.zeros(m, dtype=torch.int32, device=device)))
    return wss[-1]


def top_logprobs_ref(logits: torch.Tensor, temps: torch.Tensor, k: int, rows: Optional[torch.Tensor] = None):
    """numpy: y = fp32(x * fp32(1 / T)) (x on a greedy row), lp = y - logZ over the whole
    row (float64), ordered by y descending, then token id; -inf logits are not listed
    (id -1, lp -inf in the slots left over)."""
    import numpy as np
    lf = logits.detach().float().cpu().numpy()
    tn = temps.detach().float().cpu().numpy()
    ridx = np.arange(lf.shape[0]) if rows is None else rows.detach().cpu().numpy().astype(np.int64)
    n = len(ridx)
    ids = np.full((n, k), -1, np.int32)
    lps = np.full((n, k), -np.inf, np.float32)
    with np.errstate(all="ignore"):
        for o, r in enumerate(ridx):
            t = np.float32(tn[r])
            y = (lf[r] * (np.float32(1) / t)).astype(np.float32) if t > 0 else lf[r]
            fin = y > -np.inf
            if not fin.any():
                continue
            y64 = y.astype(np.float64)
            m = y64[fin].max()
            logz = m + np.log(np.exp(y64[fin] - m).sum())
            order = np.argsort(-y, kind="stable")[:k]
            order = order[fin[order]]
            ids[o, :len(order)] = order
            lps[o, :len(order)] = (y64[order] - logz).astype(np.float32)
    return torch.from_numpy(ids), torch.from_numpy(lps)


def top_logprobs(logits: torch.Tensor, temps: torch.Tensor, k: int, rows: Optional[torch.Tensor] = None,
                 out_ids: Optional[torch.Tensor] = None, out_lps: Optional[torch.Tensor] = None):
    """The k (1..TOPLP_MAX) most likely tokens of the asked rows of a [R, V] logits matrix
    and their log-probabilities under the temperature-scaled distribution of the whole row
    (the one the samplers' logprob refers to; temps <= 0: the raw logits). rows: int32
    indices of the logits rows that asked (None: all, in order); temps: fp32 indexed by
    logits row. Returns (ids int32 [n, k], lps fp32 [n, k]), best first, equal values to
    the lower id; id -1 / lp -inf past the last finite entry."""
    if not 1 <= k <= TOPLP_MAX:
        raise ValueError(f"top_logprobs: k must be in [1, {TOPLP_MAX}]")
    R, V = logits.shape
    n = R if rows is None else rows.numel()
    if not use_native(logits):
        ids, lps = top_logprobs_ref(logits, temps, k, rows)
        if out_ids is not None:
            out_ids[:n, :k].copy_(ids)
            out_lps[:n, :k].copy_(lps)
        return ids, lps
    assert logits.stride(1) == 1 and logits.dtype in (torch.bfloat16, torch.float32)
    assert temps.dtype == torch.float32 and temps.is_contiguous() and temps.numel() >= R
    assert rows is None or (rows.dtype == torch.int32 and rows.is_contiguous())
    if out_ids is None:
        out_ids = torch.empty(n, k, dtype=torch.int32, device=logits.device)
        out_lps = torch.empty(n, k, dtype=torch.float32, device=logits.device)
    else:  # the first n * k elements of the caller's buffers, as [n, k]
        assert out_ids.dtype == torch.int32 and out_lps.dtype == torch.float32
        assert out_ids.is_contiguous() and out_lps.is_contiguous() and min(out_ids.numel(), out_lps.numel()) >= n * k
        out_ids = out_ids.view(-1)[:n * k].view(n, k)
        out_lps = out_lps.view(-1)[:n * k].view(n, k)
    if n == 0:
        return out_ids, out_lps
    ws = tk = wrows = 0
    if V >= ARGMAX_SPLIT_MIN_V:
        w, t = _toplp_ws(logits.device, n)
        ws, tk, wrows = w.data_ptr(), t.data_ptr(), t.numel()
    kernels().top_logprobs(logits.data_ptr(), 1 if logits.dtype == torch.float32 else 0, logits.stride(0), R, V,
                           ptr(rows), n, temps.data_ptr(), k, out_ids.data_ptr(), out_lps.data_ptr(), stream_ptr(),
                           ws, tk, wrows)
    return out_ids, out_lps


# Split-row sampler (csrc/kernels/sampling.hip "sample v2": several workgroups per row,
# histogram thresholds instead of a 24-pass bisection); False selects the
# one-workgroup-per-row kernel (the tests' cross-check; A/B in profiles/r2_sampling.md).
SAMPLE_SPLIT = True
_SAMPLE_WS = {}


def _sample_workspace(device, B: int) -> torch.Tensor:
    """Per-device zeroed scratch of the split-row sampler, one row per batch row; the
    kernels leave it zero after every call (ticket winners re-zero what they used), so
    one allocation serves eager calls and captured graphs. Grown (never shrunk, never
    freed) to the largest batch seen."""
    key = (device.type, device.index)
    wss = _SAMPLE_WS.setdefault(key, [])
    if not wss or wss[-1].shape[0] < B:
        row = kernels().sample_ws_row_bytes()
        # earlier (smaller) workspaces stay alive: captured graphs may still use them
        wss.append(torch.zeros(max(B, 256), row // 8, dtype=torch.int64, device=device))
    return wss[-1]


# ---------------------------------------------------------------------------
# Speculative sampling (csrc/kernels/spec_sample.hip): rejection-sampling verification
# of sampled verify blocks. The contract (streams, accept test, residual and bonus draws)
# is written at the head of that file; the CPU path below implements it in float64 with
# the same counter hash, so a seed gives the same tokens wherever float rounding does not
# decide.
# ---------------------------------------------------------------------------
_SPEC_WS = {}
_M32 = 0xFFFFFFFF
# Scratch per logical row of a truncated block (spec::TRow: two 1024-bin histogram levels of
# u64 mass and u32 counts) and the most one call's workspace may take. 256 MiB holds about
# 10 900 truncated rows (3 600 blocks of k = 1; 1 500 of k = 3) -- many times a step's worth
# at max_num_seqs = 256 -- and keeps a mistaken huge call from taking the KV cache's memory.
SPEC_TROW = 24624
SPEC_WS_CAP = 256 << 20


def spec_ws_need(Lp: int, Lq: int, V: int, n_trunc: int) -> int:
    """Workspace bytes of a call (spec_ws_bytes of the native library, in Python so that
    the cap also guards the CPU path): chunk partials, and per truncated row SPEC_TROW plus
    one float per chunk."""
    P = max(1, min(64, (512 + Lp - 1) // max(1, Lp)))
    P = max(1, min(P, (V + 2047) // 2048))
    base = Lp * P * 32 + (Lp + Lq) * P * 8 + Lp * 8
    if n_trunc <= 0:
        return base
    return ((base + 15) & ~15) + Lp * 16 + n_trunc * SPEC_TROW + n_trunc * P * 4


def _hash32i(x: int) -> int:
    x &= _M32
    x ^= x >> 16
    x = (x * 0x7FEB352D) & _M32
    x ^= x >> 15
    x = (x * 0x846CA68B) & _M32
    return x ^ (x >> 16)


def _hash32v(x):
    import numpy as np
    m = np.uint64(_M32)
    x = x & m
    x = x ^ (x >> np.uint64(16))
    x = (x * np.uint64(0x7FEB352D)) & m
    x = x ^ (x >> np.uint64(15))
    x = (x * np.uint64(0x846CA68B)) & m
    return x ^ (x >> np.uint64(16))


def _stream_key(seed: int, step: int) -> int:
    seed &= (1 << 64) - 1
    return _hash32i((seed & _M32) ^ _hash32i((seed >> 32) + 0x85EBCA6B)
                    ^ _hash32i((step & _M32) * 0x27D4EB2F + 0x165667B1))


def _gumbel_row(key: int, V: int):
    """g(x) = -log(-log u(x)), u = ((hash >> 9) + 0.5) / 2^23, for x in [0, V)."""
    import numpy as np
    i = np.arange(V, dtype=np.uint64)
    h = _hash32v(np.uint64(key) ^ _hash32v((i * np.uint64(0x9E3779B9)) & np.uint64(_M32)))
    u = ((h >> np.uint64(9)).astype(np.float64) + 0.5) / 8388608.0
    return -np.log(-np.log(u))


def _spec_blocks(p_rows, q_rows, n_draft, n_out, V, p_row0, q_row0, d_off, ks, temps, out_row0):
    """Checked int64 / float32 block arrays + (lrow0, Lp, Lq); ValueError on anything the
    kernels would index out of range."""
    import numpy as np
    ks = np.asarray(ks, np.int64).reshape(-1)
    nb = ks.shape[0]
    p_row0, q_row0, d_off = (np.asarray(a, np.int64).reshape(-1) for a in (p_row0, q_row0, d_off))
    temps = np.asarray(temps, np.float32).reshape(-1)
    if V <= 0:
        raise ValueError("spec_verify_sample: V must be positive")
    if not (p_row0.shape[0] == q_row0.shape[0] == d_off.shape[0] == temps.shape[0] == nb):
        raise ValueError("spec_verify_sample: per-block arrays differ in length")
    if nb and ks.min() < 1:
        raise ValueError("spec_verify_sample: a block has k < 1")
    lrow0 = np.concatenate([[0], np.cumsum(ks + 1)[:-1]]) if nb else np.zeros(0, np.int64)
    out_row0 = lrow0 if out_row0 is None else np.asarray(out_row0, np.int64).reshape(-1)
    Lp, Lq = int((ks + 1).sum()), int(ks.sum())
    if nb:
        if Lp > 65535:
            raise ValueError("spec_verify_sample: more than 65535 target rows")
        if not (np.isfinite(temps).all() and (temps > 0).all()):
            raise ValueError("spec_verify_sample: temperatures must be positive and finite")
        if p_row0.min() < 0 or (p_row0 + ks + 1).max() > p_rows or q_row0.min() < 0 or (q_row0 + ks).max() > q_rows:
            raise ValueError("spec_verify_sample: a block leaves the logits rows")
        if d_off.min() < 0 or (d_off + ks).max() > n_draft:
            raise ValueError("spec_verify_sample: a block leaves the draft tokens")
        if out_row0.shape[0] != nb or out_row0.min() < 0 or (out_row0 + ks + 1).max() > n_out:
            raise ValueError("spec_verify_sample: a block leaves the output rows")
    return p_row0, q_row0, d_off, ks, temps, lrow0, out_row0, Lp, Lq


def _spec_verify_ref(p_logits, q_logits, draft, p_row0, q_row0, d_off, ks, temps, lrow0, out_row0, seeds, out_tok,
                     out_lp, accepted, top_ps=None, top_ks=None) -> None:
    import numpy as np
    P = p_logits.detach().float().cpu().numpy()
    Q = q_logits.detach().float().cpu().numpy()
    V = P.shape[1]
    rows = {}
    kept = {}

    def trunc(which, r, t, tp, tk, y):
        """(kept mask, log of the kept mass) of a truncated row: the kept set is exactly what
        _sample_ref keeps for this row (the CPU draft sampler drew from it)."""
        key = (which, r, t.tobytes(), tp, tk)
        v = kept.get(key)
        if v is None:
            x = (p_logits if which == 0 else q_logits)[r].detach().float() / float(t)
            m = _kept_mask(x, torch.log_softmax(x, -1), tp, tk).numpy()
            top = y[m].max()
            v = kept[key] = (m, top + np.log(np.exp(y[m] - top).sum()))
        return v

    def row(which, r, t):  # (y float64, logZ) of a logits row under temperature t, computed once
        key = (which, r, t.tobytes())
        v = rows.get(key)
        if v is None:
            x = (P if which == 0 else Q)[r]
            y = (x * (np.float32(1) / t)).astype(np.float32).astype(np.float64)
            m = y.max()
            v = rows[key] = (y, m + np.log(np.exp(y - m).sum()))
        return v

    ot, ol, ac = out_tok.numpy(), out_lp.numpy(), accepted.numpy()
    with np.errstate(all="ignore"):
        for j in range(ks.shape[0]):
            k, t = int(ks[j]), temps[j]
            tp = 1.0 if top_ps is None else float(top_ps[j])
            tk = 0 if top_ks is None else int(top_ks[j])
            tr = tp < 1.0 or 0 < tk < V
            a = k
            for i in range(k + 1):
                seed = int(seeds[lrow0[j] + i])
                yp, zp = row(0, int(p_row0[j]) + i, t)
                o = int(out_row0[j]) + i
                if tr:
                    # p' / q': -inf off the kept sets, normalised on them; the emitted logprob
                    # stays y_p - logZ_p of the whole row
                    mp, ztp = trunc(0, int(p_row0[j]) + i, t, tp, tk, yp)
                    if i < k:
                        d = int(draft[d_off[j] + i])
                        yq, zq = row(1, int(q_row0[j]) + i, t)
                        mq, ztq = trunc(1, int(q_row0[j]) + i, t, tp, tk, yq)
                        ok = False
                        if 0 <= d < V and mp[d]:
                            u = ((_hash32i(_stream_key(seed, 1)) >> 9) + 0.5) / 8388608.0
                            ok = bool(not mq[d] or math.log(u) + (yq[d] - ztq) <= yp[d] - ztp)
                        if ok:
                            ot[o], ol[o] = d, yp[d] - zp
                            continue
                        a = i
                        lp = np.where(mp, yp - ztp, -np.inf)
                        lq = np.where(mq, yq - ztq, -np.inf)
                        keep = mp & (lp > lq)
                        if keep.any():
                            w = lp + np.log(-np.expm1(np.where(keep & mq, lq - lp, -np.inf)))
                            tok = int(np.argmax(np.where(keep, w + _gumbel_row(_stream_key(seed, 2), V), -np.inf)))
                        else:
                            tok = int(np.argmax(yp))
                    else:
                        tok = int(np.argmax(np.where(mp, yp + _gumbel_row(_stream_key(seed, 2), V), -np.inf)))
                    ot[o], ol[o] = tok, yp[tok] - zp
                    break
                if i < k:
                    d = int(draft[d_off[j] + i])
                    yq, zq = row(1, int(q_row0[j]) + i, t)
                    ok = False
                    if 0 <= d < V:
                        u = ((_hash32i(_stream_key(seed, 1)) >> 9) + 0.5) / 8388608.0
                        ok = math.log(u) + (yq[d] - zq) <= yp[d] - zp
                    if ok:
                        ot[o], ol[o] = d, yp[d] - zp
                        continue
                    a = i
                    lp, lq = yp - zp, yq - zq
                    keep = lp > lq
                    if keep.any():
                        score = np.where(keep, lp + np.log(-np.expm1(np.where(keep, lq - lp, -1.0)))
                                         + _gumbel_row(_stream_key(seed, 2), V), -np.inf)
                        tok = int(np.argmax(score))
                    else:
                        tok = int(np.argmax(yp))
                else:
                    tok = int(np.argmax(yp + _gumbel_row(_stream_key(seed, 2), V)))
                ot[o], ol[o] = tok, yp[tok] - zp
                break
            ac[j] = a


def _spec_truncation(nb: int, V: int, ks, top_ps, top_ks):
    """Checked float32 / int32 per-block top_p / top_k (None: off), the first scratch row of
    every truncated block (-1: the block is untruncated) and the number of such rows."""
    import numpy as np
    tps = np.ones(nb, np.float32) if top_ps is None else np.asarray(top_ps, np.float32).reshape(-1)
    tks = np.zeros(nb, np.int64) if top_ks is None else np.asarray(top_ks, np.int64).reshape(-1)
    if tps.shape[0] != nb or tks.shape[0] != nb:
        raise ValueError("spec_verify_sample: top_ps / top_ks need one entry per block")
    if nb and not (np.isfinite(tps).all() and (tps > 0).all() and (tps <= 1).all()):
        raise ValueError("spec_verify_sample: top_p must lie in (0, 1]")
    if nb and tks.min() < 0:
        raise ValueError("spec_verify_sample: top_k must not be negative")
    tks = np.minimum(tks, V).astype(np.int32)  # >= V is off, as 0
    tr = (tps < 1) | ((tks > 0) & (tks < V))
    rows = np.where(tr, 2 * np.asarray(ks, np.int64) + 1, 0)
    trow0 = np.where(tr, np.cumsum(rows) - rows, -1)
    return tps, tks, trow0, int(rows.sum())


def spec_verify_sample(p_logits: torch.Tensor, q_logits: torch.Tensor, draft, p_row0, q_row0, d_off, ks, temps, seeds,
                       out_row0=None, out_tok: Optional[torch.Tensor] = None, out_lp: Optional[torch.Tensor] = None,
                       top_ps=None, top_ks=None):
    """Speculative-sampling verification of nb blocks in one call. Block j: ks[j] >= 1 draft
    tokens draft[d_off[j]:d_off[j] + k], target rows p_logits[p_row0[j]:p_row0[j] + k + 1],
    draft rows q_logits[q_row0[j]:q_row0[j] + k], temperature temps[j] > 0 (host arrays of
    length nb; blocks may share rows). seeds: one int64 per position, sum(k + 1) in block
    order (host array). draft: int32 host array or tensor on the logits' device.
    Writes, for i <= accepted[j], the emitted token and its log-probability under the
    target at row out_row0[j] + i of out_tok / out_lp (default: positions in block order,
    fresh tensors); rows after that are left alone. Returns (out_tok int32, out_lp fp32,
    accepted int32 [nb]), on the logits' device; nothing is synchronised.
    top_ps / top_ks (host arrays of length nb, None: off): block j verifies against the
    truncated distributions of its rows, the kept sets of sample_tokens for (temps[j],
    top_ps[j], top_ks[j]); the logprobs stay those of the whole row. A block with top_p >= 1
    and top_k of 0 or >= V is untruncated and behaves as without the arrays. Every row of a
    truncated block needs SPEC_TROW scratch; a call whose workspace would exceed
    SPEC_WS_CAP bytes raises ValueError (split it into several calls)."""
    import numpy as np
    Rp, V = p_logits.shape
    Rq = q_logits.shape[0]
    if q_logits.shape[1] != V or q_logits.dtype != p_logits.dtype or q_logits.device != p_logits.device:
        raise ValueError("spec_verify_sample: target and draft logits differ in width, dtype or device")
    # (the row stride of a one-row matrix is never used and may be anything)
    ps, qs = (t.stride(0) if t.shape[0] > 1 else V for t in (p_logits, q_logits))
    if p_logits.stride(1) != 1 or q_logits.stride(1) != 1 or ps < V or qs < V:
        raise ValueError("spec_verify_sample: a row stride is smaller than V")
    dev = p_logits.device
    host_draft = not isinstance(draft, torch.Tensor)
    n_draft = len(draft) if host_draft else draft.numel()
    nb = len(ks)
    n_out = None if out_tok is None else min(out_tok.numel(), out_lp.numel())
    p_row0, q_row0, d_off, ks, temps, lrow0, out_row0, Lp, Lq = _spec_blocks(
        Rp, Rq, n_draft, (1 << 62) if n_out is None else n_out, V, p_row0, q_row0, d_off, ks, temps, out_row0)
    if out_tok is None:
        n_out = int((out_row0 + ks + 1).max()) if nb else 0
        out_tok = torch.zeros(n_out, dtype=torch.int32, device=dev)
        out_lp = torch.zeros(n_out, dtype=torch.float32, device=dev)
    assert out_tok.dtype == torch.int32 and out_lp.dtype == torch.float32
    assert out_tok.is_contiguous() and out_lp.is_contiguous()
    accepted = torch.zeros(nb, dtype=torch.int32, device=dev)
    seeds = np.asarray(seeds).astype(np.int64).reshape(-1)
    if seeds.shape[0] != Lp:
        raise ValueError("spec_verify_sample: one seed per position (sum of k + 1)")
    n_trunc = 0  # without the arrays the call does what it did before they existed
    if top_ps is not None or top_ks is not None:
        tps, tks, trow0, n_trunc = _spec_truncation(nb, V, ks, top_ps, top_ks)
    if nb == 0:
        return out_tok, out_lp, accepted
    if n_trunc and spec_ws_need(Lp, Lq, V, n_trunc) > SPEC_WS_CAP:
        raise ValueError(f"spec_verify_sample: {n_trunc} truncated rows need more than {SPEC_WS_CAP} bytes of "
                         f"workspace; verify fewer blocks per call")
    if not use_native(p_logits):
        d = np.asarray(draft, np.int64) if host_draft else draft.numpy()
        _spec_verify_ref(p_logits, q_logits, d, p_row0, q_row0, d_off, ks, temps, lrow0, out_row0, seeds, out_tok,
                         out_lp, accepted, tps if n_trunc else None, tks if n_trunc else None)
        return out_tok, out_lp, accepted
    assert p_logits.dtype in (torch.bfloat16, torch.float32)
    K = kernels()
    BW = K.spec_block_words()
    # one pinned staging, one H2D: seeds (int64) | blocks | row map | draft tokens
    n_dr = n_draft if host_draft else 0
    stage = torch.empty(2 * Lp + BW * nb + Lp + Lq + n_dr, dtype=torch.int32, pin_memory=True)
    h = stage.numpy()
    h[:2 * Lp].view(np.int64)[:] = seeds
    blk = h[2 * Lp:2 * Lp + BW * nb].reshape(nb, BW)
    blk[:, 0], blk[:, 1], blk[:, 2], blk[:, 3], blk[:, 4], blk[:, 5] = p_row0, q_row0, d_off, ks, lrow0, out_row0
    blk[:, 6] = temps.view(np.int32)
    if n_trunc:
        blk[:, 7], blk[:, 8], blk[:, 9] = tks, tps.view(np.int32), trow0
    else:
        blk[:, 7], blk[:, 8], blk[:, 9] = 0, 0x3F800000, -1  # top_k off, top_p = 1.0f, no scratch rows
    o_map = 2 * Lp + BW * nb
    idx = np.arange(nb, dtype=np.int32)
    h[o_map:o_map + Lp] = np.repeat(idx, ks + 1)
    h[o_map + Lp:o_map + Lp + Lq] = np.repeat(idx, ks)
    if host_draft:
        h[o_map + Lp + Lq:] = np.asarray(draft, np.int32)
    d_stage = stage.to(dev, non_blocking=True)
    if host_draft:
        draft = d_stage[o_map + Lp + Lq:]
    assert draft.dtype == torch.int32 and draft.is_contiguous() and draft.device == dev
    need = K.spec_ws_bytes(Lp, Lq, V, n_trunc)
    # scratch of the launches, any content on entry; never part of a captured graph,
    # so a grown one simply replaces the old (stream-ordered)
    ws = _SPEC_WS.get((dev.type, dev.index))
    if ws is None or ws.numel() < need:
        ws = _SPEC_WS[(dev.type, dev.index)] = torch.empty(max(need, 1 << 20), dtype=torch.uint8, device=dev)
    base = d_stage.data_ptr()
    K.spec_verify_sample(p_logits.data_ptr(), Rp, ps, q_logits.data_ptr(), Rq, qs,
                         1 if p_logits.dtype == torch.float32 else 0, V, nb, blk.ctypes.data, base + 8 * Lp,
                         base + 4 * o_map, base, draft.data_ptr(), n_draft, out_tok.data_ptr(), out_lp.data_ptr(),
                         n_out, accepted.data_ptr(), ws.data_ptr(), ws.numel(), stream_ptr())
    return out_tok, out_lp, accepted


# ---------------------------------------------------------------------------
# Logit processors (csrc/kernels/logit_proc.hip): repetition / frequency / presence
# penalties, logit_bias and min_p, applied to a step's logits rows in front of the
# samplers, and the per-slot token statistics they read. On CPU tensors the same
# arithmetic runs in numpy (one fp32 rounding per step, as the kernels).
# ---------------------------------------------------------------------------
LOGIT_BIAS_MAX = 128       # logit_bias entries per request (LP_BIAS_MAX)
LOGIT_COUNT_MAX = 0x7FFF   # a cell's generated-count saturates here
LOGIT_PROMPT_FLAG = 0x8000  # cell bit 15: the token occurs in the prompt
_LOGIT_CHUNK = 4096        # LP_CHUNK: tokens per workgroup
LOGIT_HIST_MAX = 16        # extra-history tokens per row of process_logits (LP_HIST_MAX)


def logit_state_alloc(num_slots: int, vocab: int, device) -> torch.Tensor:
    """The zeroed state table: one row of `vocab` 16-bit cells per engine slot (the bits
    are unsigned: view the numpy array as uint16)."""
    return torch.zeros(num_slots, vocab, dtype=torch.int16, device=device)


def logit_state_cells(prompt_ids, generated_ids):
    """Unique token ids of a sequence and their cells (prompt flag | saturating count of
    the generated tokens), as two int32 arrays: what logit_state_reset scatters."""
    import numpy as np
    gen = np.asarray(generated_ids, dtype=np.int64).reshape(-1)
    pro = np.unique(np.asarray(prompt_ids, dtype=np.int64).reshape(-1))
    gu, gc = np.unique(gen, return_counts=True)
    ids = np.union1d(pro, gu)
    cells = np.zeros(ids.shape[0], np.int64)
    cells[np.searchsorted(ids, pro)] |= LOGIT_PROMPT_FLAG
    cells[np.searchsorted(ids, gu)] |= np.minimum(gc, LOGIT_COUNT_MAX)
    return ids.astype(np.int32), cells.astype(np.int32)


def pack_state_resets(resets):
    """[(slot, ids, cells)] -> one int32 array [3 nres descriptors | ids | cells] and
    (nres, total): the staging layout of logit_state_reset."""
    import numpy as np
    nres = len(resets)
    total = sum(len(r[1]) for r in resets)
    buf = np.empty(3 * nres + 2 * total, np.int32)
    off = 0
    for j, (slot, ids, cells) in enumerate(resets):
        n = len(ids)
        buf[3 * j:3 * j + 3] = (slot, off, n)
        buf[3 * nres + off:3 * nres + off + n] = ids
        buf[3 * nres + total + off:3 * nres + total + off + n] = cells
        off += n
    return buf, nres, total


def logit_state_reset(state: torch.Tensor, packed: torch.Tensor, nres: int, total: int) -> None:
    """Zero the rows of `nres` slots and scatter their cells; `packed` (int32, on the
    state's device) has the layout of pack_state_resets. Two resets of one call never
    name the same slot."""
    S, V = state.shape
    assert packed.dtype == torch.int32 and packed.numel() >= 3 * nres + 2 * total and state.is_contiguous()
    if nres == 0:
        return
    if not use_native(state):
        st = state.numpy().view("uint16")
        p = packed.numpy()
        for j in range(nres):
            slot, off, n = (int(v) for v in p[3 * j:3 * j + 3])
            if not 0 <= slot < S:
                continue
            st[slot] = 0
            ids = p[3 * nres + off:3 * nres + off + n]
            st[slot, ids] = p[3 * nres + total + off:3 * nres + total + off + n].astype("uint16")
        return
    base = packed.data_ptr()
    kernels().logit_state_reset(state.data_ptr(), S, V, base, nres, base + 12 * nres, base + 12 * nres + 4 * total,
                                total, stream_ptr())


def logit_state_update(state: torch.Tensor, slots: torch.Tensor, toks: torch.Tensor, n: int) -> None:
    """count[slots[i]][toks[i]] += 1 (saturating) for i < n with slots[i] >= 0; int32 inputs."""
    S, V = state.shape
    assert slots.dtype == toks.dtype == torch.int32 and slots.numel() >= n and toks.numel() >= n
    if not use_native(state):
        st = state.numpy().view("uint16")
        for s, t in zip(slots[:n].tolist(), toks[:n].tolist()):
            if 0 <= s < S and 0 <= t < V and (st[s, t] & LOGIT_COUNT_MAX) < LOGIT_COUNT_MAX:
                st[s, t] += 1
        return
    kernels().logit_state_update(state.data_ptr(), S, V, slots.data_ptr(), toks.data_ptr(), n, stream_ptr())


def logit_state_add(state: torch.Tensor, slots: torch.Tensor, toks: torch.Tensor, n: int) -> None:
    """count[slots[i]][toks[i]] += 1 (saturating, prompt flag kept) for every i < n; int32
    inputs. Unlike logit_state_update, entries may repeat a slot and a (slot, token) pair:
    the commit of the tokens a verify block emitted. Entries with a slot or a token out of
    range are skipped. The table needs an even number of cells (the kernel updates the
    aligned 32-bit word that holds a cell)."""
    S, V = state.shape
    assert slots.dtype == toks.dtype == torch.int32 and slots.numel() >= n and toks.numel() >= n
    assert state.is_contiguous()
    if n <= 0:
        return
    if not use_native(state):
        st = state.numpy().view("uint16")
        for s, t in zip(slots[:n].tolist(), toks[:n].tolist()):
            if 0 <= s < S and 0 <= t < V and (st[s, t] & LOGIT_COUNT_MAX) < LOGIT_COUNT_MAX:
                st[s, t] += 1
        return
    if (S * V) % 2:
        raise ValueError("logit_state_add: the state table needs an even number of cells")
    assert slots.is_contiguous() and toks.is_contiguous()
    kernels().logit_state_add(state.data_ptr(), S, V, slots.data_ptr(), toks.data_ptr(), n, stream_ptr())


def check_hist_pos(hist_pos, n_ids: int, rows: Optional[int] = None) -> None:
    """ValueError on what process_logits' extra history would index out of range: hist_pos
    (host int32 [2, R] = offset | length) against a list of n_ids tokens."""
    import numpy as np
    hp = np.asarray(hist_pos)
    if hp.ndim != 2 or hp.shape[0] != 2:
        raise ValueError("process_logits: hist_pos must be [2, R] = offset | length")
    off, ln = hp[0, :rows].astype(np.int64), hp[1, :rows].astype(np.int64)
    if off.size == 0:
        return
    if ln.min() < 0 or ln.max() > LOGIT_HIST_MAX:
        raise ValueError(f"process_logits: a row's extra history must have 0..{LOGIT_HIST_MAX} tokens")
    if off.min() < 0 or (off + ln).max() > n_ids:
        raise ValueError("process_logits: a row's extra history leaves the token list")


_PROC_WS = {}


def _proc_ws(device, rows: int, V: int) -> torch.Tensor:
    """Per-chunk row maxima of the min_p pass; grown on demand, earlier ones kept alive
    for captured graphs."""
    need = rows * ((V + _LOGIT_CHUNK - 1) // _LOGIT_CHUNK)
    wss = _PROC_WS.setdefault((device.type, device.index), [])
    if not wss or wss[-1].numel() < need:
        wss.append(torch.empty(max(need, 64 * 32), dtype=torch.float32, device=device))
    return wss[-1]


def process_scratch(rows: int, V: int, device) -> torch.Tensor:
    """An fp32 [rows, V] scratch for process_logits whose rows start 16-byte aligned."""
    return torch.empty(rows, (V + 3) & ~3, dtype=torch.float32, device=device)[:, :V]


def process_logits(logits: torch.Tensor, out: torch.Tensor, state: Optional[torch.Tensor], pi: torch.Tensor,
                   pf: torch.Tensor, temps: torch.Tensor, bias_ids: Optional[torch.Tensor] = None,
                   bias_vals: Optional[torch.Tensor] = None, hist_ids: Optional[torch.Tensor] = None,
                   hist_pos: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out[i] = processed fp32 logits of row i (bf16 or fp32 `logits`, any row stride).
    pi: int32 [3, R] = slot (-1: no history) | offset into bias_ids / bias_vals | number
    of bias entries; pf: fp32 [4, R] = repetition | frequency | presence penalty |
    ln(min_p) (-inf: off); temps: fp32 [>= rows] (min_p applies where temps > 0); R >= rows.
    hist_ids (int32 token list) and hist_pos (int32 [2, R] = offset | length into it, length
    <= LOGIT_HIST_MAX): row i is processed as if the listed tokens had been generated after
    what its slot's table row holds -- a token's count is raised by its multiplicity in the
    list (saturating, prompt flag kept); ids outside [0, V) are ignored; rows of a verify
    block share one list and differ in length. Host (CPU) positions are checked here; the
    positions of a device call are checked by whoever stages them (check_hist_pos) and the
    kernel drops a list that would leave hist_ids. Without the two the call is the one of
    before they existed."""
    rows, V = logits.shape
    R = pi.shape[1]
    hist = hist_pos is not None
    if hist:
        if hist_ids is None:
            raise ValueError("process_logits: hist_pos without hist_ids")
        assert hist_ids.dtype == torch.int32 and hist_pos.dtype == torch.int32
        assert tuple(hist_pos.shape) == (2, R) and hist_pos.is_contiguous() and hist_ids.is_contiguous()
        assert hist_ids.device == logits.device and hist_pos.device == logits.device
        if hist_pos.device.type == "cpu":
            check_hist_pos(hist_pos.numpy(), hist_ids.numel(), rows)
    assert pi.dtype == torch.int32 and pf.dtype == torch.float32 and temps.dtype == torch.float32
    assert pi.shape[0] == 3 and tuple(pf.shape) == (4, R) and R >= rows and temps.numel() >= rows
    assert pi.is_contiguous() and pf.is_contiguous() and temps.is_contiguous()
    assert out.dtype == torch.float32 and tuple(out.shape) == (rows, V) and out.stride(1) == 1 and logits.stride(1) == 1
    assert state is None or (state.shape[1] == V and state.is_contiguous())
    cap = 0 if bias_ids is None else min(bias_ids.numel(), bias_vals.numel())
    if not use_native(logits):
        _process_logits_ref(logits, out, state, pi, pf, temps, bias_ids, bias_vals, hist_ids if hist else None,
                            hist_pos)
        return out
    assert logits.dtype in (torch.bfloat16, torch.float32)
    ws = _proc_ws(logits.device, rows, V)
    if hist:
        kernels().process_logits_hist(logits.data_ptr(), 1 if logits.dtype == torch.float32 else 0, logits.stride(0),
                                      out.data_ptr(), out.stride(0), rows, V, ptr(state),
                                      0 if state is None else state.shape[0], pi.data_ptr(), pf.data_ptr(), R,
                                      temps.data_ptr(), ptr(bias_ids), ptr(bias_vals), cap, ws.data_ptr(),
                                      hist_ids.data_ptr(), hist_ids.numel(), hist_pos.data_ptr(), stream_ptr())
        return out
    kernels().process_logits(logits.data_ptr(), 1 if logits.dtype == torch.float32 else 0, logits.stride(0),
                             out.data_ptr(), out.stride(0), rows, V, ptr(state),
                             0 if state is None else state.shape[0], pi.data_ptr(), pf.data_ptr(), R,
                             temps.data_ptr(), ptr(bias_ids), ptr(bias_vals), cap, ws.data_ptr(), stream_ptr())
    return out


def _process_logits_ref(logits, out, state, pi, pf, temps, bias_ids, bias_vals, hist_ids=None, hist_pos=None) -> None:
    import numpy as np
    f32 = np.float32
    rows, V = logits.shape
    x_all = logits.float().numpy()
    o = out.numpy()
    pin, pfn, tn = pi.numpy(), pf.numpy(), temps.numpy()
    st = state.numpy().view("uint16") if state is not None else None
    with np.errstate(all="ignore"):
        for i in range(rows):
            x = x_all[i].astype(f32)
            slot, boff, blen = int(pin[0, i]), int(pin[1, i]), int(pin[2, i])
            r, f, p, lm = f32(pfn[0, i]), f32(pfn[1, i]), f32(pfn[2, i]), f32(pfn[3, i])
            cell = st[slot] if (st is not None and 0 <= slot < st.shape[0]) else np.zeros(V, np.uint16)
            c = (cell & LOGIT_COUNT_MAX).astype(np.int32)
            if hist_pos is not None:
                # the row's extra history: counts raised by the multiplicities, flag kept
                hoff, hlen = int(hist_pos[0, i]), int(hist_pos[1, i])
                h = hist_ids.numpy()[hoff:hoff + hlen].astype(np.int64)
                h = h[(h >= 0) & (h < V)]
                c = np.minimum(c + np.bincount(h, minlength=V).astype(np.int32), LOGIT_COUNT_MAX)
                cell = (cell & LOGIT_PROMPT_FLAG) | c.astype(np.uint16)
            x = np.where(cell != 0, np.where(x > 0, x / r, x * r), x).astype(f32)
            x = (x - (f * c.astype(f32)).astype(f32)).astype(f32)
            x = np.where(c > 0, x - p, x).astype(f32)
            if blen > 0:
                ids = bias_ids.numpy()[boff:boff + blen]
                x[ids] = x[ids] + bias_vals.numpy()[boff:boff + blen].astype(f32)
            t = f32(tn[i])
            if t > 0 and lm > -np.inf:
                y = (x * (f32(1) / t)).astype(f32)
                x = np.where(y < f32(y.max() + lm), f32(-np.inf), x).astype(f32)
            o[i] = x


def segment_sum(hidden: torch.Tensor, cu: torch.Tensor, out: torch.Tensor,
                out_rows: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out[rows[s]] += sum(hidden[cu[s]:cu[s+1]]) (fp32)."""
    S = cu.shape[0] - 1
    if not use_native(hidden):
        for s in range(S):
            r = int(out_rows[s]) if out_rows is not None else s
            if r < 0:
                continue
            out[r] += hidden[int(cu[s]):int(cu[s + 1])].float().sum(0)
        return out
    H = hidden.shape[-1]
    kernels().segment_sum(hidden.data_ptr(), H, cu.data_ptr(), ptr(out_rows), out.data_ptr(), S, stream_ptr())
    return out


def subst_tokens(ids: torch.Tensor, src: torch.Tensor, prev: torch.Tensor) -> torch.Tensor:
    """ids[i] <- prev[src[i]] where src[i] >= 0 (int32, in place): the decode rows of
    a step planned before the previous step's tokens reached the host."""
    n = ids.shape[0]
    assert ids.dtype == src.dtype == prev.dtype == torch.int32 and src.shape[0] >= n
    if not use_native(ids):
        s = src[:n].long()
        m = s >= 0
        ids[m] = prev[s[m]]
        return ids
    kernels().subst_tokens(ids.data_ptr(), src.data_ptr(), prev.data_ptr(), n, stream_ptr())
    return ids
