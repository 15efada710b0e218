"""Float64 numpy reference of speculative-sampling verification on truncated (top-p /
top-k) distributions, written from the contract at the head of csrc/kernels/spec_sample.hip
on top of tests/_spec_ref.py (nothing of the package is imported here).

Contract. A block carries (top_p, top_k); top_p >= 1 and top_k in {0, >= V} is untruncated
and is checked by _spec_ref.verify itself. Otherwise, per target row and per draft row, K is
the split-row sampler's kept set for (T, top_p, top_k); p' = norm(p on K_p), q' = norm(q on
K_q); lp'(x) = y_p(x) - logZ'_p on K_p, -inf off it, lq' likewise.
  accept (i < k):   d not in K_p: reject; d in K_p, not in K_q: accept; else
                    log(u_i) + lq'(d) <= lp'(d)
  residual (i < k): argmax over K_p and lp' > lq' of lp' + log(1 - exp(lq' - lp')) + g (the
                    weight is lp' off K_q); no such token: the row's p-argmax
  bonus (i = k):    argmax over K_p of y_p + g
  logprobs:         y_p - logZ_p of the whole row, as without truncation.

The kernels keep whole sub-bins, so K is only bracketed: L (certainly kept) and U (possibly
kept), the `bracket` rule of tests/test_sampling_gpu.py (copied: importing that module
imports the device tests) with W = two sub-bins and EPS = 2e-5 of top-p mass. A position is
ambiguous when
  * its draft token lies in U \\ L of its p row or of its q row;
  * the accept margin changes sign, or comes within ACCEPT_MARGIN of zero, over the range of
    logZ' spanned by L and U, for p and for q;
  * the residual or bonus winner differs between the four (L | U)_p x (L | U)_q choices,
    lies in U_p \\ L_p, or is ambiguous by _spec_ref's draw rules in any of the four.
Unambiguous positions must match exactly (token, accepted, logprob within 1e-3).

Figures of this reference on `trunc_case` inputs (CYCLE per block, draft tokens drawn from
truncated q on stream 0), float64 alone: see the docstring of tests/test_spec_trunc_cpu.py.
"""
import math

import numpy as np

import _spec_ref as R

W = 2 * 40.0 / 2 ** 20   # two sub-bins of the split-row sampler, in y
EPS = 2e-5               # slack on the top-p mass
CYCLE = ((0.9, 0), (1.0, 40), (0.95, 64), (1.0, 0))


def bracket(y, top_p, top_k, eps=None):
    """(L, U, logZ): the certainly-kept and possibly-kept sets of a non-greedy row
    (tests/test_sampling_gpu.py)."""
    eps = EPS if eps is None else eps
    V = y.size
    ys = np.sort(y)[::-1]
    m = ys[0]
    logZ = m + math.log(np.exp(ys - m).sum())
    L = np.ones(V, dtype=bool)
    U = np.ones(V, dtype=bool)
    top_p = float(np.float32(top_p))
    if top_p < 1.0:
        cum = np.cumsum(np.exp(ys - logZ))
        n_lo = min(int(np.searchsorted(cum, top_p - eps, side="left")), V - 1)
        n_hi = min(int(np.searchsorted(cum, top_p + eps, side="left")), V - 1)
        L &= y >= ys[n_lo]
        U &= y >= ys[n_hi] - W
    k = int(top_k)
    if 0 < k < V:
        L &= y > ys[k] + W
        U &= y >= ys[k - 1]
    L |= y == m
    U |= y == m
    return L, U, logZ


def truncated(top_p, top_k, V):
    return float(np.float32(top_p)) < 1.0 or 0 < int(top_k) < V


def _lse(y, mask):
    m = y[mask].max()
    return m + math.log(np.exp(y[mask] - m).sum())


class TruncRow:
    """y (float64 of the fp32 scaled logits), logZ of the whole row, the bracket and the
    kept log-mass under L and under U (zL <= zU)."""
    __slots__ = ("y", "z", "L", "U", "zL", "zU")

    def __init__(self, x, T, top_p, top_k):
        self.y = R.scaled(x, T)
        self.L, self.U, self.z = bracket(self.y, top_p, top_k)
        self.zL, self.zU = _lse(self.y, self.L), _lse(self.y, self.U)


def trunc_draw(xq, temp, seed, top_p, top_k):
    """The draft's own token on stream 0 with top_p / top_k: the winner over U (ambiguous
    for the verification when it lies outside L)."""
    y = R.scaled(xq, temp)
    _, U, _ = bracket(y, top_p, top_k)
    return int(np.argmax(np.where(U, y + R.gumbel(R.stream_key(seed, 0), len(xq)), -np.inf)))


def residual_scores_trunc(yp, Sp, zp, yq, Sq, zq, g):
    """Scores of the residual draw with K_p = Sp, K_q = Sq; (scores, keep, near)."""
    with np.errstate(all="ignore"):
        lp = np.where(Sp, yp - zp, -np.inf)
        lq = np.where(Sq, yq - zq, -np.inf)
        keep = Sp & (lp > lq)
        both = keep & Sq
        w = np.where(both, lp + np.log(-np.expm1(np.where(both, lq - lp, -1.0))), lp)
        near = both & (lp - lq < R.NEAR_GAP)
        return np.where(keep, w + g, -np.inf), keep, near


def _verify_block(P, Q, blk, draft, seeds, top_p, top_k):
    p0, q0, d0, k, T = blk
    V = P.shape[1]
    toks, lps, amb = [], [], []
    dirty = False
    a = k
    for i in range(k + 1):
        seed = int(seeds[i])
        rp = TruncRow(P[p0 + i], T, top_p, top_k)
        lp_full = rp.y - rp.z
        if i < k:
            d = int(draft[d0 + i])
            rq = TruncRow(Q[q0 + i], T, top_p, top_k)
            if (rp.U[d] and not rp.L[d]) or (rq.U[d] and not rq.L[d]):
                dirty = True
            if not rp.U[d]:
                ok = False
            elif not rq.U[d]:
                ok = True
            else:
                base = math.log(float(R.uniform(R.stream_key(seed, 1), 0))) + rq.y[d] - rp.y[d]
                lo, hi = base - rq.zU + rp.zL, base - rq.zL + rp.zU
                if not (hi <= -R.ACCEPT_MARGIN or lo >= R.ACCEPT_MARGIN):
                    dirty = True
                ok = base - rq.zL + rp.zL <= 0
            if ok:
                toks.append(d)
                lps.append(lp_full[d])
                amb.append(dirty)
                continue
            a = i
            g = R.gumbel(R.stream_key(seed, 2), V)
            winners = []
            for Sp, zp in ((rp.L, rp.zL), (rp.U, rp.zU)):
                for Sq, zq in ((rq.L, rq.zL), (rq.U, rq.zU)):
                    score, keep, near = residual_scores_trunc(rp.y, Sp, zp, rq.y, Sq, zq, g)
                    if keep.any():
                        winners.append(int(np.argmax(score)))
                        dirty = dirty or R._draw_ambiguous(score, near)
                    else:
                        winners.append(-1 - int(np.argmax(rp.y)))  # the fallback, told apart from a draw
            t = winners[0] if winners[0] >= 0 else -1 - winners[0]
            if len(set(winners)) > 1 or not rp.L[t]:
                dirty = True
        else:
            score = np.where(rp.U, rp.y + R.gumbel(R.stream_key(seed, 2), V), -np.inf)
            t = int(np.argmax(score))
            if not rp.L[t] or R._draw_ambiguous(score):
                dirty = True
        toks.append(t)
        lps.append(lp_full[t])
        amb.append(dirty)
        break
    return R.BlockRef(a, toks, lps, amb)


def verify(P, Q, blocks, draft, seeds, top_ps, top_ks):
    """_spec_ref.verify with per-block top_p / top_k; a BlockRef per block."""
    V = P.shape[1]
    out, pos = [], 0
    for j, blk in enumerate(blocks):
        k = blk[3]
        sd = seeds[pos:pos + k + 1]
        if truncated(top_ps[j], top_ks[j], V):
            out.append(_verify_block(P, Q, blk, draft, sd, float(top_ps[j]), int(top_ks[j])))
        else:
            out.extend(R.verify(P, Q, [blk], draft, sd))
        pos += k + 1
    return out


def trunc_case(V, bf16, nblocks, pad=0, seed=0, cycle=CYCLE):
    """_spec_ref.exact_case with (top_p, top_k) cycling per block over `cycle` and the draft
    tokens drawn from the truncated q on stream 0 (keys top_ps / top_ks added)."""
    c = R.exact_case(V, bf16, nblocks, pad, seed)
    c["top_ps"] = np.array([cycle[j % len(cycle)][0] for j in range(nblocks)], np.float32)
    c["top_ks"] = np.array([cycle[j % len(cycle)][1] for j in range(nblocks)], np.int32)
    Qf = c["q"].float().numpy()
    draft = c["draft"].copy()
    for j, (p0, q0, d0, k, T) in enumerate(c["blocks"]):
        if truncated(c["top_ps"][j], c["top_ks"][j], V):
            for i in range(k):
                draft[d0 + i] = trunc_draw(Qf[q0 + i], T, int(c["seeds"][p0 + i]), c["top_ps"][j], c["top_ks"][j])
    c["draft"] = draft
    return c


# ------------------------------------------------------------------ distribution
class DistRef:
    """One target row and one draft row shared by N blocks of k = 1 under (top_p, top_k):
    kept sets (L must equal U), p', q', 1 - TV(p', q')."""

    def __init__(self, xp, xq, temp, top_p, top_k):
        self.rp, self.rq = TruncRow(xp, temp, top_p, top_k), TruncRow(xq, temp, top_p, top_k)
        self.exact = bool(np.array_equal(self.rp.L, self.rp.U) and np.array_equal(self.rq.L, self.rq.U))
        self.Kp, self.Kq = self.rp.L, self.rq.L
        self.pt = np.where(self.Kp, np.exp(self.rp.y - self.rp.zL), 0.0)
        self.qt = np.where(self.Kq, np.exp(self.rq.y - self.rq.zL), 0.0)
        self.one_minus_tv = 1.0 - 0.5 * np.abs(self.pt - self.qt).sum()

    def first_tokens(self, seeds, untruncated_q=False, chunk=4096):
        """(draft tokens drawn from q', accepted flags, first emitted tokens), vectorised over
        the seeds. untruncated_q: the accept / residual step wrongly uses the whole q (the
        power check)."""
        rp, rq = self.rp, self.rq
        V = len(rp.y)
        idx = np.arange(V)
        Sq = np.ones(V, bool) if untruncated_q else self.Kq
        zq = rq.z if untruncated_q else rq.zL
        base, _, _ = residual_scores_trunc(rp.y, self.Kp, rp.zL, rq.y, Sq, zq, 0.0)
        with np.errstate(all="ignore"):
            lp = np.where(self.Kp, rp.y - rp.zL, -np.inf)
            lq = np.where(Sq, rq.y - zq, -np.inf)
        yq_kept = np.where(self.Kq, rq.y, -np.inf)
        ds, acc, first = [], [], []
        for s in range(0, len(seeds), chunk):
            sd = np.asarray(seeds[s:s + chunk], dtype=np.uint64)
            g0 = -np.log(-np.log(R.uniform(R.stream_key(sd, 0)[:, None], idx)))
            d = np.argmax(yq_kept[None, :] + g0, axis=1)
            u = R.uniform(R.stream_key(sd, 1), 0)
            with np.errstate(all="ignore"):
                ok = self.Kp[d] & (~Sq[d] | (np.log(u) + lq[d] <= lp[d]))
            g2 = -np.log(-np.log(R.uniform(R.stream_key(sd, 2)[:, None], idx)))
            r = np.argmax(base[None, :] + g2, axis=1)
            ds.append(d)
            acc.append(ok)
            first.append(np.where(ok, d, r))
        return np.concatenate(ds), np.concatenate(acc), np.concatenate(first)

    def chi_square_z(self, tokens):
        """_spec_ref.chi_square_z over the kept tokens only (it pools zero-probability bins
        into 0 / 0 otherwise); every token must lie in K_p."""
        kept = np.flatnonzero(self.Kp)
        where = np.full(len(self.Kp), -1, np.int64)
        where[kept] = np.arange(len(kept))
        t = where[np.asarray(tokens, np.int64)]
        assert (t >= 0).all(), "an emitted token lies outside K_p"
        return R.chi_square_z(t, self.pt[kept])
