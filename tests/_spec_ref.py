"""Float64 numpy reference of speculative-sampling verification, written from the contract
of csrc/kernels/spec_sample.hip (nothing of the package is imported here).

Contract. Per block: k draft tokens d_0..d_{k-1}, k + 1 target rows, k draft rows, one
temperature T > 0, one seed per position. y = fp32(x) * fp32(1 / T) rounded to fp32;
lp = y_p - logZ_p, lq = y_q - logZ_q with logZ = max + log sum exp(y - max).
RNG: hash32 and the (seed, step) key mix of the samplers, u = ((hsh >> 9) + 0.5) / 2^23;
stream (step) 0 is the draft's own Gumbel-max draw of d_i, stream 1 index 0 the acceptance
uniform u_i, stream 2 index x the Gumbel noise g_i(x) = -log(-log u) of the residual or
bonus draw.
  accept (i < k):   log(u_i) + lq_i(d_i) <= lp_i(d_i)
  residual (i < k): argmax_x [lp_i(x) + log(1 - exp(lq_i(x) - lp_i(x))) + g_i(x)] over
                    lp_i(x) > lq_i(x), ties to the lowest index; no such token: argmax p
  bonus (i = k):    argmax_x [y_p(x) + g_k(x)]
  a = first i that does not accept, else k; tokens d_0..d_{a-1}, r_a; logprobs lp_i(token).

Ambiguity (positions where fp32 rounding may decide, so an fp32 implementation is free):
  * an accept test with |log u + lq(d) - lp(d)| < ACCEPT_MARGIN;
  * a draw whose two best scores are closer than DRAW_MARGIN;
  * a draw in which a token with 0 < lp - lq < NEAR_GAP (its weight is a cancelling
    difference) scores within NEAR_SCORE of the best.
"""
import math

import numpy as np

M32 = np.uint64(0xFFFFFFFF)
ACCEPT_MARGIN = 1e-4
DRAW_MARGIN = 1e-3
NEAR_GAP = 1e-2
NEAR_SCORE = 0.05


def hash32(x):
    x = np.asarray(x, dtype=np.uint64) & M32
    x = x ^ (x >> np.uint64(16))
    x = (x * np.uint64(0x7FEB352D)) & M32
    x = x ^ (x >> np.uint64(15))
    x = (x * np.uint64(0x846CA68B)) & M32
    return x ^ (x >> np.uint64(16))


def stream_key(seed, step):
    """Key of (seed, step); seed an int or an integer array (int64 wraps to uint64)."""
    if isinstance(seed, (int, np.integer)):
        s = np.uint64(int(seed) % 2 ** 64)
    else:
        s = np.asarray(seed).astype(np.int64).astype(np.uint64) if np.asarray(seed).dtype != np.uint64 else np.asarray(seed)
    lo, hi = s & M32, s >> np.uint64(32)
    st = np.uint64(step % 2 ** 32)
    return hash32(lo ^ hash32((hi + np.uint64(0x85EBCA6B)) & M32)
                  ^ hash32((st * np.uint64(0x27D4EB2F) + np.uint64(0x165667B1)) & M32))


def uniform(key, index):
    """u of (key, index); broadcasts key [..., 1] against index [V]."""
    i = np.asarray(index, dtype=np.uint64)
    h = hash32(np.asarray(key, dtype=np.uint64) ^ hash32((i * np.uint64(0x9E3779B9)) & M32))
    return ((h >> np.uint64(9)).astype(np.float64) + 0.5) / 8388608.0


def gumbel(key, V):
    return -np.log(-np.log(uniform(key, np.arange(V))))


def scaled(x, temp):
    it = np.float32(1.0) / np.float32(temp)
    return (np.asarray(x, dtype=np.float32) * it).astype(np.float32).astype(np.float64)


def log_z(y):
    m = y.max()
    return m + math.log(np.exp(y - m).sum())


def draft_draw(xq, temp, seed):
    """The draft's own token: sample_tokens semantics on stream 0, no top-p / top-k."""
    return int(np.argmax(scaled(xq, temp) + gumbel(stream_key(seed, 0), len(xq))))


def residual_scores(lp, lq, g):
    with np.errstate(all="ignore"):
        keep = lp > lq
        w = lp + np.log(-np.expm1(np.where(keep, lq - lp, -1.0)))
        return np.where(keep, w + g, -np.inf), keep


class BlockRef:
    """accepted, toks / lps of positions 0..accepted, ambiguous[i] for those positions
    (True from the first ambiguous position on: what follows it is not determined)."""
    __slots__ = ("accepted", "toks", "lps", "ambiguous")

    def __init__(self, accepted, toks, lps, ambiguous):
        self.accepted, self.toks, self.lps, self.ambiguous = accepted, toks, lps, ambiguous

    @property
    def clean(self):
        return not any(self.ambiguous)


def _draw_ambiguous(score, near=None):
    s = np.sort(score)[::-1]
    if len(s) > 1 and s[0] - s[1] < DRAW_MARGIN:
        return True
    return bool(near is not None and (near & (score > s[0] - NEAR_SCORE)).any())


def verify(P, Q, blocks, draft, seeds, wrong_residual=False):
    """P, Q: float32 arrays of the logits as the kernel reads them (bf16 values widened);
    blocks: (p_row0, q_row0, d_off, k, T) per block; seeds: one per position in block
    order. wrong_residual: draw the residual from p itself (the self-check of the
    distribution test). Returns a BlockRef per block."""
    V = P.shape[1]
    cache = {}

    def row(which, r, T):
        key = (which, r, np.float32(T).tobytes())
        v = cache.get(key)
        if v is None:
            y = scaled((P if which == 0 else Q)[r], T)
            v = cache[key] = (y, log_z(y))
        return v

    out, pos = [], 0
    for (p0, q0, d0, k, T) in blocks:
        toks, lps, amb = [], [], []
        dirty = False
        a = k
        for i in range(k + 1):
            seed = int(seeds[pos + i])
            yp, zp = row(0, p0 + i, T)
            lp = yp - zp
            if i < k:
                d = int(draft[d0 + i])
                yq, zq = row(1, q0 + i, T)
                lq = yq - zq
                u = float(uniform(stream_key(seed, 1), 0))
                margin = math.log(u) + lq[d] - lp[d]
                dirty = dirty or abs(margin) < ACCEPT_MARGIN
                if margin <= 0:
                    toks.append(d)
                    lps.append(lp[d])
                    amb.append(dirty)
                    continue
                a = i
                g = gumbel(stream_key(seed, 2), V)
                if wrong_residual:
                    score, near = lp + g, None
                else:
                    score, keep = residual_scores(lp, lq, g)
                    near = keep & (lp - lq < NEAR_GAP)
                    if not keep.any():
                        score, near = yp, None  # p == q: the row's p-argmax (lowest index)
            else:
                score, near = yp + gumbel(stream_key(seed, 2), V), None
            t = int(np.argmax(score))
            toks.append(t)
            lps.append(lp[t])
            amb.append(dirty or _draw_ambiguous(score, near))
            break
        out.append(BlockRef(a, toks, lps, amb))
        pos += k + 1
    return out


def first_tokens_shared(xp, xq, temp, seeds, wrong_residual=False, chunk=4096):
    """N blocks of k = 1 over one target row and one draft row (the distribution test),
    vectorised over the seeds (seeds[j]: the seed of block j's position 0). Returns
    (draft tokens, accepted flags, first emitted tokens)."""
    V = len(xp)
    yp, yq = scaled(xp, temp), scaled(xq, temp)
    lp, lq = yp - log_z(yp), yq - log_z(yq)
    idx = np.arange(V)
    ds, acc, first = [], [], []
    for s in range(0, len(seeds), chunk):
        sd = np.asarray(seeds[s:s + chunk], dtype=np.uint64)
        g0 = -np.log(-np.log(uniform(stream_key(sd, 0)[:, None], idx)))
        d = np.argmax(yq[None, :] + g0, axis=1)
        u = uniform(stream_key(sd, 1), 0)
        ok = np.log(u) + lq[d] <= lp[d]
        g2 = -np.log(-np.log(uniform(stream_key(sd, 2)[:, None], idx)))
        if wrong_residual:
            r = np.argmax(lp[None, :] + g2, axis=1)
        else:
            base, _ = residual_scores(lp, lq, 0.0)
            r = np.argmax(base[None, :] + g2, axis=1)
        ds.append(d)
        acc.append(ok)
        first.append(np.where(ok, d, r))
    return np.concatenate(ds), np.concatenate(acc), np.concatenate(first)


def exact_case(V, bf16, nblocks, pad=0, seed=0):
    """Inputs of the exact tests: blocks with k cycling 1, 2, 4 and T cycling 0.7, 1.0, 1.3,
    every block on rows of its own; target N(0, 3), draft = target + N(0, 1); the logits
    sit in [rows, V + pad] buffers (pad > 0: rows off 16-byte alignment, padding 1e30).
    Draft tokens are the draft's stream-0 draws. Returns a dict with torch tensors
    p / q (views [:, :V]), the block arrays, draft tokens and per-position seeds."""
    import torch
    ks = np.array([1, 2, 4], np.int64)[np.arange(nblocks) % 3]
    temps = np.array([0.7, 1.0, 1.3], np.float32)[(np.arange(nblocks) // 3) % 3]
    Lp, Lq = int((ks + 1).sum()), int(ks.sum())
    g = torch.Generator().manual_seed(7919 * seed + V)
    dt = torch.bfloat16 if bf16 else torch.float32
    tp = torch.randn(Lp, V, generator=g) * 3
    p_row0 = np.concatenate([[0], np.cumsum(ks + 1)[:-1]])
    q_row0 = np.concatenate([[0], np.cumsum(ks)[:-1]])
    src = np.concatenate([np.arange(p_row0[j], p_row0[j] + ks[j]) for j in range(nblocks)])
    tq = tp[torch.from_numpy(src)] + torch.randn(Lq, V, generator=g)
    pbuf = torch.full((Lp, V + pad), 1e30, dtype=dt)
    qbuf = torch.full((Lq, V + pad), 1e30, dtype=dt)
    pbuf[:, :V] = tp.to(dt)
    qbuf[:, :V] = tq.to(dt)
    p, q = pbuf[:, :V], qbuf[:, :V]
    seeds = (np.arange(1, Lp + 1, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15)) >> np.uint64(1)
    seeds = seeds.astype(np.int64)
    Qf = q.float().numpy()
    draft = np.empty(Lq, np.int32)
    for j in range(nblocks):
        for i in range(int(ks[j])):
            draft[q_row0[j] + i] = draft_draw(Qf[q_row0[j] + i], temps[j], int(seeds[p_row0[j] + i]))
    return {"p": p, "q": q, "ks": ks, "temps": temps, "p_row0": p_row0, "q_row0": q_row0, "d_off": q_row0.copy(),
            "draft": draft, "seeds": seeds, "Lp": Lp,
            "blocks": [(int(p_row0[j]), int(q_row0[j]), int(q_row0[j]), int(ks[j]), float(temps[j]))
                       for j in range(nblocks)]}


def check_against(case, out_tok, out_lp, accepted, refs, name, max_ambiguous=0.03):
    """Unambiguous positions match exactly (token, accepted, logprob within 1e-3); at most
    max_ambiguous of the positions are ambiguous. Prints the figures before asserting."""
    n_pos = n_amb = 0
    bad = []
    worst = 0.0
    for j, (r, (p0, _, _, k, _)) in enumerate(zip(refs, case["blocks"])):
        n_pos += k + 1
        first_amb = next((i for i, a in enumerate(r.ambiguous) if a), None)
        if first_amb is not None:
            n_amb += k + 1 - first_amb  # the position and whatever follows it in the block
        upto = len(r.toks) if first_amb is None else first_amb
        for i in range(upto):
            t, l = int(out_tok[p0 + i]), float(out_lp[p0 + i])
            worst = max(worst, abs(l - r.lps[i]))
            if t != r.toks[i] or not abs(l - r.lps[i]) <= 1e-3:
                bad.append((j, i, t, r.toks[i], l, float(r.lps[i])))
        if first_amb is None and int(accepted[j]) != r.accepted:
            bad.append((j, "accepted", int(accepted[j]), r.accepted))
    print(f"[spec] {name}: blocks={len(refs)} positions={n_pos} ambiguous={n_amb} mismatches={len(bad)} "
          f"max_lp_err={worst:.2e} mean_accepted={np.mean([r.accepted for r in refs]):.3f}")
    assert not bad, f"{name}: (block, position, got, expected, ...): {bad[:5]}"
    assert n_amb <= max_ambiguous * n_pos, f"{name}: {n_amb} of {n_pos} positions ambiguous"


def chi_square_z(tokens, p, min_expected=20.0):
    """z = (chi2 - df) / sqrt(2 df) of a token histogram against probabilities p, bins of
    expected count below min_expected pooled into one."""
    N = len(tokens)
    exp = N * p
    cnt = np.bincount(tokens, minlength=len(p)).astype(np.float64)
    small = exp < min_expected
    e = np.concatenate([exp[~small], [exp[small].sum()]]) if small.any() else exp
    c = np.concatenate([cnt[~small], [cnt[small].sum()]]) if small.any() else cnt
    chi2 = float(((c - e) ** 2 / e).sum())
    df = len(e) - 1
    return (chi2 - df) / math.sqrt(2 * df), chi2, df
