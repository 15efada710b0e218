"""Helpers of the processed-speculation tests: a state table and processor rows built from
per-slot histories, and the numpy references of ops.process_logits with per-row extra
history (on _logit_ref.process_row) and of ops.logit_state_add."""
from __future__ import annotations

import math

import numpy as np

from _logit_ref import process_row

FLAG, CMAX = 0x8000, 0x7FFF


def state_add_ref(table: np.ndarray, slots, toks) -> np.ndarray:
    """The numpy loop ops.logit_state_add must equal: table is uint16 [S, V]."""
    out = table.copy()
    S, V = out.shape
    for s, t in zip(np.asarray(slots).tolist(), np.asarray(toks).tolist()):
        if 0 <= s < S and 0 <= t < V and (out[s, t] & CMAX) < CMAX:
            out[s, t] += 1
    return out


def cells_row_ref(x, cells, *, rep, freq, pres, bias=None, min_p=0.0, temperature=0.0, extra=()):
    """One row on explicit uint16 cells (counts beyond what a token list could spell out,
    such as 0x7fff): the steps of process_row with the cells' counts raised by `extra`."""
    F = np.float32
    V = x.shape[0]
    cells = np.asarray(cells, np.uint16)
    c = (cells & CMAX).astype(np.int64)
    e = np.asarray([t for t in extra if 0 <= t < V], np.int64)
    c = np.minimum(c + np.bincount(e, minlength=V), CMAX).astype(np.int32)
    seen = (c > 0) | ((cells & FLAG) != 0)
    x = np.asarray(x, F).copy()
    r, f, p = F(rep), F(freq), F(pres)
    with np.errstate(all="ignore"):
        x = np.where(seen, np.where(x > 0, x / r, x * r), x).astype(F)
        x = (x - (f * c.astype(F)).astype(F)).astype(F)
        x = np.where(c > 0, (x - p).astype(F), x)
        for t, b in (bias or {}).items():
            x[int(t)] = F(x[int(t)] + F(b))
        if temperature > 0 and min_p > 0:
            y = (x * (F(1) / F(temperature))).astype(F)
            x = np.where(y < F(y.max() + F(math.log(min_p))), F(-np.inf), x)
    return x.astype(F)


def history_row_ref(x, prompt, generated, extra, V, **params):
    """process_row on the table's history plus the extra tokens inside [0, V)."""
    extra = [int(t) for t in extra if 0 <= int(t) < V]
    return process_row(x, prompt, list(generated) + extra, **params)
