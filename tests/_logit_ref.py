"""numpy fp32 reference of the logit processors for the engine-level tests: the steps of
ops.process_logits on one row, from a sequence's prompt and generated history."""
from __future__ import annotations

import math

import numpy as np

F32 = np.float32


def process_row(row, prompt, history, *, repetition_penalty=1.0, frequency_penalty=0.0, presence_penalty=0.0,
                logit_bias=None, min_p=0.0, temperature=0.0):
    x = np.asarray(row, dtype=F32).copy()
    V = x.shape[0]
    c = np.bincount(np.asarray(history, dtype=np.int64), minlength=V).astype(np.int32)
    seen = c > 0
    seen[np.asarray(prompt, dtype=np.int64)] = True
    r, f, p = F32(repetition_penalty), F32(frequency_penalty), F32(presence_penalty)
    with np.errstate(all="ignore"):
        x = np.where(seen, np.where(x > 0, x / r, x * r), x).astype(F32)
        x = (x - (f * c.astype(F32)).astype(F32)).astype(F32)
        x = np.where(c > 0, (x - p).astype(F32), x)
        for t, b in (logit_bias or {}).items():
            x[int(t)] = F32(x[int(t)] + F32(b))
        if temperature > 0 and min_p > 0:
            y = (x * (F32(1) / F32(temperature))).astype(F32)
            x = np.where(y < F32(y.max() + F32(math.log(min_p))), F32(-np.inf), x)
    return x.astype(F32)


def greedy_reference(logits_fn, prompt, n, **params):
    """Greedy decoding of n tokens on processed reference logits: logits_fn(ids) -> the
    fp32 logits row after the last id."""
    gen = []
    for _ in range(n):
        gen.append(int(process_row(logits_fn(prompt + gen), prompt, gen, **params).argmax()))
    return gen
