"""Model-level references for the regime tests: checkpoints whose norm weights and biases are
not the identity, the float64 function such a checkpoint defines, a bf16 emulation of the
serving chain with planted errors, and the two error measures.

tests/test_model_refs_cpu.py checks this module against itself on the CPU (the emulation's own
error, every planted error's displacement, the RoPE table); tests/test_model_regimes_gpu.py
drives the engine through every LayerDispatch regime and compares its logits with
reference64 under the bound the emulation gives.

  trained_like(model, seed)   overwrite the norm weights (llama / mixtral) or the LayerNorm
                              weights and every bias (gpt2) in place, BEFORE folding. After
                              build_model call model.fold_norms() again: folding resets a
                              folded norm to 1, so the second call folds only what is new.
  Snapshot(model)             float64 copy of every parameter, taken before fold_norms and
                              quantize_weights: the function the checkpoint defines.
  reference64(snap, cfg, tokens)
                              plain float64 forward of one sequence -> logits of its last row.
                              The RoPE table is rope_table64 below (the published formula,
                              written out here), not ops.build_cos_sin.
  emulate(snap, cfg, tokens, plant=None, quant=None)
                              the same forward with one bf16 rounding at every point where the
                              serving chain stores bf16: the folded weights (rounded once), the
                              residual stream, the norm output, q / k / v, the attention output,
                              the SiLU-gate (GELU) output, the logits' input and the bf16 logits
                              themselves. Sums stay float64: the bound derived from it allows a
                              factor 2 for the kernels' fp32 summation order and bf16 P.V.
                              quant = "fp8" / "int8" / "int4" passes the projection weights
                              through quantize_weight's round trip; such a model is not folded
                              (build_model), so the norm output carries the norm weight. plant = one of
                              PLANTS puts one wrong model in its place.
  routed(snap, cfg, tokens, route)
                              reference64 and emulate of a MoE sequence under the expert choice
                              a kernel chain recorded, and whether that choice is admissible.
  rel(got, ref)               relative L2 error of last-row logits.
  gap(got, ref)               ref.max() - ref[argmax(got)]: what the greedy choice of `got`
                              loses under `ref` (0 when they agree).
"""
from __future__ import annotations

import math
from typing import Optional, Sequence

import torch

from xgserve.ops.linear import WQ_FORMATS, dequantize_weight, quantize_weight

PAGE = 16   # tokens per KV page (EngineConfig.block_size default): the span "kv_page" loses

# planted errors (emulate(plant=...)); the comment says what a kernel chain with that bug does
NORM_PLANTS = (
    "input_norm",       # layer 0 reads rmsnorm(x) without its input_norm weight
    "post_norm",        # layer 0 reads the post-attention norm without its weight
    "final_norm",       # the final norm's weight is dropped
    "norm_twice",       # input_norm folded into qkv AND still applied by the norm
)
FOLD_PLANTS = (
    "post_into_qkv",    # qkv folded with post_norm's weight instead of input_norm's
    "input_into_gate_up",  # ... and gate_up with input_norm's
)
MOE_PLANTS = ("moe_post_folded",)  # post_norm folded into w13: the router reads the unscaled stream
GPT2_PLANTS = ("qkv_b", "o_b", "fc_b", "proj_b", "ln_b")  # that bias of layer 0 dropped (ln_b: ln1_b)
ATTN_PLANTS = (
    "rope_q_shift",     # q rotated for position p + 1, k for p
    "kv_page",          # the first KV page (positions < PAGE) never reaches the attention
)
PLANTS = NORM_PLANTS + FOLD_PLANTS + MOE_PLANTS + GPT2_PLANTS + ATTN_PLANTS


def plants_for(cfg) -> tuple:
    if cfg.arch == "gpt2":
        return GPT2_PLANTS + ("final_norm", "kv_page")
    if cfg.arch == "mixtral":
        return ("input_norm", "post_norm", "final_norm", "norm_twice", "post_into_qkv") + MOE_PLANTS + ATTN_PLANTS
    return NORM_PLANTS + FOLD_PLANTS + ATTN_PLANTS


# ------------------------------------------------------------------------------ checkpoints
def _norm_vector(n: int, g: torch.Generator) -> torch.Tensor:
    """1 + 0.3 randn with the outliers real checkpoints carry, at distinct random places: one
    entry per 1024 (at least one) x 8, as many / 16, and half as many (at least one) negated --
    4 + 4 + 2 of the 4096 entries of an 8B norm."""
    v = 1 + 0.3 * torch.randn(n, generator=g, dtype=torch.float64)
    big, neg = max(1, n // 1024), max(1, n // 2048)
    idx = torch.randperm(n, generator=g)[:2 * big + neg]
    v[idx[:big]] *= 8.0
    v[idx[big:2 * big]] /= 16.0
    v[idx[2 * big:]] *= -1.0
    return v


@torch.no_grad()
def trained_like(model, seed: int):
    """Overwrite the norm weights / biases of `model` in place (see the module docstring).
    Drawn on the CPU, so a CPU and a GPU model of one seed hold the same values."""
    g = torch.Generator().manual_seed(seed)
    for name, p in model.named_parameters():
        leaf = name.rsplit(".", 1)[-1]
        if model.cfg.arch == "gpt2":
            if leaf.startswith("ln") and leaf.endswith("_w"):
                v = 1 + 0.3 * torch.randn(p.shape, generator=g, dtype=torch.float64)
            elif leaf.endswith("_b"):
                v = 0.1 * torch.randn(p.shape, generator=g, dtype=torch.float64)
            else:
                continue
        elif "norm" in leaf:
            v = _norm_vector(p.numel(), g)
        else:
            continue
        p.copy_(v.to(device=p.device, dtype=p.dtype))
    if hasattr(model, "norms_folded"):
        model.norms_folded = False
    return model


class Snapshot:
    """float64 copies of every parameter of a TP = 1 model, keyed by parameter name."""

    def __init__(self, model, device=None):
        self.cfg = model.cfg
        self.device = torch.device(device) if device is not None else model.device
        self.memo = {}  # emulate's folded / quantized weights
        self.p = {n: p.detach().to(device=self.device, dtype=torch.float64).clone()
                  for n, p in model.named_parameters()}

    def __getitem__(self, name: str) -> torch.Tensor:
        return self.p[name]

    def layer(self, i: int, name: str) -> torch.Tensor:
        return self.p[f"layers.{i}.{name}"]


# ------------------------------------------------------------------------------ RoPE
def rope_inv_freq64(head_dim: int, theta: float, scaling: Optional[dict]) -> list:
    """The rotary frequencies theta^(-2i/d) (Su et al., RoFormer), with the "llama3" context
    extension of the Llama 3.1 release where `scaling` asks for it: wavelengths above
    L / low_freq_factor are slowed by `factor`, those below L / high_freq_factor are kept, and
    the band between is interpolated linearly in L / wavelength."""
    inv = [float(theta) ** (-(2.0 * i) / head_dim) for i in range(head_dim // 2)]
    kind = (scaling or {}).get("rope_type", (scaling or {}).get("type"))
    if kind != "llama3":
        return inv
    factor = float(scaling.get("factor", 8.0))
    low, high = float(scaling.get("low_freq_factor", 1.0)), float(scaling.get("high_freq_factor", 4.0))
    L = float(scaling.get("original_max_position_embeddings", 8192))
    out = []
    for f in inv:
        wavelen = 2.0 * math.pi / f
        if wavelen < L / high:
            out.append(f)
        elif wavelen > L / low:
            out.append(f / factor)
        else:
            s = (L / wavelen - low) / (high - low)
            out.append((1.0 - s) * f / factor + s * f)
    return out


def rope_table64(head_dim: int, n_pos: int, theta: float, scaling: Optional[dict], device="cpu") -> torch.Tensor:
    """float64 [n_pos, head_dim] = [cos(p f_i) | sin(p f_i)]."""
    inv = torch.tensor(rope_inv_freq64(head_dim, theta, scaling), dtype=torch.float64, device=device)
    ang = torch.arange(n_pos, dtype=torch.float64, device=device)[:, None] * inv[None, :]
    return torch.cat([ang.cos(), ang.sin()], -1)


def check_rope_tables(n_pos: int = 8192) -> dict:
    """rope_table64 against ops.build_cos_sin (the table the kernels read) for every rope-using
    model of the registry; returns {model: max |difference|} and asserts each <= 1e-6."""
    from xgserve import ops
    from xgserve.models import get_config, list_models
    out = {}
    for name in list_models():
        cfg = get_config(name)
        if cfg.arch == "gpt2":
            continue
        n = min(n_pos, cfg.max_position)
        got = ops.build_cos_sin(cfg.head_dim, n, cfg.rope_theta, cfg.rope_scaling).double()
        want = rope_table64(cfg.head_dim, n, cfg.rope_theta, cfg.rope_scaling)
        out[name] = float((got - want).abs().max())
        assert out[name] <= 1e-6, (name, out[name])
    return out


def _rotate(x, cos, sin):
    h = x.shape[-1] // 2
    x1, x2 = x[..., :h], x[..., h:]
    return torch.cat([x1 * cos - x2 * sin, x2 * cos + x1 * sin], -1)


# ------------------------------------------------------------------------------ forwards
def _bf16(t: torch.Tensor) -> torch.Tensor:
    return t.to(torch.bfloat16).to(torch.float64)


def _same(t: torch.Tensor) -> torch.Tensor:
    return t


def _degroup(w: torch.Tensor):
    """[2F, H] stored g0..g15 u0..u15 g16.. -> gate [F, H], up [F, H]."""
    v = w.reshape(w.shape[0] // 32, 2, 16, w.shape[1])
    return v[:, 0].reshape(-1, w.shape[1]), v[:, 1].reshape(-1, w.shape[1])


def _attend(q, k, v, kv_page: bool):
    """Causal attention of one sequence: q [T, Hq, D], k / v [T, Hkv, D] -> [T, Hq * D]."""
    T, Hq, D = q.shape
    G = Hq // k.shape[1]
    k, v = k.repeat_interleave(G, 1), v.repeat_interleave(G, 1)
    s = torch.einsum("thd,shd->hts", q, k) / math.sqrt(D)
    mask = torch.ones(T, T, dtype=torch.bool, device=q.device).tril()
    if kv_page and T > PAGE:
        mask[PAGE:, :PAGE] = False
    s = s.masked_fill(~mask[None], float("-inf"))
    return torch.einsum("hts,shd->thd", torch.softmax(s, -1), v).reshape(T, Hq * D)


def _quant(w, r, quant: Optional[str], quant_bf16: bool, memo: Optional[dict] = None, key=None) -> torch.Tensor:
    """The weight the chain multiplies by: rounded once to bf16 (r), then quantize_weight's
    round trip on the bf16 tensor, as quantize_weights does. `w` may be a function that makes
    the weight; memo[key] keeps the result (the unplanted emulation of one snapshot makes the
    same weights for every sequence)."""
    if memo is not None and key in memo:
        return memo[key]
    w = r(w() if callable(w) else w)
    if quant is not None:
        fmt = WQ_FORMATS[quant]
        w = dequantize_weight(*quantize_weight(w.to(torch.bfloat16), fmt), fmt).double()
        w = _bf16(w) if quant_bf16 else w
    if memo is not None:
        memo[key] = w
    return w


def _llama(snap: Snapshot, cfg, ids, r, plant, quant, quant_bf16, trace=None, route=None, quant_last=None):
    T, D, Hq, Hkv = ids.shape[0], cfg.head_dim, cfg.num_heads, cfg.num_kv_heads
    moe = cfg.arch == "mixtral"
    folded = r is not _same         # the serving chain folds; the reference applies the norm itself
    tab = rope_table64(D, T + 1, cfg.rope_theta, cfg.rope_scaling, device=ids.device)
    cos, sin = tab[:T, None, :D // 2], tab[:T, None, D // 2:]
    cos1, sin1 = tab[1:T + 1, None, :D // 2], tab[1:T + 1, None, D // 2:]
    ones = torch.ones(cfg.hidden_size, dtype=torch.float64, device=ids.device)

    def rms(x):
        return x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + cfg.norm_eps)

    memo = snap.memo if plant is None else None

    def weight(i, name, w):
        if not folded:   # the reference: the stored weight, or what its quantized codes stand for
            return w if quant is None else _quant(w, _same, quant, False, memo, ("ref", i, name, quant))
        return _quant(w, r, quant, quant_bf16, memo, (i, name, quant, quant_bf16))

    # quant_last: only the last so many tokens ran on the quantized weights; the earlier ones
    # (a prompt step above 64 rows) on the resident bf16 weights of the same unfolded model
    qrows = None
    if quant is not None and quant_last is not None:
        qrows = (torch.arange(T, device=ids.device) >= T - quant_last)[:, None]

    def mm(h, i, name, w):
        y = h @ weight(i, name, w).t()
        return y if qrows is None else torch.where(qrows, y, h @ w.t())

    def proj(i, name, g_fold, g_apply, x):
        """rmsnorm(x, g_apply) through the weight W diag(g_fold)."""
        w = snap.layer(i, name)
        if not folded:
            return mm(rms(x) * g_fold * g_apply, i, name, w)
        if quant is not None:   # a quantized model is not folded: its norms keep their weights
            return mm(r(rms(x) * g_fold * g_apply), i, name, w)
        return r(rms(x) * g_apply) @ weight(i, name, lambda: w * g_fold[None, :]).t()

    x = snap["embed"][ids]
    for i in range(cfg.num_layers):
        L = lambda n: snap.layer(i, n)  # noqa: E731
        g_in, g_post = L("input_norm"), L("post_norm")
        first = i == 0
        fold_q, apply_q = g_in, ones
        if first and plant == "input_norm":
            fold_q = ones
        elif first and plant == "norm_twice":
            apply_q = g_in
        elif first and plant == "post_into_qkv":
            fold_q = g_post
        qkv = proj(i, "qkv", fold_q, apply_q, x)
        q = qkv[:, :Hq * D].view(T, Hq, D)
        k = qkv[:, Hq * D:(Hq + Hkv) * D].view(T, Hkv, D)
        v = qkv[:, (Hq + Hkv) * D:].view(T, Hkv, D)
        q = r(_rotate(q, cos1, sin1) if plant == "rope_q_shift" else _rotate(q, cos, sin))
        k, v = r(_rotate(k, cos, sin)), r(v)
        a = r(_attend(q, k, v, plant == "kv_page"))
        x = r(x + mm(a, i, "o", L("o")))
        fold_m = g_post
        if first and plant == "post_norm":
            fold_m = ones
        elif first and plant == "input_into_gate_up":
            fold_m = g_in
        if moe:
            # the post-attention norm of a MoE layer keeps its weight: router and experts read it
            h = r(rms(x) * fold_m)
            h_router = r(rms(x)) if (first and plant == "moe_post_folded") else h
            z = h_router @ L("router").t()
            if trace is not None:
                trace.append(z)
            p = torch.softmax(z, -1)
            wts, eid = torch.topk(p, cfg.experts_per_token, -1)
            if route is not None:   # the experts another chain chose, weighted by this one's router
                eid = route[i].to(ids.device).long()
                wts = p.gather(-1, eid)
            wts = wts / wts.sum(-1, keepdim=True)
            out = torch.zeros_like(x)
            w13, w2 = L("w13"), L("w2")
            for e in range(cfg.num_experts):
                rows, slot = (eid == e).nonzero(as_tuple=True)
                if rows.numel() == 0:
                    continue
                gw, uw = _degroup(w13[e])
                he = h[rows]
                act = r(torch.nn.functional.silu(he @ gw.t()) * (he @ uw.t()))
                out.index_add_(0, rows, wts[rows, slot][:, None] * (act @ w2[e].t()))
            x = r(x + out)
        else:
            gu = proj(i, "gate_up", fold_m, ones, x)
            F2 = gu.shape[1]
            gu = gu.view(T, F2 // 32, 2, 16)
            act = r(torch.nn.functional.silu(gu[:, :, 0]) * gu[:, :, 1]).reshape(T, F2 // 2)
            x = r(x + mm(act, i, "down", L("down")))
    g = ones if plant == "final_norm" else snap["norm"]
    h = r(rms(x[-1]) * g)
    head = snap["lm_head"][:cfg.vocab_size] if "lm_head" in snap.p else snap["embed"]
    return r(head @ h)


def _gpt2(snap: Snapshot, cfg, ids, r, plant):
    T, D, Hh, H = ids.shape[0], cfg.head_dim, cfg.num_heads, cfg.hidden_size

    def ln(x, w, b):
        mu = x.mean(-1, keepdim=True)
        var = (x - mu).pow(2).mean(-1, keepdim=True)
        return r((x - mu) * torch.rsqrt(var + cfg.norm_eps) * w + b)

    def lin(x, w, b, drop):
        return r(x @ w.t() + (0 if drop else b))

    x = r(snap["wte"][ids] + snap["wpe"][:T])
    for i in range(cfg.num_layers):
        L = lambda n: snap.layer(i, n)  # noqa: E731
        bad = plant if i == 0 else None
        h = ln(x, L("ln1_w"), 0 if bad == "ln_b" else L("ln1_b"))
        qkv = lin(h, L("qkv_w"), L("qkv_b"), bad == "qkv_b")
        q, k, v = (t.view(T, Hh, D) for t in qkv.split(H, -1))
        a = r(_attend(q, k, v, plant == "kv_page"))
        x = r(x + lin(a, L("o_w"), L("o_b"), bad == "o_b"))
        h = ln(x, L("ln2_w"), L("ln2_b"))
        u = lin(h, L("fc_w"), L("fc_b"), bad == "fc_b")
        act = r(0.5 * u * (1 + torch.tanh(math.sqrt(2 / math.pi) * (u + 0.044715 * u ** 3))))
        x = r(x + lin(act, L("proj_w"), L("proj_b"), bad == "proj_b"))
    if plant == "final_norm":
        h = ln(x[-1], 1.0, 0.0)
    else:
        h = ln(x[-1], snap["lnf_w"], snap["lnf_b"])
    return r(snap["wte"] @ h)


@torch.no_grad()
def _forward(snap: Snapshot, cfg, tokens: Sequence[int], r, plant, quant=None, quant_bf16=False,
             trace=None, route=None, quant_last=None) -> torch.Tensor:
    assert plant is None or plant in plants_for(cfg), plant
    ids = torch.as_tensor(list(tokens), dtype=torch.long, device=snap.device)
    if cfg.arch == "gpt2":
        assert quant is None
        return _gpt2(snap, cfg, ids, r, plant)
    return _llama(snap, cfg, ids, r, plant, quant, quant_bf16, trace, route, quant_last)


def reference64(snap: Snapshot, cfg, tokens: Sequence[int], quant: Optional[str] = None,
                quant_last: Optional[int] = None) -> torch.Tensor:
    """float64 logits [V] of the last token of one sequence under the checkpoint `snap`.
    quant: under the quantized checkpoint instead -- every projection weight replaced by what
    its fp8 / int8 / int4 codes stand for (quantize_weight's round trip, no other rounding).
    Kernels and emulation read the same codes, so the quantization error is no part of what a
    test has to allow: only the bf16 storage of the chain is. quant_last = n: only the last n
    tokens ran on the quantized weights, the earlier ones on the bf16 weights the model keeps
    for steps above 64 rows."""
    return _forward(snap, cfg, tokens, _same, None, quant, quant_last=quant_last)


def emulate(snap: Snapshot, cfg, tokens: Sequence[int], plant: Optional[str] = None, quant: Optional[str] = None,
            quant_bf16: bool = False, quant_last: Optional[int] = None) -> torch.Tensor:
    """The bf16 serving chain's logits [V] of the last token (see the module docstring).
    quant_bf16: the dequantized weight is rounded to bf16 once more (the "dq" regime)."""
    return _forward(snap, cfg, tokens, _bf16, plant, quant, quant_bf16, quant_last=quant_last)


def routed(snap: Snapshot, cfg, tokens: Sequence[int], route):
    """A MoE sequence under the routing another chain took: route[layer] = expert ids [T, k] (the
    ids a kernel chain recorded). Returns (slack, allowed, ref logits, emulate logits), both
    forwards run with that routing.

    Top-k routing is a step function: where two router logits of a token are closer than storage
    noise moves them, bf16 chains that differ only in rounding order pick different experts,
    and the logits jump by far more than any rounding bound. So the chain's routing is checked
    on its own, and its logits against the float64 function under ITS routing. At each layer
    and token, slack = (k-th largest reference router logit) - (smallest reference logit of a
    chosen expert), 0 when the chain chose the reference's experts; delta = the largest
    |router logit of emulate - of reference| of that token. A chain that keeps the tolerance
    rule moves each router logit by at most 2 delta, a difference of two by at most 4 delta:
    slack <= allowed = 4 delta must hold everywhere. Returned for the worst place."""
    assert cfg.arch == "mixtral"
    zr, ze = [], []
    ref = _forward(snap, cfg, tokens, _same, None, trace=zr, route=route)
    emu = _forward(snap, cfg, tokens, _bf16, None, trace=ze, route=route)
    k = cfg.experts_per_token
    z = torch.cat(zr)
    eid = torch.cat([e.to(z.device).long() for e in route])
    assert eid.shape == (z.shape[0], k) and bool((eid[:, 0] != eid[:, 1]).all())
    slack = z.topk(k, -1).values[:, k - 1] - z.gather(-1, eid).amin(-1)
    allowed = 4 * torch.cat([(a - b).abs().amax(-1) for a, b in zip(zr, ze)])
    worst = int((slack - allowed).argmax())
    return float(slack[worst]), float(allowed[worst]), ref, emu


# ------------------------------------------------------------------------------ measures
def rel(got: torch.Tensor, ref: torch.Tensor) -> float:
    got, ref = got.detach().double().cpu().reshape(-1), ref.detach().double().cpu().reshape(-1)
    assert got.shape == ref.shape and bool(torch.isfinite(got).all())
    return float((got - ref).norm() / ref.norm())


def ambiguity(emu: torch.Tensor, ref: torch.Tensor) -> float:
    """The largest gap() the emulation's own error explains. A perturbation e of the logits
    moves the argmax only to a token within 2 max|e| of the best one; the chain under test is
    allowed twice the emulation's error (the tolerance rule), so 4 max|emu - ref|."""
    return 4.0 * float((emu.detach().double().cpu() - ref.detach().double().cpu()).abs().max())


def gap(got: torch.Tensor, ref: torch.Tensor) -> float:
    got, ref = got.detach().double().cpu().reshape(-1), ref.detach().double().cpu().reshape(-1)
    return float(ref.max() - ref[int(got.argmax())])
