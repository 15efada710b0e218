"""ops.top_logprobs on the GPU against a numpy reference: float64 log-sum-exp of the whole
row, a stable sort on (-y, id), y = fp32(x * fp32(1 / T)) computed as the kernel does.

Ids must match exactly; log-probabilities within LP_TOL = 1e-3, the bound the sampler tests
allow a logprob (fp32 online log-sum-exp with hardware exp / log over up to 128K terms).
Every test prints the worst error it saw."""
import numpy as np
import pytest
import torch

from xgserve import ops
from xgserve.ops import _native
from xgserve.ops import sampling as SP

pytestmark = pytest.mark.gpu
DEV = "cuda"
LP_TOL = 1e-3
PARTS = 8  # workgroups per row of the split form


@pytest.fixture(autouse=True, scope="module")
def _native_loaded():
    _native.kernels()


def reference(x: torch.Tensor, temps: torch.Tensor, rows, k: int):
    """x: [R, V] (any dtype / device), temps: [R]; rows: list of row indices."""
    xf = x.detach().float().cpu().numpy()
    tn = temps.detach().float().cpu().numpy()
    ids = np.full((len(rows), k), -1, np.int32)
    lps = np.full((len(rows), k), -np.inf, np.float32)
    with np.errstate(all="ignore"):
        for o, r in enumerate(rows):
            t = np.float32(tn[r])
            y = (xf[r] * (np.float32(1) / t)).astype(np.float32) if t > 0 else xf[r]
            fin = np.isfinite(y)
            if not fin.any():
                continue
            y64 = y.astype(np.float64)
            m = y64[fin].max()
            logz = m + np.log(np.exp(y64[fin] - m).sum())
            order = np.argsort(-y, kind="stable")[:k]  # stable: equal y keeps the lower id first
            order = order[fin[order]]
            ids[o, :len(order)] = order
            lps[o, :len(order)] = y64[order] - logz
    return ids, lps


def check(got_ids, got_lps, want_ids, want_lps, what=""):
    gi, gl = got_ids.cpu().numpy(), got_lps.cpu().numpy()
    assert gi.shape == want_ids.shape and gl.shape == want_lps.shape
    assert np.array_equal(gi, want_ids), (what, np.argwhere(gi != want_ids)[:5], gi[gi != want_ids][:5],
                                          want_ids[gi != want_ids][:5])
    live = want_ids >= 0
    assert np.all(np.isneginf(gl[~live]))
    err = float(np.abs(gl[live].astype(np.float64) - want_lps[live]).max()) if live.any() else 0.0
    print(f"top_logprobs {what}: worst |lp error| = {err:.3e}")
    assert err <= LP_TOL, (what, err)
    return err


_CASES = {}


def _case(V, dtype):
    """One logits matrix per (V, dtype): 64 rows inside a wider buffer (a strided view),
    per-row temperatures with zeros, 24 asking rows in shuffled order, and its top-20
    reference -- computed once, shared by every K, never modified."""
    key = (V, dtype)
    if key not in _CASES:
        g = torch.Generator(device="cpu").manual_seed(1000 + V)
        B = 64
        wide = (torch.randn(B, V + 24, generator=g) * 3.0).to(dtype).to(DEV)
        x = wide[:, 8:8 + V]  # rows stay 16-byte aligned where the buffer's row pitch allows
        temps = torch.tensor([0.0, 1.0, 0.7, 1.3, 0.0, 2.0, 0.25, 1.0] * 8, dtype=torch.float32)
        rows = torch.randperm(B, generator=g)[:24].tolist()
        want = reference(x, temps, rows, 20)
        _CASES[key] = (x, temps.to(DEV), rows, want)
    return _CASES[key]


@pytest.mark.parametrize("K", [1, 5, 20])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "f32"])
@pytest.mark.parametrize("V", [16, 1000, 4099, 32000, 128256])
def test_shape_sweep(V, dtype, K):
    x, temps, rows, (wi, wl) = _case(V, dtype)
    assert (V >= SP.ARGMAX_SPLIT_MIN_V) == (V in (32000, 128256))  # both sides of the split threshold
    rt = torch.tensor(rows, dtype=torch.int32, device=DEV)
    ids, lps = ops.top_logprobs(x, temps, K, rows=rt)
    # the first K of the top-20 reference: the order is total, so a prefix is the answer for K
    wi_k, wl_k = wi[:, :K].copy(), wl[:, :K].copy()
    check(ids, lps, wi_k, wl_k, f"V={V} {dtype} K={K}")
    if V == 16:
        assert (wi[:, 16:] == -1).all()  # V < 20: the reference itself ran out of entries


def test_all_rows_without_row_list():
    x, temps, _, _ = _case(4099, torch.bfloat16)
    ids, lps = ops.top_logprobs(x, temps, 5)
    wi, wl = reference(x, temps, list(range(x.shape[0])), 5)
    check(ids, lps, wi, wl, "rows=None")


def test_bf16_rows_hold_exact_ties():
    """bf16 randn at V = 128256 repeats values many times over: the reference's top 20 of
    these rows contain equal neighbours, so the tie rule decides ids here."""
    x, temps, rows, (wi, wl) = _case(128256, torch.bfloat16)
    tied = sum(int((np.diff(wl[o]) == 0).any()) for o in range(len(rows)))
    assert tied >= len(rows) // 2, tied


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "f32"])
@pytest.mark.parametrize("off", [0, 1], ids=["aligned", "unaligned"])
def test_unaligned_and_odd_views(dtype, off):
    """A view that starts `off` elements into its buffer with an odd row pitch: rows that
    are not 16-byte aligned take the scalar loads."""
    torch.manual_seed(5)
    V = 20011
    wide = (torch.randn(6, V + 13, device=DEV) * 2.0).to(dtype)
    x = wide[:, off:off + V]
    temps = torch.tensor([0.0, 0.5, 1.0, 1.5, 0.0, 3.0], device=DEV)
    ids, lps = ops.top_logprobs(x, temps, 20)
    wi, wl = reference(x, temps, list(range(6)), 20)
    check(ids, lps, wi, wl, f"view off={off} {dtype}")


def _slice_edges(V):
    per = ((V + PARTS - 1) // PARTS + 7) & ~7
    pos = []
    for p in range(PARTS):
        lo, hi = min(V, p * per), min(V, (p + 1) * per)
        pos += [lo, hi - 1]
    return pos


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "f32"])
@pytest.mark.parametrize("V", [4099, 128259])
def test_crafted_rows(V, dtype):
    """Rows built to break a selection: ascending (every element passes the running
    bound), descending, all equal, the winners on the first and last element of every
    slice of the split and on both sides of the vector / scalar-tail boundary, three finite
    entries, and winners that all tie. The buffer's row pitch is a multiple of 8 elements,
    so every row starts 16-byte aligned and the vector path with its tail is what runs."""
    g = torch.Generator().manual_seed(V)
    R = 7
    x = torch.randn(R, V, generator=g).clamp_(-3, 3)
    x[0] = torch.linspace(-8, 8, V)
    x[1] = torch.linspace(8, -8, V)
    x[2] = 1.5
    W = 8 if dtype == torch.bfloat16 else 4
    per = ((V + PARTS - 1) // PARTS + 7) & ~7 if V >= SP.ARGMAX_SPLIT_MIN_V else V
    last_lo = (V - 1) // per * per
    vec_end = last_lo + (V - last_lo) // W * W  # first element of the last slice's scalar tail
    assert vec_end < V
    pos = (_slice_edges(V) if V >= SP.ARGMAX_SPLIT_MIN_V else [0, V - 1, 2048, 2047]) + [vec_end - 1, vec_end]
    pos = list(dict.fromkeys(pos))
    extra = [p for p in torch.randperm(V, generator=g)[:40].tolist() if p not in pos]
    pos = (pos + extra)[:20]
    assert len(pos) == 20
    perm = torch.randperm(20, generator=g).tolist()
    for j, p in enumerate(pos):
        x[3, p] = 6.0 + 0.25 * perm[j]   # exact in bf16
    x[4] = -float("inf")
    x[4, [5, V // 2, V - 1]] = torch.tensor([0.5, 2.0, 0.5])
    tie = torch.randperm(V, generator=g)[:40]
    x[5, tie] = 7.0                       # 40 tie for 20 places: the 20 lowest ids
    x[6] = -float("inf")
    x[6, V - 2] = 1.0                     # a single finite entry
    wide = torch.zeros(R, (V + 7) & ~7, dtype=dtype, device=DEV)
    wide[:, :V] = x.to(dtype).to(DEV)
    xv = wide[:, :V]
    for T in (0.0, 0.7):
        temps = torch.full((R,), T, device=DEV)
        for K in (1, 5, 20):
            ids, lps = ops.top_logprobs(xv, temps, K)
            wi, wl = reference(xv, temps, list(range(R)), K)
            check(ids, lps, wi, wl, f"crafted V={V} {dtype} T={T} K={K}")
            gi = ids.cpu().numpy()
            if K == 20:
                assert sorted(gi[3].tolist()) == sorted(pos)
                assert gi[2].tolist() == list(range(20))
                assert gi[5].tolist() == sorted(tie.tolist())[:20]
                assert gi[4].tolist() == [V // 2, 5, V - 1] + [-1] * 17
                assert gi[6].tolist() == [V - 2] + [-1] * 19


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "f32"])
@pytest.mark.parametrize("V", [4099, 128256])
def test_greedy_entry_zero_is_argmax_logprob(V, dtype):
    x, _, _, _ = _case(V, dtype)
    xc = x.contiguous()
    tok, lp = ops.argmax_logprob(xc)
    ids, lps = ops.top_logprobs(xc, torch.zeros(xc.shape[0], device=DEV), 5)
    assert torch.equal(ids[:, 0], tok)
    err = float((lps[:, 0] - lp).abs().max())
    print(f"greedy consistency V={V} {dtype}: worst |lp - argmax lp| = {err:.3e}")
    assert err <= LP_TOL


def _three_calls(xs, temps, rows, outs, K):
    for x, t, r, (oi, ol) in zip(xs, temps, rows, outs):
        ops.top_logprobs(x, t, K, rows=r, out_ids=oi, out_lps=ol)


@pytest.mark.parametrize("V", [1000, 128256])
def test_rearm_and_graph_capture(V):
    """Three calls on one workspace with different data and different n (the per-row tickets
    must come back to zero after each), then the same three calls captured in one graph
    and replayed after every input was overwritten."""
    K = 20
    g = torch.Generator().manual_seed(9)
    ns = [5, 12, 3]
    xs = [(torch.randn(12, V, generator=g) * 2).to(torch.bfloat16).to(DEV) for _ in ns]
    temps = [torch.rand(12, generator=g).to(DEV) + 0.3 for _ in ns]
    rows = [torch.randperm(12, generator=g)[:n].to(torch.int32).to(DEV) for n in ns]
    outs = [(torch.empty(n, K, dtype=torch.int32, device=DEV), torch.empty(n, K, dtype=torch.float32, device=DEV))
            for n in ns]

    def verify(what):
        for x, t, r, (oi, ol) in zip(xs, temps, rows, outs):
            wi, wl = reference(x, t, r.tolist(), K)
            check(oi, ol, wi, wl, what)

    _three_calls(xs, temps, rows, outs, K)
    verify(f"eager V={V}")
    if V >= SP.ARGMAX_SPLIT_MIN_V:
        tickets = SP._TOPLP_WS[("cuda", torch.cuda.current_device())][-1][1]
        assert int(tickets.abs().sum()) == 0
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        _three_calls(xs, temps, rows, outs, K)
    for x, t, (oi, ol) in zip(xs, temps, outs):
        x.copy_((torch.randn(12, V, generator=g) * 2).to(torch.bfloat16))
        t.copy_(torch.rand(12, generator=g) + 0.3)
        oi.fill_(-7)
        ol.fill_(7.0)
    for r, n in zip(rows, ns):
        r.copy_(torch.randperm(12, generator=g)[:n].to(torch.int32))
    graph.replay()
    torch.cuda.synchronize()
    verify(f"replay 1 V={V}")
    graph.replay()
    torch.cuda.synchronize()
    verify(f"replay 2 V={V}")


def test_bad_arguments():
    x, temps, _, _ = _case(1000, torch.float32)
    for k in (0, 21):
        with pytest.raises(ValueError):
            ops.top_logprobs(x, temps, k)
