"""Every kernel that sums split-K partial slabs in its prologue or tail (the order that
csrc/kernels/partials.h defines), against an fp32 CPU loop that adds the slabs in slab order and
applies the site's own final step: the summed values are compared bit for bit, derived
quantities (norm outputs, block-reduced sums of squares) with the project's tolerances.
Output buffers start as NaN, so an element the kernel does not write fails."""
import pytest
import torch
import torch.nn.functional as F

from xgserve import ops
from xgserve.ops import _native
from xgserve.ops import linear as lin
from xgserve.ops._native import stream_ptr
from xgserve.ops.linear import MODE_PARTIAL, MODE_SILU, PendingSum, ResidWorkspace, interleave_gate_up

pytestmark = pytest.mark.gpu
DEV = "cuda"
NORM = dict(atol=3e-2, rtol=3e-2)  # norm outputs, as tests/test_skinny_gpu.py
SS = dict(rtol=1e-4, atol=1e-2)    # sums of squares, as tests/test_custom_ar_gpu.py
S_ALL = [1, 2, 3, 4, 5, 8, 9]      # the specialised counts and the runtime loop


@pytest.fixture(autouse=True, scope="module")
def _k():
    _native.kernels()


def _gen(*key):
    g = torch.Generator()
    g.manual_seed(sum(int(v) * 1000003 ** i for i, v in enumerate(key)) % (1 << 31))
    return g


def _slab_sum(part, init=None):
    """fp32, slab order: ((init + part[0]) + part[1]) + ..."""
    a = torch.zeros_like(part[0]) if init is None else init.clone()
    for s in range(part.shape[0]):
        a = a + part[s]
    return a


def _nan(*shape, dtype):
    return torch.full(shape, float("nan"), dtype=dtype, device=DEV)


# ---------------------------------------------------------------- 1. add_partials_rmsnorm
def run_add_partials_rmsnorm(H, S, T=3):
    g = _gen(1, H, S)
    part = torch.randn(S, T, H, generator=g)
    res0 = torch.randn(T, H, generator=g).bfloat16()
    w = (torch.rand(H, generator=g) + 0.5).bfloat16()
    want = _slab_sum(part, res0.float()).bfloat16()
    res = res0.to(DEV)
    y, r = ops.fused_add_rmsnorm(PendingSum(part.to(DEV), S), res, w.to(DEV), 1e-5, out=_nan(T, H, dtype=torch.bfloat16))
    return dict(resid=r.cpu(), y=y.cpu()), dict(resid=want, y=ops.rmsnorm_ref(want, w, 1e-5))


@pytest.mark.parametrize("H", [512, 2048, 4096, 8192, 16384])
@pytest.mark.parametrize("S", S_ALL)
def test_add_partials_rmsnorm(H, S):
    got, want = run_add_partials_rmsnorm(H, S)
    assert torch.equal(got["resid"], want["resid"])
    torch.testing.assert_close(got["y"].float(), want["y"].float(), **NORM)


# ---------------------------------------------------------------- 2. add_partials_resid
def run_add_partials_resid(T, H, S):
    g = _gen(2, T, H, S)
    part = torch.randn(S, T, H, generator=g)
    res0 = torch.randn(T, H, generator=g).bfloat16()
    want = _slab_sum(part, res0.float()).bfloat16()
    want_ss = want.float().view(T, H // 1024, 1024).pow(2).sum(-1).t().contiguous()  # [chunk, T]
    res, ss = res0.to(DEV), _nan(H // 1024, T, dtype=torch.float32)
    _native.kernels().add_partials_resid(part.to(DEV).data_ptr(), S, T, res.data_ptr(), ss.data_ptr(), H, stream_ptr())
    return dict(resid=res.cpu(), ss=ss.cpu()), dict(resid=want, ss=want_ss)


@pytest.mark.parametrize("T", [1, 5])
@pytest.mark.parametrize("H", [1024, 4096])
@pytest.mark.parametrize("S", S_ALL)
def test_add_partials_resid(T, H, S):
    got, want = run_add_partials_resid(T, H, S)
    assert torch.equal(got["resid"], want["resid"])
    torch.testing.assert_close(got["ss"], want["ss"], **SS)


# ---------------------------------------------------------------- 3. PendingSum.materialize
def run_materialize(M, N, S):
    part = torch.randn(S, M, N, generator=_gen(3, M, N, S))
    return dict(out=PendingSum(part.to(DEV), S).materialize().cpu()), dict(out=_slab_sum(part).bfloat16())


# [64, 40000]: more float4s than the 2048 x 256 threads of the capped grid (the grid-stride loop)
@pytest.mark.parametrize("M,N,S", [(3, 1028, S) for S in (1, 2, 3, 8, 9)] + [(64, 40000, 3)])
def test_materialize(M, N, S):
    got, want = run_materialize(M, N, S)
    assert torch.equal(got["out"], want["out"])


# ---------------------------------------------------------------- 4. / 5. moe_combine(_resid)
def _fma32(a, b, c):
    """fl32(a * b + c) for fp32 a, b, c: the product of two fp32 values is exact in
    fp64, so one fp64 add and one rounding to fp32 is the fused multiply-add."""
    return (a.double() * b.double() + c.double()).float()


def _combine_ref(rows, dest, w, T, k, H):
    """acc += wt * f per choice in order, skipping dest < 0. The compiler contracts that
    line of combine_kernel / combine_resid_kernel into v_fma_f32 / v_fmac_f32 (hipcc's
    default -ffp-contract=fast), so the reference uses the same fused multiply-add."""
    acc = torch.zeros(T, H)
    for t in range(T):
        for j in range(k):
            p = int(dest[t * k + j])
            if p >= 0:
                acc[t] = _fma32(w[t * k + j].expand(H), rows[p], acc[t])
    return acc


def _moe_inputs(key, S, T, k, H):
    g = _gen(*key)
    P = T * k + 3
    dest = torch.randperm(P, generator=g)[:T * k].int()
    dest[1::4] = -1  # another rank's expert
    w = torch.rand(T * k, generator=g) + 0.1
    if S == 0:  # bf16 rows, no slabs
        y = torch.randn(P, H, generator=g).bfloat16()
        rows = y.float()
    else:
        y = torch.randn(S, P, H, generator=g)
        rows = _slab_sum(y)
    return g, P, dest, w, y, rows


def run_moe_combine(S, out_f32, H, T=5, k=2):
    g, P, dest, w, y, rows = _moe_inputs((4, S, H), S, T, k, H)
    want = _combine_ref(rows, dest, w, T, k, H)
    out = _nan(T, H, dtype=torch.float32 if out_f32 else torch.bfloat16)
    yd, dd, wd = y.to(DEV), dest.to(DEV), w.to(DEV)
    _native.kernels().moe_combine(yd.data_ptr(), S, P, dd.data_ptr(), wd.data_ptr(), out.data_ptr(), T, k, H,
                                  stream_ptr(), int(out_f32))
    return dict(out=out.cpu()), dict(out=want if out_f32 else want.bfloat16())


@pytest.mark.parametrize("S", [0, 1, 2, 4])
@pytest.mark.parametrize("out_f32", [False, True])
@pytest.mark.parametrize("H", [256, 4096])
def test_moe_combine(S, out_f32, H):
    got, want = run_moe_combine(S, out_f32, H)
    assert torch.equal(got["out"], want["out"])


def test_moe_combine_rejects_other_split_counts():
    T, k, H, S = 5, 2, 256, 3
    g, P, dest, w, y, _ = _moe_inputs((4, S, H), S, T, k, H)
    out = _nan(T, H, dtype=torch.float32)
    yd, dd, wd = y.to(DEV), dest.to(DEV), w.to(DEV)
    with pytest.raises(ValueError):
        _native.kernels().moe_combine(yd.data_ptr(), S, P, dd.data_ptr(), wd.data_ptr(), out.data_ptr(), T, k, H,
                                      stream_ptr(), 1)
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all())


def run_moe_combine_resid(S, H, T, k=2):
    g, P, dest, w, y, rows = _moe_inputs((5, S, H, T), S, T, k, H)
    res0 = torch.randn(T, H, generator=g).bfloat16()
    want = (res0.float() + _combine_ref(rows, dest, w, T, k, H)).bfloat16()
    want_ss = want.float().view(T, H // 1024, 1024).pow(2).sum(-1).t().contiguous()
    res, ss = res0.to(DEV), _nan(H // 1024, T, dtype=torch.float32)
    yd, dd, wd = y.to(DEV), dest.to(DEV), w.to(DEV)
    _native.kernels().moe_combine_resid(yd.data_ptr(), S, P, dd.data_ptr(), wd.data_ptr(), res.data_ptr(),
                                        ss.data_ptr(), T, k, H, stream_ptr())
    return dict(resid=res.cpu(), ss=ss.cpu()), dict(resid=want, ss=want_ss)


@pytest.mark.parametrize("S", [1, 2, 4])
@pytest.mark.parametrize("H", [1024, 8192])
@pytest.mark.parametrize("T", [1, 5])
def test_moe_combine_resid(S, H, T):
    got, want = run_moe_combine_resid(S, H, T)
    assert torch.equal(got["resid"], want["resid"])
    torch.testing.assert_close(got["ss"], want["ss"], **SS)


@pytest.mark.parametrize("S", [3, 8])
def test_moe_combine_resid_rejects_other_split_counts(S):
    T, k, H = 5, 2, 1024
    g, P, dest, w, y, _ = _moe_inputs((5, S, H, T), S, T, k, H)
    res0 = torch.randn(T, H, generator=g).bfloat16()
    res, ss = res0.to(DEV), _nan(H // 1024, T, dtype=torch.float32)
    yd, dd, wd = y.to(DEV), dest.to(DEV), w.to(DEV)
    with pytest.raises(ValueError):
        _native.kernels().moe_combine_resid(yd.data_ptr(), S, P, dd.data_ptr(), wd.data_ptr(), res.data_ptr(),
                                            ss.data_ptr(), T, k, H, stream_ptr())
    torch.cuda.synchronize()
    assert torch.equal(res.cpu(), res0) and bool(torch.isnan(ss).all())


# ---------------------------------------------------------------- 6. gemm_m64g GG_RESID tail
RESID_N, RESID_K = 1024, 2304
# (nw, cfg): 4 waves x 32 columns = a 128-column tile; cfg 7 = the 8-wave tile, 256 columns
RESID_TILES = [(2, 1), (2, 7)]


def run_m64_resid(M, S, nw, cfg, monkeypatch):
    """S = 1: the LDS-staged tile; 2, 3: one batch of 4 (3: clamped tail); 5, 8: one batch
    of 8; 9: two batches of 4 and a tail. The slabs come from the same GEMM template in
    MODE_PARTIAL, so the reference differs from the kernel only in who adds them."""
    monkeypatch.setattr(lin, "RESID_INLAUNCH_MAX_BYTES", 1 << 30)
    N, K = RESID_N, RESID_K
    g = _gen(6, M, S, nw, cfg)
    x = torch.randn(M, K, generator=g).bfloat16().to(DEV)
    w = (torch.randn(N, K, generator=g) * 0.02).bfloat16().to(DEV)
    r0 = torch.randn(M, N, generator=g).bfloat16()
    part = lin.m64_linear(x, w, MODE_PARTIAL, split_k=S, nw=nw, cfg=cfg).part.cpu()
    assert part.shape[0] == S
    want = (_slab_sum(part) + r0.float()).bfloat16()
    cols = 16 * nw * lin.M64G_CFGS[cfg][0]
    want_ss = want.float().view(M, N // cols, cols).pow(2).sum(-1).t().contiguous()  # [tile, M]
    ws = ResidWorkspace(2, 64, N, DEV)
    ws.ss.fill_(float("nan"))
    r = r0.to(DEV)
    st = lin.m64_resid_linear(x, w, r, ws, 1, 1e-5, plan=(nw, S, cfg))
    torch.cuda.synchronize()
    assert st.n == N // cols and st.stride == M  # reduced in the launch, one sum per column tile
    ss = st.ss.reshape(-1)[: st.n * st.stride].view(st.n, st.stride).cpu()
    return dict(resid=r.cpu(), ss=ss, counters=ws.counters.cpu()), dict(resid=want, ss=want_ss)


@pytest.mark.parametrize("M", [1, 17, 64])
@pytest.mark.parametrize("S", [1, 2, 3, 5, 8, 9])
@pytest.mark.parametrize("nw,cfg", RESID_TILES)
def test_m64_resid_tail(M, S, nw, cfg, monkeypatch):
    got, want = run_m64_resid(M, S, nw, cfg, monkeypatch)
    assert torch.equal(got["resid"], want["resid"])
    torch.testing.assert_close(got["ss"], want["ss"], **SS)
    assert int(got["counters"].abs().sum()) == 0


# ---------------------------------------------------------------- 7. gemm_m64g split-K SiLU tail
def run_m64_silu(M, S, cfg):
    K, F2 = 2304, 1024
    g = _gen(7, M, S, cfg)
    x = torch.randn(M, K, generator=g).bfloat16().to(DEV)
    gate = (torch.randn(F2 // 2, K, generator=g) * 0.02).bfloat16().to(DEV)
    up = (torch.randn(F2 // 2, K, generator=g) * 0.02).bfloat16().to(DEV)
    w = interleave_gate_up(gate, up)
    ref = F.silu(x.float() @ gate.float().t()) * (x.float() @ up.float().t())
    assert lin._m64_valid(F2, K, MODE_SILU, 2, S, cfg, M)
    lin._M64_TUNED[(F2, K, MODE_SILU)] = {64: (2, S, cfg), 32: (2, S, cfg), 16: (2, S, cfg)}
    try:
        y = lin.m64_linear(x, w, MODE_SILU)
    finally:
        del lin._M64_TUNED[(F2, K, MODE_SILU)]
    torch.cuda.synchronize()
    return dict(y=y.cpu(), counters=lin.tile_counters(x.device, F2).cpu()), dict(y=ref.cpu())


@pytest.mark.parametrize("M", [17, 64])
@pytest.mark.parametrize("S", [3, 9])
@pytest.mark.parametrize("cfg", [1, 7])
def test_m64_silu_tail(M, S, cfg):
    got, want = run_m64_silu(M, S, cfg)
    rel = float((got["y"].float() - want["y"]).norm() / want["y"].norm().clamp_min(1e-6))
    assert rel < 1e-2  # tests/test_fused_decode_gpu.py test_split_silu_and_wide_tile
    assert int(got["counters"].abs().sum()) == 0
