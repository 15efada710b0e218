"""dequant_w8 (csrc/kernels/dequant.hip) on the MI355X: the bf16 weight it writes from
fp8 / int8 / int4 codes is bit-identical to dequantize_weight(...).to(bfloat16) -- for
quantizer output at small, odd and real shapes, for every code value, inside the
bounds of a larger scratch -- and the wrapper rejects what the kernel cannot take."""
import pytest
import torch

from xgserve.ops import _native
from xgserve.ops.linear import (WQ_FP8, WQ_INT4, WQ_INT8, dequantize_into, dequantize_weight, quantize_weight)

pytestmark = pytest.mark.gpu
DEV = "cuda"
FMTS = [WQ_FP8, WQ_INT8, WQ_INT4]


@pytest.fixture(autouse=True, scope="module")
def _k():
    _native.kernels()  # fail loudly: the HIP library must be the one that runs
    torch.manual_seed(0)


def _bits(t):
    return t.view(torch.int16)


def _exact(q, s, fmt, out=None):
    got = dequantize_into(q, s, fmt, out=out)
    ref = dequantize_weight(q, s, fmt).to(torch.bfloat16)
    assert got.dtype == torch.bfloat16 and got.shape == ref.shape and got.is_contiguous()
    assert torch.equal(got, ref)
    assert torch.equal(_bits(got), _bits(ref))  # (-0 and +0 told apart too)
    return got


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("N,K", [(1, 128), (3, 256), (65, 384), (1024, 512), (4096, 14336)])
def test_dequant_matches_quantizer(fmt, N, K):
    q, s = quantize_weight(torch.randn(N, K, device=DEV) * 0.02, fmt)
    _exact(q, s, fmt)


def test_dequant_every_int8_code():
    q = torch.arange(256, device=DEV, dtype=torch.uint8)[:, None].repeat(1, 128).contiguous()  # row r = byte r
    s = torch.rand(256, device=DEV) * 0.01 + 1e-4
    w = _exact(q, s, WQ_INT8)
    assert float(w[128, 0]) < 0 and float(w[127, 0]) > 0  # byte 128 is -128


def test_dequant_every_int4_code():
    # row r, word position p (0..7), nibble value v: 16 x 8 rows put v at position p of
    # every word and a position-dependent other value elsewhere; two 128-k groups with
    # different scales
    rows = []
    for v in range(16):
        for p in range(8):
            nib = [(v + 3 * (j + 1)) % 16 for j in range(8)]
            nib[p] = v
            word = 0
            for j, u in enumerate(nib):  # nibble index j holds bits 4j..4j+3
                word |= u << (4 * j)
            rows.append(word)
    word = torch.tensor(rows, dtype=torch.int64)
    word = torch.where(word >= 2 ** 31, word - 2 ** 32, word).to(torch.int32)  # the same 32 bits
    N, K = word.numel(), 256
    q = word[:, None].repeat(1, K // 8).contiguous().view(torch.uint8).view(N, K // 2).to(DEV)
    s = (torch.rand(K // 128, N, device=DEV) * 0.01 + 1e-4)
    s[1] *= 3.0
    w = _exact(q, s, WQ_INT4)
    assert w.unique().numel() > 16  # both groups' scales were applied


def test_dequant_every_fp8_code():
    codes = torch.tensor([b for b in range(256) if b not in (0x7F, 0xFF)], dtype=torch.uint8)  # no NaN encodings
    N, K = 8, 256
    q = torch.cat([codes, codes.flip(0)[:2]]).repeat(N * K // 256).view(N, K).contiguous().to(DEV)
    assert set(q.flatten().tolist()) == set(codes.tolist())
    s = torch.rand(N, device=DEV) * 0.01 + 1e-4
    _exact(q, s, WQ_FP8)


@pytest.mark.parametrize("fmt", FMTS)
def test_dequant_writes_stay_inside_out(fmt):
    N, K, TAIL = 65, 384, 4096
    q, s = quantize_weight(torch.randn(N, K, device=DEV) * 0.02, fmt)
    buf = torch.full((N * K + TAIL,), -7.0, dtype=torch.bfloat16, device=DEV)
    w = _exact(q, s, fmt, out=buf)
    assert w.data_ptr() == buf.data_ptr() and tuple(w.shape) == (N, K)
    assert bool((buf[N * K:] == -7.0).all())


@pytest.mark.parametrize("fmt", FMTS)
def test_dequant_wrapper_contract(fmt):
    with pytest.raises(ValueError):  # K % 128 != 0
        kq = 192 // 2 if fmt == WQ_INT4 else 192
        dequantize_into(torch.zeros(4, kq, dtype=torch.uint8, device=DEV),
                        torch.ones(4, dtype=torch.float32, device=DEV), fmt)
    q, s = quantize_weight(torch.randn(4, 256, device=DEV) * 0.02, fmt)
    with pytest.raises(ValueError):  # a wrong scale size
        dequantize_into(q, torch.ones(s.numel() + 1, dtype=torch.float32, device=DEV), fmt)
    with pytest.raises(ValueError):  # an undersized out
        dequantize_into(q, s, fmt, out=torch.empty(4 * 256 - 1, dtype=torch.bfloat16, device=DEV))
