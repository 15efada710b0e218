"""The attention kernels on inputs whose answer is known exactly, and on random inputs with
bounds that scale with the row: prefill_attn2_kernel at every configuration of the
launcher's switch and at its own KS = 1 and KS = 2 choices, the 16-row prefill kernel,
decode_attention at every compiled (D, G) up to 64 splits, and decode_attention_fused,
whose attention must see the K/V row that its own prologue appends.

The older attention tests (test_kernels_gpu.py, test_paged_kv_gpu.py, test_fused_decode_gpu.py)
compare unit-normal inputs with atol = rtol = 2e-2, which one wrong key among a few hundred
passes. Here a mask that is off by one in either direction, a wrong page, kv head or
key-phase merge, or a stale read of the appended row changes the answer of every row by far
more than the bound. Inputs, float64 references, bounds and the sections' reasoning are in
tests/_attn_ref.py; tests/test_attn_refs_cpu.py holds the package's fp32 CPU paths to the
same bounds and shows that the checks refuse five planted errors.

Every launch reads Q as a strided view into a wider NaN-filled QKV row and writes `out` as
a row slice of a sentinel-filled buffer; rows past a sequence's end hold NaN / +Inf; the
prefill launches hold two sequences of qlen = 0 and run with max_q_len once exact and once
padded to the next multiple of 256.
"""
import pytest
import torch

import _attn_ref as A
from xgserve.ops import _native

pytestmark = pytest.mark.gpu
DEV = "cuda"

_PF_ALL = A.PF2_CFGS + [(8, 2, 128, 0)] + A.PF16_CFGS
# section 2: the first and last configuration of each kernel on every shape, the others on the long sequences
_PF_COUNT_FULL = {A.PF2_CFGS[0], A.PF2_CFGS[-1], A.PF16_CFGS[0], A.PF16_CFGS[-1]}
_DG_COUNT_FULL = {A.DG[0], A.DG[-1]}


@pytest.fixture(autouse=True, scope="module")
def _native_loaded():
    _native.kernels()  # fail loudly: the HIP library must be the one that runs
    torch.manual_seed(0)


# ---------------------------------------------------------------- 1. staircase
@pytest.mark.parametrize("pad", [False, True])
@pytest.mark.parametrize("bs", A.PF_BS)
@pytest.mark.parametrize("Hq,Hkv,D,gh", _PF_ALL)
def test_prefill_staircase(Hq, Hkv, D, gh, bs, pad):
    """gh = 0 on these 116 sequences is the launcher's KS = 1 choice."""
    A.run_prefill(DEV, "stair", A.prefill_shapes(), Hq, Hkv, D, gh, bs, pad)


@pytest.mark.parametrize("kind", ["stair", "count"])
@pytest.mark.parametrize("pad", [False, True])
@pytest.mark.parametrize("bs", A.PF_BS)
def test_prefill_own_choice_ks2(bs, pad, kind):
    """24 sequences: gh = 0 takes two key phases."""
    A.run_prefill(DEV, kind, A.PF_KS2, 8, 2, 128, 0, bs, pad)


@pytest.mark.parametrize("kind", ["stair", "count"])
@pytest.mark.parametrize("Hq,Hkv,D,gh", [(8, 2, 128, 0), (8, 2, 128, 2)])
def test_prefill_page_size_64(Hq, Hkv, D, gh, kind):
    A.run_prefill(DEV, kind, A.prefill_shapes(), Hq, Hkv, D, gh, 64, False)


@pytest.mark.parametrize("splits", A.DEC_SPLITS)
@pytest.mark.parametrize("bs", A.PF_BS)
@pytest.mark.parametrize("D,G", A.DG)
def test_decode_staircase(D, G, bs, splits):
    """The answer is V[L - 1] or V[0]; with the ascending sign every split but the last has an
    lse thousands of nats below the last one; at 64 splits most splits own no key."""
    A.run_decode(DEV, "stair", A.DEC_LENS, D, G, bs, splits)


# ---------------------------------------------------------------- 2. counted keys
@pytest.mark.parametrize("pad", [False, True])
@pytest.mark.parametrize("bs", A.PF_BS)
@pytest.mark.parametrize("Hq,Hkv,D,gh", _PF_ALL)
def test_prefill_counted_keys(Hq, Hkv, D, gh, bs, pad):
    full = (Hq, Hkv, D, gh) in _PF_COUNT_FULL or gh == 0
    A.run_prefill(DEV, "count", A.prefill_shapes(long_only=not full), Hq, Hkv, D, gh, bs, pad)


@pytest.mark.parametrize("splits", A.DEC_SPLITS)
@pytest.mark.parametrize("bs", A.PF_BS)
@pytest.mark.parametrize("D,G", A.DG)
def test_decode_counted_keys(D, G, bs, splits):
    lens = A.DEC_LENS if (D, G) in _DG_COUNT_FULL else A.DEC_LENS_LONG
    A.run_decode(DEV, "count", lens, D, G, bs, splits)


# ---------------------------------------------------------------- 3. the fused decode's own row
@pytest.mark.parametrize("G,S,depth,bs,splits,rope", A.FUSED_CASES)
def test_fused_decode_sees_its_own_row(G, S, depth, bs, splits, rope):
    """The cache rows at L - 1 and past it are NaN in K and V before the launch: attending to
    the stale row gives NaN, missing the new key gives some other V row."""
    A.run_fused(DEV, "own", G, S, depth, bs, splits, rope)


# ---------------------------------------------------------------- 4. random inputs, row-scaled bounds
@pytest.mark.parametrize("Hq,Hkv,D,gh,bs", A.RAND_PF)
def test_prefill_random(Hq, Hkv, D, gh, bs):
    A.run_prefill(DEV, "rand", (A.RAND_QLENS, A.RAND_CTXS), Hq, Hkv, D, gh, bs, False)


@pytest.mark.parametrize("splits", [1, 5])
@pytest.mark.parametrize("D,G,bs", A.RAND_DEC)
def test_decode_random(D, G, bs, splits):
    A.run_decode(DEV, "rand", A.DEC_LENS, D, G, bs, splits)


def test_fused_decode_random():
    G, S, depth, bs, splits, rope = A.RAND_FUSED
    A.run_fused(DEV, "rand", G, S, depth, bs, splits, rope)
