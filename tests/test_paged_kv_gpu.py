"""The decode half of the paged-KV path -- rope_cache, rope_cache_partials,
decode_attention and the fused-QKV decode_attention_fused -- at every compiled
(D, G) instantiation, at page sizes other than 16 (a non-power-of-two one
included), above 16 key splits and at every QKV partial count with a clamped
tail, plus the 16-row prefill kernel at those page sizes.

Every comparison is against a plain high-precision PyTorch computation on the
CPU, never against another HIP kernel:
  * attention: the fp32 ops.decode_attention_ref / ops.prefill_attention_ref
    (they slice the gathered cache to [:L], so rows past a sequence's end never
    enter them), atol = rtol = 2e-2 on the bf16 outputs (one wrong key among a few
    hundred passes that: tests/test_attn_exact_gpu.py holds the one-key checks);
  * RoPE + KV append: the fp32 partials summed in float64, rotated in float64 with
    the build_cos_sin table and rounded once to bf16. The kernels sum in fp32 in
    another order (error <= S * 2^-24 of the largest partial) and round once too,
    so a value may land one bf16 step away, never further: rtol = 2^-7, atol = 1e-5;
  * every cache row that slot_mapping does not name must keep its 16-bit pattern.
"""
import math
from dataclasses import replace

import pytest
import torch

from xgserve import ops
from xgserve.ops import _native
from xgserve.ops.attention import DecodeWorkspace
from xgserve.ops.linear import PendingSum

pytestmark = pytest.mark.gpu
DEV = "cuda"
ATT = dict(atol=2e-2, rtol=2e-2)
ULP = dict(atol=1e-5, rtol=2.0 ** -7)
NAN, INF = float("nan"), float("inf")
# every (D, G) pair decode_attention compiles; the fused form: D = 128, G in 1, 2, 4, 8
DG = [(128, 1), (128, 2), (128, 4), (128, 8), (128, 16), (64, 1), (64, 2), (64, 4), (64, 8)]


@pytest.fixture(autouse=True, scope="module")
def _native_loaded():
    _native.kernels()  # fail loudly: the HIP library must be the one that runs
    torch.manual_seed(0)


def rnd(*shape, scale=1.0):
    return (torch.randn(*shape, device=DEV) * scale).bfloat16()


def _paged(lens, Hkv, D, bs, extra_pages=8):
    """Random caches and a shuffled block table; a zero-length row still owns one page."""
    pages_per = [(max(1, L) + bs - 1) // bs for L in lens]
    NB = sum(pages_per) + extra_pages
    kc, vc = rnd(NB, Hkv, bs, D), rnd(NB, Hkv, bs, D)
    perm = torch.randperm(NB).tolist()
    bt = torch.zeros(len(lens), max(pages_per), dtype=torch.int32)
    i = 0
    for s, n in enumerate(pages_per):
        bt[s, :n] = torch.tensor(perm[i:i + n])
        i += n
    return kc, vc, bt.to(DEV)


def _poison_past_end(kc, vc, bt, lens, bs):
    """K rows past each sequence's end -> NaN, V rows -> +Inf (its last, partly filled page)."""
    n = 0
    for b, L in enumerate(lens):
        if L > 0 and L % bs:
            pg = int(bt[b, (L - 1) // bs])
            kc[pg, :, L % bs:] = NAN
            vc[pg, :, L % bs:] = INF
            n += 1
    assert n > 0


def _q_view(B, Hq, Hkv, D):
    """q as a strided view into a wider QKV row, like the engine passes it."""
    qkv = rnd(B, (Hq + 2 * Hkv) * D)
    return qkv[:, :Hq * D].view(B, Hq, D)


def _i32(x):
    return torch.tensor(x, dtype=torch.int32, device=DEV)


def _check_decode(q, kc, vc, bt, lens, scale, splits, ws=None):
    sl = _i32(lens)
    out = ops.decode_attention(q, kc, vc, bt, sl, scale, num_splits=splits, workspace=ws)
    ref = ops.decode_attention_ref(q.cpu(), kc.cpu(), vc.cpu(), bt.cpu(), sl.cpu(), scale)
    assert torch.isfinite(ref.float()).all()
    torch.testing.assert_close(out.cpu().float(), ref.float(), **ATT)
    return out


# ---- 1. every compiled decode instantiation

@pytest.mark.parametrize("D,G", DG)
@pytest.mark.parametrize("bs", [16, 48])
@pytest.mark.parametrize("splits", [1, 5])
def test_decode_every_instantiation(D, G, bs, splits):
    """One key, the 16-key tile edges, the edge of one full pass of 4 waves x 2
    register tiles (128 keys), a long row and a zero-length row (output exactly 0)."""
    Hkv = 2
    Hq = Hkv * G
    lens = [1, 15, 16, 17, 127, 128, 129, 333, 0]
    kc, vc, bt = _paged(lens, Hkv, D, bs)
    q = _q_view(len(lens), Hq, Hkv, D)
    out = _check_decode(q, kc, vc, bt, lens, 1.0 / math.sqrt(D), splits)
    assert out[-1].float().abs().max().item() == 0.0


# ---- 2. page sizes

@pytest.mark.parametrize("Hq,Hkv,D", [(32, 8, 128), (12, 12, 64)])
@pytest.mark.parametrize("bs", [16, 32, 48, 64])
@pytest.mark.parametrize("splits", [1, 3])
def test_decode_page_sizes(Hq, Hkv, D, bs, splits):
    lens = [bs - 1, bs, bs + 1, 2 * bs + 5, 300]
    kc, vc, bt = _paged(lens, Hkv, D, bs)
    q = _q_view(len(lens), Hq, Hkv, D)
    _check_decode(q, kc, vc, bt, lens, 1.0 / math.sqrt(D), splits)


# ---- 3. more than 16 splits: combine_splits' second batch and its rescale

@pytest.mark.parametrize("splits", [17, 32, 64])
def test_decode_more_than_16_splits(splits):
    """Twice on one workspace; a split past a sequence's tiles must publish lse = -inf
    (at 64 splits and 1100 keys: 69 tiles, two per split, splits 35.. empty)."""
    Hq, Hkv, D, bs = 32, 8, 128, 16
    lens = [1, 40, 1100]
    B = len(lens)
    kc, vc, bt = _paged(lens, Hkv, D, bs)
    q = _q_view(B, Hq, Hkv, D)
    ws = DecodeWorkspace(B, Hq, D, splits, DEV)
    ws.part_out.fill_(NAN)  # every (row, head, split) entry must be written, the empty ones too
    ws.part_lse.fill_(NAN)
    for _ in range(2):
        _check_decode(q, kc, vc, bt, lens, 1.0 / math.sqrt(D), splits, ws)
    lse = ws.part_lse[:B * Hq * splits].view(B, Hq, splits).cpu()
    for b, L in enumerate(lens):
        ntiles = (L + 15) // 16
        tps = (ntiles + splits - 1) // splits
        empty = torch.arange(splits) * tps >= ntiles
        assert torch.isfinite(lse[b][:, ~empty]).all()
        assert (lse[b][:, empty] == -INF).all()
    if splits == 64:
        assert empty.nonzero().flatten().tolist() == list(range(35, 64))  # the 1100-key row
    assert torch.isfinite(ws.part_out[:B * Hq * splits * D]).all()


# ---- 4. rescale spike

def _spike_case(Hq, Hkv, D, bs=16, L=1100):
    """Keys 3, 40 and 700 aligned with the queries at 4x, 6x, 8x: the running max
    jumps twice, so the output is the V row of key 700 to bf16. The G heads of a
    group are one direction at different lengths, so each of them sees the spike."""
    G = Hq // Hkv
    kc, vc, bt = _paged([L], Hkv, D, bs)
    base = rnd(1, Hkv, 1, D)
    q = (base.float() * (1.0 + 0.25 * torch.arange(G, device=DEV).view(1, 1, G, 1) / G)).bfloat16().view(1, Hq, D)
    for key, f in ((3, 4.0), (40, 6.0), (700, 8.0)):
        kc[int(bt[0, key // bs]), :, key % bs] = (base[0, :, 0].float() * f).bfloat16()
    return q.contiguous(), kc, vc, bt


@pytest.mark.parametrize("Hq,Hkv,D", [(8, 8, 128), (16, 2, 128), (4, 2, 64)])
@pytest.mark.parametrize("splits", [1, 4, 64])
def test_decode_spike_forces_rescale(Hq, Hkv, D, splits):
    """A missed rescale inside a wave, in the four-wave merge or in combine_splits
    (at 64 splits the keys sit in splits 0, 1 and 21: across a combine batch) leaves
    an O(1) error."""
    q, kc, vc, bt = _spike_case(Hq, Hkv, D)
    out = _check_decode(q, kc, vc, bt, [1100], 0.088, splits)
    G = Hq // Hkv
    v700 = vc[int(bt[0, 700 // 16]), :, 700 % 16].float().repeat_interleave(G, dim=0)
    torch.testing.assert_close(out[0].float(), v700, **ATT)


# ---- 5. rows past the end never reach the output

@pytest.mark.parametrize("D,G", [(128, 4), (128, 8), (64, 1), (64, 4)])
@pytest.mark.parametrize("bs", [16, 32, 48])
@pytest.mark.parametrize("splits", [1, 3])
def test_decode_poison_past_end(D, G, bs, splits):
    """Pages are recycled without clearing: NaN keys and Inf values past L in the last
    page have probability exactly 0 and must not reach the output (0 * Inf = NaN)."""
    Hkv = 2
    lens = [1, 17, 37, 129]
    kc, vc, bt = _paged(lens, Hkv, D, bs, extra_pages=0)
    _poison_past_end(kc, vc, bt, lens, bs)
    q = _q_view(len(lens), Hkv * G, Hkv, D)
    _check_decode(q, kc, vc, bt, lens, 1.0 / math.sqrt(D), splits)


# ---- float64 reference of the QKV reduce + RoPE + KV append

def _rotate64(x, cs_rows):
    h = x.shape[-1] // 2
    cos, sin = cs_rows[:, None, :h], cs_rows[:, None, h:]
    x1, x2 = x[..., :h], x[..., h:]
    return torch.cat([x1 * cos - x2 * sin, x2 * cos + x1 * sin], dim=-1)


def _qkv_ref(rows64, pos, cs, Hq, Hkv, D, rope):
    """rows64 [T, >= (Hq + 2 Hkv) D] float64 -> bf16 q [T, Hq, D], k, v [T, Hkv, D]: rounded once."""
    T = rows64.shape[0]
    q = rows64[:, :Hq * D].reshape(T, Hq, D)
    k = rows64[:, Hq * D:(Hq + Hkv) * D].reshape(T, Hkv, D)
    v = rows64[:, (Hq + Hkv) * D:(Hq + 2 * Hkv) * D].reshape(T, Hkv, D)
    if rope:
        rows = cs.cpu().double()[pos.cpu().long()]
        q, k = _rotate64(q, rows), _rotate64(k, rows)
    return q.bfloat16(), k.bfloat16(), v.bfloat16()


def _append(kc, vc, k, v, slots, bs):
    """The reference cache update on CPU copies: row slots[t] <- k[t], v[t]."""
    kc, vc = kc.cpu().clone(), vc.cpu().clone()
    for t, s in enumerate(slots.cpu().tolist()):
        if s >= 0:
            kc[s // bs, :, s % bs] = k[t]
            vc[s // bs, :, s % bs] = v[t]
    return kc, vc


def _rows(cache, slots, bs):
    """[n, Hkv, D]: the cache rows named by the valid slots, in order."""
    s = slots.cpu()[slots.cpu() >= 0].long()
    return cache.cpu()[s // bs, :, s % bs]


def _assert_untouched(after, before, slots, bs):
    """Every row not named by slot_mapping >= 0 keeps its raw 16-bit pattern."""
    keep = torch.ones(after.shape[0], bs, dtype=torch.bool)
    s = slots.cpu()[slots.cpu() >= 0].long()
    keep[s // bs, s % bs] = False
    a = after.cpu().view(torch.int16).permute(0, 2, 1, 3)[keep]
    b = before.cpu().view(torch.int16).permute(0, 2, 1, 3)[keep]
    assert torch.equal(a, b)


def _check_appended(kc, vc, kc0, vc0, k_ref, v_ref, slots, bs, v_exact=False):
    valid = (slots.cpu() >= 0)
    torch.testing.assert_close(_rows(kc, slots, bs).float(), k_ref[valid].float(), **ULP)
    if v_exact:
        assert torch.equal(_rows(vc, slots, bs).view(torch.int16), v_ref[valid].view(torch.int16))
    else:
        torch.testing.assert_close(_rows(vc, slots, bs).float(), v_ref[valid].float(), **ULP)
    _assert_untouched(kc, kc0, slots, bs)
    _assert_untouched(vc, vc0, slots, bs)


# ---- 5 (fused form) and 6: the fused prologue against the float64 reference

def _fused_case(G, S, depth, bs, splits, lens, rope=True, poison=False, Hkv=2):
    D = 128
    Hq = Hkv * G
    B = len(lens)
    kc, vc, bt = _paged(lens, Hkv, D, bs, extra_pages=0 if poison else 8)
    if poison:  # before the call: the row at L - 1 is then written by the kernel itself
        _poison_past_end(kc, vc, bt, lens, bs)
    part = torch.randn(S, B, (Hq + 2 * Hkv) * D, device=DEV) * 0.3
    pos = _i32([max(0, L - 1) for L in lens])
    slots = _i32([int(bt[b, (L - 1) // bs]) * bs + (L - 1) % bs if L > 0 else -1 for b, L in enumerate(lens)])
    sl = _i32(lens)
    cs = ops.build_cos_sin(D, 512, 500000.0, device=DEV)
    scale = 1.0 / math.sqrt(D)
    kc0, vc0 = kc.clone(), vc.clone()
    ws = DecodeWorkspace(B, Hq, D, splits, DEV)
    out = ops.decode_attention_fused(PendingSum(part, S), pos, slots, cs, kc, vc, bt, sl, Hq, scale, splits,
                                     workspace=ws, apply_rope=rope, depth=depth)
    q_ref, k_ref, v_ref = _qkv_ref(part.double().sum(0).cpu(), pos, cs, Hq, Hkv, D, rope)
    kc_ref, vc_ref = _append(kc0, vc0, k_ref, v_ref, slots, bs)
    ref = ops.decode_attention_ref(q_ref, kc_ref, vc_ref, bt.cpu(), sl.cpu(), scale)
    assert torch.isfinite(ref.float()).all()
    torch.testing.assert_close(out.view(B, Hq, D).cpu().float(), ref.float(), **ATT)
    _check_appended(kc, vc, kc0, vc0, k_ref, v_ref, slots, bs)
    for b, L in enumerate(lens):
        if L == 0:
            assert out[b].float().abs().max().item() == 0.0


@pytest.mark.parametrize("G", [4, 8])
@pytest.mark.parametrize("depth", [2, 4])
@pytest.mark.parametrize("bs", [16, 32, 48])
@pytest.mark.parametrize("splits", [1, 3])
def test_fused_decode_poison_past_end(G, depth, bs, splits):
    """Poisoned before the call; the row at L - 1 is written by the kernel's own prologue,
    which the clamped V loads of the last tile must then see."""
    _fused_case(G, 4, depth, bs, splits, [1, 17, 37, 129], poison=True)


_GS, _SS, _DEPTHS, _BSS = [1, 2, 4, 8], [2, 3, 5, 7, 9, 16], [2, 3, 4], [16, 32, 48]
# half of the G x S x depth product (36 cases): every (G, S) pair and every (S, depth)
# pair occurs; the page size moves with G and the depth, the split count with S
_FUSED_CASES = [(G, S, dp, _BSS[(ig + idp) % 3], (1, 3)[(i_s + idp) % 2])
                for ig, G in enumerate(_GS) for i_s, S in enumerate(_SS) for idp, dp in enumerate(_DEPTHS)
                if (ig + i_s + idp) % 2 == 0]


@pytest.mark.parametrize("G,S,depth,bs,splits", _FUSED_CASES)
def test_fused_prologue_float64_reference(G, S, depth, bs, splits):
    """S <= 8 at depth 2 / 3: the split prologue; S > 8 or depth 4: the classic one;
    both have clamped tails at S = 3, 5, 7, 9. Row 3 is a padding row (no KV write, no
    attention); row 2's new key is the first of a fresh page."""
    _fused_case(G, S, depth, bs, splits, [1, bs, bs + 1, 0, 2 * bs + 5, 300])


@pytest.mark.parametrize("G,S,depth,bs,splits", [(4, 3, 2, 48, 3), (2, 9, 2, 32, 1)])
def test_fused_prologue_no_rope(G, S, depth, bs, splits):
    _fused_case(G, S, depth, bs, splits, [1, bs, bs + 1, 0, 2 * bs + 5, 300], rope=False)


# ---- 7. rope_cache and rope_cache_partials against the float64 reference

T_ROPE, MAX_POS = 37, 512


def _rope_inputs(Hkv, D, bs):
    NB = 8
    pos = torch.randint(0, MAX_POS, (T_ROPE,), dtype=torch.int32)
    pos[0], pos[1] = 0, MAX_POS - 1
    slots = torch.randperm(NB * bs)[:T_ROPE].to(torch.int32)
    slots[3] = slots[20] = -1
    cs = ops.build_cos_sin(D, MAX_POS, 500000.0, device=DEV)
    return pos.to(DEV), slots.to(DEV), cs, rnd(NB, Hkv, bs, D), rnd(NB, Hkv, bs, D)


_ROPE_SHAPES = [(D, bs, Hq, Hkv) for D in (64, 128) for bs in (16, 32, 48) for Hq, Hkv in ((32, 8), (8, 1), (12, 12))]


def _rope_cache_case(D, bs, Hq, Hkv, rope):
    pos, slots, cs, kc, vc = _rope_inputs(Hkv, D, bs)
    W = (Hq + 2 * Hkv) * D
    buf = rnd(T_ROPE, W + 192)  # a row stride wider than the QKV width
    qkv = buf[:, :W]
    buf0, kc0, vc0 = buf.clone(), kc.clone(), vc.clone()
    ops.rope_cache(qkv, pos, cs, kc, vc, slots, Hq, Hkv, D, rope)
    q_ref, k_ref, v_ref = _qkv_ref(buf0[:, :W].cpu().double(), pos, cs, Hq, Hkv, D, rope)
    if rope:
        torch.testing.assert_close(qkv[:, :Hq * D].cpu().float(), q_ref.view(T_ROPE, Hq * D).float(), **ULP)
    else:  # in place: q is left untouched
        assert torch.equal(qkv[:, :Hq * D].view(torch.int16), buf0[:, :Hq * D].view(torch.int16))
    # the k / v columns and the columns past the QKV width are never written
    assert torch.equal(buf[:, Hq * D:].view(torch.int16), buf0[:, Hq * D:].view(torch.int16))
    _check_appended(kc, vc, kc0, vc0, k_ref, v_ref, slots, bs, v_exact=True)


@pytest.mark.parametrize("D,bs,Hq,Hkv", _ROPE_SHAPES)
def test_rope_cache_float64_reference(D, bs, Hq, Hkv):
    _rope_cache_case(D, bs, Hq, Hkv, True)


@pytest.mark.parametrize("D,bs,Hq,Hkv", [(64, 48, 12, 12), (128, 32, 32, 8)])
def test_rope_cache_no_rope(D, bs, Hq, Hkv):
    _rope_cache_case(D, bs, Hq, Hkv, False)


def _rope_partials_case(D, bs, Hq, Hkv, S, rope):
    pos, slots, cs, kc, vc = _rope_inputs(Hkv, D, bs)
    part = torch.randn(S, T_ROPE, (Hq + 2 * Hkv) * D, device=DEV) * 0.3
    kc0, vc0 = kc.clone(), vc.clone()
    q = torch.empty(T_ROPE, Hq * D, dtype=torch.bfloat16, device=DEV)
    ops.rope_cache_partials(PendingSum(part, S), q, pos, cs, kc, vc, slots, Hq, Hkv, D, rope)
    # rope False: q_out receives the plain sum
    q_ref, k_ref, v_ref = _qkv_ref(part.double().sum(0).cpu(), pos, cs, Hq, Hkv, D, rope)
    torch.testing.assert_close(q.cpu().float(), q_ref.view(T_ROPE, Hq * D).float(), **ULP)
    _check_appended(kc, vc, kc0, vc0, k_ref, v_ref, slots, bs)


@pytest.mark.parametrize("D,bs,Hq,Hkv", _ROPE_SHAPES)
@pytest.mark.parametrize("S", [1, 2, 3, 4, 8, 12])
def test_rope_cache_partials_float64_reference(D, bs, Hq, Hkv, S):
    """S = 1, 2, 4, 8: the specialised forms; 3 and 12: the runtime-S form."""
    _rope_partials_case(D, bs, Hq, Hkv, S, True)


@pytest.mark.parametrize("D,bs,Hq,Hkv,S", [(64, 48, 12, 12, 3), (128, 32, 32, 8, 4), (128, 16, 8, 1, 12)])
def test_rope_cache_partials_no_rope(D, bs, Hq, Hkv, S):
    _rope_partials_case(D, bs, Hq, Hkv, S, False)


# ---- 8. the prefill kernels at other page sizes

def _check_prefill(Hq, Hkv, D, gh, qlens, ctxs, bs, poison=False):
    lens = [a + c for a, c in zip(qlens, ctxs)]
    kc, vc, bt = _paged(lens, Hkv, D, bs, extra_pages=0 if poison else 8)
    if poison:
        _poison_past_end(kc, vc, bt, lens, bs)
    T = sum(qlens)
    q = _q_view(T, Hq, Hkv, D)
    qsl = _i32([0] + torch.cumsum(torch.tensor(qlens), 0).tolist())
    sl = _i32(lens)
    scale = 1.0 / math.sqrt(D)
    out = ops.prefill_attention(q, kc, vc, bt, qsl, sl, max(qlens), scale, gh=gh)
    ref = ops.prefill_attention_ref(q.cpu(), kc.cpu(), vc.cpu(), bt.cpu(), qsl.cpu(), sl.cpu(), scale)
    assert torch.isfinite(ref.float()).all()
    torch.testing.assert_close(out.cpu().float(), ref.float(), **ATT)


_PF_LENS = [([64, 1, 130, 7], [0, 5, 40, 300]), ([5, 5], [1000, 17])]


@pytest.mark.parametrize("Hq,Hkv,D,gh", [(32, 8, 128, 1), (32, 8, 128, 2), (32, 8, 128, 4), (16, 4, 64, 0),
                                         (16, 4, 64, 2), (12, 12, 64, 0), (12, 12, 64, 2)])
@pytest.mark.parametrize("bs", [32, 48, 64])
@pytest.mark.parametrize("qlens,ctxs", _PF_LENS)
def test_prefill16_page_sizes(Hq, Hkv, D, gh, bs, qlens, ctxs):
    """prefill_attn_kernel (gh > 0, and every D = 64 model). gh heads of ONE GQA group
    share a workgroup's K/V tiles, so gh = 2 at G = 1 (12, 12, 64) is not a supported
    configuration: the wrapper must reject it and launch nothing."""
    if (Hq // Hkv) % max(gh, 1):
        with pytest.raises(ValueError):
            _check_prefill(Hq, Hkv, D, gh, qlens, ctxs, bs)
        torch.cuda.synchronize()
        return
    _check_prefill(Hq, Hkv, D, gh, qlens, ctxs, bs)


@pytest.mark.parametrize("gh", [0, -44, -84, -1284])
@pytest.mark.parametrize("qlens,ctxs", _PF_LENS)
def test_prefill2_page_size_48(gh, qlens, ctxs):
    _check_prefill(32, 8, 128, gh, qlens, ctxs, 48)


@pytest.mark.parametrize("Hq,Hkv,D,gh", [(32, 8, 128, 1), (32, 8, 128, 2), (32, 8, 128, 4), (16, 4, 64, 0),
                                         (16, 4, 64, 2), (12, 12, 64, 0), (32, 8, 128, 0), (32, 8, 128, -44),
                                         (32, 8, 128, -84), (32, 8, 128, -1284)])
def test_prefill_poison_past_end_page_size_48(Hq, Hkv, D, gh):
    _check_prefill(Hq, Hkv, D, gh, [1, 17, 37, 129], [0, 0, 0, 0], 48, poison=True)
    _check_prefill(Hq, Hkv, D, gh, [3, 5], [34, 124], 48, poison=True)


# ---- 9. rejections: the binding raises before any launch

def test_rejections_launch_nothing():
    lens = [40, 17]
    sent = 7.0  # the output buffers keep this value: nothing ran

    def plain(Hq, Hkv, D, bs):
        kc, vc, bt = _paged(lens, Hkv, D, bs)
        out = torch.full((2, Hq, D), sent, dtype=torch.bfloat16, device=DEV)
        with pytest.raises(ValueError):
            ops.decode_attention(rnd(2, Hq, D), kc, vc, bt, _i32(lens), 0.088, num_splits=1, out=out)
        torch.cuda.synchronize()
        assert (out == sent).all()

    plain(6, 2, 128, 16)   # G = 3: not compiled
    plain(8, 2, 128, 24)   # a page size that is no multiple of 16
    # the fused form is D = 128 only
    Hq, Hkv, D, bs = 8, 2, 64, 16
    kc, vc, bt = _paged(lens, Hkv, D, bs)
    kc0, vc0 = kc.clone(), vc.clone()
    out = torch.full((2, Hq * D), sent, dtype=torch.bfloat16, device=DEV)
    part = torch.randn(2, 2, (Hq + 2 * Hkv) * D, device=DEV)
    slots = _i32([int(bt[b, (L - 1) // bs]) * bs + (L - 1) % bs for b, L in enumerate(lens)])
    with pytest.raises(ValueError):
        ops.decode_attention_fused(PendingSum(part, 2), _i32([L - 1 for L in lens]), slots,
                                   ops.build_cos_sin(D, 64, 500000.0, device=DEV), kc, vc, bt, _i32(lens), Hq, 0.125,
                                   1, out=out, depth=2)
    torch.cuda.synchronize()
    assert (out == sent).all()
    assert torch.equal(kc.view(torch.int16), kc0.view(torch.int16))
    assert torch.equal(vc.view(torch.int16), vc0.view(torch.int16))


# ---- 10. one end-to-end check per uncovered configuration

@pytest.fixture(scope="module")
def llama_1b_small():
    from xgserve.models import build_model, get_config
    cfg = replace(get_config("llama3.2-1b"), num_layers=2, name="llama3.2-1b-2l")
    return build_model(cfg, device="cuda:0", seed=3)


@pytest.fixture(scope="module")
def llama_8b_small():
    from xgserve.models import build_model, get_config
    cfg = replace(get_config("llama3-8b"), num_layers=2, name="llama3-8b-2l")
    return build_model(cfg, device="cuda:0", seed=3)


_REF_LOGITS = {}


def _decode_step_rel_err(model, block_size):
    """Relative norm error of the last decode step's logits (eager engine) against the
    dense fp32 reference forward with the same weights."""
    from xgserve.engine import EngineConfig, LLMEngine, SamplingParams
    from xgserve.models.reference import reference_logits
    eng = LLMEngine(EngineConfig(model=model.cfg.name, device="cuda:0", num_blocks=256, max_num_seqs=8,
                                 max_num_batched_tokens=1024, max_model_len=512, use_graphs=False,
                                 block_size=block_size), model=model)
    eng.runner.capture_logits = True
    prompt = [128000] + list(range(700, 790))  # 91 tokens: a partly filled last page at 16, 32 and 48
    eng.add_request("d", prompt, SamplingParams(max_tokens=2, temperature=0.0, ignore_eos=True))
    toks = []
    while eng.has_work():
        for o in eng.step():
            toks += o.new_token_ids
    assert len(toks) == 2
    got = eng.runner.last_logits[-1]
    key = (model.cfg.name, tuple(prompt + toks[:1]))
    if key not in _REF_LOGITS:  # computed once per model and token sequence, then shared
        _REF_LOGITS[key] = reference_logits(model, prompt + toks[:1])[-1].float().cpu()
    ref = _REF_LOGITS[key]
    return float((got - ref).norm() / ref.norm())


@pytest.mark.parametrize("block_size", [16, 48])
def test_llama32_1b_decode_step_logits_match_reference(llama_1b_small, block_size):
    """D = 64, G = 4 on the unfused chain (rope_cache -> decode_attention)."""
    assert not llama_1b_small._fused_ok
    assert llama_1b_small.cfg.head_dim == 64 and llama_1b_small.cfg.num_heads // llama_1b_small.cfg.num_kv_heads == 4
    assert _decode_step_rel_err(llama_1b_small, block_size) < 2e-2


def test_llama3_8b_fused_decode_step_block_size_32(llama_8b_small, monkeypatch):
    import xgserve.models.llama as ll
    monkeypatch.setattr(ll, "FUSED_DECODE", True)
    assert llama_8b_small._fused_ok and llama_8b_small.norms_folded
    assert _decode_step_rel_err(llama_8b_small, 32) < 2e-2
