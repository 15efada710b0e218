"""LayerDispatch (xgserve/models/llama.py): which GEMM kernel family each projection
of the unfused layer chain runs on, and which attention entry, per step size.

EXPECTED was recorded from LlamaLayer.forward as it stood before the selector
existed (seven hand-copied regime blocks): one layer per case on meta tensors with
the six GEMM wrappers, F.linear and the three attention entries replaced by
recorders, at (T tokens, num_decodes = T) and (T, T - 1). It is the record of what
the engine ran, not a print-out of the selector.

The selector relies on gemm_m64g having a plan for every shape that passes the
layer's dimension checks at 16 < M <= 64 (so that chain has no library arm);
test_m64_plans_cover_every_fast_shape pins that."""
import pytest

from xgserve.models import get_config
from xgserve.models.llama import PROJECTIONS, LayerDispatch
from xgserve.ops import linear as lin
from xgserve.ops.linear import MODE_PARTIAL, MODE_SILU, m64_plan

# "qkv o gate_up down attention"; MoE layers run their experts in place of gate_up / down
M64F, M64 = "m64 m64 m64 m64 fused_decode", "m64 m64 m64 m64 from_partials"
SKINNY, MW = "skinny skinny skinny skinny from_partials", "mw mw mw mw from_partials"
W8, LIB = "w8 w8 w8 w8 from_partials", "lib lib lib lib rope"
PF_GU, PF_GU_DOWN = "lib lib pf lib rope", "lib lib pf pf rope"
M64F_E, M64_E = "m64 m64 experts experts fused_decode", "m64 m64 experts experts from_partials"
MW_E, LIB_E = "mw mw experts experts from_partials", "lib lib experts experts rope"

# (model, tp, all four projections quantized) -> {T: (num_decodes = T, num_decodes = T - 1)}
EXPECTED = {
    ('llama3-8b', 1, False): {
        1: (M64F, M64), 16: (M64F, M64), 17: (M64F, M64), 64: (M64F, M64), 65: (MW, MW), 320: (MW, MW),
        321: (LIB, LIB), 447: (LIB, LIB), 448: (PF_GU, PF_GU), 512: (PF_GU, PF_GU), 513: (PF_GU_DOWN, PF_GU_DOWN),
        576: (PF_GU_DOWN, PF_GU_DOWN), 577: (LIB, LIB), 2048: (LIB, LIB),
    },
    ('llama3-8b', 2, False): {
        1: (M64F, M64), 16: (M64F, M64), 17: (M64F, M64), 64: (M64F, M64), 65: (MW, MW), 320: (MW, MW),
        321: (LIB, LIB), 447: (LIB, LIB), 448: (LIB, LIB), 512: (LIB, LIB), 513: (LIB, LIB), 576: (LIB, LIB),
        577: (LIB, LIB), 2048: (LIB, LIB),
    },
    ('llama3-70b', 1, False): {
        1: (M64F, M64), 16: (M64F, M64), 17: (M64F, M64), 64: (M64F, M64), 65: (MW, MW), 320: (MW, MW),
        321: (LIB, LIB), 447: (LIB, LIB), 448: (PF_GU, PF_GU), 512: (PF_GU, PF_GU), 513: (PF_GU_DOWN, PF_GU_DOWN),
        576: (PF_GU_DOWN, PF_GU_DOWN), 577: (LIB, LIB), 2048: (LIB, LIB),
    },
    ('llama3-70b', 2, False): {
        1: (M64F, M64), 16: (M64F, M64), 17: (M64F, M64), 64: (M64F, M64), 65: (MW, MW), 320: (MW, MW),
        321: (LIB, LIB), 447: (LIB, LIB), 448: (LIB, LIB), 512: (LIB, LIB), 513: (LIB, LIB), 576: (LIB, LIB),
        577: (LIB, LIB), 2048: (LIB, LIB),
    },
    ('mixtral-8x7b', 1, False): {
        1: (M64F_E, M64_E), 16: (M64F_E, M64_E), 17: (M64F_E, M64_E), 64: (M64F_E, M64_E), 65: (MW_E, MW_E),
        320: (MW_E, MW_E), 321: (LIB_E, LIB_E), 447: (LIB_E, LIB_E), 448: (LIB_E, LIB_E), 512: (LIB_E, LIB_E),
        513: (LIB_E, LIB_E), 576: (LIB_E, LIB_E), 577: (LIB_E, LIB_E), 2048: (LIB_E, LIB_E),
    },
    ('mixtral-8x7b', 2, False): {
        1: (M64F_E, M64_E), 16: (M64F_E, M64_E), 17: (M64F_E, M64_E), 64: (M64F_E, M64_E), 65: (MW_E, MW_E),
        320: (MW_E, MW_E), 321: (LIB_E, LIB_E), 447: (LIB_E, LIB_E), 448: (LIB_E, LIB_E), 512: (LIB_E, LIB_E),
        513: (LIB_E, LIB_E), 576: (LIB_E, LIB_E), 577: (LIB_E, LIB_E), 2048: (LIB_E, LIB_E),
    },
    ('llama3.2-1b', 1, False): {
        1: (SKINNY, SKINNY), 16: (SKINNY, SKINNY), 17: (M64, M64), 64: (M64, M64), 65: (MW, MW), 320: (MW, MW),
        321: (LIB, LIB), 447: (LIB, LIB), 448: (PF_GU, PF_GU), 512: (PF_GU, PF_GU), 513: (PF_GU_DOWN, PF_GU_DOWN),
        576: (PF_GU_DOWN, PF_GU_DOWN), 577: (LIB, LIB), 2048: (LIB, LIB),
    },
    ('llama-tiny', 1, False): {
        1: (SKINNY, SKINNY), 16: (SKINNY, SKINNY), 17: (M64, M64), 64: (M64, M64), 65: (MW, MW), 320: (MW, MW),
        321: (LIB, LIB), 447: (LIB, LIB), 448: (PF_GU, PF_GU), 512: (PF_GU, PF_GU), 513: (PF_GU_DOWN, PF_GU_DOWN),
        576: (PF_GU_DOWN, PF_GU_DOWN), 577: (LIB, LIB), 2048: (LIB, LIB),
    },
    ('llama-tiny', 2, False): {  # a 128-wide attention shard: the dimension checks fail, library everywhere
        1: (LIB, LIB), 16: (LIB, LIB), 17: (LIB, LIB), 64: (LIB, LIB), 65: (LIB, LIB), 320: (LIB, LIB),
        321: (LIB, LIB), 447: (LIB, LIB), 448: (LIB, LIB), 512: (LIB, LIB), 513: (LIB, LIB), 576: (LIB, LIB),
        577: (LIB, LIB), 2048: (LIB, LIB),
    },
    ('llama3-8b', 1, True): {
        1: (W8, W8), 64: (W8, W8), 65: (MW, MW),
    },
}


@pytest.mark.parametrize("model,tp,quantized", list(EXPECTED))
def test_step_families_match_recorded_forward(model, tp, quantized):
    cfg = get_config(model)
    d = LayerDispatch.for_layer(cfg, tp, on_gpu=True)
    if quantized:
        d.set_quantized(PROJECTIONS)
    moe = cfg.arch == "mixtral"
    for T, rows in EXPECTED[(model, tp, quantized)].items():
        for nd, want in zip((T, T - 1), rows):
            s = d.select(T, nd)
            mlp = ("experts", "experts") if moe else (s.gate_up, s.down)
            assert " ".join((s.qkv, s.o) + mlp + (s.attn,)) == want, (T, nd)


def test_partly_quantized_layer_keeps_the_rest_on_m64():
    d = LayerDispatch.for_layer(get_config("llama3-8b"), 1, on_gpu=True)
    d.set_quantized(("gate_up", "down"))
    assert tuple(d.select(64, 64)) == ("m64", "m64", "w8", "w8", "from_partials")
    assert tuple(d.select(65, 65)) == tuple(MW.split())


def test_cpu_layer_is_library_only():
    d = LayerDispatch.for_layer(get_config("llama3-8b"), 1, on_gpu=False)
    assert not (d.fast_ok or d.m64_small_ok or d.mw_ok or d.pf_ok or d.attn_fq_ok)
    assert all(tuple(d.select(T, T)) == tuple(LIB.split()) for T in (1, 17, 64, 65, 512, 2048))


def _layer_shapes():
    """(N, K, mode) of every projection of every registered model at TP 1/2/4/8 whose
    layer passes the dimension checks, plus every shape of the tuned plan table."""
    from xgserve.models.base import local_heads
    from xgserve.models.config import list_models
    shapes = set(lin._M64_TUNED)
    for cfg in (c for c in map(get_config, list_models()) if c.arch in ("llama", "mixtral")):
        for tp in (1, 2, 4, 8):
            try:
                Hq, Hkv = local_heads(cfg, tp)
            except ValueError:
                continue
            if not LayerDispatch.for_layer(cfg, tp, on_gpu=True).fast_ok:
                continue
            H, D = cfg.hidden_size, cfg.head_dim
            shapes |= {((Hq + 2 * Hkv) * D, H, MODE_PARTIAL), (H, Hq * D, MODE_PARTIAL)}
            if cfg.arch != "mixtral":
                Fl = cfg.intermediate_size // tp
                shapes |= {(2 * Fl, H, MODE_SILU), (H, Fl, MODE_PARTIAL)}
    return shapes


def test_m64_plans_cover_every_fast_shape():
    """What lets 16 < M <= 64 run every projection on gemm_m64g with no library arm:
    a partials plan for every N % 64 == 0, K % 256 == 0 (a tuned plan that fails its
    validity rule falls through to the default rule, which ends at split 1, 64
    columns), and a SiLU-gate plan for every gate_up of 2 Fl rows with Fl % 256 == 0."""
    for N, K, mode in _layer_shapes():
        if mode == MODE_PARTIAL and N % 64 == 0 and K % 256 == 0:
            assert all(m64_plan(M, N, K, MODE_PARTIAL) is not None for M in (17, 40, 64)), (N, K)
        if mode == MODE_SILU and N % 512 == 0 and K % 256 == 0:
            assert m64_plan(64, N, K, MODE_SILU) is not None, (N, K)
    # the default rule reads N and K only through N % 128, (N / 128) * S >= 192 and K % 1024
    for N in range(64, 65536, 64):
        for K in (256, 512, 768, 1024, 2048, 4096, 8192, 14336, 28672, 32512):
            assert all(m64_plan(M, N, K, MODE_PARTIAL) is not None for M in (17, 40, 64)), (N, K)
            if N % 512 == 0:
                assert m64_plan(64, N, K, MODE_SILU) is not None, (N, K)
