"""moe_w8_plan (xgserve/ops/moe.py) against the library's no-launch predicate: the table mirror
equals MOE_W8_CFGS, and every plan for every registered Mixtral model is one moe_gemm_w8 takes."""
import itertools

from xgserve.models.config import get_config, list_models
from xgserve.ops import linear as L
from xgserve.ops import moe as MOE
from xgserve.ops._native import kernels

PAIRS = (1, 2, 4, 8, 9, 16, 17, 63, 64, 128)
FMTS = (L.WQ_FP8, L.WQ_INT8, L.WQ_INT4)


def test_every_moe_w8_plan_is_one_the_library_takes():
    k = kernels()
    assert MOE.MOE_W8_GEOM == dict(enumerate(k.gemm_cfgs()["moe_w8"]))
    models = [get_config(n) for n in list_models() if get_config(n).arch == "mixtral"]
    assert models
    for c, pairs, fmt in itertools.product(models, PAIRS, FMTS):
        E, H, F = c.num_experts, c.hidden_size, c.intermediate_size
        P = 64 * (-(-pairs // 64) + E)  # moe_align's capacity
        plan = MOE.moe_w8_plan(pairs, E, H, F, fmt)
        assert plan is not None, (c.name, pairs, fmt)
        cfg13, cfg2, S = plan
        assert k.moe_w8_supports(E, H, 2 * F, P, 1, L.MODE_SILU, cfg13, fmt, pairs), (c.name, pairs, fmt, plan)
        assert k.moe_w8_supports(E, F, H, P, S, L.MODE_PARTIAL, cfg2, fmt, pairs), (c.name, pairs, fmt, plan)
    # the int4 stage: 112 groups x 64 columns do not fit at one split, so the plan raised it
    assert not k.moe_w8_supports(8, 14336, 4096, 576, 1, L.MODE_PARTIAL, 2, L.WQ_INT4, 1)
    assert MOE.moe_w8_plan(1, 8, 4096, 14336, L.WQ_INT4)[2] > 1
