"""The model runner's host bookkeeping (engine/runner.py, engine/staging.py) without a GPU:
the decode-graph input layout, the pinned staging ring driven with counting fake events,
and step handles that carry their own top-N / speculative-acceptance records while two
steps are in flight."""
import numpy as np
import pytest
import torch

from xgserve import _runtime as R
from xgserve.engine import EngineConfig, LLMEngine
from xgserve.engine.runner import SamplingRows, SpecVerifyRows, stage_decode_inputs
from xgserve.engine.staging import StagingRing


def _scheduler(block_size, num_blocks):
    c = R.SchedulerConfig()
    c.block_size, c.num_blocks, c.max_num_seqs = block_size, num_blocks, 8
    c.max_num_batched_tokens, c.max_model_len, c.enable_prefix_cache = 256, 256, False
    return R.StepScheduler(c)


def test_stage_decode_inputs_layout():
    s = _scheduler(16, 64)
    for i in range(3):
        assert s.add(i + 1, list(range(10 + i, 30 + i)), 20, 1, True, False, [], 0)
    s.schedule()
    s.update(np.array([7, 8, 9], np.int32), np.ones(3, np.int32))
    plan = s.schedule()  # three decode rows at position 20: two pages each
    n, bs, B, W = 3, 4, 8, 5
    w = int(plan["bt_width"])
    assert int(plan["num_decodes"]) == int(plan["num_tokens"]) == n and w == 2
    SENT = 12345
    hi = np.full(5 * B + B * W, SENT, np.int32)
    src = np.array([0, -1, 2], np.int32)  # rows 0 and 2 take their id from the previous step
    stage_decode_inputs(plan, n, bs, B, W, src, hi)
    for k, key, pad in ((0, "input_ids", 0), (1, "positions", 0), (2, "slot_mapping", -1), (3, "seq_lens", 0)):
        sec = hi[k * B:(k + 1) * B]
        np.testing.assert_array_equal(sec[:n], plan[key][:n])
        assert (sec[n:bs] == pad).all()
        assert (sec[bs:] == SENT).all()  # rows past the bucket are not this step's
    assert list(hi[B:B + n]) == [20, 20, 20] and list(hi[3 * B:3 * B + n]) == [21, 21, 21]
    assert list(hi[4 * B:5 * B]) == [0, -1, 2, -1] + [SENT] * (B - bs)
    bt = hi[5 * B:5 * B + bs * W].reshape(bs, W)
    np.testing.assert_array_equal(bt[:n, :w], plan["block_tables"].reshape(n, w))
    assert (bt[:n, w:] == SENT).all() and (bt[n:] == SENT).all()  # beyond the plan's width / rows: untouched
    assert (hi[5 * B + bs * W:] == SENT).all()
    hi2 = np.full_like(hi, SENT)
    stage_decode_inputs(plan, n, bs, B, W, None, hi2)
    assert list(hi2[4 * B:4 * B + bs]) == [-1] * bs
    hi2[4 * B:4 * B + bs] = hi[4 * B:4 * B + bs]
    np.testing.assert_array_equal(hi2, hi)


class _Event:
    made = []

    def __init__(self):
        self.syncs = self.records = 0
        _Event.made.append(self)

    def synchronize(self):
        self.syncs += 1

    def record(self):
        self.records += 1


@pytest.fixture
def events():
    _Event.made = []
    return _Event.made


def test_ring_alternates_and_waits_the_slots_own_event(events):
    ring = StagingRing({"a": (8, torch.int32), "b": (2, torch.float32)}, True, units=1, event=_Event)
    seen = []
    for step in range(6):
        before = [e.syncs for e in events]
        slot = ring.acquire()
        seen.append(slot)
        assert slot["a"].numel() == 8 and slot["b"].dtype == torch.float32
        assert ring.slot == step % 2
        waited = [e.syncs - b for e, b in zip(events, before)]
        if step < 2:
            assert sum(waited) == 0  # nothing read this slot yet
        else:  # exactly the event recorded two acquisitions earlier, and no other
            assert waited == [1 if i == step % 2 else 0 for i in range(2)]
        ring.fence()
        assert events[step % 2].records == step // 2 + 1
    assert len(events) == 2  # an event per slot, reused
    assert all(s is seen[i % 2] for i, s in enumerate(seen)) and seen[0] is not seen[1]
    assert seen[0]["a"].data_ptr() != seen[1]["a"].data_ptr()


def test_ring_growth_and_lazily_added_buffers(events):
    ring = StagingRing({"x": (2, torch.int32), "y": (1, torch.int64)}, True, event=_Event)
    a = ring.acquire(64)
    assert a["x"].numel() == 128 and a["y"].numel() == 64
    a["x"].fill_(7)
    ring.fence()
    b = ring.acquire(64)
    b["x"].fill_(8)
    ring.fence()
    ea, eb = events
    # slot 0 comes round too small: its event is waited BEFORE its buffers are replaced (the
    # copy that reads them has run), and the new buffers are not the old ones
    big = ring.acquire(100)
    assert (ea.syncs, eb.syncs) == (1, 0)
    assert big["x"].numel() == 200 and big["y"].numel() == 100
    assert big["x"].data_ptr() != a["x"].data_ptr() and (a["x"] == 7).all()
    ring.fence()
    assert (ea.records, eb.records) == (2, 1) and len(events) == 2
    # the other slot kept its size, its contents and its own fence
    same = ring.acquire(64)
    assert same is b and (b["x"] == 8).all() and (ea.syncs, eb.syncs) == (1, 1)
    # a smaller request never shrinks a slot
    assert ring.acquire(10) is big
    # buffers added later join both slots at the slots' sizes, under the same events
    ring.add({"z": (3, torch.float32)})
    assert big["z"].numel() == 300 and b["z"].numel() == 192 and len(events) == 2


def test_ring_on_a_cpu_device_creates_no_events(events):
    ring = StagingRing({"x": (4, torch.int32)}, False, units=1, event=_Event)
    slots = []
    for _ in range(4):
        slots.append(ring.acquire())
        ring.fence()
    assert not events and slots[0] is slots[2] and slots[0] is not slots[1]
    assert not slots[0]["x"].is_cuda


# ---------------------------------------------------------------- handles, two steps in flight
@pytest.fixture(scope="module")
def cpu_step():
    """A CPU engine's runner and one plan that prefills two prompts (two sampled rows). The
    runner keeps nothing of a plan between steps, so the same plan launches again and again."""
    eng = LLMEngine(EngineConfig(model="llama-tiny", device="cpu", dtype="float32", num_blocks=64, max_num_seqs=4,
                                 max_num_batched_tokens=128, use_graphs=False, seed=7))
    r = eng.runner
    s = _scheduler(r.bs, r.num_blocks)
    for i in range(2):
        assert s.add(i + 1, list(range(10 + i, 22 + i)), 8, 1, True, False, [], 0)
    plan = s.schedule()
    assert int(plan["num_sample"]) == 2 and plan["logits_indices"].shape[0] == 2
    return r, plan


def _rows(**kw):
    return SamplingRows(np.array([0.8, 0.8], np.float32), np.ones(2, np.float32), np.zeros(2, np.int32),
                        np.array([11, 12], np.int64), **kw)


@pytest.mark.parametrize("order", ["AB", "BA"])
def test_top_result_is_the_waited_steps_own(cpu_step, order):
    r, plan = cpu_step
    r.capture_logits = True
    r.execute(plan, _rows())
    r.capture_logits = False
    assert r.top_result is None and r.spec_result is None
    want = torch.log_softmax(r.last_logits / 0.8, -1)
    hs = {"A": r.launch(plan, _rows(topn=np.array([3, 0], np.int32))),
          "B": r.launch(plan, _rows(topn=np.array([0, 2], np.int32)))}
    asked = {"A": (0, 3), "B": (1, 2)}
    for name in order:
        toks, lps, _ = r.wait(hs[name])
        assert toks.shape == (2,) and lps.shape == (2,)
        row, K = asked[name]
        top = r.top_result
        assert len(top) == 2 and top[1 - row] is None and len(top[row]) == K
        lp, ids = want[row].topk(K)
        assert [t for t, _ in top[row]] == ids.tolist()
        np.testing.assert_allclose([x for _, x in top[row]], lp.numpy(), rtol=0, atol=1e-5)
        assert r.spec_result is None
    r.wait(r.launch(plan, _rows()))  # a step that asked nothing leaves nothing of an earlier one
    assert r.top_result is None


@pytest.mark.parametrize("order", ["AB", "BA"])
def test_spec_result_is_the_waited_steps_own(cpu_step, order):
    """One sampled verify block over the step's two logits rows, built from SpecVerifyRows
    at vocabulary size. A's draft distribution is the target's own row (p == q bit for bit:
    accepted); B's puts all its mass on the target's least likely token (accepted with
    probability p(d) < 1e-3; the seeds below reject it)."""
    r, plan = cpu_step
    r.capture_logits = True
    r.execute(plan, _rows())
    r.capture_logits = False
    p = r.last_logits
    V = p.shape[1]

    def block(q, d):
        return SpecVerifyRows(np.zeros(1, np.int64), np.zeros(1, np.int64), np.ones(1, np.int64),
                              np.array([0.8], np.float32), np.array([11, 12], np.int64), np.array([d], np.int32), q)
    least = int(p[0].argmin())
    assert torch.softmax(p[0] / 0.8, -1)[least] < 1e-3
    q_b = torch.full((1, V), -30.0)
    q_b[0, least] = 30.0
    hs = {"A": r.launch(plan, _rows(spec=block(p[:1].clone(), int(p[0].argmax())))),
          "B": r.launch(plan, _rows(spec=block(q_b, least)))}
    want = {"A": [1], "B": [0]}
    for name in order:
        toks, _, _ = r.wait(hs[name])
        assert r.spec_result.dtype == np.int32 and r.spec_result.tolist() == want[name]
        assert r.top_result is None
        if name == "A":
            assert int(toks[0]) == int(p[0].argmax())  # the accepted draft token, written over row 0
        else:
            assert int(toks[0]) != least  # the residual draw excludes the rejected token
    r.wait(r.launch(plan, _rows()))
    assert r.spec_result is None
