"""Two-deep pinned host staging for the runner's H2D inputs."""
from __future__ import annotations

from typing import Dict, Tuple

import torch


def pinned(n: int, dtype) -> torch.Tensor:
    t = torch.empty(n, dtype=dtype)
    return t.pin_memory() if torch.cuda.is_available() else t


class StagingRing:
    """Named pinned host buffers x 2 slots, one event per slot. A step may return before
    its async H2D copies ran, so the host must not rewrite a slot until the copies that
    last read it have completed: acquire() takes the next slot and waits for its event,
    the caller fills the buffers and enqueues its copies, fence() records the event behind
    them. On a CPU device (cuda=False) the buffers are plain tensors and no event exists.

    specs: name -> (elements per unit, dtype). A ring of fixed size passes `units` here; a
    lazily sized one passes 0 and asks acquire() for what the step needs."""

    def __init__(self, specs: Dict[str, Tuple[int, torch.dtype]], cuda: bool, units: int = 0,
                 event=torch.cuda.Event):
        self.specs = dict(specs)
        self.cuda = cuda
        self._event = event
        self._units = [0, 0]
        self._slots = [None, None]
        self._events = [None, None]
        self._next = 0
        self.slot = 0  # index of the slot acquire() last returned (device twins are indexed by it)
        if units:
            for i in range(2):
                self._alloc(i, units)

    def _alloc(self, i: int, units: int) -> None:
        self._slots[i] = {k: pinned(per * units, dt) for k, (per, dt) in self.specs.items()}
        self._units[i] = units

    def add(self, specs: Dict[str, Tuple[int, torch.dtype]]) -> None:
        """More buffers under the same fence (both slots, at the slots' current sizes)."""
        self.specs.update(specs)
        for i in range(2):
            if self._slots[i] is not None:
                self._slots[i].update({k: pinned(per * self._units[i], dt) for k, (per, dt) in specs.items()})

    def acquire(self, units: int = 0) -> Dict[str, torch.Tensor]:
        i = self.slot = self._next
        self._next ^= 1
        if self._events[i] is not None:
            self._events[i].synchronize()  # the H2D copies that last read this slot have run
        if self._units[i] < units or self._slots[i] is None:
            self._alloc(i, units)  # after the wait: nothing still reads the buffers dropped here
        return self._slots[i]

    def fence(self) -> None:
        if self.cuda:
            i = self.slot
            if self._events[i] is None:
                self._events[i] = self._event()
            self._events[i].record()
