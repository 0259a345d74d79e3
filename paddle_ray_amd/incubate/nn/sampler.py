"""Token sampling for a serving loop: per-slot temperature / top-k / top-p on device."""
import math

import torch

from ...framework.core import Tensor, _default_device
from ...ops.fused import sample_top_p


class TokenSampler:
    """Picks the next token of every slot of a running batch from its logits, with per-slot
    temperature, top-k and top-p (``ops.fused.sample_top_p`` states the kept set and the draw):

        sampler = TokenSampler(batch_size=8, temperature=0.8, top_p=0.95, seed=1234)
        sampler.set(3, temperature=0.0)               # slot 3 decodes greedily from now on
        for _ in range(n):
            h = dec.step(embed(tok))                  # [B, 1, E]
            tok = sampler(head(h)[:, 0])              # [B] int64, no host sync

    The three parameters live in persistent device buffers (``temperature`` fp32, ``top_k`` int32,
    ``top_p`` fp32, each [B]); ``set(b, ...)`` rewrites one slot with a small device write, so a
    captured graph that calls the sampler keeps serving when a slot's request changes (continuous
    batching). ``__call__`` takes logits [B, V] or [B, T, V] (every slot's T rows share its
    parameters, as for the rows of ``step_multi``) and returns ids [B] or [B, T]; the chosen
    tokens' probabilities are kept in ``last_probs``. On the GPU a [B, V] call is the sampling
    kernel plus the counter's increment; a [B, T, V] call also expands the three parameter buffers
    to B * T rows first (three small copies).

    Every call draws from the counter hash of ``(seed, counter, row)``: ``counter`` is a device
    int64 that the call advances with a device-side add after the launch. Inside a
    ``torch.cuda.graph`` capture that add is captured with the launch, so each replay draws new
    numbers. ``state()`` returns ``(seed, counter)`` (one host read) and ``set_state`` restores
    it, which repeats a run; the seed is a host value, so a graph captured earlier keeps the seed
    it was captured with."""

    def __init__(self, batch_size, temperature=1.0, top_k=0, top_p=1.0, seed=0, device=None):
        self.B = int(batch_size)
        if self.B < 1:
            raise ValueError(f"TokenSampler: batch_size must be >= 1, got {batch_size}")
        dev = torch.device(device) if device is not None else _default_device()
        self.temperature = torch.empty(self.B, dtype=torch.float32, device=dev)
        self.top_k = torch.empty(self.B, dtype=torch.int32, device=dev)
        self.top_p = torch.empty(self.B, dtype=torch.float32, device=dev)
        self.counter = torch.zeros(1, dtype=torch.int64, device=dev)
        self.seed = int(seed)
        self.last_probs = None
        for name, v in (('temperature', temperature), ('top_k', top_k), ('top_p', top_p)):
            self._fill(name, slice(None), v)

    def _fill(self, name, where, v):
        buf = getattr(self, name)
        if name == 'top_k':
            if int(v) != v:
                raise ValueError(f"TokenSampler: top_k must be an integer, got {v!r}")
            v = max(-(2 ** 31), min(2 ** 31 - 1, int(v)))
        else:
            v = float(v)
            if not math.isfinite(v):
                raise ValueError(f"TokenSampler: {name} must be finite, got {v!r}")
        buf[where].fill_(v)

    def set(self, b, temperature=None, top_k=None, top_p=None):
        """Change slot ``b``'s parameters (those given); the other slots keep theirs."""
        b = int(b)
        if not 0 <= b < self.B:
            raise IndexError(f"TokenSampler: slot {b} out of range for batch_size {self.B}")
        for name, v in (('temperature', temperature), ('top_k', top_k), ('top_p', top_p)):
            if v is not None:
                self._fill(name, slice(b, b + 1), v)

    def state(self):
        """(seed, counter): what the next call draws from."""
        return self.seed, int(self.counter.item())

    def set_state(self, state):
        seed, counter = state
        self.seed = int(seed)
        self.counter.fill_(int(counter))

    def __call__(self, logits):
        wrap = isinstance(logits, Tensor)
        x = logits._t if wrap else logits
        if x.dim() not in (2, 3) or x.shape[0] != self.B:
            raise ValueError(f"TokenSampler: logits must be [{self.B}, V] or [{self.B}, T, V], got "
                             f"{tuple(x.shape)}")
        t, k, p = self.temperature, self.top_k, self.top_p
        if x.dim() == 3:
            T = x.shape[1]
            t, k, p = (v[:, None].expand(self.B, T).reshape(-1) for v in (t, k, p))
        ids, self.last_probs = sample_top_p(x, t, k, p, seed=self.seed, step=self.counter)
        self.counter.add_(1)
        return Tensor(ids) if wrap else ids
