"""Token sampling on the device (include/npm_hip.h npm_sample_rows, csrc/npm_sample.hip).

``Sampler(batch)`` keeps, per slot of a continuous batch, the temperature, top-k, top-p, seed and draw counter in HBM with a
host mirror.  ``sampler(logits)`` turns a [B, V] ``DeviceArray`` into one token id per row in ONE launch; the ids stay on the
device (``result.ids``) for ``layers.embedding.Embedding.forward``, and ``result.numpy()`` copies 4 bytes per sequence.

    sampler = sampling.Sampler(batch)
    sampler.set(b, temperature=0.8, top_k=50, top_p=0.9, seed=1234)        # when dec.admit fills slot b
    result = sampler(logits, active=new_lengths)                           # rows with n[b] == 0 are left alone: token -1
    x = embedding.forward(result.ids)

A slot's tokens depend on its own logits, parameters, seed and counter only -- never on the batch around it -- and the same
(seed, counter) gives the same token on every run.  A slot that was never ``set`` samples greedily.
"""

from __future__ import annotations

import ctypes as C
import math
from typing import Optional

import numpy as np

from np_modeling_amd import _C
from np_modeling_amd import device as D


class SampleResult:
    """What one ``Sampler`` call produced.  ``ids``: device int32 [B] (-1 for an inactive or invalid row); ``numpy()``: the
    same on the host; ``kept``: how many tokens survived top-k / top-p, int32 [B]; ``prob``: the drawn token's share of the
    kept mass, float32 [B].  The host copies are made on first use."""

    def __init__(self, out: D.ByteBuffer, batch: int):
        self._out, self._batch, self._host = out, batch, None
        self.ids = D.IdBuffer([batch], out._buf, out.ptr)

    def _fetch(self) -> np.ndarray:
        if self._host is None:
            self._host = self._out.numpy()
        return self._host

    def numpy(self) -> np.ndarray:
        return self._fetch()[:4 * self._batch].view(np.int32).copy()

    @property
    def kept(self) -> np.ndarray:
        return self._fetch()[4 * self._batch:8 * self._batch].view(np.int32).copy()

    @property
    def prob(self) -> np.ndarray:
        return self._fetch()[8 * self._batch:12 * self._batch].view(np.float32).copy()


class Sampler:
    def __init__(self, batch: int):
        if int(batch) < 1:
            raise ValueError(f'Sampler: batch must be at least 1, got {batch!r}')
        self.batch = int(batch)
        self.temperature = np.zeros([self.batch], dtype=np.float32)          # 0: greedy until set() says otherwise
        self.top_k = np.zeros([self.batch], dtype=np.int32)
        self.top_p = np.ones([self.batch], dtype=np.float32)
        self.seed = np.zeros([self.batch], dtype=np.uint64)
        self.draw = np.zeros([self.batch], dtype=np.uint64)                  # mirror of the device counters
        self._device: Optional[D.ByteBuffer] = None                          # the five vectors back to back, 28 B per slot
        self._stale = True

    def set(self, b: int, temperature: float = 1.0, top_k: int = 0, top_p: float = 1.0, seed: int = 0) -> None:
        """Parameters of slot ``b``; its draw counter restarts at 0.  ``temperature`` >= 0 (0: greedy), ``top_k`` an integer
        (<= 0: off), ``top_p`` in (0, 1] (1: off), ``seed`` in 0 .. 2^64 - 1.  ValueError otherwise, before anything changes."""
        if isinstance(b, bool) or not isinstance(b, (int, np.integer)) or not 0 <= b < self.batch:
            raise ValueError(f'Sampler.set: slot must be an integer in 0 .. {self.batch - 1}, got {b!r}')
        if not isinstance(temperature, (int, float, np.integer, np.floating)) or not (math.isfinite(temperature) and temperature >= 0):
            raise ValueError(f'Sampler.set: temperature must be a finite number >= 0, got {temperature!r}')
        if isinstance(top_k, bool) or not isinstance(top_k, (int, np.integer)) or not -2 ** 31 <= top_k < 2 ** 31:
            raise ValueError(f'Sampler.set: top_k must be an int32 integer (<= 0: off), got {top_k!r}')
        if not isinstance(top_p, (int, float, np.integer, np.floating)) or not 0 < top_p <= 1 or not np.float32(top_p) > 0:
            raise ValueError(f'Sampler.set: top_p must lie in (0, 1], got {top_p!r}')
        if isinstance(seed, bool) or not isinstance(seed, (int, np.integer)) or not 0 <= seed < 2 ** 64:
            raise ValueError(f'Sampler.set: seed must be an integer in 0 .. 2^64 - 1, got {seed!r}')
        self.temperature[b], self.top_k[b], self.top_p[b] = temperature, top_k, top_p
        self.seed[b], self.draw[b] = seed, 0
        self._stale = True

    def _pointers(self):
        """Device addresses of (seed, draw, temperature, top_k, top_p); one upload after a ``set``."""
        n = self.batch
        if self._stale or self._device is None:
            host = np.concatenate([self.seed.view(np.uint8), self.draw.view(np.uint8), self.temperature.view(np.uint8),
                                   self.top_k.view(np.uint8), self.top_p.view(np.uint8)])
            if self._device is None:
                self._device = D.ByteBuffer(host.nbytes)
            _C.check(_C.lib().npm_h2d(self._device.ptr, host.ctypes.data, host.nbytes), 'npm_h2d')
            self._stale = False
        p = self._device.ptr
        return p, p + 8 * n, p + 16 * n, p + 20 * n, p + 24 * n

    def device_draw(self) -> np.ndarray:
        """The draw counters as the device holds them, uint64 [B] (equal to ``draw`` at any time)."""
        self._pointers()
        return self._device.numpy()[8 * self.batch:16 * self.batch].view(np.uint64).copy()

    def __call__(self, logits, active=None) -> SampleResult:
        """One token per row of ``logits`` [B, V].  ``active``: [B] integers, a row with ``active[b] <= 0`` is left alone (the
        ``new_lengths`` vector of ``decode``: sequences that brought no token this step)."""
        if not isinstance(logits, D.DeviceArray) or logits.ndim != 2 or logits.shape[0] != self.batch:
            raise ValueError(f'Sampler: logits must be a DeviceArray of shape [{self.batch}, V], got '
                             f'{getattr(logits, "shape", type(logits).__name__)}')
        vocab = logits.shape[1]
        if not 1 <= vocab <= _C.SAMPLE_MAX_VOCAB:
            raise ValueError(f'Sampler: the vocabulary must be 1 .. {_C.SAMPLE_MAX_VOCAB}, got {vocab}')
        mask = None
        if active is not None:
            a = np.asarray(active)
            if a.shape != (self.batch,) or not (np.issubdtype(a.dtype, np.integer) or a.dtype == np.bool_):
                raise ValueError(f'Sampler: active must be {self.batch} integers, got {np.asarray(active).tolist()!r}')
            mask = a > 0
        seed, draw, temperature, top_k, top_p = self._pointers()
        out = D.ByteBuffer(12 * self.batch)
        active_dev = None if mask is None else D.bytes_from_host(mask.astype(np.int32))
        desc = _C.npm_sample(logits=logits.ptr, pitch=vocab, batch=self.batch, vocab=vocab, temperature=temperature, top_k=top_k,
                             top_p=top_p, seed=seed, draw=draw, active=None if active_dev is None else active_dev.ptr,
                             token=out.ptr, kept=out.ptr + 4 * self.batch, prob=out.ptr + 8 * self.batch)
        _C.check(_C.lib().npm_sample_rows(C.byref(desc)), 'npm_sample_rows')
        self.draw += np.uint64(1) if mask is None else mask.astype(np.uint64)
        return SampleResult(out, self.batch)
