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

Speculative decoding (include/npm_hip.h npm_verify_rows, npm_ngram_draft; ``speculative.decode_step`` runs the whole step):
``NgramDrafter`` keeps every slot's tokens so far in HBM and proposes, as the next T tokens, what followed the most recent earlier
occurrence of the last few; ``Sampler.verify`` samples the T + 1 logit rows the model returned for them, row r at counter
``draw + r``, and accepts drafted tokens while they are the tokens sampled.  The tokens emitted are those of the one-token loop
from the same logits, seed for seed and counter for counter: a draft changes when tokens appear, never which.

Logit processors (include/npm_hip.h npm_logits_process, npm_history_append, npm_logprob_rows): ``LogitProcessor`` applies, per slot,
repetition / presence / frequency penalties over the slot's ``TokenHistory``, a bias list (-inf bans a token) and the minimum
length before end-of-sequence, IN PLACE on the logits a sampler is about to read -- the few logits those name, one launch,
nothing copied to the host; ``logprobs`` returns the log-sum-exp of every row, the log-probability of chosen tokens and the top n.

    history = sampling.TokenHistory(batch, capacity)                       # or the NgramDrafter of a speculative loop
    proc = sampling.LogitProcessor(batch, vocab, max_bias=8)
    proc.set(b, repetition_penalty=1.2, logit_bias={13: -math.inf}, eos=2, min_new_tokens=16, prompt_length=len(prompt_b))
    history.admit(b, prompt_b)
    result = sampler(proc(logits, history))                                # logits are edited in place: calling twice applies twice
    history.append(result)
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


class VerifyResult:
    """What one ``Sampler.verify`` produced, for T + 1 = ``rows`` logit rows per slot.  ``ids``: device int32 [B, rows], the
    tokens sampled up to and including the first that is not the drafted one, -1 behind it (and everywhere for an inactive slot);
    ``numpy()``: the same on the host; ``accepted``: int32 [B], how many drafted tokens were confirmed -- slot b emitted
    ``accepted[b] + 1`` tokens; ``kept`` / ``prob``: [B, rows] as in ``SampleResult``.  One host copy serves all four."""

    def __init__(self, out: D.ByteBuffer, batch: int, rows: int):
        self._out, self._batch, self._rows, self._host = out, batch, rows, None
        self.ids = D.IdBuffer([batch, rows], out._buf, out.ptr)

    @property
    def extra(self) -> np.ndarray:
        """The int32 words behind the four results (``Sampler.verify(..., extra_words=)``): what ``before_fetch`` had written
        there came to the host in the same copy."""
        return self._fetch()[3 * self._batch * self._rows + self._batch:].copy()

    def _fetch(self) -> np.ndarray:
        if self._host is None:
            self._host = self._out.numpy().view(np.int32)
        return self._host

    def _rows_of(self, first: int) -> np.ndarray:
        n = self._batch * self._rows
        return self._fetch()[first:first + n].reshape(self._batch, self._rows)

    def numpy(self) -> np.ndarray:
        return self._rows_of(0).copy()

    @property
    def accepted(self) -> np.ndarray:
        n = self._batch * self._rows
        return self._fetch()[n:n + self._batch].copy()

    @property
    def kept(self) -> np.ndarray:
        return self._rows_of(self._batch * self._rows + self._batch).copy()

    @property
    def prob(self) -> np.ndarray:
        return self._rows_of(2 * self._batch * self._rows + self._batch).view(np.float32).copy()


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

    def verify(self, logits, draft, n_draft, history: Optional['NgramDrafter'] = None, draft_pitch: Optional[int] = None,
               extra_words: int = 0, before_fetch=None) -> VerifyResult:
        """The T + 1 logit rows of every slot of a speculative step, ``logits`` [B * (T + 1), V] with slot b's rows together, in
        one call of npm_verify_rows: row r is sampled with slot b's parameters at counter ``draw[b] + r``, and drafted tokens are
        accepted while they equal the token sampled.  ``draft``: [B, >= T] integers or an ``IdBuffer`` (``draft_pitch``: its row
        pitch when that is not its last dimension -- ``NgramDrafter.propose``'s chunk from its second column on has pitch T + 1);
        ``n_draft``: [B] integers or an ``IdBuffer``, 0 .. T drafted tokens per slot, below 0 for a slot left alone (an
        ``IdBuffer`` is copied to the host once: the counters need it).  ``history``: the ``NgramDrafter`` whose histories the
        emitted tokens are appended to, on the device; ValueError before the launch when one might not fit.

        The host mirror ``draw`` advances by ``accepted + 1``, so the result is copied to the host here.  ``extra_words`` int32
        words are allocated behind the results and ``before_fetch(address)`` is called between the launch and that copy: what it
        launches may write them, and they arrive as ``result.extra`` without a copy of their own (``speculative.decode_step``
        has the next draft's lengths ride along)."""
        if not isinstance(logits, D.DeviceArray) or logits.ndim != 2 or logits.shape[0] % self.batch or logits.shape[0] == 0:
            raise ValueError(f'Sampler.verify: logits must be a DeviceArray of shape [{self.batch} * (T + 1), V], got '
                             f'{getattr(logits, "shape", type(logits).__name__)}')
        rows, vocab = logits.shape[0] // self.batch, logits.shape[1]
        if rows > _C.VERIFY_MAX_ROWS:
            raise ValueError(f'Sampler.verify: at most {_C.VERIFY_MAX_ROWS} rows per slot, got {rows}')
        if not 1 <= vocab <= _C.SAMPLE_MAX_VOCAB:
            raise ValueError(f'Sampler.verify: the vocabulary must be 1 .. {_C.SAMPLE_MAX_VOCAB}, got {vocab}')
        n_host = np.asarray(n_draft.numpy() if isinstance(n_draft, D.IdBuffer) else n_draft)
        if n_host.shape != (self.batch,) or not np.issubdtype(n_host.dtype, np.integer) or (n_host >= rows).any():
            raise ValueError(f'Sampler.verify: n_draft must be {self.batch} integers below {rows}, got {n_host.tolist()!r}')
        n_host = np.maximum(n_host.astype(np.int64), -1)
        n_dev = n_draft if isinstance(n_draft, D.IdBuffer) else D.ids_from_host(n_host)
        draft_dev = D.as_ids(draft)
        if draft_pitch is None:
            if len(draft_dev.shape) != 2 or draft_dev.shape[0] != self.batch:
                raise ValueError(f'Sampler.verify: draft must be [{self.batch}, >= {rows - 1}] integers, got {draft_dev.shape}')
            draft_pitch = draft_dev.shape[1]
        if draft_pitch < rows - 1:
            raise ValueError(f'Sampler.verify: the draft holds fewer than {rows - 1} tokens per slot (pitch {draft_pitch})')
        active = n_host >= 0
        if history is not None:
            if not isinstance(history, NgramDrafter) or history.batch != self.batch:
                raise ValueError(f'Sampler.verify: history must be an NgramDrafter of batch {self.batch}')
            if (history.lengths + np.where(active, n_host + 1, 0) > history.capacity).any():
                raise ValueError(f'Sampler.verify: up to {(n_host + 1).tolist()} more tokens after {history.lengths.tolist()} do not fit '
                                 f'the history capacity {history.capacity}')
        seed, draw, temperature, top_k, top_p = self._pointers()
        cells = self.batch * rows
        out = D.ByteBuffer(4 * (3 * cells + self.batch + int(extra_words)))
        if history is not None:
            history._ahead = None                                            # the histories are about to change
        desc = _C.npm_verify(logits=logits.ptr, pitch=vocab, batch=self.batch, rows=rows, vocab=vocab,
                             history_cap=0 if history is None else history.capacity, temperature=temperature, top_k=top_k,
                             top_p=top_p, seed=seed, draw=draw, draft=draft_dev.ptr, draft_pitch=draft_pitch, n_draft=n_dev.ptr,
                             token=out.ptr, accepted=out.ptr + 4 * cells, kept=out.ptr + 4 * (cells + self.batch),
                             prob=out.ptr + 4 * (2 * cells + self.batch),
                             history=None if history is None else history._history.ptr,
                             history_pitch=0 if history is None else history.capacity,
                             history_len=None if history is None else history._lengths.ptr)
        _C.check(_C.lib().npm_verify_rows(C.byref(desc)), 'npm_verify_rows')
        if before_fetch is not None:
            before_fetch(out.ptr + 4 * (3 * cells + self.batch))
        result = VerifyResult(out, self.batch, rows)
        emitted = np.where(active, result.accepted.astype(np.int64) + 1, 0)
        self.draw += emitted.astype(np.uint64)
        if history is not None:
            history.lengths += ((result.numpy() >= 0) & (np.arange(rows)[None, :] < emitted[:, None])).sum(axis=1)
        return result


class TokenHistory:
    """The tokens of every slot so far on the device, int32 [batch, capacity], with a host mirror ``lengths`` of how many each slot
    holds: what ``LogitProcessor`` reads its penalties from and ``NgramDrafter`` its drafts.  ``admit`` starts a slot over,
    ``append`` puts one sampled token behind every slot's history on the device (npm_history_append)."""

    def __init__(self, batch: int, capacity: int):
        if int(batch) < 1 or int(capacity) < 1:
            raise ValueError(f'{type(self).__name__}: batch and capacity must be at least 1, got {batch!r}, {capacity!r}')
        self.batch, self.capacity = int(batch), int(capacity)
        self.lengths = np.zeros([self.batch], dtype=np.int64)
        self._history = D.IdBuffer([self.batch, self.capacity])
        self._lengths = D.ids_from_host(np.zeros([self.batch], dtype=np.int32))
        self._ahead = None                # NgramDrafter: a proposal launched ahead; anything that changes a history drops it

    def _slot(self, b, what: str) -> int:
        if isinstance(b, bool) or not isinstance(b, (int, np.integer)) or not 0 <= b < self.batch:
            raise ValueError(f'{type(self).__name__}.{what}: slot must be an integer in 0 .. {self.batch - 1}, got {b!r}')
        return int(b)

    def _set_length(self, b: int, n: int) -> None:
        host = np.array([n], dtype=np.int32)
        _C.check(_C.lib().npm_h2d(self._lengths.ptr + 4 * b, host.ctypes.data, 4), 'npm_h2d')
        self.lengths[b] = n
        self._ahead = None

    def admit(self, b: int, ids) -> None:
        """Slot ``b`` starts over with the tokens ``ids`` (1-D, 0 .. 2^31 - 1 each, at most ``capacity``): a sequence's prompt
        and whatever it has emitted already.  ValueError before anything changes."""
        name = type(self).__name__
        b = self._slot(b, 'admit')
        host = np.asarray(ids)
        if host.ndim != 1 or host.dtype == np.bool_ or not (np.issubdtype(host.dtype, np.integer) or host.size == 0):
            raise ValueError(f'{name}.admit: ids must be a 1-D integer array, got {host.dtype} {host.shape}')
        if host.size > self.capacity or (host.size and (host.min() < 0 or host.max() >= 2 ** 31)):
            raise ValueError(f'{name}.admit: at most {self.capacity} token ids in 0 .. 2^31 - 1, got {host.size} in '
                             f'{int(host.min()) if host.size else 0} .. {int(host.max()) if host.size else 0}')
        host = np.ascontiguousarray(host.astype(np.int32))
        if host.size:
            _C.check(_C.lib().npm_h2d(self._history.ptr + 4 * b * self.capacity, host.ctypes.data, host.nbytes), 'npm_h2d')
        self._set_length(b, host.size)

    def release(self, b: int) -> None:
        """Slot ``b`` holds no tokens until the next ``admit``."""
        self._set_length(self._slot(b, 'release'), 0)

    def append(self, result_or_ids, active=None) -> None:
        """The token every slot just sampled goes behind its history, on the device: ``result_or_ids`` a ``SampleResult`` (its
        cached ``numpy()``, which the loop fetches anyway, advances the host mirror) or an ``IdBuffer`` [batch] (one copy of 4 bytes
        per slot).  A token below 0 (an inactive or invalid row) and a slot with ``active[b] <= 0`` append nothing.  ValueError
        before the launch when a token does not fit the capacity."""
        name = type(self).__name__
        if isinstance(result_or_ids, SampleResult):
            ids, host = result_or_ids.ids, result_or_ids.numpy()
        elif isinstance(result_or_ids, D.IdBuffer):
            ids, host = result_or_ids, None
        else:
            raise ValueError(f'{name}.append: a SampleResult or an IdBuffer is required, got {type(result_or_ids).__name__}')
        if ids.size != self.batch:
            raise ValueError(f'{name}.append: {self.batch} token ids are required, got shape {ids.shape}')
        mask = None
        if active is not None:
            a = np.asarray(active)
            if a.shape != (self.batch,) or not (np.issubdtype(a.dtype, np.integer) or a.dtype == np.bool_):
                raise ValueError(f'{name}.append: active must be {self.batch} integers, got {np.asarray(active).tolist()!r}')
            mask = a > 0
        if host is None:
            host = ids.numpy()
        grows = (host.reshape(-1) >= 0) if mask is None else ((host.reshape(-1) >= 0) & mask)
        if (self.lengths + grows > self.capacity).any():
            raise ValueError(f'{name}.append: one more token after {self.lengths.tolist()} does not fit the capacity {self.capacity}')
        active_dev = None if mask is None else D.ids_from_host(mask.astype(np.int32))
        self._ahead = None                                                   # the histories are about to change
        _C.check(_C.lib().npm_history_append(self._history.ptr, self.capacity, self.capacity, self._lengths.ptr, ids.ptr,
                                             None if active_dev is None else active_dev.ptr, self.batch), 'npm_history_append')
        self.lengths += grows

    def device_lengths(self) -> np.ndarray:
        """The history lengths as the device holds them, int64 [batch] (equal to ``lengths`` at any time)."""
        return self._lengths.numpy().astype(np.int64)

    def numpy(self) -> np.ndarray:
        """The histories on the host, int32 [batch, capacity]; slot b's first ``lengths[b]`` entries are its tokens."""
        return self._history.numpy()


class NgramDrafter(TokenHistory):
    """Drafts by prompt lookup (include/npm_hip.h npm_ngram_draft): the tokens of every slot so far live on the device, int32
    [batch, capacity], with a host mirror ``lengths`` of how many each slot holds.  ``propose`` returns, per slot, its last token
    followed by up to ``max_draft`` tokens that followed the most recent earlier occurrence of its last n tokens, n from
    ``ngram[0]`` down to ``ngram[1]``; ``Sampler.verify(..., history=drafter)`` appends what a step emitted without a trip
    through the host.  Integers only: the same history gives the same draft on every run."""

    def __init__(self, batch: int, capacity: int, max_draft: int, ngram=(3, 1)):
        if int(batch) < 1 or int(capacity) < 1:
            raise ValueError(f'NgramDrafter: batch and capacity must be at least 1, got {batch!r}, {capacity!r}')
        if not 1 <= int(max_draft) <= _C.VERIFY_MAX_ROWS - 1:
            raise ValueError(f'NgramDrafter: max_draft must be 1 .. {_C.VERIFY_MAX_ROWS - 1}, got {max_draft!r}')
        nmax, nmin = (int(v) for v in ngram)
        if not 1 <= nmin <= nmax <= _C.DRAFT_MAX_NGRAM:
            raise ValueError(f'NgramDrafter: ngram is (nmax, nmin) with 1 <= nmin <= nmax <= {_C.DRAFT_MAX_NGRAM}, got {ngram!r}')
        TokenHistory.__init__(self, batch, capacity)
        self.max_draft, self.ngram = int(max_draft), (nmax, nmin)
        self._ahead = None                # [limits, chunk, n_new] of a proposal launched ahead; n_new None until it reached the host

    def propose(self, limit=None):
        """(chunk, n_new): ``chunk`` an ``IdBuffer`` [batch, max_draft + 1] -- slot b's last token, then its draft, then -1 -- and
        ``n_new`` host int64 [batch], 1 + the drafted tokens (0: an empty slot, or one with ``limit[b] < 0``).  ``limit``: [batch]
        integers, the most tokens slot b may be drafted (None: ``max_draft``).  ``chunk`` feeds ``Embedding.forward``, ``n_new``
        is ``decode``'s ``new_lengths``; one launch and one host copy of 4 bytes per slot."""
        lim = self._limits(limit)
        ahead, self._ahead = self._ahead, None
        if ahead is not None and ahead[2] is not None and np.array_equal(ahead[0], lim):
            return ahead[1], ahead[2]                                        # launched behind the last verify: nothing to do
        cells = self.batch * (self.max_draft + 1)
        out = D.IdBuffer([cells + self.batch])
        n_new = D.IdBuffer([self.batch], out._buf, out.ptr + 4 * cells)
        self._launch(lim, out.ptr, n_new.ptr)
        return D.IdBuffer([self.batch, self.max_draft + 1], out._buf, out.ptr), n_new.numpy().astype(np.int64)

    def _limits(self, limit) -> np.ndarray:
        if limit is None:
            return np.full([self.batch], self.max_draft, dtype=np.int32)
        lim = np.asarray(limit)
        if lim.shape != (self.batch,) or not np.issubdtype(lim.dtype, np.integer):
            raise ValueError(f'NgramDrafter.propose: limit must be {self.batch} integers, got {np.asarray(limit).tolist()!r}')
        return np.clip(lim, -1, self.max_draft).astype(np.int32)

    def _launch(self, lim: np.ndarray, chunk_ptr: int, n_new_ptr: int) -> None:
        limit_dev = D.ids_from_host(lim)
        _C.check(_C.lib().npm_ngram_draft(self._history.ptr, self.capacity, self.capacity, self._lengths.ptr, limit_dev.ptr, self.batch,
                                          self.max_draft, self.ngram[0], self.ngram[1], chunk_ptr, n_new_ptr), 'npm_ngram_draft')

    def propose_ahead(self, limit, n_new_ptr: int) -> None:
        """``propose(limit)`` launched now, its ``n_new`` written to device address ``n_new_ptr`` instead of copied: the caller
        brings it to the host with something else (``Sampler.verify(..., before_fetch=)``) and hands it to ``settle_ahead``.  The
        next ``propose`` with the same limits returns this proposal without a launch or a copy; ``admit``, ``release``, another
        ``verify`` on these histories or other limits drop it."""
        lim = self._limits(limit)
        chunk = D.IdBuffer([self.batch, self.max_draft + 1])
        self._launch(lim, chunk.ptr, n_new_ptr)
        self._ahead = [lim, chunk, None]

    def settle_ahead(self, n_new) -> None:
        if self._ahead is not None:
            self._ahead[2] = np.asarray(n_new).astype(np.int64)


def _is_real(v) -> bool:
    return not isinstance(v, bool) and isinstance(v, (int, float, np.integer, np.floating))


def _is_int32(v) -> bool:
    return not isinstance(v, bool) and isinstance(v, (int, np.integer)) and -2 ** 31 <= v < 2 ** 31


class LogitProcessor:
    """Per-slot logit processors applied on the device, in place, before sampling (include/npm_hip.h npm_logits_process).

    ``set(b, ...)`` gives slot b its rules; a slot that was never ``set`` is neutral.  ``proc(logits, history)`` edits the [B, V]
    logits of a one-token step, ``proc(logits, history, draft=, n_draft=, draft_pitch=)`` the [B (T + 1), V] logits of a
    speculative chunk -- row r as if ``draft[b, :r]`` had been appended to the history, which is what the one-token loop would
    hold when it samples that token.  It returns ``logits`` (the same array).  Calling it twice on the same logits applies the
    rules twice.  Only the logits that the history, the draft, the bias list and eos name are touched; one launch, no copy to the
    host; while every slot is neutral nothing is launched at all."""

    def __init__(self, batch: int, vocab: int, max_bias: int = 0):
        if int(batch) < 1 or not 1 <= int(vocab) <= _C.SAMPLE_MAX_VOCAB:
            raise ValueError(f'LogitProcessor: batch >= 1 and a vocabulary of 1 .. {_C.SAMPLE_MAX_VOCAB}, got {batch!r}, {vocab!r}')
        if not 0 <= int(max_bias) <= _C.LOGITS_MAX_BIAS:
            raise ValueError(f'LogitProcessor: max_bias must be 0 .. {_C.LOGITS_MAX_BIAS}, got {max_bias!r}')
        self.batch, self.vocab, self.max_bias = int(batch), int(vocab), int(max_bias)
        b, m = self.batch, self.max_bias
        self.repetition = np.ones([b], dtype=np.float32)
        self.presence = np.zeros([b], dtype=np.float32)
        self.frequency = np.zeros([b], dtype=np.float32)
        self.eos = np.full([b], -1, dtype=np.int32)
        self.min_new = np.zeros([b], dtype=np.int32)
        self.prompt_len = np.zeros([b], dtype=np.int32)
        self.bias_count = np.zeros([b], dtype=np.int32)
        self.bias_index = np.full([b, m], -1, dtype=np.int32)
        self.bias_value = np.zeros([b, m], dtype=np.float32)
        self._device: Optional[D.ByteBuffer] = None                          # the nine arrays back to back
        self._stale = True
        self._workspace = D.IdBuffer([b, self.vocab])                        # all zero between calls
        _C.check(_C.lib().npm_fill_f32(self._workspace.ptr, 0.0, b * self.vocab), 'npm_fill_f32')

    def set(self, b: int, repetition_penalty: float = 1.0, presence_penalty: float = 0.0, frequency_penalty: float = 0.0,
            logit_bias=None, eos: Optional[int] = None, min_new_tokens: int = 0, prompt_length: int = 0) -> None:
        """The rules of slot ``b``.  ``repetition_penalty`` finite and > 0 (1: off); ``presence_penalty`` and
        ``frequency_penalty`` finite (0: off) -- they count the tokens behind the first ``prompt_length`` of the history, the
        repetition penalty counts all of it; ``logit_bias`` a mapping or pairs of distinct token ids in 0 .. vocab - 1 to a finite
        number or -inf (a ban), at most ``max_bias``; ``eos`` (None: no rule) gets -inf while fewer than ``min_new_tokens``
        tokens stand behind the prompt.  ValueError before anything changes."""
        if isinstance(b, bool) or not isinstance(b, (int, np.integer)) or not 0 <= b < self.batch:
            raise ValueError(f'LogitProcessor.set: slot must be an integer in 0 .. {self.batch - 1}, got {b!r}')
        with np.errstate(over='ignore'):                                     # a value that overflows fp32 is refused, not warned about
            pairs = self._check(repetition_penalty, presence_penalty, frequency_penalty, logit_bias, eos, min_new_tokens, prompt_length)
        self.repetition[b], self.presence[b], self.frequency[b] = repetition_penalty, presence_penalty, frequency_penalty
        self.eos[b], self.min_new[b], self.prompt_len[b] = -1 if eos is None else eos, min_new_tokens, prompt_length
        self.bias_count[b] = len(pairs)
        self.bias_index[b], self.bias_value[b] = -1, 0
        for j, (k, v) in enumerate(pairs):
            self.bias_index[b, j], self.bias_value[b, j] = k, v
        self._stale = True

    def _check(self, repetition_penalty, presence_penalty, frequency_penalty, logit_bias, eos, min_new_tokens, prompt_length) -> list:
        """ValueError for anything ``set`` refuses; the bias list as pairs."""
        if not _is_real(repetition_penalty) or not (math.isfinite(repetition_penalty) and np.float32(repetition_penalty) > 0
                                                    and math.isfinite(np.float32(repetition_penalty))):
            raise ValueError(f'LogitProcessor.set: repetition_penalty must be a finite number > 0, got {repetition_penalty!r}')
        for name, v in (('presence_penalty', presence_penalty), ('frequency_penalty', frequency_penalty)):
            if not _is_real(v) or not math.isfinite(v) or not math.isfinite(np.float32(v)):
                raise ValueError(f'LogitProcessor.set: {name} must be a finite number, got {v!r}')
        for name, v in (('min_new_tokens', min_new_tokens), ('prompt_length', prompt_length)) + ((('eos', eos),) if eos is not None else ()):
            if not _is_int32(v):
                raise ValueError(f'LogitProcessor.set: {name} must be an int32 integer, got {v!r}')
        try:
            pairs = [] if logit_bias is None else [(k, v) for k, v in (logit_bias.items() if hasattr(logit_bias, 'items') else logit_bias)]
        except (TypeError, ValueError):
            raise ValueError(f'LogitProcessor.set: logit_bias must be a mapping or pairs (token id, value), got {logit_bias!r}') from None
        if len(pairs) > self.max_bias:
            raise ValueError(f'LogitProcessor.set: at most max_bias = {self.max_bias} bias entries, got {len(pairs)}')
        for k, v in pairs:
            if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or not 0 <= k < self.vocab:
                raise ValueError(f'LogitProcessor.set: a bias token id must be an integer in 0 .. {self.vocab - 1}, got {k!r}')
            if not _is_real(v) or math.isnan(v) or v == math.inf or np.float32(v) == np.inf:
                raise ValueError(f'LogitProcessor.set: a bias value must be a finite number or -inf, got {v!r}')
        if len({int(k) for k, _ in pairs}) != len(pairs):
            raise ValueError(f'LogitProcessor.set: a token id occurs twice in logit_bias: {[int(k) for k, _ in pairs]}')
        return pairs

    def neutral(self) -> bool:
        """Whether no rule of any slot can change a logit, whatever the histories hold."""
        return bool(((self.repetition == 1) & (self.presence == 0) & (self.frequency == 0) & (self.bias_count == 0)
                     & ((self.eos < 0) | (self.eos >= self.vocab) | (self.min_new <= 0))).all())

    def _pointers(self) -> dict:
        """Device addresses of the per-slot arrays; one upload after a ``set``."""
        arrays = [('repetition', self.repetition), ('presence', self.presence), ('frequency', self.frequency), ('eos', self.eos),
                  ('min_new', self.min_new), ('prompt_len', self.prompt_len), ('bias_count', self.bias_count),
                  ('bias_index', self.bias_index), ('bias_value', self.bias_value)]
        if self._stale or self._device is None:
            host = np.concatenate([a.reshape(-1).view(np.uint8) for _, a in arrays])
            if self._device is None:
                self._device = D.ByteBuffer(host.nbytes)
            _C.check(_C.lib().npm_h2d(self._device.ptr, host.ctypes.data, host.nbytes), 'npm_h2d')
            self._stale = False
        out, at = {}, self._device.ptr
        for name, a in arrays:
            out[name] = at
            at += a.nbytes
        if self.max_bias == 0:
            out['bias_index'] = out['bias_value'] = out['bias_count'] = None
        return out

    def __call__(self, logits, history: Optional[TokenHistory] = None, active=None, draft=None, n_draft=None,
                 draft_pitch: Optional[int] = None):
        """``logits`` [B, V], or with ``draft`` / ``n_draft`` (what ``Sampler.verify`` takes: [B, >= T] integers or an ``IdBuffer``
        with an optional ``draft_pitch``; [B] integers or an ``IdBuffer``, below 0 for a slot left alone) [B (T + 1), V] with slot
        b's rows together.  ``history``: the ``TokenHistory`` (or ``NgramDrafter``) of the batch, None for empty histories;
        ``active``: [B] integers, a slot with ``active[b] <= 0`` is left alone.  ValueError before anything is launched."""
        if not isinstance(logits, D.DeviceArray) or logits.ndim != 2 or logits.shape[0] % self.batch or logits.shape[0] == 0 \
                or logits.shape[1] != self.vocab:
            raise ValueError(f'LogitProcessor: logits must be a DeviceArray of shape [{self.batch} * rows, {self.vocab}], got '
                             f'{getattr(logits, "shape", type(logits).__name__)}')
        rows = logits.shape[0] // self.batch
        if rows > _C.VERIFY_MAX_ROWS:
            raise ValueError(f'LogitProcessor: at most {_C.VERIFY_MAX_ROWS} rows per slot, got {rows}')
        if history is not None and (not isinstance(history, TokenHistory) or history.batch != self.batch):
            raise ValueError(f'LogitProcessor: history must be a TokenHistory of batch {self.batch}')
        if (draft is None or n_draft is None) and rows != 1:
            raise ValueError(f'LogitProcessor: {rows} rows per slot need draft and n_draft')
        mask = None
        if active is not None:
            a = np.asarray(active)
            if a.shape != (self.batch,) or not (np.issubdtype(a.dtype, np.integer) or a.dtype == np.bool_):
                raise ValueError(f'LogitProcessor: active must be {self.batch} integers, got {np.asarray(active).tolist()!r}')
            mask = a > 0
        n_host = None
        if n_draft is not None and not isinstance(n_draft, D.IdBuffer):
            n_host = np.asarray(n_draft)
            if n_host.shape != (self.batch,) or not np.issubdtype(n_host.dtype, np.integer) or (n_host >= rows).any():
                raise ValueError(f'LogitProcessor: n_draft must be {self.batch} integers below {rows}, got {n_host.tolist()!r}')
            n_host = np.maximum(n_host.astype(np.int64), -1)
        elif n_draft is not None and n_draft.size != self.batch:
            raise ValueError(f'LogitProcessor: n_draft must hold {self.batch} integers, got shape {n_draft.shape}')
        draft_dev = None
        if draft is not None:
            if not isinstance(draft, D.IdBuffer):
                host = np.asarray(draft)
                if host.dtype == np.bool_ or not np.issubdtype(host.dtype, np.integer) or (host.size and (host.min() < -2 ** 31
                                                                                                          or host.max() >= 2 ** 31)):
                    raise ValueError(f'LogitProcessor: draft must be int32 integers, got dtype {host.dtype}')
            shape = draft.shape if isinstance(draft, D.IdBuffer) else np.asarray(draft).shape
            if draft_pitch is None:
                if len(shape) != 2 or shape[0] != self.batch:
                    raise ValueError(f'LogitProcessor: draft must be [{self.batch}, >= {rows - 1}] integers, got {tuple(shape)}')
                draft_pitch = shape[1]
            if draft_pitch < rows - 1:
                raise ValueError(f'LogitProcessor: the draft holds fewer than {rows - 1} tokens per slot (pitch {draft_pitch})')
        if self.neutral():
            return logits                                                    # nothing can change: nothing is launched
        if draft is not None and rows > 1:
            draft_dev = D.as_ids(draft)
        n_dev = None if n_draft is None else (n_draft if isinstance(n_draft, D.IdBuffer) else D.ids_from_host(n_host))
        active_dev = None if mask is None else D.ids_from_host(mask.astype(np.int32))
        p = self._pointers()
        desc = _C.npm_logits(logits=logits.ptr, pitch=self.vocab, batch=self.batch, rows=rows, vocab=self.vocab,
                             history_cap=0 if history is None else history.capacity,
                             history=None if history is None else history._history.ptr,
                             history_pitch=0 if history is None else history.capacity,
                             history_len=None if history is None else history._lengths.ptr, prompt_len=p['prompt_len'],
                             draft=None if draft_dev is None else draft_dev.ptr, draft_pitch=0 if draft_dev is None else draft_pitch,
                             n_draft=None if n_dev is None else n_dev.ptr, active=None if active_dev is None else active_dev.ptr,
                             repetition=p['repetition'], presence=p['presence'], frequency=p['frequency'], eos=p['eos'],
                             min_new=p['min_new'], bias_index=p['bias_index'], bias_value=p['bias_value'], bias_count=p['bias_count'],
                             bias_cap=self.max_bias, workspace=self._workspace.ptr)
        _C.check(_C.lib().npm_logits_process(C.byref(desc)), 'npm_logits_process')
        return logits


class LogProbs:
    """What ``logprobs`` produced for R logit rows.  ``lse``: float32 [R], the log-sum-exp (NaN for a skipped or invalid row);
    ``chosen``: float32 [R], the log-probability of ``ids[r]`` (None without ``ids``); ``top_tokens`` int32 and ``top_logprobs``
    float32 [R, top_n]: the most probable tokens in the sampler's order, -1 / -inf behind the last that exists.  The host copies
    are made on first use, one copy for all four."""

    def __init__(self, out: D.ByteBuffer, rows: int, top_n: int, with_ids: bool):
        self._out, self._rows, self._top, self._with_ids, self._host = out, rows, top_n, with_ids, None

    def _fetch(self) -> np.ndarray:
        if self._host is None:
            self._host = self._out.numpy().view(np.uint32)
        return self._host

    @property
    def lse(self) -> np.ndarray:
        return self._fetch()[:self._rows].view(np.float32).copy()

    @property
    def chosen(self) -> Optional[np.ndarray]:
        return self._fetch()[self._rows:2 * self._rows].view(np.float32).copy() if self._with_ids else None

    @property
    def top_tokens(self) -> np.ndarray:
        n = self._rows * self._top
        return self._fetch()[2 * self._rows:2 * self._rows + n].view(np.int32).reshape(self._rows, self._top).copy()

    @property
    def top_logprobs(self) -> np.ndarray:
        n = self._rows * self._top
        return self._fetch()[2 * self._rows + n:2 * self._rows + 2 * n].view(np.float32).reshape(self._rows, self._top).copy()


def logprobs(logits, ids=None, top_n: int = 0) -> LogProbs:
    """Log-probabilities of the rows of ``logits`` [R, V] in one launch (include/npm_hip.h npm_logprob_rows): the normaliser is the
    sampler's integer mass at temperature 1, so the call is bitwise reproducible.  ``ids``: [R] integers or an ``IdBuffer`` of R
    entries (``result.ids`` of a ``Sampler`` call, a ``VerifyResult``'s); a row with ``ids[r] < 0`` is not read.  ``top_n``:
    0 .. 64 most probable tokens per row.  Apply a ``LogitProcessor`` first for the log-probabilities the sampler saw."""
    if not isinstance(logits, D.DeviceArray) or logits.ndim != 2 or logits.shape[0] < 1:
        raise ValueError(f'logprobs: logits must be a DeviceArray of shape [R, V], got {getattr(logits, "shape", type(logits).__name__)}')
    rows, vocab = logits.shape
    if not 1 <= vocab <= _C.SAMPLE_MAX_VOCAB:
        raise ValueError(f'logprobs: the vocabulary must be 1 .. {_C.SAMPLE_MAX_VOCAB}, got {vocab}')
    if isinstance(top_n, bool) or not isinstance(top_n, (int, np.integer)) or not 0 <= top_n <= _C.LOGPROB_MAX_TOP:
        raise ValueError(f'logprobs: top_n must be an integer in 0 .. {_C.LOGPROB_MAX_TOP}, got {top_n!r}')
    ids_dev = None
    if ids is not None:
        ids_dev = D.as_ids(ids)
        if ids_dev.size != rows:
            raise ValueError(f'logprobs: ids must hold {rows} integers, got shape {ids_dev.shape}')
    top_n = int(top_n)
    out = D.ByteBuffer(4 * (2 * rows + 2 * rows * top_n))
    desc = _C.npm_logprob(logits=logits.ptr, pitch=vocab, rows=rows, vocab=vocab, top_n=top_n,
                          ids=None if ids_dev is None else ids_dev.ptr, lse=out.ptr, chosen=out.ptr + 4 * rows,
                          top_token=out.ptr + 8 * rows if top_n else None,
                          top_logprob=out.ptr + 4 * (2 * rows + rows * top_n) if top_n else None)
    _C.check(_C.lib().npm_logprob_rows(C.byref(desc)), 'npm_logprob_rows')
    return LogProbs(out, rows, top_n, ids_dev is not None)
