"""Speculative decoding: several tokens per decode step, exactly the tokens of the one-token-per-step loop.

A step feeds every sequence its last token and up to T drafted tokens (``sampling.NgramDrafter``: what followed the most recent
earlier occurrence of its last few tokens), runs ``TransformerDecoder.decode`` and the vocabulary projection on all T + 1 rows
-- the rows of a decode step are nearly free -- and samples every row with the sequence's own parameters and counters
(``sampling.Sampler.verify``).  Drafted tokens are accepted while they are the tokens sampled; the K / V rows of the others leave
the cache again (``DecodeState.truncate``).  Since row r is sampled at counter ``draw + r`` from the logits that follow the
accepted prefix, the tokens emitted are those ``sampler(logits)`` gives one step at a time, seed for seed; only the logits'
last bits can differ, as between any two chunk sizes of ``decode``.

    drafter = sampling.NgramDrafter(batch, capacity, max_draft=4)
    ...                                    # the prompt through decode(); first = sampler(logits).numpy()
    drafter.admit(b, list(prompt_b) + [first[b]])
    while ...:
        emitted = speculative.decode_step(dec, state, emb, head, sampler, drafter)        # per slot: 1 .. T + 1 tokens
"""

from __future__ import annotations

from typing import List, Optional

import numpy as np

from np_modeling_amd import device as D


def decode_step(dec, state, emb, head, sampler, drafter, active=None, processor=None) -> List[List[int]]:
    """One speculative step for the sequences of ``state``; the tokens each slot emitted (an empty list for a slot that is not
    ``active``, holds no history or has no room left).  ``dec`` a ``TransformerDecoder``, ``state`` its ``DecodeState``, ``emb`` an
    ``Embedding``, ``head`` the layer that turns [rows, F] into logits, ``sampler`` a ``Sampler`` and ``drafter`` an
    ``NgramDrafter`` whose slot b holds sequence b's tokens so far, the last of which the cache has not seen yet.

    Propose (``limit[b] = min(T, capacity - lengths[b] - 1)``, so that the chunk always fits the cache) -> ``emb.forward(chunk)``
    -> ``dec.decode(x, state, new_lengths=n_new)`` -> ``head`` on all B (T + 1) rows -> ``sampler.verify(..., history=drafter)`` ->
    ``state.truncate(n_new - 1 - accepted)``.

    ``processor``: a ``sampling.LogitProcessor`` applied to the logits between ``head`` and the verify, with the drafter as its
    history and the chunk as its draft: one more launch, no copy to the host.  Row r is processed as if the r drafted tokens
    before it stood in the history already, and it counts only when they were the tokens sampled -- so the step emits the tokens of
    the loop ``processor(logits, history) -> sampler(logits) -> history.append(result)``, seed for seed and counter for counter.

    One copy to the host per step in the steady state: right behind the verify the NEXT step's proposal is launched, with the
    limits the next step will ask for if the same slots stay active and none comes within 2 T + 2 rows of its capacity, and its
    ``n_new`` comes to the host in the verify result's copy.  A step whose limits turn out different (a slot finished, was
    admitted or nears its capacity) proposes again and pays a second copy of 4 bytes per slot; never more than two."""
    cache = state.self_cache
    batch, t = drafter.batch, drafter.max_draft
    if cache.batch != batch or sampler.batch != batch:
        raise ValueError(f'decode_step: the cache ({cache.batch}), the sampler ({sampler.batch}) and the drafter ({batch}) differ in batch')
    limit = np.minimum(t, cache.capacity - cache.lengths - 1)
    if active is not None:
        on = np.asarray(active)
        if on.shape != (batch,):
            raise ValueError(f'decode_step: active must be {batch} flags, got {on.tolist()!r}')
        limit = np.where(on.astype(bool), limit, -1)
    chunk, n_new = drafter.propose(limit)
    x = emb.forward(chunk)                                               # [B, T + 1, F]; a -1 gives a row of zeros
    hidden = dec.decode(x, state, new_lengths=n_new)
    logits = head(hidden.reshape(batch * (t + 1), hidden.shape[2]))
    draft = D.IdBuffer([batch, t], chunk._buf, chunk.ptr + 4)            # the chunk behind its first column
    if processor is not None:
        processor(logits, drafter, draft=draft, n_draft=n_new - 1, draft_pitch=t + 1)
    # the limits of the next step when every drafted token is accepted: they are the next step's own wherever both are T
    ahead = np.where(limit >= 0, np.minimum(t, cache.capacity - cache.lengths - 1), -1)
    result = sampler.verify(logits, draft, n_new - 1, history=drafter, draft_pitch=t + 1, extra_words=batch,
                            before_fetch=lambda address: drafter.propose_ahead(ahead, address))
    drafter.settle_ahead(result.extra)
    accepted, tokens = result.accepted, result.numpy()
    state.truncate(np.where(n_new > 0, n_new - 1 - accepted, 0))
    return [[int(v) for v in tokens[b, :accepted[b] + 1] if v >= 0] if n_new[b] > 0 else [] for b in range(batch)]
