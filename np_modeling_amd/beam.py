"""Beam search on the device (include/npm_hip.h npm_beam_step, csrc/npm_beam.hip).

``BeamSearch(groups, width)`` runs ``groups`` prompts with ``width`` beams each; slot ``g * width + w`` of the batch is beam w of
prompt g.  The beams' running scores live in HBM.  ``search(logits)`` scores the W x V continuations of every prompt, keeps the
best 2 W, and splits them into finished hypotheses (an ``eos`` among the first W) and the next W beams in ONE call of
npm_beam_step; one host copy of 36 G W bytes brings parents, tokens, log-sum-exps and the candidates.  The ids stay on
the device for ``Embedding.forward``; the parents go to ``DecodeState.reorder``, which on a paged cache moves table rows and
leaves the sharing to copy-on-write.

    search = beam.BeamSearch(groups, width, eos=2, max_new_tokens=64)
    # chunk [G W, T]: the prompt of group g in row g * width, -1 elsewhere; new_lengths: its length there, 0 elsewhere
    done = beam.decode_step(dec, state, emb, head, search, prompt=(chunk, new_lengths))
    while not done.all():
        done = beam.decode_step(dec, state, emb, head, search)
    best_tokens, best_score = search.hypotheses(0)[0]

A group's result depends on its own rows only, and the same logits give the same beams on every run.
"""

from __future__ import annotations

import ctypes as C
from typing import List, Optional, Tuple

import numpy as np

from np_modeling_amd import _C
from np_modeling_amd import device as D


class BeamStep:
    """What one ``BeamSearch.search`` produced, for the slots of the NEXT step.  ``ids``: device int32 [G W], the token every
    slot continues with (-1: dead -- ``Embedding.forward`` makes that a row of zeros), and ``host_ids`` the same on the host;
    ``parents``: host int64 [G W], the slot each one continues (-1: dead) -- ``DecodeState.reorder``'s vector; ``scores``: host
    float32 [G W], the running scores (-inf: dead); ``new_lengths``: host int64 [G W], 1 for a live slot and 0 for a dead one --
    ``decode``'s ``new_lengths``; ``done``: host bool [G].  ``lse`` (float32 [G W], of the rows just scored) and ``cand_slot`` /
    ``cand_token`` / ``cand_score`` ([G, 2 W]) are the call's other results as the device wrote them."""

    def __init__(self, ids, host_ids, parents, scores, done, lse, cand_slot, cand_token, cand_score):
        self.host_ids = host_ids
        self.ids, self.parents, self.scores, self.done, self.lse = ids, parents, scores, done, lse
        self.cand_slot, self.cand_token, self.cand_score = cand_slot, cand_token, cand_score
        self.new_lengths = (parents >= 0).astype(np.int64)


class BeamSearch:
    """``groups`` prompts of ``width`` beams (1 .. 32).  ``eos``: the token that ends a hypothesis (None: none does);
    ``length_penalty`` p: a hypothesis of n generated tokens (``eos`` included) with summed log-probability s scores
    ``s / n ** p``; ``max_new_tokens``: a group ends there and its live beams enter as unterminated hypotheses;
    ``early_stopping``: a group is done as soon as it holds ``width`` hypotheses -- otherwise only once its best live beam, over
    its length to the ``p``, cannot beat the worst one kept.

    Host state: every live beam's tokens and every group's best ``width`` hypotheses.  Device state: ``cum`` float32 [G W],
    ``[0, -inf, ...]`` per group at the start, so that only beam 0 is live and the prompt is scored once."""

    def __init__(self, groups: int, width: int, eos: Optional[int] = None, length_penalty: float = 1.0,
                 max_new_tokens: Optional[int] = None, early_stopping: bool = True):
        if int(groups) < 1 or not 1 <= int(width) <= _C.BEAM_MAX_WIDTH:
            raise ValueError(f'BeamSearch: groups >= 1 and width in 1 .. {_C.BEAM_MAX_WIDTH}, got {groups!r}, {width!r}')
        if eos is not None and (isinstance(eos, bool) or not isinstance(eos, (int, np.integer)) or not 0 <= eos < 2 ** 31):
            raise ValueError(f'BeamSearch: eos must be None or a token id in 0 .. 2^31 - 1, got {eos!r}')
        if max_new_tokens is not None and int(max_new_tokens) < 1:
            raise ValueError(f'BeamSearch: max_new_tokens must be None or at least 1, got {max_new_tokens!r}')
        self.groups, self.width, self.batch = int(groups), int(width), int(groups) * int(width)
        self.eos = None if eos is None else int(eos)
        self.length_penalty, self.early_stopping = float(length_penalty), bool(early_stopping)
        self.max_new_tokens = None if max_new_tokens is None else int(max_new_tokens)
        self._cum = D.ByteBuffer(4 * self.batch)
        self._workspace = D.ByteBuffer(_C.beam_workspace_bytes(self.groups, self.width))
        self.step: Optional[BeamStep] = None                  # the last search's result: what the next decode step is fed
        self.tokens: List[List[List[int]]] = [[] for _ in range(self.groups)]
        self.steps = np.zeros([self.groups], dtype=np.int64)
        self.done = np.zeros([self.groups], dtype=bool)
        self._hyps: List[List[Tuple[float, List[int]]]] = [[] for _ in range(self.groups)]
        for g in range(self.groups):
            self.reset(g)

    def _group(self, g) -> int:
        if isinstance(g, bool) or not isinstance(g, (int, np.integer)) or not 0 <= g < self.groups:
            raise ValueError(f'BeamSearch: group must be an integer in 0 .. {self.groups - 1}, got {g!r}')
        return int(g)

    def _write(self, address: int, values: np.ndarray) -> None:
        host = np.ascontiguousarray(values)
        _C.check(_C.lib().npm_h2d(address, host.ctypes.data, host.nbytes), 'npm_h2d')

    def reset(self, g: int) -> None:
        """Group ``g`` starts over for a newly admitted prompt: beam 0 live with score 0, the others dead, no tokens and no
        hypotheses.  The prompt goes into slot ``g * width`` of the cache; the first ``reorder`` forks it."""
        g = self._group(g)
        start = np.full([self.width], -np.inf, dtype=np.float32)
        start[0] = 0
        self._write(self._cum.ptr + 4 * g * self.width, start)
        self.tokens[g] = [[]] + [None] * (self.width - 1)
        self._hyps[g], self.steps[g], self.done[g] = [], 0, False

    def scores(self) -> np.ndarray:
        """The running scores as the device holds them, float32 [G W]."""
        return self._cum.numpy().view(np.float32).copy()

    def hypotheses(self, g: int) -> List[Tuple[List[int], float]]:
        """Group ``g``'s kept hypotheses, best first: [(tokens, score)], at most ``width``."""
        return [(list(tokens), score) for score, tokens in self._hyps[self._group(g)]]

    def _keep(self, g: int, score: float, tokens: List[int]) -> None:
        hyps = self._hyps[g]
        hyps.append((score, tokens))
        hyps.sort(key=lambda h: -h[0])                         # stable: the earlier of two equal scores stays in front
        del hyps[self.width:]

    def search(self, logits) -> BeamStep:
        """One beam step from ``logits`` [G W, V] (a ``DeviceArray``: row g W + w is what follows beam w of prompt g): one
        npm_beam_step and one host copy.  Finished candidates become hypotheses, the others the next beams; a group that is
        done has its beams set dead (two small uploads, only in the step that ends it)."""
        if not isinstance(logits, D.DeviceArray) or logits.ndim != 2 or logits.shape[0] != self.batch:
            raise ValueError(f'BeamSearch: logits must be a DeviceArray of shape [{self.batch}, V], got '
                             f'{getattr(logits, "shape", type(logits).__name__)}')
        vocab = logits.shape[1]
        if not 1 <= vocab <= _C.SAMPLE_MAX_VOCAB:
            raise ValueError(f'BeamSearch: the vocabulary must be 1 .. {_C.SAMPLE_MAX_VOCAB}, got {vocab}')
        g_, w_, n, c = self.groups, self.width, self.batch, 2 * self.width
        out = D.ByteBuffer(4 * (3 * n + 3 * g_ * c))           # parent | ids | lse | cand_slot | cand_token | cand_score
        at = [out.ptr + 4 * k for k in (0, n, 2 * n, 3 * n, 3 * n + g_ * c, 3 * n + 2 * g_ * c)]
        desc = _C.npm_beam(logits=logits.ptr, pitch=vocab, groups=g_, width=w_, vocab=vocab, eos=-1 if self.eos is None else self.eos,
                           cum=self._cum.ptr, parent=at[0], ids=at[1], lse=at[2], cand_slot=at[3], cand_token=at[4], cand_score=at[5],
                           workspace=self._workspace.ptr, workspace_bytes=self._workspace.nbytes)
        _C.check(_C.lib().npm_beam_step(C.byref(desc)), 'npm_beam_step')
        words = out.numpy().view(np.int32)
        parents, ids = words[:n].astype(np.int64), words[n:2 * n].copy()
        lse = words[2 * n:3 * n].view(np.float32).copy()
        cand_slot, cand_token = (words[3 * n + k * g_ * c:3 * n + (k + 1) * g_ * c].reshape(g_, c).copy() for k in (0, 1))
        cand_score = words[3 * n + 2 * g_ * c:].view(np.float32).reshape(g_, c).copy()
        scores = np.full([n], -np.inf, dtype=np.float32)
        for g in range(g_):
            if self.done[g]:
                continue
            first = g * w_
            old, length = self.tokens[g], int(self.steps[g]) + 1
            others = [p for p in range(c) if cand_slot[g, p] >= 0 and not (self.eos is not None and cand_token[g, p] == self.eos)][:w_]
            scores[first:first + len(others)] = cand_score[g, others]        # what the device wrote into cum: the split is integer logic
            for p in range(w_):
                if cand_slot[g, p] >= 0 and self.eos is not None and cand_token[g, p] == self.eos:
                    self._keep(g, float(np.float64(cand_score[g, p]) / length ** self.length_penalty),
                               old[cand_slot[g, p] - first] + [self.eos])
            self.tokens[g] = [old[parents[first + j] - first] + [int(ids[first + j])] if parents[first + j] >= 0 else None
                              for j in range(w_)]
            self.steps[g] = length
            live = [j for j in range(w_) if parents[first + j] >= 0]
            if not live:
                self.done[g] = True
            elif len(self._hyps[g]) >= w_:
                best = float(np.float64(scores[first + live[0]]) / length ** self.length_penalty)
                self.done[g] = self.early_stopping or best <= self._hyps[g][-1][0]
            if not self.done[g] and self.max_new_tokens is not None and length >= self.max_new_tokens:
                for j in live:
                    self._keep(g, float(np.float64(scores[first + j]) / length ** self.length_penalty), self.tokens[g][j])
                self.done[g] = True
            if self.done[g] and live:
                dead = np.full([w_], -1, dtype=np.int32)
                self._write(self._cum.ptr + 4 * first, np.full([w_], -np.inf, dtype=np.float32))
                self._write(at[1] + 4 * first, dead)
                parents[first:first + w_], ids[first:first + w_], scores[first:first + w_] = -1, -1, -np.inf
                self.tokens[g] = [None] * w_
        self.step = BeamStep(D.IdBuffer([n], out._buf, at[1]), ids, parents, scores, self.done.copy(), lse, cand_slot, cand_token,
                             cand_score)
        return self.step

    __call__ = search


def decode_step(dec, state, emb, head, search: BeamSearch, prompt=None) -> np.ndarray:
    """One beam step for the ``groups * width`` slots of ``state``; which groups are done, bool [G].  ``dec`` a
    ``TransformerDecoder``, ``state`` its ``DecodeState``, ``emb`` an ``Embedding``, ``head`` the layer that turns [rows, F] into
    logits, ``search`` a ``BeamSearch``.

    ``emb.forward(ids)`` -> ``dec.decode(x, state, new_lengths=)`` -> ``head`` on the G W rows -> ``search(logits)`` ->
    ``state.reorder(parents)``.  The ids and ``new_lengths`` are those of the last ``search``; the first step of a prompt takes
    ``prompt = (chunk, new_lengths)`` instead: ``chunk`` int [G W, T], right-padded with -1, holding group g's prompt in row
    ``g * width`` only, and ``new_lengths`` [G W] its length there and 0 for the other beams, both as host integers.  Groups that
    are in flight ride along: their rows of the chunk are replaced by the token each beam continues with.  The first reorder
    makes the other beams forks of slot ``g * width``; a slot that is empty in the cross-attention cache receives its parent's
    memory by a copy first (the beams of a prompt admitted into a finished group's slots).

    A step costs the decode step's launches, two for npm_beam_step and one host copy; on a paged cache the reorder launches
    nothing and the next append copies at most one partly filled page per beam that shares its tail."""
    batch = search.batch
    if state.self_cache.batch != batch:
        raise ValueError(f'decode_step: the cache holds {state.self_cache.batch} slots, the search {batch}')
    if prompt is not None:
        chunk, new_lengths = (np.array(v) for v in prompt)
        if chunk.ndim != 2 or chunk.shape[0] != batch or new_lengths.shape != (batch,) or not np.issubdtype(chunk.dtype, np.integer):
            raise ValueError(f'decode_step: prompt is (ids [{batch}, T], new_lengths [{batch}]) as host integers, got {chunk.shape} '
                             f'and {new_lengths.shape}')
        running = np.repeat((search.steps > 0) & ~search.done, search.width)
        if running.any():                                                     # groups in flight ride along with their own token
            chunk[running, 0], chunk[running, 1:] = search.step.host_ids[running], -1
            new_lengths[running] = search.step.new_lengths[running]
        tokens = chunk.shape[1]
        last = np.arange(batch) * tokens + np.maximum(new_lengths, 1) - 1
    elif search.step is None:
        raise ValueError('decode_step: nothing was searched yet: the first step takes prompt=(chunk, new_lengths)')
    else:
        chunk, new_lengths, tokens, last = search.step.ids, search.step.new_lengths, 1, None
    x = emb.forward(chunk)
    features = x.shape[-1]
    hidden = dec.decode(x.reshape(batch, tokens, features), state, new_lengths=new_lengths)
    rows = hidden.reshape(batch * tokens, features)
    logits = head(rows if last is None else D.take_rows(rows, last))
    step = search(logits)
    cross, parents = state.cross_cache, step.parents
    for b in np.nonzero((parents >= 0) & (cross.lengths == 0))[0]:            # a beam slot that was dead: its parent's memory
        if cross.lengths[parents[b]] > 0:
            cross.fork(int(parents[b]), int(b))
    state.reorder(parents)
    return step.done
