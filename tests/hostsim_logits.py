"""TEST INFRASTRUCTURE ONLY -- tests/hostsim_beam.py's simulator plus the entry points of the logit processors: npm_logits_process,
npm_history_append, npm_logprob_rows and npm_last_logits_kernel, restated through tests/logits_reference.py with the argument
checks of the entry points.  The workspace must be all zero on entry (AssertionError otherwise: the caller broke the contract)
and is left all zero; inactive slots' rows are never touched.  ``processed`` and ``logprob_calls`` record the arguments of every
call; ``d2h`` (tests/hostsim_spec.py) the byte count of every copy to the host."""

import ctypes as C

import numpy as np

import hostsim_beam
import logits_reference as LR
from hostsim import _addr, _deref, _mat
from hostsim_sample import _words

BAD = 10002


def _opt(ptr, n, ctype):
    return _words(ptr, n, ctype) if _addr(ptr) else None


class LogitsHostSim(hostsim_beam.BeamHostSim):
    def __init__(self):
        super().__init__()
        self.processed = []
        self.logprob_calls = []
        self._last_logits = b''

    def npm_logits_process(self, pref):
        self.calls.append('npm_logits_process')
        if pref is None:
            return BAD
        p = _deref(pref)
        self.processed.append(dict(batch=p.batch, rows=p.rows, vocab=p.vocab, history=_addr(p.history), bias_cap=p.bias_cap))
        if not _addr(p.logits) or not _addr(p.workspace):
            return BAD
        if p.batch < 1 or not 1 <= p.rows <= 64 or not 1 <= p.vocab <= (1 << 20) or p.pitch < p.vocab or p.batch * p.rows >= 2 ** 31:
            return BAD
        if not _addr(p.n_draft) and p.rows != 1:
            return BAD
        if p.rows > 1 and (not _addr(p.draft) or p.draft_pitch < p.rows - 1):
            return BAD
        if _addr(p.history) and (not _addr(p.history_len) or p.history_cap < 1 or p.history_pitch < p.history_cap):
            return BAD
        if not 0 <= p.bias_cap <= 256:
            return BAD
        if p.bias_cap > 0 and not (_addr(p.bias_index) and _addr(p.bias_value) and _addr(p.bias_count)):
            return BAD
        b, rows = p.batch, p.rows
        workspace = _words(p.workspace, b * p.vocab, C.c_int32)
        assert not workspace.any(), 'npm_logits_process: the workspace is not all zero on entry'
        active, n_draft = _opt(p.active, b, C.c_int32), _opt(p.n_draft, b, C.c_int32)
        live = [s for s in range(b) if (active is None or active[s] != 0) and (n_draft is None or n_draft[s] >= 0)]
        history = draft = None
        if _addr(p.history):
            history = np.lib.stride_tricks.as_strided(_words(p.history, (b - 1) * p.history_pitch + p.history_cap, C.c_int32),
                                                      shape=(b, p.history_cap), strides=(4 * p.history_pitch, 4))
        if _addr(p.draft) and rows > 1:
            draft = np.lib.stride_tricks.as_strided(_words(p.draft, (b - 1) * p.draft_pitch + rows - 1, C.c_int32),
                                                    shape=(b, rows - 1), strides=(4 * p.draft_pitch, 4))
        bias = dict(bias_cap=p.bias_cap)
        if p.bias_cap > 0:
            bias.update(bias_index=_words(p.bias_index, b * p.bias_cap, C.c_int32).reshape(b, p.bias_cap),
                        bias_value=_words(p.bias_value, b * p.bias_cap, C.c_float).reshape(b, p.bias_cap),
                        bias_count=_words(p.bias_count, b, C.c_int32))
        params = dict(history_len=_opt(p.history_len, b, C.c_int32), prompt_len=_opt(p.prompt_len, b, C.c_int32),
                      repetition=_opt(p.repetition, b, C.c_float), presence=_opt(p.presence, b, C.c_float),
                      frequency=_opt(p.frequency, b, C.c_float), eos=_opt(p.eos, b, C.c_int32), min_new=_opt(p.min_new, b, C.c_int32))
        for s in live:                                 # slot by slot: an inactive slot's memory is never touched
            z = _mat(_addr(p.logits) + 4 * s * rows * p.pitch, rows, p.vocab, p.pitch)
            one = lambda v: None if v is None else v[s:s + 1]
            LR.process(z, 1, rows, p.vocab, history=one(history), history_cap=p.history_cap, draft=one(draft),
                       n_draft=one(n_draft), **{k: one(v) for k, v in params.items()},
                       **{k: (v if k == 'bias_cap' else one(v)) for k, v in bias.items()})
        self._last_logits = b'hostsim npm_logits_process'
        return 0

    def npm_history_append(self, history, history_pitch, history_cap, history_len, ids, active, batch):
        self.calls.append('npm_history_append')
        if batch < 1 or history_cap < 1 or history_pitch < history_cap:
            return BAD
        if not all(_addr(q) for q in (history, history_len, ids)):
            return BAD
        lines = np.lib.stride_tricks.as_strided(_words(history, (batch - 1) * history_pitch + history_cap, C.c_int32),
                                                shape=(batch, history_cap), strides=(4 * history_pitch, 4))
        LR.history_append(lines, _words(history_len, batch, C.c_int32), history_cap, _words(ids, batch, C.c_int32),
                          _opt(active, batch, C.c_int32))
        self._last_logits = b'hostsim npm_history_append'
        return 0

    def npm_logprob_rows(self, pref):
        self.calls.append('npm_logprob_rows')
        if pref is None:
            return BAD
        p = _deref(pref)
        self.logprob_calls.append(dict(rows=p.rows, vocab=p.vocab, top_n=p.top_n, ids=_addr(p.ids)))
        if p.rows < 1 or not 1 <= p.vocab <= (1 << 20) or p.pitch < p.vocab or not 0 <= p.top_n <= 64:
            return BAD
        if not _addr(p.logits) or not _addr(p.lse) or (_addr(p.ids) and not _addr(p.chosen)):
            return BAD
        if p.top_n > 0 and not (_addr(p.top_token) and _addr(p.top_logprob)):
            return BAD
        ids = _opt(p.ids, p.rows, C.c_int32)
        lse = _words(p.lse, p.rows, C.c_float)
        chosen = _words(p.chosen, p.rows, C.c_float) if ids is not None else None
        for r in range(p.rows):
            skipped = ids is not None and ids[r] < 0
            z = np.zeros([p.vocab], dtype=np.float32) if skipped else _mat(_addr(p.logits) + 4 * r * p.pitch, 1, p.vocab, p.pitch)[0]
            out = LR.logprob_row(z, None if ids is None else int(ids[r]), p.top_n)
            lse[r] = out[0]
            if chosen is not None:
                chosen[r] = out[1]
            if p.top_n:
                _words(p.top_token, p.rows * p.top_n, C.c_int32)[r * p.top_n:(r + 1) * p.top_n] = out[2]
                _words(p.top_logprob, p.rows * p.top_n, C.c_float)[r * p.top_n:(r + 1) * p.top_n] = out[3]
        return 0

    def npm_last_logits_kernel(self):
        return self._last_logits


def install():
    from np_modeling_amd import _C
    sim = LogitsHostSim()
    _C._LIB = sim
    _C._DEVICE = 0
    return sim


uninstall = hostsim_beam.uninstall
