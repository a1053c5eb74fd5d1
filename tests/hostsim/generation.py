"""TEST INFRASTRUCTURE ONLY -- the entry points of token generation, each restated once through its reference with the argument
checks of the entry point: npm_take_rows and npm_embedding_bwd (a float32 loop in the stated order), npm_sample_rows
(tests/sample_reference.py), npm_verify_rows and npm_ngram_draft (tests/spec_reference.py), npm_beam_step
(tests/beam_reference.py), npm_logits_process, npm_history_append and npm_logprob_rows (tests/logits_reference.py).

General rows take NumPy's float32 exponential (``sample_reference.weights32``) in the sampler, the verifier and the beam step
alike, so the simulated loops agree with each other: the contract's steps, not the device's last bit.  Dead beam rows and
inactive slots' rows are never touched; the beam workspace is filled with a pattern, as memory whose contents are unspecified;
the logit processors' workspace must be all zero on entry (AssertionError otherwise: the caller broke the contract) and is left
all zero.  ``samples``, ``verifies``, ``beams``, ``processed`` and ``logprob_calls`` record the arguments of every call."""

import ctypes as C

import numpy as np

import beam_reference as BR
import logits_reference as LR
import sample_reference as SR
import spec_reference as XR

from .memory import BAD, _addr, _deref, _ints, _mat, _vec, _words


def _opt(ptr, n, ctype):
    return _words(ptr, n, ctype) if _addr(ptr) else None


class Generation:
    def __init__(self):
        super().__init__()
        self.samples, self.verifies, self.beams, self.processed, self.logprob_calls = [], [], [], [], []
        self._last_logits = b''

    # ---- rows in, rows out ---------------------------------------------------------------------------------------------------------------
    def npm_take_rows(self, src, src_pitch, src_rows, idx, dst, dst_pitch, n, cols):
        self.calls.append('npm_take_rows')
        if min(n, cols, src_rows) < 0 or src_pitch < cols or dst_pitch < cols:
            return BAD
        if n == 0 or cols == 0:
            return 0
        if not (_addr(idx) and _addr(dst) and (_addr(src) or src_rows == 0)):
            return BAD
        index = _words(idx, n, C.c_int32)
        inside = (index >= 0) & (index < src_rows)
        out = _mat(dst, n, cols, dst_pitch)
        out[~inside] = 0
        if inside.any():
            out[inside] = _mat(src, src_rows, cols, src_pitch)[index[inside]]
        return 0

    def npm_embedding_bwd(self, dy, dy_pitch, order, starts, tokens, distinct, dw, dw_pitch, cols):
        self.calls.append('npm_embedding_bwd')
        if distinct < 0 or cols < 0 or dy_pitch < cols or dw_pitch < cols:
            return BAD
        if distinct == 0 or cols == 0:
            return 0
        if not (_addr(dy) and _addr(order) and _addr(starts) and _addr(tokens) and _addr(dw)):
            return BAD
        seg, tok = _words(starts, distinct + 1, C.c_int32), _words(tokens, distinct, C.c_int32)
        rows = _words(order, seg[-1], C.c_int32)
        grad = _mat(dy, int(rows.max()) + 1, cols, dy_pitch)
        for s in range(distinct):
            acc = grad[rows[seg[s]]].copy()
            for j in range(seg[s] + 1, seg[s + 1]):
                acc += grad[rows[j]]
            _mat(dw, int(tok[s]) + 1, cols, dw_pitch)[tok[s]] = acc
        return 0

    def npm_sample_rows(self, sref):
        s = _deref(sref)
        self.calls.append('npm_sample_rows')
        self.samples.append(dict(batch=s.batch, vocab=s.vocab, pitch=s.pitch, active=_addr(s.active)))
        if s.batch < 1 or not 1 <= s.vocab <= (1 << 20) or s.pitch < s.vocab:
            return BAD
        if not all(_addr(p) for p in (s.logits, s.temperature, s.top_k, s.top_p, s.seed, s.draw, s.token)):
            return BAD
        b = s.batch
        z = _mat(s.logits, b, s.vocab, s.pitch)
        t, p, k = _words(s.temperature, b, C.c_float), _words(s.top_p, b, C.c_float), _ints(s.top_k, b)
        seed, draw = _words(s.seed, b, C.c_uint64), _words(s.draw, b, C.c_uint64)
        active = _ints(s.active, b) if _addr(s.active) else np.ones(b, dtype=np.int64)
        token = _words(s.token, b, C.c_int32)
        kept = _words(s.kept, b, C.c_int32) if _addr(s.kept) else np.zeros(b, dtype=np.int32)
        prob = _words(s.prob, b, C.c_float) if _addr(s.prob) else np.zeros(b, dtype=np.float32)
        for r in range(b):
            if not active[r]:
                token[r], kept[r], prob[r] = -1, 0, 0
                continue
            general = t[r] > 0 and k[r] != 1 and not SR.invalid_row(z[r], t[r], p[r])
            row = SR.ExactRow(z[r], float(t[r]), int(k[r]), float(p[r]), SR.weights32(z[r], t[r]) if general else None)
            token[r], kept[r], prob[r] = row.draw(int(seed[r]), int(draw[r]))
            draw[r] += np.uint64(1)
        return 0

    # ---- speculative decoding ---------------------------------------------------------------------------------------------------------------
    def npm_verify_rows(self, vref):
        v = _deref(vref)
        self.calls.append('npm_verify_rows')
        self.verifies.append(dict(batch=v.batch, rows=v.rows, vocab=v.vocab, history=_addr(v.history)))
        if v.batch < 1 or not 1 <= v.rows <= 64 or not 1 <= v.vocab <= (1 << 20) or v.pitch < v.vocab or v.batch * v.rows >= 2 ** 31:
            return BAD
        if not all(_addr(p) for p in (v.logits, v.temperature, v.top_k, v.top_p, v.seed, v.draw, v.n_draft, v.token, v.accepted)):
            return BAD
        if v.rows > 1 and (not _addr(v.draft) or v.draft_pitch < v.rows - 1):
            return BAD
        if _addr(v.history) and (not _addr(v.history_len) or v.history_cap < 1 or v.history_pitch < v.history_cap):
            return BAD
        b, rows = v.batch, v.rows
        z = _mat(v.logits, b * rows, v.vocab, v.pitch)
        t, p, k = _words(v.temperature, b, C.c_float), _words(v.top_p, b, C.c_float), _ints(v.top_k, b)
        seed, draw = _words(v.seed, b, C.c_uint64), _words(v.draw, b, C.c_uint64)
        n = np.minimum(_ints(v.n_draft, b), rows - 1)
        token, accepted = _words(v.token, b * rows, C.c_int32).reshape(b, rows), _words(v.accepted, b, C.c_int32)
        kept = _words(v.kept, b * rows, C.c_int32).reshape(b, rows) if _addr(v.kept) else np.zeros([b, rows], dtype=np.int32)
        prob = _words(v.prob, b * rows, C.c_float).reshape(b, rows) if _addr(v.prob) else np.zeros([b, rows], dtype=np.float32)
        for s in range(b):
            drafted = _words(v.draft, (b - 1) * v.draft_pitch + rows - 1, C.c_int32)[s * v.draft_pitch:] if rows > 1 else []
            token[s], accepted[s], after, kept[s], prob[s] = XR.verify(z[s * rows:(s + 1) * rows], float(t[s]), int(k[s]), float(p[s]),
                                                                       int(seed[s]), int(draw[s]), drafted, int(n[s]), SR.weights32)
            draw[s] = np.uint64(after)
            if _addr(v.history) and n[s] >= 0:
                length = _words(v.history_len, b, C.c_int32)
                line = _words(v.history, (b - 1) * v.history_pitch + v.history_cap, C.c_int32)[s * v.history_pitch:]
                for tok in token[s, :accepted[s] + 1]:
                    if tok >= 0 and length[s] < v.history_cap:
                        line[length[s]] = tok
                        length[s] += 1
        return 0

    def npm_ngram_draft(self, history, history_pitch, history_cap, history_len, limit, batch, max_draft, nmax, nmin, chunk, n_new):
        self.calls.append('npm_ngram_draft')
        if batch < 1 or not 0 <= max_draft <= 63 or nmin < 1 or nmax < nmin or nmax > 8 or history_cap < 1 or history_pitch < history_cap:
            return BAD
        if not all(_addr(p) for p in (history, history_len, chunk, n_new)):
            return BAD
        lengths = np.minimum(_ints(history_len, batch), history_cap)
        limits = _ints(limit, batch) if _addr(limit) else np.full([batch], max_draft)
        lines = _words(history, (batch - 1) * history_pitch + history_cap, C.c_int32)
        out, count = _words(chunk, batch * (max_draft + 1), C.c_int32).reshape(batch, max_draft + 1), _words(n_new, batch, C.c_int32)
        for s in range(batch):
            line = lines[s * history_pitch:s * history_pitch + max(int(lengths[s]), 0)]
            out[s], count[s], _ = XR.draft(line, max_draft, int(limits[s]), nmax, nmin)
        return 0

    def npm_last_sample_kernel(self):
        last = [c for c in self.calls if c in ('npm_sample_rows', 'npm_verify_rows')][-1:]
        if last == ['npm_verify_rows']:
            return b'hostsim npm_verify_rows'
        return b'hostsim npm_sample_rows' if self.samples else b''

    def npm_last_draft_kernel(self):
        return b'hostsim npm_ngram_draft' if 'npm_ngram_draft' in self.calls else b''

    # ---- beam search ------------------------------------------------------------------------------------------------------------------------
    def npm_beam_step(self, sref):
        self.calls.append('npm_beam_step')
        if sref is None:
            return BAD
        s = _deref(sref)
        self.beams.append(dict(groups=s.groups, width=s.width, vocab=s.vocab, pitch=s.pitch, eos=s.eos))
        if s.groups < 1 or not 1 <= s.width <= 32 or not 1 <= s.vocab <= (1 << 20) or s.pitch < s.vocab:
            return BAD
        if s.groups * s.width * 2 * s.width >= 2 ** 31:
            return BAD
        if not all(_addr(p) for p in (s.logits, s.cum, s.lse, s.parent, s.ids, s.cand_slot, s.cand_token, s.cand_score, s.workspace)):
            return BAD
        need = 4 * s.groups * s.width * (1 + 4 * s.width)
        if s.workspace_bytes < need or _addr(s.workspace) % 4:
            return BAD
        n, cands = s.groups * s.width, 2 * s.width
        cum = _words(s.cum, n, C.c_float)
        # rows one at a time: a dead row's memory is never touched
        rows = {r: _vec(_addr(s.logits) + 4 * r * s.pitch, s.vocab) for r in range(n) if BR.live(cum[r])}
        out = BR.step(rows, cum, s.groups, s.width, s.eos)
        _words(s.workspace, need // 4, C.c_int32)[:] = 0x5A5A5A5A
        _words(s.cand_slot, s.groups * cands, C.c_int32)[:] = out['cand_slot'].ravel()
        _words(s.cand_token, s.groups * cands, C.c_int32)[:] = out['cand_token'].ravel()
        _words(s.cand_score, s.groups * cands, C.c_float)[:] = out['cand_score'].ravel()
        _words(s.parent, n, C.c_int32)[:] = out['parent']
        _words(s.ids, n, C.c_int32)[:] = out['ids']
        _words(s.lse, n, C.c_float)[:] = out['lse']
        cum[:] = out['cum']
        return 0

    def npm_last_beam_kernel(self):
        return b'hostsim npm_beam_step' if self.beams else b''

    # ---- logit processors ---------------------------------------------------------------------------------------------------------------------
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
