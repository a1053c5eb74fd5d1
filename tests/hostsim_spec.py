"""TEST INFRASTRUCTURE ONLY -- tests/hostsim_sample.py's simulator plus the entry points of speculative decoding, npm_verify_rows and
npm_ngram_draft, restated through tests/spec_reference.py with the argument checks of the entry points.  General rows take
NumPy's float32 exponential, as ``SampleHostSim.npm_sample_rows`` does, so the simulated verify and the simulated one-token loop
agree with each other.  ``d2h`` records the byte count of every npm_d2h call."""

import ctypes as C

import numpy as np

import hostsim_sample
import sample_reference as SR
import spec_reference as XR
from hostsim import HostSim, _addr, _deref, _mat
from hostsim_sample import _words
from hostsim_varlen import _ints

BAD = 10002


class SpecHostSim(hostsim_sample.SampleHostSim):
    def __init__(self):
        super().__init__()
        self.d2h = []
        self.verifies = []

    def npm_d2h(self, dst, src, nbytes):
        self.d2h.append(int(nbytes))
        return HostSim.npm_h2d(self, dst, src, nbytes)

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
        if self.calls and [c for c in self.calls if c in ('npm_sample_rows', 'npm_verify_rows')][-1:] == ['npm_verify_rows']:
            return b'hostsim npm_verify_rows'
        return super().npm_last_sample_kernel()

    def npm_last_draft_kernel(self):
        return b'hostsim npm_ngram_draft' if 'npm_ngram_draft' in self.calls else b''


def install():
    from np_modeling_amd import _C
    sim = SpecHostSim()
    _C._LIB = sim
    _C._DEVICE = 0
    return sim


uninstall = hostsim_sample.uninstall
