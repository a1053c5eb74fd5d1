"""TEST INFRASTRUCTURE ONLY -- tests/hostsim_window.py's simulator plus the entry points of token generation: npm_take_rows,
npm_embedding_bwd (a float32 loop in the stated order) and npm_sample_rows, restated through tests/sample_reference.py with the
argument checks of the entry points.  The simulator's weights come from NumPy's float32 exponential: the contract's steps, not
the device's last bit.  ``samples`` records the arguments of every npm_sample_rows call."""

import ctypes as C

import numpy as np

import hostsim_window
import sample_reference as SR
from hostsim import _addr, _deref, _mat
from hostsim_varlen import _ints


def _words(ptr, n, ctype):
    return np.ctypeslib.as_array((ctype * int(n)).from_address(_addr(ptr)))


class SampleHostSim(hostsim_window.WindowHostSim):
    def __init__(self):
        super().__init__()
        self.samples = []

    def npm_take_rows(self, src, src_pitch, src_rows, idx, dst, dst_pitch, n, cols):
        self.calls.append('npm_take_rows')
        if min(n, cols, src_rows) < 0 or src_pitch < cols or dst_pitch < cols:
            return 10002
        if n == 0 or cols == 0:
            return 0
        if not (_addr(idx) and _addr(dst) and (_addr(src) or src_rows == 0)):
            return 10002
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
            return 10002
        if distinct == 0 or cols == 0:
            return 0
        if not (_addr(dy) and _addr(order) and _addr(starts) and _addr(tokens) and _addr(dw)):
            return 10002
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
            return 10002
        if not all(_addr(p) for p in (s.logits, s.temperature, s.top_k, s.top_p, s.seed, s.draw, s.token)):
            return 10002
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

    def npm_last_sample_kernel(self):
        return b'hostsim npm_sample_rows' if self.samples else b''


def install():
    from np_modeling_amd import _C
    sim = SampleHostSim()
    _C._LIB = sim
    _C._DEVICE = 0
    return sim


uninstall = hostsim_window.uninstall
