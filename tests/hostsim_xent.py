"""TEST INFRASTRUCTURE ONLY -- the host simulator plus npm_softmax_xent_rows, by composition.

The simulator's entry points are pinned to its recorded profiles (tests/test_hostsim_host.py) and ``HostSim`` has no subclasses, so
the two entry points of np_modeling_amd/csrc/npm_xent.hip are not part of it.  ``XentLib`` wraps an installed simulator: every
attribute it does not define is the simulator's (memory, copies, ``calls``, ``live`` / ``peak``, every other entry point), and the two
entry points are restated here with tests/xent_reference.py over the simulator's memory views.  ``install()`` puts it where the
product looks for its library."""

import numpy as np
import xent_cases
import xent_reference
from hostsim import install as install_sim
from hostsim.memory import BAD, _addr, _deref, _ints, _mat, _vec


class XentLib:
    def __init__(self, sim):
        self.sim = sim
        self._last_xent = b''

    def __getattr__(self, name):                # only what this class does not define
        return getattr(self.sim, name)

    def npm_softmax_xent_rows(self, logits, ld, targets, rows, vocab, smoothing, grad_scale, dlogits, ldd, row_loss, row_lse, loss_sum):
        self.sim.calls.append('npm_softmax_xent_rows')
        rows, vocab, ld, ldd = int(rows), int(vocab), int(ld), int(ldd)
        z_at, d_at = _addr(logits), _addr(dlogits)
        if loss_sum is None or not 0 <= rows < 2 ** 31 or not 1 <= vocab <= 2 ** 30 or ld < vocab or not 0.0 <= smoothing < 1.0:
            return BAD
        if d_at and ldd < vocab:
            return BAD
        if rows == 0:
            self._last_xent = b'xent_none rows=0'
            _deref(loss_sum).value = 0.0
            return 0
        if not z_at or not _addr(targets) or not _addr(row_loss):
            return BAD
        if d_at == z_at and d_at:
            if ldd != ld:
                return BAD
        elif d_at:
            z_end, d_end = z_at + 4 * ((rows - 1) * ld + vocab), d_at + 4 * ((rows - 1) * ldd + vocab)
            if not (z_end <= d_at or d_end <= z_at):
                return BAD
        t = _ints(targets, rows)
        z = _mat(logits, rows, vocab, ld)
        # an ignored row is not read: it may hold anything
        seen = np.where((t >= 0)[:, None], z, 0.0).astype(np.float64)
        ref = xent_reference.reference(seen, t, smoothing, grad_scale, need_grad=bool(d_at))
        with np.errstate(over='ignore'):
            if d_at:
                _mat(dlogits, rows, vocab, ldd)[:] = ref.grad.astype(np.float32)
            _vec(row_loss, rows)[:] = ref.row_loss.astype(np.float32)
            if _addr(row_lse):
                _vec(row_lse, rows)[:] = ref.lse.astype(np.float32)
        _deref(loss_sum).value = float(_vec(row_loss, rows).astype(np.float64).sum())
        vec = z_at % 16 == 0 and ld % 4 == 0 and (not d_at or (d_at % 16 == 0 and ldd % 4 == 0))
        self._last_xent = ('%s V=%d grad=%d inplace=%d vec=%d nt=%d' % (xent_cases.instance_of(vocab), vocab, bool(d_at), d_at == z_at,
                                                                        vec, 4 * rows * vocab >= 32 << 20)).encode()
        return 0

    def npm_last_xent_kernel(self):
        return self._last_xent


def install(profile=None):
    """A fresh simulator wrapped in an ``XentLib``, installed as the product's library handle; returns the wrapper."""
    from np_modeling_amd import _C
    lib = XentLib(install_sim(profile))
    _C._LIB = lib
    return lib
