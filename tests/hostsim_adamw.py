"""TEST INFRASTRUCTURE ONLY -- the host simulator plus npm_sumsq_ranges, npm_clip_finish and npm_adamw_step, by composition.

The simulator's entry points are pinned to its recorded profiles (tests/test_hostsim_host.py) and ``HostSim`` has no subclasses, so
the three entry points of np_modeling_amd/csrc/npm_clip.hip are not part of it.  ``AdamWLib`` wraps tests/hostsim_lm.py's ``LmLib``
(a decoder-only language model is what the optimizer is for) exactly as that wraps the simulator: every attribute it does not define
is the inner library's, and the three entry points are restated here with tests/adamw_reference.py over the simulator's memory
views.  It also lists ``npm_fill_f64`` in ``calls`` (the simulator's runtime does not record it), so that a test can see the clip
state being zeroed in front of the sum.  ``install()`` puts it where the product looks for its library."""

import ctypes as C

import adamw_reference as AR
import numpy as np
from hostsim import install as install_sim
from hostsim.memory import BAD, _addr, _deref, _vec
from hostsim_lm import LmLib

MAX_RANGES = 32


def _doubles(ptr, n):
    return np.ctypeslib.as_array((C.c_double * int(n)).from_address(_addr(ptr)))


class AdamWLib:
    def __init__(self, inner):
        self.inner = inner
        self.sumsq_tables = []                  # [(address, n), ...] of every npm_sumsq_ranges call

    def __getattr__(self, name):                # only what this class does not define
        return getattr(self.inner, name)

    def npm_fill_f64(self, dst, value, n):
        self.inner.calls.append('npm_fill_f64')
        return self.inner.npm_fill_f64(dst, value, n)

    def npm_sumsq_ranges(self, ranges, acc):
        self.inner.calls.append('npm_sumsq_ranges')
        if ranges is None or not _addr(acc):
            return BAD
        table = _deref(ranges)
        if not 0 <= table.count <= MAX_RANGES:
            return BAD
        parts = [(int(table.ptr[i] or 0), int(table.n[i])) for i in range(table.count)]
        if any(n > 0 and (not ptr or ptr % 4) for ptr, n in parts):
            return BAD
        self.sumsq_tables.append(parts)
        if not any(n for _, n in parts):
            return 0
        total = AR.exact_sumsq(*[_vec(ptr, n) for ptr, n in parts if n])       # the exact sum, rounded once
        out = _doubles(acc, 1)
        with np.errstate(all='ignore'):
            out[0] = out[0] + total
        return 0

    def npm_clip_finish(self, state, max_norm):
        self.inner.calls.append('npm_clip_finish')
        if not _addr(state) or not max_norm > 0.0:
            return BAD
        s = _doubles(state, 4)
        s[1], s[2], s[3] = AR.clip_finish(s[0], max_norm)
        return 0

    def npm_adamw_step(self, var, grad, m, v, n, lr, beta1, beta2, eps, step, weight_decay, clip_state):
        self.inner.calls.append('npm_adamw_step')
        n = int(n)
        if step < 1 or not weight_decay >= 0.0:
            return BAD
        if n == 0:
            return 0
        if not (_addr(var) and _addr(grad) and _addr(m) and _addr(v)):
            return BAD
        clip = None
        if _addr(clip_state):
            s = _doubles(clip_state, 4)
            clip = (float(s[2]), float(s[3]))
            if clip[1] == 0:
                return 0                        # nothing at all is written
        mm, vv = _doubles(m, n), _doubles(v, n)
        out = AR.adamw_model(_vec(var, n), _vec(grad, n), mm, vv, int(step), (lr, beta1, beta2, eps), weight_decay, clip)
        mm[:], vv[:] = out.m, out.v
        _vec(var, n)[:] = out.p
        return 0


def install(profile=None):
    """A fresh simulator wrapped in an ``LmLib`` wrapped in an ``AdamWLib``, installed as the product's library handle."""
    from np_modeling_amd import _C
    lib = AdamWLib(LmLib(install_sim(profile)))
    _C._LIB = lib
    return lib
