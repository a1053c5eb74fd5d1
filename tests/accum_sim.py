"""TEST INFRASTRUCTURE ONLY -- the host simulator (tests/hostsim/) with the two entry points of csrc/npm_accum.hip beside it.

``AccumSim`` is NOT a ``HostSim``: it holds a fresh one and hands every attribute it does not define on to it, so the simulator, its
profiles and its name lists stay what tests/test_hostsim_host.py pins them to.  ``install()`` sets ``np_modeling_amd._C._LIB``, as
``hostsim.install()`` does.  The restatements follow include/npm_hip.h: the fold with tests/accum_reference.py, the fused sum with
the simulator's own model of npm_sumsq_ranges (the exact sum, rounded once), so that "the bits of npm_sumsq_ranges afterwards"
can be asserted on the host as it is on the device."""

import ctypes as C

import numpy as np

import accum_reference as XR
import hostsim
from hostsim.memory import BAD, _addr, _deref, _vec, _words

MAX_RANGES = 32


class AccumSim:
    def __init__(self):
        object.__setattr__(self, '_sim', hostsim.HostSim())
        object.__setattr__(self, 'accum_tables', [])       # [(dst, src, n), ...] of every npm_accumulate_ranges, and whether it summed

    def __getattr__(self, name):                            # only what this class does not define
        return getattr(object.__getattribute__(self, '_sim'), name)

    def __setattr__(self, name, value):
        setattr(object.__getattribute__(self, '_sim'), name, value)

    def npm_accumulate_ranges(self, dst, src, sumsq_acc):
        self.calls.append('npm_accumulate_ranges')
        if dst is None or src is None:
            return BAD
        d, s = _deref(dst), _deref(src)
        if not 0 <= d.count <= MAX_RANGES or s.count != d.count:
            return BAD
        pairs = []
        for i in range(d.count):
            if int(d.n[i]) != int(s.n[i]):
                return BAD
            dp, sp, n = int(d.ptr[i] or 0), int(s.ptr[i] or 0), int(d.n[i])
            if (n > 0 and not (dp and sp)) or dp % 4 or sp % 4:
                return BAD
            pairs.append((dp, sp, n))

        def meet(a, an, b, bn):
            return an and bn and a < b + 4 * bn and b < a + 4 * an
        for i, (dp, _, n) in enumerate(pairs):
            for j, (dq, sq, m) in enumerate(pairs):
                if (i != j and meet(dp, n, dq, m)) or meet(dp, n, sq, m):
                    return BAD
        self.accum_tables.append((pairs, bool(_addr(sumsq_acc))))
        if not any(n for _, _, n in pairs):
            return 0
        for dp, sp, n in pairs:
            if n:
                _vec(dp, n)[:] = XR.fold([_vec(dp, n), _vec(sp, n)])
        if _addr(sumsq_acc):
            total = XR.exact_sumsq(*[_vec(dp, n) for dp, _, n in pairs if n])
            out = _words(sumsq_acc, 1, C.c_double)
            with np.errstate(all='ignore'):
                out[0] = out[0] + total
        return 0

    def npm_clip_finish_scaled(self, state, max_norm, grad_scale):
        self.calls.append('npm_clip_finish_scaled')
        if not _addr(state) or not max_norm > 0.0 or not 0.0 < grad_scale < float('inf'):
            return BAD
        s = _words(state, 4, C.c_double)
        s[1], s[2], s[3] = XR.clip_finish_scaled(s[0], max_norm, grad_scale)
        return 0


def install():
    """A fresh ``AccumSim`` as the product's library handle; returns it."""
    from np_modeling_amd import _C
    sim = AccumSim()
    _C._LIB = sim
    _C._DEVICE = 0
    return sim
