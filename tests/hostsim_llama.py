"""TEST INFRASTRUCTURE ONLY -- the host simulator plus npm_rmsnorm_fwd / _bwd and npm_swiglu_fwd / _bwd, by composition.

The simulator's entry points are pinned to its recorded profiles (tests/test_hostsim_host.py) and ``HostSim`` has no subclasses, so
the four entry points of the rms / swiglu block are not part of it.  ``LlamaLib`` wraps an installed simulator exactly as
tests/hostsim_xent.py's ``XentLib`` does: every attribute it does not define is the simulator's, and the four entry points are
restated here with tests/llama_reference.py over the simulator's memory views.  ``install()`` puts it where the product looks for
its library."""

import llama_reference as LR
import numpy as np
from hostsim import install as install_sim
from hostsim.memory import BAD, _addr, _mat, _vec


class LlamaLib:
    def __init__(self, sim):
        self.sim = sim

    def __getattr__(self, name):                # only what this class does not define
        return getattr(self.sim, name)

    def npm_rmsnorm_fwd(self, x, gamma, eps, rows, d, z, rstd):
        self.sim.calls.append('npm_rmsnorm_fwd')
        rows, d = int(rows), int(d)
        if rows < 0 or d < 1:
            return BAD
        if rows == 0:
            return 0
        if not all(_addr(p) for p in (x, gamma, z, rstd)):
            return BAD
        out, rs = LR.rmsnorm_fwd(_mat(x, rows, d, d), _vec(gamma, d), eps)
        _mat(z, rows, d, d)[:] = out
        _vec(rstd, rows)[:] = rs[:, 0]
        return 0

    def npm_rmsnorm_bwd(self, dz, x, rstd, gamma, residual, rows, d, dx, dgamma):
        self.sim.calls.append('npm_rmsnorm_bwd')
        rows, d = int(rows), int(d)
        if rows < 0 or d < 1 or not _addr(dgamma):
            return BAD
        if rows == 0:
            _vec(dgamma, d)[:] = 0
            return 0
        if not all(_addr(p) for p in (dz, x, rstd, gamma, dx)):
            return BAD
        # from the saved rstd, as the kernel: xh = x rstd
        xv, rs = _mat(x, rows, d, d).astype(np.float64), _vec(rstd, rows).astype(np.float64)[:, None]
        dzv, gm = _mat(dz, rows, d, d).astype(np.float64), _vec(gamma, d).astype(np.float64)
        xh, g = xv * rs, dzv * gm
        out = rs * (g - xh * (g * xh).mean(axis=1, keepdims=True))
        if _addr(residual):
            out = out + _mat(residual, rows, d, d)
        _mat(dx, rows, d, d)[:] = out
        _vec(dgamma, d)[:] = (dzv * xh).sum(axis=0)
        return 0

    def npm_swiglu_fwd(self, pre, ld, rows, units, h, ldh):
        self.sim.calls.append('npm_swiglu_fwd')
        ld, rows, units, ldh = int(ld), int(rows), int(units), int(ldh)
        if rows < 0 or units < 1 or ld < 2 * units or ldh < units:
            return BAD
        if rows == 0:
            return 0
        if not (_addr(pre) and _addr(h)):
            return BAD
        with np.errstate(over='ignore', invalid='ignore'):
            _mat(h, rows, units, ldh)[:] = LR.swiglu_fwd(_mat(pre, rows, 2 * units, ld))
        return 0

    def npm_swiglu_bwd(self, pre, ld, dh, lddh, rows, units, dpre, lddpre):
        self.sim.calls.append('npm_swiglu_bwd')
        ld, lddh, rows, units, lddpre = int(ld), int(lddh), int(rows), int(units), int(lddpre)
        if rows < 0 or units < 1 or ld < 2 * units or lddh < units or lddpre < 2 * units:
            return BAD
        if rows == 0:
            return 0
        if not (_addr(pre) and _addr(dh) and _addr(dpre)):
            return BAD
        with np.errstate(over='ignore', invalid='ignore'):
            _mat(dpre, rows, 2 * units, lddpre)[:] = LR.swiglu_bwd(_mat(pre, rows, 2 * units, ld), _mat(dh, rows, units, lddh))
        return 0


def install(profile=None):
    """A fresh simulator wrapped in a ``LlamaLib``, installed as the product's library handle; returns the wrapper."""
    from np_modeling_amd import _C
    lib = LlamaLib(install_sim(profile))
    _C._LIB = lib
    return lib
