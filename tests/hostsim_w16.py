"""TEST INFRASTRUCTURE ONLY -- tests/hostsim_skinny.py's simulator plus the four entry points of the half-precision weight copies
(npm_cvt_f32_f16, npm_cvt_f16_f32, npm_sgemm_skinny_w16, npm_sgemm_skinny_w16_supported), restated with NumPy: a conversion is
``astype(np.float16)`` / ``astype(np.float32)`` on pitched host memory; the product converts B back exactly and is npm_sgemm's
float64 restatement on that, so ``device.gemm`` gives array_equal results on its w16 route and on its cvt + npm_sgemm route.  A
w16 call is recorded as 'npm_sgemm_skinny_w16' and never as 'npm_sgemm' or 'npm_sgemm_skinny'; ``w16`` keeps (layout, m, n, k,
epilogue, address of b) of every call and ``cvt`` (entry point, rows, cols, source address) of every conversion."""

import ctypes as C

import numpy as np

import hostsim
import hostsim_skinny
from hostsim import _addr, _deref, _mat
from hostsim_kv16 import _half_rows


def supported(g):
    """include/npm_hip.h: what npm_sgemm_skinny_w16 takes -- npm_sgemm_skinny's rule with ldb a multiple of 8 halves."""
    return hostsim_skinny.supported(g) and g.ldb % 8 == 0


class W16HostSim(hostsim_skinny.SkinnyHostSim):
    def __init__(self):
        super().__init__()
        self.w16 = []
        self.cvt = []

    @staticmethod
    def _cvt_args_ok(src, src_pitch, dst, dst_pitch, rows, cols):
        return rows >= 0 and cols >= 0 and src_pitch >= cols and dst_pitch >= cols

    def npm_cvt_f32_f16(self, src, src_pitch, dst, dst_pitch, rows, cols):
        self.calls.append('npm_cvt_f32_f16')
        if not self._cvt_args_ok(src, src_pitch, dst, dst_pitch, rows, cols):
            return 10002
        if rows == 0 or cols == 0:
            return 0
        if not (_addr(src) and _addr(dst)):
            return 10002
        self.cvt.append(('npm_cvt_f32_f16', int(rows), int(cols), _addr(src)))
        with np.errstate(over='ignore'):
            _half_rows(dst, rows, cols, dst_pitch)[:] = _mat(src, rows, cols, src_pitch).astype(np.float16)
        return 0

    def npm_cvt_f16_f32(self, src, src_pitch, dst, dst_pitch, rows, cols):
        self.calls.append('npm_cvt_f16_f32')
        if not self._cvt_args_ok(src, src_pitch, dst, dst_pitch, rows, cols):
            return 10002
        if rows == 0 or cols == 0:
            return 0
        if not (_addr(src) and _addr(dst)):
            return 10002
        self.cvt.append(('npm_cvt_f16_f32', int(rows), int(cols), _addr(src)))
        _mat(dst, rows, cols, dst_pitch)[:] = _half_rows(src, rows, cols, src_pitch).astype(np.float32)
        return 0

    def npm_sgemm_skinny_w16_supported(self, gref):
        return int(supported(_deref(gref)))

    def npm_sgemm_skinny_w16(self, gref):
        g = _deref(gref)
        self.calls.append('npm_sgemm_skinny_w16')
        if not supported(g):
            return 10003
        rows, cols = (g.n, g.k) if g.trans_b else (g.k, g.n)
        rounded = np.ascontiguousarray(_half_rows(g.b, rows, cols, g.ldb).astype(np.float32))
        as_floats = type(g).from_buffer_copy(g)
        as_floats.b, as_floats.ldb = rounded.ctypes.data, cols
        rc = super().npm_sgemm(C.byref(as_floats))
        assert self.calls.pop() == 'npm_sgemm'
        layout = 'NT' if g.trans_b else 'NN'
        self.w16.append((layout, g.m, g.n, g.k, g.epilogue, _addr(g.b)))
        self.last_skinny = 'sgemm_skinny_kernel %s M=%d N=%d K=%d rb=%d splits=%d nt=0 w=f16' % (
            layout, g.m, g.n, g.k, (g.m + 15) // 16, hostsim_skinny.auto_splits(g.n, g.k))
        return rc


def install():
    from np_modeling_amd import _C
    sim = W16HostSim()
    _C._LIB = sim
    _C._DEVICE = 0
    return sim


uninstall = hostsim.uninstall
