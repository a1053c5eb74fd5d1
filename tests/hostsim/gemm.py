"""TEST INFRASTRUCTURE ONLY -- the GEMM variants of a decode step: the skinny-M GEMM (npm_sgemm_skinny, its support and split
rules, npm_last_skinny_kernel) and the half-precision weight copies (npm_cvt_f32_f16, npm_cvt_f16_f32, npm_sgemm_skinny_w16).
Every product is npm_sgemm's float64 restatement on the same descriptor -- the w16 form converts B back exactly first -- so the
routes of ``device.gemm`` give array_equal results here; the support rules restate include/npm_hip.h.  A call is recorded under
its own name and never as 'npm_sgemm'.  ``skinny`` keeps (layout, m, n, k, epilogue) of every skinny call, ``w16`` the same and
the address of b of every w16 call, ``cvt`` (entry point, rows, cols, source address) of every conversion."""

import numpy as np

from .memory import BAD, UNSUPPORTED, _addr, _deref, _half_rows, _mat

MAX_M, MAX_SPLITS = 64, 64
EPI_BIAS, EPI_RESIDUAL, EPI_RELU_SAVE, EPI_RELU = 1, 2, 4, 16


def supported(g):
    """include/npm_hip.h: what npm_sgemm_skinny takes."""
    if g.trans_a or g.trans_b not in (0, 1) or g.batch0 != 1 or g.batch1 != 1 or not 1 <= g.m <= MAX_M:
        return False
    if g.n < 16 or g.n % 16 or g.k < 16 or g.k % 16:
        return False
    if not (_addr(g.a) and _addr(g.b) and _addr(g.c)) or _addr(g.a) % 16 or _addr(g.b) % 16 or _addr(g.c) % 16:
        return False
    if g.lda % 4 or g.ldb % 4 or g.ldc % 4 or g.lda < g.k or g.ldb < (g.k if g.trans_b else g.n) or g.ldc < g.n:
        return False
    e = g.epilogue
    if e & ~(EPI_BIAS | EPI_RESIDUAL | EPI_RELU_SAVE | EPI_RELU) or (e & EPI_RELU and e & EPI_RELU_SAVE):
        return False
    if e & EPI_BIAS and (not _addr(g.bias) or _addr(g.bias) % 16):
        return False
    if e & EPI_RESIDUAL and (not _addr(g.residual) or _addr(g.residual) % 16 or g.ldr % 4 or g.ldr < g.n):
        return False
    if e & EPI_RELU_SAVE and (not _addr(g.aux) or _addr(g.aux) % 16 or g.ldaux % 4 or g.ldaux < g.n):
        return False
    return not (_addr(g.colsum) or _addr(g.bsum) or _addr(g.asum) or _addr(g.rowdot) or g.split_k)


def auto_splits(n, k):
    """npm_sgemm_skinny_splits with NPM_TUNE_SKINNY_SPLITS = 0."""
    strips = (n + 63) // 64
    return max(1, min((512 + strips - 1) // strips, max(1, k // 128), 16))


def supported_w16(g):
    """include/npm_hip.h: what npm_sgemm_skinny_w16 takes -- npm_sgemm_skinny's rule with ldb a multiple of 8 halves."""
    return supported(g) and g.ldb % 8 == 0


class SkinnyGemm:
    def __init__(self):
        super().__init__()
        self.skinny, self.w16, self.cvt = [], [], []
        self.last_skinny = ''

    def npm_sgemm_skinny_supported(self, gref):
        return int(supported(_deref(gref)))

    def npm_sgemm_skinny_splits(self, n, k, trans_b):
        return auto_splits(n, k) if n >= 1 and k >= 1 else 1

    def npm_last_skinny_kernel(self):
        return self.last_skinny.encode()

    def _ran(self, g, tail=''):
        layout = 'NT' if g.trans_b else 'NN'
        self.last_skinny = 'sgemm_skinny_kernel %s M=%d N=%d K=%d rb=%d splits=%d nt=0%s' % (
            layout, g.m, g.n, g.k, (g.m + 15) // 16, auto_splits(g.n, g.k), tail)
        return layout, g.m, g.n, g.k, g.epilogue

    def npm_sgemm_skinny(self, gref):
        g = _deref(gref)
        self.calls.append('npm_sgemm_skinny')
        if not supported(g):
            return UNSUPPORTED
        rc = self._sgemm(g)
        self.skinny.append(self._ran(g))
        return rc

    def _cvt(self, entry, src, src_pitch, dst, dst_pitch, rows, cols):
        self.calls.append(entry)
        if rows < 0 or cols < 0 or src_pitch < cols or dst_pitch < cols:
            return BAD
        if rows == 0 or cols == 0:
            return 0
        if not (_addr(src) and _addr(dst)):
            return BAD
        self.cvt.append((entry, int(rows), int(cols), _addr(src)))
        from_view, to_view = (_mat, _half_rows) if entry == 'npm_cvt_f32_f16' else (_half_rows, _mat)
        to = to_view(dst, rows, cols, dst_pitch)
        with np.errstate(over='ignore'):                   # a float past the halves' range becomes inf
            to[:] = from_view(src, rows, cols, src_pitch).astype(to.dtype)
        return 0

    def npm_cvt_f32_f16(self, src, src_pitch, dst, dst_pitch, rows, cols):
        return self._cvt('npm_cvt_f32_f16', src, src_pitch, dst, dst_pitch, rows, cols)

    def npm_cvt_f16_f32(self, src, src_pitch, dst, dst_pitch, rows, cols):
        return self._cvt('npm_cvt_f16_f32', src, src_pitch, dst, dst_pitch, rows, cols)

    def npm_sgemm_skinny_w16_supported(self, gref):
        return int(supported_w16(_deref(gref)))

    def npm_sgemm_skinny_w16(self, gref):
        g = _deref(gref)
        self.calls.append('npm_sgemm_skinny_w16')
        if not supported_w16(g):
            return UNSUPPORTED
        rows, cols = (g.n, g.k) if g.trans_b else (g.k, g.n)
        rounded = np.ascontiguousarray(_half_rows(g.b, rows, cols, g.ldb).astype(np.float32))
        as_floats = type(g).from_buffer_copy(g)
        as_floats.b, as_floats.ldb = rounded.ctypes.data, cols
        rc = self._sgemm(as_floats)
        self.w16.append(self._ran(g, ' w=f16') + (_addr(g.b),))
        return rc
