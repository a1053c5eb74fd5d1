"""TEST INFRASTRUCTURE ONLY -- tests/hostsim_paged.py's simulator plus the entry points of the skinny-M GEMM (npm_sgemm_skinny,
npm_sgemm_skinny_supported, npm_sgemm_skinny_splits, npm_last_skinny_kernel).  The product is npm_sgemm's float64 restatement on
the same descriptor, so the two routes of ``device.gemm`` give array_equal results here; the support rule restates
include/npm_hip.h.  A skinny call is recorded as 'npm_sgemm_skinny' and never as 'npm_sgemm'; ``skinny`` keeps (layout, m, n, k,
epilogue) of every call."""

import hostsim
import hostsim_paged
from hostsim import _addr, _deref

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


class SkinnyHostSim(hostsim_paged.PagedHostSim):
    def __init__(self):
        super().__init__()
        self.skinny = []
        self.last_skinny = ''

    def npm_sgemm_skinny_supported(self, gref):
        return int(supported(_deref(gref)))

    def npm_sgemm_skinny_splits(self, n, k, trans_b):
        return auto_splits(n, k) if n >= 1 and k >= 1 else 1

    def npm_last_skinny_kernel(self):
        return self.last_skinny.encode()

    def npm_sgemm_skinny(self, gref):
        g = _deref(gref)
        self.calls.append('npm_sgemm_skinny')
        if not supported(g):
            return 10003
        rc = super().npm_sgemm(gref)
        assert self.calls.pop() == 'npm_sgemm'
        layout = 'NT' if g.trans_b else 'NN'
        self.skinny.append((layout, g.m, g.n, g.k, g.epilogue))
        self.last_skinny = 'sgemm_skinny_kernel %s M=%d N=%d K=%d rb=%d splits=%d nt=0' % (
            layout, g.m, g.n, g.k, (g.m + 15) // 16, auto_splits(g.n, g.k))
        return rc


def install():
    from np_modeling_amd import _C
    sim = SkinnyHostSim()
    _C._LIB = sim
    _C._DEVICE = 0
    return sim


uninstall = hostsim.uninstall
