"""GPU: npm_swiglu_fwd / npm_swiglu_bwd (csrc/npm_swiglu.hip) against float64 (tests/llama_reference.py) under bounds DERIVED here
from the formula the header states, not tuned on what the kernels return.

u = 2^-24 is the unit roundoff of float32; every +, *, / below rounds once, relative error at most u (the build's float32 division
IS correctly rounded: hipcc compiles HIP with -fhip-fp32-correctly-rounded-divide-sqrt by default and csrc/Makefile does not switch
it off).  expf: the ROCm documentation's table of the device math library (HIP "Math API" reference, single precision floating-point
functions: "expf -- 1 ULP") gives at most 1 ulp, i.e. a relative error of at most 2 u.

  t      = expf(-|g|)                2 u
  1 + t                              the error of t enters with weight t / (1 + t) <= 1/2: u, plus the rounding: u      -> 2 u
  p      = 1 / (1 + t)               + u                                                                                 -> 3 u
  q      = t / (1 + t)               the error of t enters with weight 1 / (1 + t) <= 1: 2 u; the two roundings: u each     -> 4 u
  sigma  = g >= 0 ? p : q,  1 - sigma = the other one                                                                    <= 4 u each
  forward   h = (g sigma) u_p : two more products                                                                        -> 6 u |h|
  backward  dup = dh (g sigma) : two more products                                                                       -> 6 u |dup|
            w = g (1 - sigma)                      5 u |w|      (4 u if the compiler contracts it into the next line's fma)
            v = 1 + w                              5 u |w| + u |v| <= u + 6 u |w|            (|v| <= 1 + |w|; v has a root: see below)
            y = sigma v                            sigma (u + 6 u |w|) + (4 u + u) sigma |v| <= sigma (6 u + 11 u |w|)
            dgate = (dh u_p) y                     two more roundings, 2 u |dh u_p| sigma |v|  ->  |dh u_p| sigma (8 u + 13 u |w|)
                                                   = 8 u T1 + 13 u T2,  T1 = |dh u_p sigma|,  T2 = |dh u_p g sigma (1 - sigma)|
The bound of dgate is relative to the two TERMS, not to their sum: 1 + g (1 - sigma) has a root near g = -1.2784645, where dgate
itself is near zero while T1 and T2 are not.  Second-order terms: a factor 1.01 on every bound.

Below the smallest normal number (2^-126) a float32 result may lose bits or be flushed: sigma for g < -87.3 and 1 - sigma for
g > 87.3 (t = exp(-|g|) < 2^-126) then carry an ABSOLUTE error of at most 2^-126, which the later factors multiply, and a product
that is itself below 2^-126 carries one more:
  forward   2^-126 (1 + |u_p| (1 + |g|))
  dup       2^-126 (1 + |dh| (1 + |g|))
  dgate     2^-126 (1 + |dh u_p| (2 + |g|))
Each test prints the worst observed fraction of each bound (``report``), as the cross-entropy tests do."""

import numpy as np
import pytest

import llama_reference as LR
import rowops_reference as RR
import test_gpu_rowops_paths as P

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
TINY = 2.0 ** -126
SLACK = 1.01
env = P.env

GATES = [0.0, -0.0, 1e-30, -1e-30, 1.0, -1.0, -1.2784645, 20.0, -20.0, 87.0, -87.0, 88.8, -88.8, 100.0, -100.0, 1e30, -1e30]
UPS = [1.7, -1.7, 3e-3, -3e-3]


@pytest.fixture(autouse=True)
def _knobs_back():
    try:
        yield
    finally:
        for knob, value in P.KNOB_DEFAULTS.items():
            P._tune(knob, value)


class Pitched:
    """A [rows, cols] device matrix with a row pitch of ``ld`` inside a guarded, sentinel-filled buffer, ``lead`` floats off the
    16-byte grid."""

    def __init__(self, D, rows, cols, ld, lead=0, host=None):
        self.rows, self.cols, self.ld = rows, cols, ld
        self.g = P.Guarded(D, [rows * ld], lead=lead)
        self.ptr = self.g.ptr
        if host is not None:
            full = np.full((rows, ld), P.SENTINEL, dtype=np.float32)
            full[:, :cols] = host
            self.g.arr.set(full.reshape(-1))

    def numpy(self, what):
        host = self.g.numpy(what).reshape(self.rows, self.ld)
        assert (host[:, self.cols:] == P.SENTINEL).all(), 'the gap between the rows of ' + what + ' was written'
        return host[:, :self.cols].copy()


def swiglu(env, pre, dh, ld_extra=0, lead=0):
    """(h, dpre) as host arrays from host ``pre`` [rows, 2 U] and ``dh`` [rows, U]; every operand with ``ld_extra`` floats between
    its rows and ``lead`` floats off the 16-byte grid; guard bands and gaps checked."""
    _C, D = env
    rows, units = dh.shape
    pre_d = Pitched(D, rows, 2 * units, 2 * units + ld_extra, lead, pre)
    dh_d = Pitched(D, rows, units, units + ld_extra, lead, dh)
    h = Pitched(D, rows, units, units + ld_extra, lead)
    dpre = Pitched(D, rows, 2 * units, 2 * units + ld_extra, lead)
    _C.check(_C.lib().npm_swiglu_fwd(pre_d.ptr, pre_d.ld, rows, units, h.ptr, h.ld), 'npm_swiglu_fwd')
    _C.check(_C.lib().npm_swiglu_bwd(pre_d.ptr, pre_d.ld, dh_d.ptr, dh_d.ld, rows, units, dpre.ptr, dpre.ld), 'npm_swiglu_bwd')
    np.testing.assert_array_equal(pre_d.numpy('pre'), pre)                     # the inputs are read only
    return h.numpy('h'), dpre.numpy('dpre')


def fractions(pre, dh, h, dpre):
    """The worst fraction of each derived bound: dict h, dgate, dup."""
    units = dh.shape[1]
    g, up = pre[:, :units].astype(np.float64), pre[:, units:].astype(np.float64)
    d64 = dh.astype(np.float64)
    ref_h, ref_d = LR.swiglu_fwd(pre), LR.swiglu_bwd(pre, dh)
    t1, t2 = LR.swiglu_bwd_terms(pre, dh)
    ag = np.abs(g)
    bound_h = SLACK * 6 * U * np.abs(ref_h) + TINY * (1 + np.abs(up) * (1 + ag))
    bound_dg = SLACK * (8 * U * t1 + 13 * U * t2) + TINY * (1 + np.abs(d64 * up) * (2 + ag))
    bound_du = SLACK * 6 * U * np.abs(ref_d[:, units:]) + TINY * (1 + np.abs(d64) * (1 + ag))
    assert np.isfinite(h).all() and np.isfinite(dpre).all()
    return dict(h=float((np.abs(h - ref_h) / bound_h).max()), dgate=float((np.abs(dpre[:, :units] - ref_d[:, :units]) / bound_dg).max()),
                dup=float((np.abs(dpre[:, units:] - ref_d[:, units:]) / bound_du).max()))


def data(rows, units, seed=0):
    rng = np.random.default_rng(100 * seed + 7 * rows + units)
    return (3 * rng.standard_normal((rows, 2 * units))).astype(np.float32), rng.standard_normal((rows, units)).astype(np.float32)


SHAPES = [(1, 4), (3, 5), (7, 6), (9, 132), (64, 1024)]


@pytest.mark.parametrize('layout', ['dense', 'pitch+8', 'pitch+3', 'base+4B', 'base+4B pitch+8'])
@pytest.mark.parametrize('rows,units', SHAPES)
def test_parity_under_the_derived_bounds(env, rows, units, layout):
    """dense and pitch+8 take the 16-byte instances when units % 4 == 0; a pitch that is no multiple of 4, a base off the 16-byte
    grid and (3, 5) / (7, 6) take the scalar ones."""
    pre, dh = data(rows, units)
    extra = 8 if 'pitch+8' in layout else 3 if 'pitch+3' in layout else 0
    h, dpre = swiglu(env, pre, dh, ld_extra=extra, lead=1 if 'base' in layout else 0)
    fr = P.report('swiglu %d x %d %s' % (rows, units, layout), **fractions(pre, dh, h, dpre))
    assert max(fr.values()) <= 1.0, fr


@pytest.mark.parametrize('lead', [0, 1])
def test_gate_grid(env, lead):
    """Every gate value against ups of both signs and two magnitudes, gradients of both signs; vector and scalar instances."""
    gates = np.array(GATES + [0.5, -0.5, 3.0], dtype=np.float32)               # 20 columns: a multiple of 4
    rows, units = 2 * len(UPS), gates.size
    pre = np.empty((rows, 2 * units), dtype=np.float32)
    dh = np.empty((rows, units), dtype=np.float32)
    for r in range(rows):
        pre[r, :units] = gates
        pre[r, units:] = UPS[r % len(UPS)]
        dh[r] = (0.9 if r < len(UPS) else -1.3) * (1 + 0.01 * np.arange(units))
    h, dpre = swiglu(env, pre, dh, lead=lead)
    fr = P.report('swiglu gate grid lead=%d' % lead, **fractions(pre, dh, h, dpre))
    assert max(fr.values()) <= 1.0, fr
    root = GATES.index(-1.2784645)
    assert (np.abs(dpre[:, root]) <= 1e-6 * np.abs(dh[:, root] * pre[:, units + root])).all()       # the root of silu', as a sanity check
    far = [GATES.index(-100.0), GATES.index(-1e30)]
    assert (np.abs(h[:, far]) <= 1e-35).all() and (h[:, GATES.index(1e30)] != 0).all()


@pytest.mark.parametrize('lead', [0, 1])
@pytest.mark.parametrize('bad', [np.inf, -np.inf, np.nan])
def test_a_non_finite_element_stays_in_its_own_outputs(env, bad, lead):
    rows, units = 9, 132
    pre, dh = data(rows, units, seed=1)
    clean_h, clean_d = swiglu(env, pre, dh, lead=lead)
    for which, (r, c) in (('gate', (4, 17)), ('up', (8, 131)), ('dh', (0, 0))):
        p2, d2 = pre.copy(), dh.copy()
        if which == 'gate':
            p2[r, c] = bad
        elif which == 'up':
            p2[r, units + c] = bad
        else:
            d2[r, c] = bad
        h, dpre = swiglu(env, p2, d2, lead=lead)
        keep_h = np.ones((rows, units), dtype=bool)
        keep_h[r, c] = False
        keep_d = np.concatenate([keep_h, keep_h], axis=1)
        P.same_bits(h[keep_h], clean_h[keep_h], 'h beside a %r %s' % (bad, which))
        P.same_bits(dpre[keep_d], clean_d[keep_d], 'dpre beside a %r %s' % (bad, which))
        if which == 'dh':
            P.same_bits(h, clean_h, 'h does not read dh')


@pytest.mark.parametrize('cap', RR.EW_CAPS)
@pytest.mark.parametrize('rows,units,lead', [(53, 132, 0), (7, 301, 0), (37, 132, 1)])
def test_grid_stride_under_a_grid_cap(env, cap, rows, units, lead):
    """53 x 33 float4 items (7 x 301 and 37 x 132 elements on the scalar route) over at most 3 blocks of 256 threads: several trips
    per thread, whose (row, column) pairs wrap rows at every step."""
    per_row = units // 4 if units % 4 == 0 and not lead else units
    assert rows * per_row > 2 * cap * 256 and (cap * 256) % per_row != 0
    pre, dh = data(rows, units, seed=2)
    free_h, free_d = swiglu(env, pre, dh, lead=lead)
    with P.tuned(P.KNOB_EW_GRID_CAP, cap):
        h, dpre = swiglu(env, pre, dh, lead=lead)
    P.same_bits(h, free_h, 'h under a cap of %d' % cap)
    P.same_bits(dpre, free_d, 'dpre under a cap of %d' % cap)
    fr = P.report('swiglu %d x %d cap %d lead %d' % (rows, units, cap, lead), **fractions(pre, dh, h, dpre))
    assert max(fr.values()) <= 1.0, fr


def test_nontemporal_instances_equal_the_plain_ones_in_bits(env):
    """units = 2048 and the smallest row count at which pre has 2^25 bytes."""
    units = 2048
    rows = -(-RR.NT_BYTES // (8 * units))
    assert 8 * rows * units >= RR.NT_BYTES > 8 * (rows - 1) * units
    rng = np.random.default_rng(11)
    pre = (3 * rng.standard_normal((rows, 2 * units), dtype=np.float32))
    dh = rng.standard_normal((rows, units), dtype=np.float32)
    got = {}
    for nt in (0, 1):
        with P.tuned(P.KNOB_STREAM_NT, nt):
            got[nt] = swiglu(env, pre, dh)
    P.same_bits(got[1][0], got[0][0], 'h with the hint against without')
    P.same_bits(got[1][1], got[0][1], 'dpre with the hint against without')
    pick = P.sample_rows(rows)
    fr = P.report('swiglu NT %d x %d' % (rows, units), **fractions(pre[pick], dh[pick], got[1][0][pick], got[1][1][pick]))
    assert max(fr.values()) <= 1.0, fr


def test_empty_batch_and_argument_checks(env):
    _C, D = env
    lib = _C.lib()
    assert lib.npm_swiglu_fwd(None, 8, 0, 4, None, 4) == 0
    assert lib.npm_swiglu_bwd(None, 8, None, 4, 0, 4, None, 8) == 0
    buf = D.zeros([64])
    assert lib.npm_swiglu_fwd(buf.ptr, 7, 2, 4, buf.ptr, 4) != 0                # a pitch below 2 units
    assert lib.npm_swiglu_fwd(buf.ptr, 8, 2, 0, buf.ptr, 4) != 0                # no units
    assert lib.npm_swiglu_fwd(None, 8, 2, 4, buf.ptr, 4) != 0
    assert lib.npm_swiglu_bwd(buf.ptr, 8, buf.ptr, 3, 2, 4, buf.ptr, 8) != 0
