"""MI355X: every path of csrc/npm_rowops.hip against float64 -- each register width (VPL 1 .. 16) with a partly filled last chunk
group, the generic kernels, the nontemporal (NT) instances, the grid-stride loops of the elementwise kernels, the LayerNorm
backward's walk over several rows per wave, wide-range data, pitched and whole-line column sums, attn_rowdot.

Cases, float32 models and bounds come from tests/rowops_reference.py; tests/test_rowops_host.py holds the models to half of every
bound used here.  The reference is always float64 NumPy on the same float32 inputs; tolerances are tests/test_gpu_rowops.py's
(z 3e-6, mean / rstd 2e-6, dx / dgamma / dbeta 5e-6, softmax 2e-6 / 5e-6, column sums 2e-6, attn_rowdot 3e-6 in
conftest.assert_close's metric) and 5e-7 between two instances of one formula (tests/test_gpu_encoder.py).  Range data uses the
conditioned bound of rowops_reference (KAPPA_DIV = 8).  Outputs sit between 64-float guard bands of a sentinel that must survive.
Every test prints the largest fraction of its bound it used (``-s``) before it asserts.

Tuning knobs (include/npm_hip.h): 6 NPM_TUNE_LN_BWD_BLOCKS, 7 NPM_TUNE_EW_GRID_CAP, 12 NPM_TUNE_STREAM_NT, 19 NPM_TUNE_LN_NT_SPLIT;
``_knobs_back`` restores 6 -> 4, 7 -> 0 (the library's 2^20), 12 -> 1, 19 -> 5 after every test.
"""

import ctypes as C
import functools
import re

import numpy as np
import pytest

import rowops_reference as RR

pytestmark = pytest.mark.gpu

GUARD = 64
SENTINEL = 777.0
KNOB_LN_BWD_BLOCKS, KNOB_EW_GRID_CAP, KNOB_STREAM_NT, KNOB_LN_NT_SPLIT = 6, 7, 12, 19
KNOB_DEFAULTS = {KNOB_LN_BWD_BLOCKS: 4, KNOB_EW_GRID_CAP: 0, KNOB_STREAM_NT: 1, KNOB_LN_NT_SPLIT: 5}
KEEP = 0.75


@pytest.fixture(scope='module')
def env():
    from np_modeling_amd import _C, device
    return _C, device


def _tune(knob, value):
    from np_modeling_amd import _C
    _C.check(_C.lib().npm_set_tuning(knob, int(value)), 'npm_set_tuning')


@pytest.fixture(autouse=True)
def _knobs_back():
    try:
        yield
    finally:
        for knob, value in KNOB_DEFAULTS.items():
            _tune(knob, value)


class tuned:
    """``with tuned(knob, value):`` -- the knob for the block, its default afterwards."""

    def __init__(self, *pairs):
        self.pairs = [(pairs[i], pairs[i + 1]) for i in range(0, len(pairs), 2)]

    def __enter__(self):
        for knob, value in self.pairs:
            _tune(knob, value)

    def __exit__(self, *exc):
        for knob, _ in self.pairs:
            _tune(knob, KNOB_DEFAULTS[knob])
        return False


@functools.lru_cache(maxsize=None)
def compute_units():
    """The device's CU count, which sizes the LayerNorm backward's grid and the whole-line column sum's: from npm_device_name's
    '... (gfx950..., N CUs)', the figure the library itself took from the device."""
    from np_modeling_amd import _C
    buf = C.create_string_buffer(256)
    _C.check(_C.lib().npm_device_name(buf, len(buf)), 'npm_device_name')
    found = re.search(r'(\d+) CUs\)$', buf.value.decode())
    assert found, buf.value
    return int(found.group(1))


class Guarded:
    """A device tensor carved out of a sentinel-filled buffer with GUARD floats before and after it."""

    def __init__(self, D, shape, lead=0):
        self.n = int(np.prod(shape))
        self.lead = GUARD + lead                            # lead = 1: a view 4 bytes off the 16-byte grid
        self.base = D.from_host(np.full(self.n + 2 * GUARD + lead, SENTINEL, dtype=np.float32))
        self.arr = self.base.flat_view(self.lead, shape)
        self.ptr = self.arr.ptr

    def numpy(self, what='output'):
        host = self.base.numpy()
        assert (host[:self.lead] == SENTINEL).all() and (host[self.lead + self.n:] == SENTINEL).all(), 'guard band of ' + what + ' written'
        return host[self.lead:self.lead + self.n].reshape(self.arr.shape)


def report(group, **fractions):
    print('%s: %s' % (group, ', '.join('%s %.3f' % (k, v) for k, v in fractions.items())))
    return fractions


def same_bits(a, b, what=''):
    a, b = np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
    assert a.shape == b.shape and (a.view(np.uint32) == b.view(np.uint32)).all(), 'bits differ: ' + what


# ---- thin callers with guarded outputs ------------------------------------------------------------------------------------------
def softmax_fwd(env, x_dev, rows, n, scale):
    _C, D = env
    y = Guarded(D, [rows, n])
    _C.check(_C.lib().npm_softmax_fwd(x_dev.ptr, y.ptr, rows, n, scale))
    return y


def softmax_bwd(env, y_dev, dy_dev, rows, n, scale):
    _C, D = env
    dx = Guarded(D, [rows, n])
    _C.check(_C.lib().npm_softmax_bwd(y_dev.ptr, dy_dev.ptr, dx.ptr, rows, n, scale))
    return dx


def ln_fwd(env, x, gamma, beta, rows, d, drop=None):
    """(z, mean, rstd) as Guarded."""
    _C, D = env
    z, mean, rstd = Guarded(D, [rows, d]), Guarded(D, [rows]), Guarded(D, [rows])
    if drop is None:
        _C.check(_C.lib().npm_layernorm_fwd(x.ptr, gamma.ptr, beta.ptr, RR.EPS, rows, d, z.ptr, mean.ptr, rstd.ptr))
    else:
        _C.check(_C.lib().npm_layernorm_dropout_fwd(x.ptr, drop.ptr, KEEP, gamma.ptr, beta.ptr, RR.EPS, rows, d, z.ptr, mean.ptr, rstd.ptr))
    return z, mean, rstd


def ln_bwd(env, dz, x, mean, rstd, gamma, res, rows, d, drop=None, bucket=False):
    """(dx, dgamma, dbeta) as host arrays, guard bands checked.  ``bucket``: dbeta == dgamma + d (one column-sum pass)."""
    _C, D = env
    dx = Guarded(D, [rows, d])
    if bucket:
        both = Guarded(D, [2 * d])
        pg, pb = both.ptr, both.ptr + 4 * d
    else:
        dg, db = Guarded(D, [d]), Guarded(D, [d])
        pg, pb = dg.ptr, db.ptr
    rp = None if res is None else res.ptr
    if drop is None:
        _C.check(_C.lib().npm_layernorm_bwd(dz.ptr, x.ptr, mean.ptr, rstd.ptr, gamma.ptr, rp, rows, d, dx.ptr, pg, pb))
    else:
        _C.check(_C.lib().npm_layernorm_dropout_bwd(dz.ptr, x.ptr, drop.ptr, KEEP, mean.ptr, rstd.ptr, gamma.ptr, rp, rows, d, dx.ptr, pg, pb))
    if bucket:
        host = both.numpy('dgamma | dbeta')
        return dx.numpy('dx'), host[:d], host[d:]
    return dx.numpy('dx'), dg.numpy('dgamma'), db.numpy('dbeta')


def dropped(x, mask):
    return np.where(mask != 0, x / np.float32(KEEP), np.float32(0)).astype(np.float32)


def ln_dropout_ref(x, mask, gamma, beta, dz, res):
    """float64 of the definition: LayerNorm of DropOut(x), the gradient through DropOut.backward, then the residual."""
    ref = RR.layernorm_ref(dropped(x, mask), gamma, beta, dz)
    ref['dx'] = np.where(mask != 0, ref['dx'] / np.float64(np.float32(KEEP)), 0.0)
    if res is not None:
        ref['dx'] = ref['dx'] + res
    return ref


# =================================================================================================================================
# a. the width grid, below the NT threshold
# =================================================================================================================================
@pytest.mark.parametrize('n', RR.ALL_WIDTHS)
def test_softmax_width_grid(env, n):
    """Forward and backward, scales 1 and 0.125, rows 1 / 5 / 7 / 9, at every width of the grid; every row of the 9-row call is,
    in bits, the same row run alone."""
    _C, D = env
    worst = dict(y=0.0, dx=0.0)
    for rows in RR.ROW_COUNTS:
        x, dy = RR.softmax_data(rows, n)
        xd, dyd = D.from_host(x), D.from_host(dy)
        for scale in (1.0, 0.125):
            yg = softmax_fwd(env, xd, rows, n, scale)
            y = yg.numpy('y')
            dx = softmax_bwd(env, yg.arr, dyd, rows, n, scale).numpy('dx')
            worst['y'] = max(worst['y'], RR.fraction(y, RR.softmax_ref(x, scale), RR.TOL_SOFTMAX))
            worst['dx'] = max(worst['dx'], RR.fraction(dx, RR.softmax_bwd_ref(y, dy, scale), RR.TOL_SOFTMAX_BWD))
            np.testing.assert_allclose(y.sum(axis=-1, dtype=np.float64), 1.0, rtol=1e-5)
            if rows == max(RR.ROW_COUNTS):
                for r in range(rows):
                    y1 = softmax_fwd(env, xd.flat_view(r * n, [1, n]), 1, n, scale)
                    same_bits(y1.numpy('y'), y[r:r + 1], 'softmax forward row %d' % r)
                    dx1 = softmax_bwd(env, y1.arr, dyd.flat_view(r * n, [1, n]), 1, n, scale)
                    same_bits(dx1.numpy('dx'), dx[r:r + 1], 'softmax backward row %d' % r)
    report('a softmax n=%d' % n, **worst)
    assert max(worst.values()) <= 1.0, worst


@pytest.mark.parametrize('d', RR.ALL_WIDTHS)
@pytest.mark.parametrize('with_residual', [False, True])
def test_layernorm_width_grid(env, d, with_residual):
    _C, D = env
    worst = {}
    for rows in RR.ROW_COUNTS:
        p = RR.grid_data(rows, d)
        dev = {k: D.from_host(v) for k, v in p.items()}
        res = dev['res'] if with_residual else None
        zg, mg, rg = ln_fwd(env, dev['x'], dev['gamma'], dev['beta'], rows, d)
        got = dict(z=zg.numpy('z'), mean=mg.numpy('mean'), rstd=rg.numpy('rstd'))
        got['dx'], got['dgamma'], got['dbeta'] = ln_bwd(env, dev['dz'], dev['x'], mg.arr, rg.arr, dev['gamma'], res, rows, d)
        ref = RR.layernorm_ref(p['x'], p['gamma'], p['beta'], p['dz'], p['res'] if with_residual else None)
        for name, tol in (('z', RR.TOL_Z), ('mean', RR.TOL_STAT), ('rstd', RR.TOL_STAT), ('dx', RR.TOL_DX), ('dgamma', RR.TOL_DX), ('dbeta', RR.TOL_DX)):
            worst[name] = max(worst.get(name, 0.0), RR.fraction(got[name], ref[name], tol))
        if rows == max(RR.ROW_COUNTS):
            for r in range(rows):
                x1 = dev['x'].flat_view(r * d, [1, d])
                z1, m1, r1 = ln_fwd(env, x1, dev['gamma'], dev['beta'], 1, d)
                same_bits(z1.numpy('z'), got['z'][r:r + 1], 'z row %d' % r)
                same_bits(m1.numpy('mean'), got['mean'][r:r + 1], 'mean row %d' % r)
                same_bits(r1.numpy('rstd'), got['rstd'][r:r + 1], 'rstd row %d' % r)
                res1 = None if res is None else res.flat_view(r * d, [1, d])
                dx1, _, _ = ln_bwd(env, dev['dz'].flat_view(r * d, [1, d]), x1, m1.arr, r1.arr, dev['gamma'], res1, 1, d)
                same_bits(dx1, got['dx'][r:r + 1], 'dx row %d' % r)
    report('a layernorm d=%d residual=%d' % (d, with_residual), **worst)
    assert max(worst.values()) <= 1.0, worst


@pytest.mark.parametrize('d', RR.ONE_PER_CLASS)
@pytest.mark.parametrize('rows,with_residual', [(9, True), (37, False)])
def test_layernorm_dropout_width_grid(env, d, rows, with_residual):
    """npm_layernorm_dropout_fwd / _bwd at one width per VPL: against the composed calls (5e-7) and the definition."""
    _C, D = env
    lib = _C.lib()
    p = RR.grid_data(rows, d, seed=3)
    mask = (np.random.default_rng(rows + d).random((rows, d)) < KEEP).astype(np.uint8)
    dev = {k: D.from_host(v) for k, v in p.items()}
    res = dev['res'] if with_residual else None
    md = D.bytes_from_host(mask)
    # composed: npm_mask_scale -> LayerNorm -> npm_mask_scale (-> add)
    xd = D.empty([rows, d])
    _C.check(lib.npm_mask_scale(dev['x'].ptr, md.ptr, xd.ptr, rows * d, KEEP))
    z0, m0, r0 = ln_fwd(env, xd, dev['gamma'], dev['beta'], rows, d)
    inner, dg0, db0 = ln_bwd(env, dev['dz'], xd, m0.arr, r0.arr, dev['gamma'], None, rows, d)
    dx0 = D.empty([rows, d])
    inner_dev = D.from_host(inner)                 # named: a raw pointer keeps nothing alive
    _C.check(lib.npm_mask_scale(inner_dev.ptr, md.ptr, dx0.ptr, rows * d, KEEP))
    dx0 = (D.add(dx0, res) if with_residual else dx0).numpy()
    # fused
    z1, m1, r1 = ln_fwd(env, dev['x'], dev['gamma'], dev['beta'], rows, d, drop=md)
    dx1, dg1, db1 = ln_bwd(env, dev['dz'], dev['x'], m1.arr, r1.arr, dev['gamma'], res, rows, d, drop=md)
    got = dict(z=z1.numpy('z'), mean=m1.numpy('mean'), rstd=r1.numpy('rstd'), dx=dx1, dgamma=dg1, dbeta=db1)
    composed = dict(z=z0.numpy('z'), mean=m0.numpy('mean'), rstd=r0.numpy('rstd'), dx=dx0, dgamma=dg0, dbeta=db0)
    ref = ln_dropout_ref(p['x'], mask, p['gamma'], p['beta'], p['dz'], p['res'] if with_residual else None)
    same = {k: RR.fraction(got[k], composed[k], RR.TOL_SAME) for k in got}
    fr = dict(z=RR.fraction(got['z'], ref['z'], RR.TOL_Z), dx=RR.fraction(got['dx'], ref['dx'], RR.TOL_DX),
              dgamma=RR.fraction(got['dgamma'], ref['dgamma'], RR.TOL_DX), dbeta=RR.fraction(got['dbeta'], ref['dbeta'], RR.TOL_DX))
    report('a dropout d=%d rows=%d' % (d, rows), **fr, **{'same_' + k: v for k, v in same.items()})
    np.testing.assert_array_equal(dx1[mask == 0], p['res'][mask == 0] if with_residual else 0)      # dropped positions: exactly the residual
    assert max(same.values()) <= 1.0 and max(fr.values()) <= 1.0, (same, fr)


# =================================================================================================================================
# b. the grid-stride loops of the elementwise kernels (NPM_TUNE_EW_GRID_CAP)
# =================================================================================================================================
def elementwise_results(env, n, a, b, c):
    """The seven elementwise operations on guarded outputs -> {name: host array}."""
    _C, D = env
    lib = _C.lib()
    da, db, dc = D.from_host(a), D.from_host(b), D.from_host(c)
    out = {}

    def run(name, call):
        g = Guarded(D, [n])
        _C.check(call(g.ptr), name)
        out[name] = g.numpy(name)

    run('relu_fwd', lambda o: lib.npm_relu_fwd(da.ptr, o, n))
    run('relu_bwd', lambda o: lib.npm_relu_bwd(da.ptr, db.ptr, o, n))
    run('add', lambda o: lib.npm_add(da.ptr, db.ptr, o, n))
    run('add3', lambda o: lib.npm_add3(da.ptr, db.ptr, dc.ptr, o, n))
    run('scale', lambda o: lib.npm_scale(da.ptr, o, 3.0, n))
    run('fill', lambda o: lib.npm_fill_f32(o, 2.5, n))
    y = Guarded(D, [n])
    y.arr.set(a)
    _C.check(lib.npm_axpy(y.ptr, db.ptr, -0.25, n), 'axpy')
    out['axpy'] = y.numpy('axpy')
    return out


def check_elementwise(out, a, b, c):
    """tests/test_gpu_rowops.py::test_elementwise's assertions."""
    np.testing.assert_array_equal(out['relu_fwd'], np.maximum(a, 0))
    np.testing.assert_array_equal(out['relu_bwd'], np.where(a >= 0, b, 0).astype(np.float32))
    np.testing.assert_array_equal(out['add'], a + b)
    np.testing.assert_array_equal(out['add3'], (a + b) + c)
    np.testing.assert_array_equal(out['scale'], a * np.float32(3.0))
    np.testing.assert_array_equal(out['fill'], np.full(a.shape, 2.5, dtype=np.float32))
    np.testing.assert_allclose(out['axpy'], a - np.float32(0.25) * b, rtol=1e-6, atol=1e-7)


def elementwise_inputs(n):
    rng = np.random.default_rng(n)
    a, b, c = (rng.standard_normal(n, dtype=np.float32) for _ in range(3))
    a[:2] = 0.0
    a[2] = -0.0
    return a, b, c


@pytest.mark.parametrize('cap', RR.EW_CAPS)
def test_elementwise_grid_stride_paths(env, cap):
    """A grid of 1 / 2 / 3 blocks: the unrolled body, a remainder of two trips for some threads and the scalar tail all run
    (tests/test_rowops_host.py recomputes the loops); same bits as under the default cap."""
    n = RR.ew_size(cap)
    a, b, c = elementwise_inputs(n)
    with tuned(KNOB_EW_GRID_CAP, cap):
        capped = elementwise_results(env, n, a, b, c)
    default = elementwise_results(env, n, a, b, c)
    check_elementwise(capped, a, b, c)
    check_elementwise(default, a, b, c)
    for name in capped:
        if name != 'axpy':
            same_bits(capped[name], default[name], name)


def test_elementwise_scalar_kernels_stride(env):
    """Views 4 bytes off the 16-byte grid take ew1 / ew2 / ew3_scalar; one block of 256 threads walks 997 elements."""
    _C, D = env
    lib = _C.lib()
    n = 997
    a, b, c = elementwise_inputs(n)
    va, vb, vc = (D.from_host(np.concatenate([[np.float32(9)], v])).flat_view(1, [n]) for v in (a, b, c))
    with tuned(KNOB_EW_GRID_CAP, 1):
        for lead in (1, 0):                      # unaligned inputs with an unaligned, then an aligned output
            g = Guarded(D, [n], lead=lead)
            _C.check(lib.npm_scale(va.ptr, g.ptr, 3.0, n))
            np.testing.assert_array_equal(g.numpy('scale'), a * np.float32(3.0))
            g = Guarded(D, [n], lead=lead)
            _C.check(lib.npm_relu_bwd(va.ptr, vb.ptr, g.ptr, n))
            np.testing.assert_array_equal(g.numpy('relu_bwd'), np.where(a >= 0, b, 0).astype(np.float32))
            g = Guarded(D, [n], lead=lead)
            _C.check(lib.npm_add3(va.ptr, vb.ptr, vc.ptr, g.ptr, n))
            np.testing.assert_array_equal(g.numpy('add3'), (a + b) + c)


# =================================================================================================================================
# c. the LayerNorm backward's walk over rows (NPM_TUNE_LN_BWD_BLOCKS = 1)
# =================================================================================================================================
@pytest.mark.parametrize('d,with_residual,drop,bucket', [(72, False, False, False), (260, True, False, True), (900, False, False, True),
                                                         (900, True, True, False), (2048, True, False, False), (3076, False, False, False),
                                                         (3076, True, True, True)])
def test_layernorm_bwd_row_walk(env, d, with_residual, drop, bucket):
    """One block per CU and 10 x CUs + 3 rows: some waves own three rows, the others two (tests/test_rowops_host.py).  dx, dgamma,
    dbeta against float64; dgamma / dbeta against the default grid's at 5e-7 (another grouping of the same sum); twice the same
    call, the same bits."""
    _C, D = env
    cus = compute_units()
    rows = RR.ln_walk_rows(cus)
    assert set(RR.ln_walk_counts(rows, RR.ln_bwd_grid(rows, 1, cus))) == {2, 3}
    rng = np.random.default_rng(d)
    x = (rng.standard_normal((rows, d), dtype=np.float32) * 2 + np.float32(0.5))
    dz, res = rng.standard_normal((rows, d), dtype=np.float32), rng.standard_normal((rows, d), dtype=np.float32)
    gamma, beta = rng.standard_normal(d, dtype=np.float32), rng.standard_normal(d, dtype=np.float32)
    mask = (rng.random((rows, d)) < KEEP).astype(np.uint8) if drop else None
    xd, dzd, gd, bd = D.from_host(x), D.from_host(dz), D.from_host(gamma), D.from_host(beta)
    rd = D.from_host(res) if with_residual else None
    md = D.bytes_from_host(mask) if drop else None
    nt_off = 4 * rows * d >= RR.NT_BYTES                           # keep the plain instances (the NT ones: group d)
    with tuned(KNOB_STREAM_NT, 0 if nt_off else 1):
        _, mg, rg = ln_fwd(env, xd, gd, bd, rows, d, drop=md)
        with tuned(KNOB_LN_BWD_BLOCKS, 1):
            dx, dg, db = ln_bwd(env, dzd, xd, mg.arr, rg.arr, gd, rd, rows, d, drop=md, bucket=bucket)
            again = ln_bwd(env, dzd, xd, mg.arr, rg.arr, gd, rd, rows, d, drop=md, bucket=bucket)
        dx4, dg4, db4 = ln_bwd(env, dzd, xd, mg.arr, rg.arr, gd, rd, rows, d, drop=md, bucket=bucket)
    for name, a, b in (('dx', dx, again[0]), ('dgamma', dg, again[1]), ('dbeta', db, again[2])):
        same_bits(a, b, name + ' of two identical calls')
    ref = ln_dropout_ref(x, mask, gamma, beta, dz, res if with_residual else None) if drop else \
        RR.layernorm_ref(x, gamma, beta, dz, res if with_residual else None)
    fr = report('c walk d=%d rows=%d' % (d, rows), dx=RR.fraction(dx, ref['dx'], RR.TOL_DX), dgamma=RR.fraction(dg, ref['dgamma'], RR.TOL_DX),
                dbeta=RR.fraction(db, ref['dbeta'], RR.TOL_DX), same_dgamma=RR.fraction(dg, dg4, RR.TOL_SAME),
                same_dbeta=RR.fraction(db, db4, RR.TOL_SAME), same_dx=RR.fraction(dx, dx4, RR.TOL_SAME))
    assert max(fr.values()) <= 1.0, fr


# =================================================================================================================================
# d. the NT instances (tensors of at least 32 MB)
# =================================================================================================================================
@pytest.fixture(scope='module')
def big():
    """2^23 + 3 * 4096 normals, twice, and as many mask bytes: every >= 32 MB shape is a reshaped prefix."""
    rng = np.random.default_rng(2025)
    n = RR.NT_ELEMS + 3 * 4096
    return dict(x=rng.standard_normal(n, dtype=np.float32), dz=rng.standard_normal(n, dtype=np.float32),
                mask=(rng.random(n, dtype=np.float32) < KEEP).astype(np.uint8))


def sample_rows(rows):
    """The first 8 rows, the last 8 and 64 seeded ones in between."""
    mid = np.random.default_rng(rows).choice(np.arange(8, rows - 8), size=64, replace=False)
    return np.concatenate([np.arange(8), np.sort(mid), np.arange(rows - 8, rows)])


def colsums64(x, dz):
    """float64 dgamma, dbeta over all rows, a slab of rows at a time."""
    d = x.shape[1]
    dg, db = np.zeros(d), np.zeros(d)
    for at in range(0, x.shape[0], 4096):
        x64, z64 = x[at:at + 4096].astype(np.float64), dz[at:at + 4096].astype(np.float64)
        yh = (x64 - x64.mean(axis=1, keepdims=True)) / np.sqrt(x64.var(axis=1, keepdims=True) + RR.EPS)
        dg += (z64 * yh).sum(axis=0)
        db += z64.sum(axis=0)
    return dg, db


def layernorm_nt_case(env, big, d, drop, split=None):
    """LayerNorm forward and backward at [2^23 / d + 3, d] with the NT instances, against the same calls without the hint (5e-7),
    those against float64 (sampled rows; dgamma / dbeta in full)."""
    _C, D = env
    rows = RR.nt_rows(d)
    assert 4 * rows * d >= RR.NT_BYTES
    x, dz = big['x'][:rows * d].reshape(rows, d), big['dz'][:rows * d].reshape(rows, d)
    res = np.ascontiguousarray(big['x'][::-1][:rows * d]).reshape(rows, d)
    mask = big['mask'][:rows * d].reshape(rows, d) if drop else None
    rng = np.random.default_rng(d)
    gamma, beta = rng.standard_normal(d, dtype=np.float32), rng.standard_normal(d, dtype=np.float32)
    xd, dzd, gd, bd = D.from_host(x), D.from_host(dz), D.from_host(gamma), D.from_host(beta)
    rd = D.from_host(res)
    md = D.bytes_from_host(mask) if drop else None
    got = {}
    for nt in (0, 1):
        with tuned(KNOB_STREAM_NT, nt, KNOB_LN_NT_SPLIT, KNOB_DEFAULTS[KNOB_LN_NT_SPLIT] if split is None else split):
            zg, mg, rg = ln_fwd(env, xd, gd, bd, rows, d, drop=md)
            cur = dict(z=zg.numpy('z'), mean=mg.numpy('mean'), rstd=rg.numpy('rstd'))
            cur['dx'], cur['dgamma'], cur['dbeta'] = ln_bwd(env, dzd, xd, mg.arr, rg.arr, gd, rd, rows, d, drop=md)
        got[nt] = cur
    same = {'same_' + k: RR.fraction(got[1][k], got[0][k], RR.TOL_SAME) for k in got[0]}
    bits = [k for k in got[0] if (got[1][k].view(np.uint32) == got[0][k].view(np.uint32)).all()]
    pick = sample_rows(rows)
    xs = dropped(x[pick], mask[pick]) if drop else x[pick]
    ref = RR.layernorm_ref(xs, gamma, beta, dz[pick])
    if drop:
        ref['dx'] = np.where(mask[pick] != 0, ref['dx'] / np.float64(np.float32(KEEP)), 0.0)
    ref['dx'] = ref['dx'] + res[pick]
    off = got[0]
    # the sampled rows' z and dx are judged on the scale of the whole tensor, which the sample's own maximum stands for
    fr = dict(z=RR.fraction(off['z'][pick], ref['z'], RR.TOL_Z), mean=RR.fraction(off['mean'][pick], ref['mean'], RR.TOL_STAT),
              rstd=RR.fraction(off['rstd'][pick], ref['rstd'], RR.TOL_STAT), dx=RR.fraction(off['dx'][pick], ref['dx'], RR.TOL_DX))
    xall = dropped(x, mask) if drop else x
    dg, db = colsums64(xall, dz)
    fr.update(dgamma=RR.fraction(off['dgamma'], dg, RR.TOL_DX), dbeta=RR.fraction(off['dbeta'], db, RR.TOL_DX))
    report('d layernorm d=%d drop=%d split=%s (NT on == off in bits: %s)' % (d, drop, split, ' '.join(bits) or 'none'), **fr, **same)
    assert max(fr.values()) <= 1.0 and max(same.values()) <= 1.0, (fr, same)


@pytest.mark.parametrize('d', RR.NT_WIDTHS)
def test_layernorm_nt(env, big, d):
    layernorm_nt_case(env, big, d, drop=False)


@pytest.mark.parametrize('d', [640, 1024])
@pytest.mark.parametrize('split', [0, 5, 10])
def test_layernorm_nt_split(env, big, d, split):
    """NPM_TUNE_LN_NT_SPLIT at d in (512, 1024]: 0 the hint on loads and stores (<4, true, true>), 5 on the loads (<4, true, false>),
    10 on the stores (<4, false, true>), forward and backward alike."""
    layernorm_nt_case(env, big, d, drop=False, split=split)


@pytest.mark.parametrize('d,split', [(d, None) for d in RR.NT_WIDTHS] + [(1024, 0)])
def test_layernorm_dropout_nt(env, big, d, split):
    """The fused-dropout forms: d = 1024 is the hard-wired <4, true, false, true> instance (and <4, true, true, true> with the
    split knob at 0), the other widths <VPL, true, true, true>."""
    layernorm_nt_case(env, big, d, drop=True, split=split)


@pytest.mark.parametrize('n', RR.NT_WIDTHS)
def test_softmax_nt(env, big, n):
    _C, D = env
    rows = RR.nt_rows(n)
    x = (big['x'][:rows * n] * np.float32(4)).reshape(rows, n)
    dy = big['dz'][:rows * n].reshape(rows, n)
    xd, dyd = D.from_host(x), D.from_host(dy)
    got = {}
    for nt in (0, 1):
        with tuned(KNOB_STREAM_NT, nt):
            yg = softmax_fwd(env, xd, rows, n, 0.5)
            got[nt] = dict(y=yg.numpy('y'), dx=softmax_bwd(env, yg.arr, dyd, rows, n, 0.5).numpy('dx'))
    pick = sample_rows(rows)
    y = got[0]['y']
    fr = report('d softmax n=%d' % n, y=RR.fraction(y[pick], RR.softmax_ref(x[pick], 0.5), RR.TOL_SOFTMAX),
                dx=RR.fraction(got[0]['dx'][pick], RR.softmax_bwd_ref(y[pick], dy[pick], 0.5), RR.TOL_SOFTMAX_BWD),
                same_y=RR.fraction(got[1]['y'], y, RR.TOL_SAME), same_dx=RR.fraction(got[1]['dx'], got[0]['dx'], RR.TOL_SAME))
    assert max(fr.values()) <= 1.0, fr


def test_elementwise_nt(env, big):
    """2^23 + 5 floats: the NT instances of ew1 / ew2 / ew3 against the plain ones in bits (axpy: its allclose), those against NumPy."""
    n = RR.NT_ELEMS + 5
    a, b, c = big['x'][:n], big['dz'][:n], big['x'][7:n + 7]
    on = elementwise_results(env, n, a, b, c)
    with tuned(KNOB_STREAM_NT, 0):
        off = elementwise_results(env, n, a, b, c)
    check_elementwise(off, a, b, c)
    check_elementwise(on, a, b, c)
    for name in on:
        if name != 'axpy':
            same_bits(on[name], off[name], name)


def rowdot_ref(a, b):
    return np.einsum('bshd,bshd->bhs', a.astype(np.float64), b.astype(np.float64))


def test_attn_rowdot_nt(env, big):
    _C, D = env
    shape = (4, 2049, 8, 128)
    n = int(np.prod(shape))
    assert 4 * n >= RR.NT_BYTES
    a, b = big['x'][:n].reshape(shape), big['dz'][:n].reshape(shape)
    ad, bd = D.from_host(a), D.from_host(b)
    got = {}
    for nt in (0, 1):
        with tuned(KNOB_STREAM_NT, nt):
            out = Guarded(D, [shape[0], shape[2], shape[1]])
            _C.check(_C.lib().npm_attn_rowdot(ad.ptr, bd.ptr, out.ptr, *shape))
            got[nt] = out.numpy('rowdot')
    fr = report('d attn_rowdot', rowdot=RR.fraction(got[0], rowdot_ref(a, b), RR.TOL_ROWDOT), same=RR.fraction(got[1], got[0], RR.TOL_SAME))
    assert max(fr.values()) <= 1.0, fr


@pytest.mark.parametrize('dim,lead', [(4, 0), (5, 0), (64, 0), (128, 0), (132, 0), (256, 0), (320, 0), (128, 1), (320, 1), (5, 1)])
def test_attn_rowdot_head_sizes(env, dim, lead):
    """Head sizes up to the ``c += 128`` loop's third trip, a size that is no multiple of 4, and one operand 4 bytes off the
    16-byte grid (the scalar branch); 21 rows of 32 lanes leave the last block partly idle."""
    _C, D = env
    shape = (1, 7, 3, dim)
    rng = np.random.default_rng(dim)
    a, b = rng.standard_normal(shape, dtype=np.float32), rng.standard_normal(shape, dtype=np.float32)
    ad = D.from_host(a)
    bg = Guarded(D, shape, lead=lead)
    bg.arr.set(b)
    out = Guarded(D, [1, 3, 7])
    _C.check(_C.lib().npm_attn_rowdot(ad.ptr, bg.ptr, out.ptr, *shape))
    fr = report('d attn_rowdot D=%d lead=%d' % (dim, lead), rowdot=RR.fraction(out.numpy('rowdot'), rowdot_ref(a, b), RR.TOL_ROWDOT))
    assert fr['rowdot'] <= 1.0, fr


# =================================================================================================================================
# e. range
# =================================================================================================================================
@pytest.mark.parametrize('d', RR.ONE_PER_CLASS + (1001,))
def test_layernorm_range(env, d):
    """Shifted rows up to kappa = 1.7e4, constant rows, a 1e6 outlier, rows of 1e-20: the conditioned bound of rowops_reference."""
    _C, D = env
    worst = {}
    for kind in RR.LN_RANGE_KINDS:
        x = RR.ln_range(kind, d)
        rows = x.shape[0]
        p = RR.grid_data(rows, d, seed=1)
        xd, gd, bd, dzd = D.from_host(x), D.from_host(p['gamma']), D.from_host(p['beta']), D.from_host(p['dz'])
        zg, mg, rg = ln_fwd(env, xd, gd, bd, rows, d)
        got = dict(z=zg.numpy('z'), mean=mg.numpy('mean'), rstd=rg.numpy('rstd'))
        got['dx'], got['dgamma'], got['dbeta'] = ln_bwd(env, dzd, xd, mg.arr, rg.arr, gd, None, rows, d)
        fr = RR.ln_range_fractions(kind, x, p['gamma'], p['beta'], p['dz'], got)
        fr['dbeta'] = RR.fraction(got['dbeta'], p['dz'].astype(np.float64).sum(axis=0), RR.TOL_DX)
        assert all(np.isfinite(v).all() for v in got.values()), kind
        if kind == 'constant':
            fr['z_beta'] = RR.cond_fraction(got['z'], np.broadcast_to(p['beta'].astype(np.float64), x.shape), RR.TOL_Z, RR.kappa(x))
            np.testing.assert_allclose(got['rstd'], 1 / np.sqrt(RR.EPS), rtol=2e-6)
        report('e layernorm d=%d %s' % (d, kind), **fr)
        worst[kind] = max(fr.values())
    assert max(worst.values()) <= 1.0, worst


@pytest.mark.parametrize('n', RR.ONE_PER_CLASS + (1001,))
def test_softmax_range(env, n):
    """Logits shifted by +-1e4, spanning 200 units, -inf at scattered positions, over a whole leading chunk group, over the tail,
    and a row that is -inf throughout (NaN across that row, as the oracle; nothing outside it)."""
    _C, D = env
    x, dead = RR.softmax_range(n)
    rows = x.shape[0]
    live = np.arange(rows) != dead
    dy = RR.softmax_data(rows, n, seed=2)[1]
    xd, dyd = D.from_host(x), D.from_host(dy)
    yg = softmax_fwd(env, xd, rows, n, 1.0)
    y = yg.numpy('y')
    dx = softmax_bwd(env, yg.arr, dyd, rows, n, 1.0).numpy('dx')
    ref = RR.softmax_ref(x)
    assert np.isnan(ref[dead]).all() and np.isnan(y[dead]).all()
    assert np.isfinite(y[live]).all() and np.isfinite(dx[live]).all()
    assert (y[live][np.isinf(x[live])] == 0).all()                                  # exact zeros where the logit is -inf
    np.testing.assert_allclose(y[live].sum(axis=1, dtype=np.float64), 1.0, rtol=1e-5)
    fr = report('e softmax n=%d' % n, y=RR.fraction(y[live], ref[live], RR.TOL_SOFTMAX),
                dx=RR.fraction(dx[live], RR.softmax_bwd_ref(y, dy)[live], RR.TOL_SOFTMAX_BWD))
    assert max(fr.values()) <= 1.0, fr


# =================================================================================================================================
# f. column sums with a pitch, at the unroll's edges, and every exit of the whole-line kernel
# =================================================================================================================================
@pytest.mark.parametrize('rows,cols,ld', [(37, 12, 20), (1000, 64, 128), (300, 200, 400), (5000, 130, 131)])
def test_colsum_pitched(env, rows, cols, ld):
    """ld > cols, as the LayerNorm backward calls it (ld = 2 d); the padding columns hold 1e30, which must never be added in."""
    _C, D = env
    rng = np.random.default_rng(rows + cols)
    buf = np.full((rows, ld), 1e30, dtype=np.float32)
    x = rng.standard_normal((rows, cols), dtype=np.float32)
    buf[:, :cols] = x
    out, bd = Guarded(D, [cols]), D.from_host(buf)
    _C.check(_C.lib().npm_colsum(bd.ptr, out.ptr, rows, cols, ld))
    fr = report('f colsum %dx%d ld %d' % (rows, cols, ld), colsum=RR.fraction(out.numpy('colsum'), x.astype(np.float64).sum(axis=0), RR.TOL_COLSUM))
    assert fr['colsum'] <= 1.0, fr


@pytest.mark.parametrize('rows', RR.COLSUM_EDGE_ROWS)
def test_colsum_unroll_edges(env, rows):
    """Rows per chunk one below, at or one above a multiple of 64, the four-row unroll's trip: one chunk up to 256 rows, then two
    chunks of 255 and of 256 rows and three of 193 (tests/test_rowops_host.py recomputes the split); 100 columns leave the second
    strip partly filled."""
    _C, D = env
    cols = 100
    rng = np.random.default_rng(rows)
    pre, dy = rng.standard_normal((rows, cols), dtype=np.float32), rng.standard_normal((rows, cols), dtype=np.float32)
    pre[0, :3] = 0.0
    out, pd, dd = Guarded(D, [cols]), D.from_host(pre), D.from_host(dy)
    _C.check(_C.lib().npm_colsum(pd.ptr, out.ptr, rows, cols, cols))
    g, gsum = Guarded(D, [rows, cols]), Guarded(D, [cols])
    _C.check(_C.lib().npm_relu_bwd_colsum(pd.ptr, dd.ptr, g.ptr, gsum.ptr, rows, cols))
    want = np.where(pre >= 0, dy, 0).astype(np.float32)
    np.testing.assert_array_equal(g.numpy('relu_bwd'), want)
    fr = report('f colsum edges rows=%d' % rows, colsum=RR.fraction(out.numpy('colsum'), pre.astype(np.float64).sum(axis=0), RR.TOL_COLSUM),
                relu_bwd_colsum=RR.fraction(gsum.numpy('colsum'), want.astype(np.float64).sum(axis=0), RR.TOL_COLSUM))
    assert max(fr.values()) <= 1.0, fr


@pytest.mark.parametrize('exit_', [0, 3, 4, 7])
def test_colsum_whole_lines_every_exit(env, big, exit_):
    """colsum_lines_kernel (cols divides 1024, >= 2^22 elements): line counts whose last block holds n lines with n % 8 = 0 / 3 /
    4 / 7 -- the closing pair of groups, the pair and single lines, one closing group, one group and single lines."""
    _C, D = env
    cus = compute_units()
    lines = RR.colsum_line_cases(cus)[exit_]
    last = RR.colsum_lines_plan(lines, cus)[2]
    assert last % 8 == exit_ and last >= 4
    cols = 128
    rows = lines * (1024 // cols)
    pre, dy = big['x'][:rows * cols].reshape(rows, cols), big['dz'][:rows * cols].reshape(rows, cols)
    out, pd, dd = Guarded(D, [cols]), D.from_host(pre), D.from_host(dy)
    _C.check(_C.lib().npm_colsum(pd.ptr, out.ptr, rows, cols, cols))
    g, gsum = Guarded(D, [rows, cols]), Guarded(D, [cols])
    _C.check(_C.lib().npm_relu_bwd_colsum(pd.ptr, dd.ptr, g.ptr, gsum.ptr, rows, cols))
    want = np.where(pre >= 0, dy, 0).astype(np.float32)
    np.testing.assert_array_equal(g.numpy('relu_bwd'), want)
    fr = report('f whole lines %d (last block %d)' % (lines, last), colsum=RR.fraction(out.numpy('colsum'), pre.astype(np.float64).sum(axis=0), RR.TOL_COLSUM),
                relu_bwd_colsum=RR.fraction(gsum.numpy('colsum'), want.astype(np.float64).sum(axis=0), RR.TOL_COLSUM))
    assert max(fr.values()) <= 1.0, fr


@pytest.mark.parametrize('cols', RR.COLSUM_NT_COLS)
def test_colsum_nt(env, big, cols):
    """>= 32 MB: the NT instances of the whole-line kernel (128 columns) and of the strip kernel, plain and with the ReLU
    backward, against the same calls without the hint and float64.  132 and 200 columns are multiples of 4 that do not divide
    1024: the strip kernel's float4 branch, the only place where its NT loads and stores are (unrolled body and single-row
    remainder, tests/test_rowops_host.py); 130 columns launch the NT instances on their scalar branch."""
    _C, D = env
    rows = RR.colsum_nt_rows(cols)
    assert 4 * rows * cols >= RR.NT_BYTES and rows * cols <= big['x'].size
    pre, dy = big['x'][:rows * cols].reshape(rows, cols), big['dz'][:rows * cols].reshape(rows, cols)
    pd, dd = D.from_host(pre), D.from_host(dy)
    want = np.where(pre >= 0, dy, 0).astype(np.float32)
    got = {}
    for nt in (0, 1):
        with tuned(KNOB_STREAM_NT, nt):
            out, g, gsum = Guarded(D, [cols]), Guarded(D, [rows, cols]), Guarded(D, [cols])
            _C.check(_C.lib().npm_colsum(pd.ptr, out.ptr, rows, cols, cols))
            _C.check(_C.lib().npm_relu_bwd_colsum(pd.ptr, dd.ptr, g.ptr, gsum.ptr, rows, cols))
            np.testing.assert_array_equal(g.numpy('relu_bwd'), want)
            got[nt] = (out.numpy('colsum'), gsum.numpy('colsum'))
    fr = report('f colsum NT cols=%d' % cols, colsum=RR.fraction(got[0][0], pre.astype(np.float64).sum(axis=0), RR.TOL_COLSUM),
                relu_bwd_colsum=RR.fraction(got[0][1], want.astype(np.float64).sum(axis=0), RR.TOL_COLSUM),
                same=RR.fraction(got[1][0], got[0][0], RR.TOL_SAME), same_relu=RR.fraction(got[1][1], got[0][1], RR.TOL_SAME))
    assert max(fr.values()) <= 1.0, fr
