"""GPU: npm_rmsnorm_fwd / npm_rmsnorm_bwd (csrc/npm_rowops.hip) against the float64 restatement of tests/llama_reference.py over
the width grid of tests/rowops_reference.py, at the tolerances tests/test_gpu_rowops.py holds LayerNorm to (the same arithmetic
class: one row reduction, a reciprocal square root, two or three products per element): conftest.assert_close with 3e-6 for z,
2e-6 for rstd, 5e-6 for dx and dgamma.  Every output sits between sentinel-filled guard bands that must survive
(test_gpu_rowops_paths.Guarded)."""

import numpy as np
import pytest

import llama_reference as LR
import rowops_reference as RR
import test_gpu_rowops_paths as P
from conftest import assert_close

pytestmark = pytest.mark.gpu

EPS = LR.RMS_EPS
env = P.env


@pytest.fixture(autouse=True)
def _knobs_back():
    try:
        yield
    finally:
        for knob, value in P.KNOB_DEFAULTS.items():
            P._tune(knob, value)


def rms_fwd(env, x, gamma, rows, d, lead=0, eps=EPS):
    """(z, rstd) as Guarded."""
    _C, D = env
    z, rstd = P.Guarded(D, [rows, d], lead=lead), P.Guarded(D, [rows])
    _C.check(_C.lib().npm_rmsnorm_fwd(x.ptr, gamma.ptr, eps, rows, d, z.ptr, rstd.ptr), 'npm_rmsnorm_fwd')
    return z, rstd


def rms_bwd(env, dz, x, rstd, gamma, res, rows, d, lead=0):
    """(dx, dgamma) as host arrays, guard bands checked."""
    _C, D = env
    dx, dg = P.Guarded(D, [rows, d], lead=lead), P.Guarded(D, [d])
    _C.check(_C.lib().npm_rmsnorm_bwd(dz.ptr, x.ptr, rstd.ptr, gamma.ptr, None if res is None else res.ptr, rows, d, dx.ptr, dg.ptr),
             'npm_rmsnorm_bwd')
    return dx.numpy('dx'), dg.numpy('dgamma')


def run(env, data, with_residual, lead=0):
    """Forward and backward of one case -> dict z, rstd, dx, dgamma (host)."""
    _C, D = env
    rows, d = data['x'].shape
    if lead:                                       # the inputs too sit 4 bytes off the 16-byte grid
        holders = {k: P.Guarded(D, data[k].shape, lead=lead) for k in ('x', 'dz', 'res')}
        for k, h in holders.items():
            h.arr.set(data[k])
        x, dz, res = (holders[k].arr for k in ('x', 'dz', 'res'))
    else:
        x, dz, res = (D.from_host(data[k]) for k in ('x', 'dz', 'res'))
    gamma = D.from_host(data['gamma'])
    z, rstd = rms_fwd(env, x, gamma, rows, d, lead=lead)
    out = dict(z=z.numpy('z'), rstd=rstd.numpy('rstd'))
    out['dx'], out['dgamma'] = rms_bwd(env, dz, x, rstd.arr, gamma, res if with_residual else None, rows, d, lead=lead)
    return out


def check(got, data, with_residual, what):
    ref = LR.rmsnorm_ref(data['x'], data['gamma'], data['dz'], data['res'] if with_residual else None, EPS)
    P.report(what, z=RR.fraction(got['z'], ref['z'], RR.TOL_Z), rstd=RR.fraction(got['rstd'], ref['rstd'], RR.TOL_STAT),
             dx=RR.fraction(got['dx'], ref['dx'], RR.TOL_DX), dgamma=RR.fraction(got['dgamma'], ref['dgamma'], RR.TOL_DX))
    assert_close(got['z'], ref['z'], tol=RR.TOL_Z, what=what + ' z')
    assert_close(got['rstd'], ref['rstd'], tol=RR.TOL_STAT, what=what + ' rstd')
    assert_close(got['dx'], ref['dx'], tol=RR.TOL_DX, what=what + ' dx')
    assert_close(got['dgamma'], ref['dgamma'], tol=RR.TOL_DX, what=what + ' dgamma')


# every width of the grid, the row counts taken in turn (d = 4 gets rows = 1)
GRID = [(d, RR.ROW_COUNTS[i % len(RR.ROW_COUNTS)]) for i, d in enumerate(RR.ALL_WIDTHS)]


@pytest.mark.parametrize('with_residual', [False, True])
@pytest.mark.parametrize('d,rows', GRID)
def test_width_grid(env, d, rows, with_residual):
    data = RR.grid_data(rows, d)
    check(run(env, data, with_residual), data, with_residual, 'rmsnorm d=%d rows=%d res=%d' % (d, rows, with_residual))


@pytest.mark.parametrize('with_residual', [False, True])
@pytest.mark.parametrize('rows', RR.ROW_COUNTS)
@pytest.mark.parametrize('d', [72, 33])
def test_row_counts(env, d, rows, with_residual):
    data = RR.grid_data(rows, d, seed=1)
    check(run(env, data, with_residual), data, with_residual, 'rmsnorm d=%d rows=%d res=%d' % (d, rows, with_residual))


@pytest.mark.parametrize('with_residual', [False, True])
def test_row_walk_and_block_partials(env, with_residual):
    """5000 rows of 256: 1250 blocks > 4 per CU on the device, so waves own several rows and the block partials are many."""
    data = RR.grid_data(5000, 256)
    check(run(env, data, with_residual), data, with_residual, 'rmsnorm 5000 x 256 res=%d' % with_residual)


@pytest.mark.parametrize('with_residual', [False, True])
@pytest.mark.parametrize('d', [256, 900])
def test_base_off_the_16_byte_grid_takes_the_generic_kernels(env, d, with_residual):
    data = RR.grid_data(7, d, seed=2)
    check(run(env, data, with_residual, lead=1), data, with_residual, 'rmsnorm misaligned d=%d res=%d' % (d, with_residual))


@pytest.mark.parametrize('d', [4, 72, 1024, 1001])
def test_edge_rows(env, d):
    """Row 0 all zero: z = 0, rstd = 1 / sqrt(eps), dx finite (= rstd dz gamma).  Row 1 one large outlier.  Row 2 ordinary."""
    data = RR.grid_data(3, d, seed=3)
    data['x'][0] = 0.0
    data['x'][1, d // 2] = 1e6
    got = run(env, data, False)
    assert (got['z'][0] == 0).all()
    assert abs(got['rstd'][0] - 1.0 / np.sqrt(np.float64(np.float32(EPS)))) <= 2 * RR.TOL_STAT / np.sqrt(EPS)
    assert np.isfinite(got['dx']).all()
    check(got, data, False, 'rmsnorm edge rows d=%d' % d)
    one = {k: (v[1:2] if v.ndim == 2 else v) for k, v in data.items()}          # rows = 1 (and d = 4)
    check(run(env, one, True), one, True, 'rmsnorm one row d=%d' % d)


@pytest.mark.parametrize('d', [72, 900, 3076, 1001])
def test_a_row_does_not_depend_on_its_neighbours_or_its_position(env, d):
    data = RR.grid_data(9, d, seed=4)
    whole = run(env, data, True)
    alone = run(env, {k: (v[3:4] if v.ndim == 2 else v) for k, v in data.items()}, True)
    P.same_bits(whole['z'][3], alone['z'][0], 'z alone')
    P.same_bits(whole['dx'][3], alone['dx'][0], 'dx alone')
    other = RR.grid_data(13, d, seed=5)
    for k in ('x', 'dz', 'res'):
        other[k][7] = data[k][3]
    other['gamma'] = data['gamma']
    moved = run(env, other, True)
    P.same_bits(whole['z'][3], moved['z'][7], 'z moved')
    P.same_bits(whole['dx'][3], moved['dx'][7], 'dx moved')
    P.same_bits(whole['dgamma'], run(env, data, True)['dgamma'], 'dgamma over two runs')


@pytest.mark.parametrize('d', [260, 1024])
def test_backward_blocks_per_cu(env, d):
    """NPM_TUNE_LN_BWD_BLOCKS 1 and 4: other groupings of the same sum -- equal to the tolerance, each reproducible in bits."""
    rows = RR.ln_walk_rows(P.compute_units())
    data = RR.grid_data(rows, d, seed=6)
    got = {}
    for blocks in (1, 4):
        with P.tuned(P.KNOB_LN_BWD_BLOCKS, blocks):
            got[blocks] = run(env, data, True)
            again = run(env, data, True)
        P.same_bits(got[blocks]['dgamma'], again['dgamma'], 'dgamma, %d blocks per CU, two runs' % blocks)
        P.same_bits(got[blocks]['dx'], again['dx'], 'dx, %d blocks per CU, two runs' % blocks)
        check(got[blocks], data, True, 'rmsnorm %d x %d, %d blocks per CU' % (rows, d, blocks))
    P.same_bits(got[1]['dx'], got[4]['dx'], 'dx does not depend on the grid')
    assert_close(got[1]['dgamma'], got[4]['dgamma'], tol=RR.TOL_DX, what='dgamma 1 against 4 blocks per CU')


@pytest.mark.parametrize('d', RR.NT_WIDTHS)
def test_nontemporal_instances_equal_the_plain_ones_in_bits(env, d):
    _C, D = env
    rows = RR.nt_rows(d)
    assert 4 * rows * d >= RR.NT_BYTES
    rng = np.random.default_rng(d)
    x = (rng.standard_normal(rows * d, dtype=np.float32) * 2 + np.float32(0.5)).reshape(rows, d)
    dz = rng.standard_normal(rows * d, dtype=np.float32).reshape(rows, d)
    res = np.ascontiguousarray(x[::-1])
    gamma = rng.standard_normal(d, dtype=np.float32)
    xd, dzd, rd, gd = D.from_host(x), D.from_host(dz), D.from_host(res), D.from_host(gamma)
    got = {}
    for nt in (0, 1):
        with P.tuned(P.KNOB_STREAM_NT, nt):
            z, rstd = rms_fwd(env, xd, gd, rows, d)
            cur = dict(z=z.numpy('z'), rstd=rstd.numpy('rstd'))
            cur['dx'], cur['dgamma'] = rms_bwd(env, dzd, xd, rstd.arr, gd, rd, rows, d)
        got[nt] = cur
    for k in got[0]:
        P.same_bits(got[1][k], got[0][k], '%s with the hint against without, d=%d' % (k, d))
    pick = P.sample_rows(rows)
    ref = LR.rmsnorm_ref(x[pick], gamma, dz[pick], res[pick], EPS)
    fr = dict(z=RR.fraction(got[1]['z'][pick], ref['z'], RR.TOL_Z), rstd=RR.fraction(got[1]['rstd'][pick], ref['rstd'], RR.TOL_STAT),
              dx=RR.fraction(got[1]['dx'][pick], ref['dx'], RR.TOL_DX))
    dg = np.zeros(d)
    for at in range(0, rows, 4096):
        x64, z64 = x[at:at + 4096].astype(np.float64), dz[at:at + 4096].astype(np.float64)
        dg += (z64 * x64 / np.sqrt((x64 * x64).mean(axis=1, keepdims=True) + EPS)).sum(axis=0)
    fr['dgamma'] = RR.fraction(got[1]['dgamma'], dg, RR.TOL_DX)
    P.report('rmsnorm NT d=%d' % d, **fr)
    assert max(fr.values()) <= 1.0, fr


def test_empty_batch_and_argument_checks(env):
    _C, D = env
    lib = _C.lib()
    dg = P.Guarded(D, [8])
    assert lib.npm_rmsnorm_fwd(None, None, EPS, 0, 8, None, None) == 0
    assert lib.npm_rmsnorm_bwd(None, None, None, None, None, 0, 8, None, dg.ptr) == 0
    assert (dg.numpy('dgamma') == 0).all()
    assert lib.npm_rmsnorm_fwd(None, None, EPS, 2, 8, None, None) != 0
    assert lib.npm_rmsnorm_bwd(None, None, None, None, None, 2, 0, None, dg.ptr) != 0
