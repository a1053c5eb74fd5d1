"""CPU: the float32 models of tests/rowops_reference.py against the float64 oracle, on exactly the grids tests/test_gpu_rowops_paths.py
runs on the device, and the case lists themselves.

Every model must stay at or below HALF of the bound the GPU test applies (``HALF``): the bound then has a twofold margin over the
kernels' own summation order, and a case that needs more on the device is a defect, not rounding.  The conditioned LayerNorm bound
is tol (|ref| + max |ref|) (1 + kappa / KAPPA_DIV) with KAPPA_DIV = 8.  With the divisor 16 the models reached 0.64 of it on the
constant row of 0.1 at d = 4096, above a half, so it was halved once; with 8 the worst fraction the models reach on the range data
is 0.35 (that constant row; 0.14 on the shifted rows, 0.02 on the outlier and the 1e-20 rows), as test_layernorm_models_on_range_data prints
(-s), and a one-pass variance still misses it more than twentyfold (test_one_pass_variance_misses_the_conditioned_bound).
"""

import numpy as np
import pytest

import rowops_reference as RR
from oracle import np_oracle as O

HALF = 0.5


def _ln_fractions(data, rows_for_grid=None, residual=True, grid=None):
    x, gamma, beta, dz = data['x'], data['gamma'], data['beta'], data['dz']
    res = data['res'] if residual else None
    z, mean, rstd = RR.layernorm_fwd_model(x, gamma, beta)
    dx, dg, db = RR.layernorm_bwd_model(dz, x, mean, rstd, gamma, res, grid)
    ref = RR.layernorm_ref(x, gamma, beta, dz, res)
    return dict(z=RR.fraction(z, ref['z'], RR.TOL_Z), mean=RR.fraction(mean, ref['mean'], RR.TOL_STAT),
                rstd=RR.fraction(rstd, ref['rstd'], RR.TOL_STAT), dx=RR.fraction(dx, ref['dx'], RR.TOL_DX),
                dgamma=RR.fraction(dg, ref['dgamma'], RR.TOL_DX), dbeta=RR.fraction(db, ref['dbeta'], RR.TOL_DX))


def test_reference_agrees_with_the_oracle():
    """rowops_reference's float64 forms are the oracle's (oracle/np_oracle.py), which the existing GPU tests compare with."""
    d = RR.grid_data(9, 72)
    x64, g64, b64, dz64 = (d[k].astype(np.float64) for k in ('x', 'gamma', 'beta', 'dz'))
    ref = RR.layernorm_ref(d['x'], d['gamma'], d['beta'], d['dz'])
    z, cache = O.layernorm_fwd(x64, g64, b64, RR.EPS)
    dx, dg, db = O.layernorm_bwd(x64, g64, RR.EPS, cache, dz64)
    for name, want in (('z', z), ('dx', dx), ('dgamma', dg), ('dbeta', db), ('mean', cache[0][:, 0]), ('rstd', 1 / np.sqrt(cache[1][:, 0] + RR.EPS))):
        np.testing.assert_allclose(ref[name], want, rtol=1e-12, atol=1e-13, err_msg=name)
    x, dy = RR.softmax_data(5, 40)
    np.testing.assert_allclose(RR.softmax_ref(x, 0.125), O.softmax_fwd(0.125 * x.astype(np.float64)), rtol=1e-13)
    y = RR.softmax_ref(x)
    np.testing.assert_allclose(RR.softmax_bwd_ref(y, dy, 0.125), 0.125 * O.softmax_bwd(y, dy.astype(np.float64)), rtol=1e-12, atol=1e-15)


def test_width_grid_has_every_class_edge():
    assert len(RR.WIDTHS) == len(RR.VPLS)
    below = 0
    for vpl, (small, part, big) in zip(RR.VPLS, RR.WIDTHS):
        assert RR.vpl_of(small) == RR.vpl_of(part) == RR.vpl_of(big) == vpl
        assert small == max(below + 4, 4) and big == 256 * vpl and small < part < big
        full, last = RR.chunk_groups(part)
        assert 0 < last < RR.WAVE and full < vpl, (part, full, last)         # a partly filled group that the guard must cut
        assert RR.chunk_groups(big) == (vpl, 0)
        below = big
    for n in RR.GENERIC_WIDTHS:
        assert RR.vpl_of(n) is None
    assert any(n % 4 for n in RR.GENERIC_WIDTHS) and any(n > 4096 and n % 4 == 0 for n in RR.GENERIC_WIDTHS)
    for ws in (RR.ONE_PER_CLASS, RR.WALK_WIDTHS, RR.NT_WIDTHS):
        assert tuple(RR.vpl_of(n) for n in ws) == RR.VPLS
    assert {r % 4 for r in RR.ROW_COUNTS} >= {1, 3} and 1 in RR.ROW_COUNTS and max(RR.ROW_COUNTS) > 8


def test_nt_shapes_are_on_their_side_of_the_threshold():
    for d in RR.NT_WIDTHS + (640,):
        rows = RR.nt_rows(d)
        assert 4 * rows * d >= RR.NT_BYTES and rows % 4 == (3 if d != 640 else 2) and rows * d <= RR.NT_ELEMS + 3 * 4096      # a last block with idle waves
    assert 4 * (RR.NT_ELEMS + 5) >= RR.NT_BYTES
    for d in RR.ALL_WIDTHS:
        assert 4 * max(RR.ROW_COUNTS) * d < RR.NT_BYTES
    for d in RR.WALK_WIDTHS:
        assert 4 * RR.ln_walk_rows() * d < RR.NT_BYTES
    assert 4 * 4 * 2049 * 8 * 128 >= RR.NT_BYTES                  # attn_rowdot's large shape
    assert 4 * max(RR.ew_size(c) for c in RR.EW_CAPS) < RR.NT_BYTES and max(RR.ew_size(c) for c in RR.EW_CAPS) < 20000


def test_colsum_nt_shapes_reach_the_vector_and_the_scalar_branch():
    """The >= 32 MB column sums: 128 columns take the whole-line kernel; 130 the strip kernel's scalar branch; 132 and 200 its
    float4 branch in more than one chunk (the only launch of the NT instances), where the last chunk runs the unrolled body and
    the single-row remainder (200: two remainder trips for some row lanes)."""
    for cols in RR.COLSUM_NT_COLS:
        rows = RR.colsum_nt_rows(cols)
        assert 4 * rows * cols >= RR.NT_BYTES and rows * cols <= RR.NT_ELEMS + 3 * 4096
        if 1024 % cols == 0:
            assert rows % (1024 // cols) == 0
            continue
        strips, chunks, rpc, last = RR.colsum_strip_plan(rows, cols)
        assert chunks > 1 and strips > 1
        if cols % 4:
            continue                                                            # ld % 4 != 0: every thread on the scalar branch
        assert cols % 64 and cols % 64 >= 4                                     # a last strip with float4 and with idle threads
        assert RR.colsum_strip_trips(rpc)[0] >= {4}
        unrolled, rest = RR.colsum_strip_trips(last)
        assert min(unrolled) >= 1 and max(rest) >= 1, (cols, last, unrolled, rest)
    assert RR.colsum_strip_trips(RR.colsum_strip_plan(RR.colsum_nt_rows(200), 200)[3])[1] == {1, 2}
    assert {c % 4 == 0 for c in RR.COLSUM_NT_COLS if 1024 % c} == {True, False}


def test_colsum_edge_rows_sit_next_to_the_unroll_trip():
    """COLSUM_EDGE_ROWS: rows per chunk one below, at or one above a multiple of 64 -- in one chunk up to 256 rows, in two (255,
    256) and in three (193)."""
    per_chunk = [RR.colsum_strip_plan(rows, 100)[1:3] for rows in RR.COLSUM_EDGE_ROWS]
    assert all(rpc % 64 in (63, 0, 1) for _, rpc in per_chunk), per_chunk
    assert {c for c, _ in per_chunk} == {1, 2, 3} and {rpc % 64 for _, rpc in per_chunk} == {63, 0, 1}


@pytest.mark.parametrize('cap', RR.EW_CAPS)
def test_elementwise_sizes_reach_every_loop(cap):
    n = RR.ew_size(cap)
    p = RR.ew_paths(n, cap)
    assert p['grid'] == cap and p['covered']
    assert p['unrolled'] == p['stride'] and p['unrolled_trips'] == 1          # every thread runs the unrolled body once
    assert p['remainder'] == {1, 2}                                            # a remainder of more than one stride
    assert p['tail'] == 3 == n % 4
    default = RR.ew_paths(n, 1 << 20)                                           # and under the default cap none of it runs
    assert default['unrolled'] == 0 and default['remainder'] == {0, 1} and default['covered']


def test_walk_shape_gives_three_and_two_rows():
    rows = RR.ln_walk_rows()
    assert RR.ln_bwd_grid(rows, 1) == RR.CUS
    counts = RR.ln_walk_counts(rows, RR.CUS)
    assert set(counts) == {2, 3} and counts[3] == 2 * RR.CUS + 3 and counts[2] == 2 * RR.CUS - 3
    assert max(RR.ln_walk_counts(rows, RR.ln_bwd_grid(rows))) == 1                   # the default grid walks nothing


@pytest.mark.parametrize('n', RR.ALL_WIDTHS)
def test_softmax_models_on_the_width_grid(n):
    worst = {}
    for rows in RR.ROW_COUNTS:
        x, dy = RR.softmax_data(rows, n)
        for scale in (1.0, 0.125):
            y = RR.softmax_fwd_model(x, scale)
            worst['y'] = max(worst.get('y', 0), RR.fraction(y, RR.softmax_ref(x, scale), RR.TOL_SOFTMAX))
            worst['dx'] = max(worst.get('dx', 0), RR.fraction(RR.softmax_bwd_model(y, dy, scale), RR.softmax_bwd_ref(y, dy, scale), RR.TOL_SOFTMAX_BWD))
    print('softmax n=%d model fractions' % n, worst)
    assert max(worst.values()) <= HALF, worst


@pytest.mark.parametrize('d', RR.ALL_WIDTHS)
def test_layernorm_models_on_the_width_grid(d):
    worst = {}
    for rows in RR.ROW_COUNTS:
        for residual in (False, True):
            for k, v in _ln_fractions(RR.grid_data(rows, d), residual=residual).items():
                worst[k] = max(worst.get(k, 0), v)
    print('layernorm d=%d model fractions' % d, worst)
    assert max(worst.values()) <= HALF, worst


@pytest.mark.parametrize('d', RR.ONE_PER_CLASS + (1001, 4096))
def test_layernorm_models_on_range_data(d):
    worst = {}
    for kind in RR.LN_RANGE_KINDS:
        x = RR.ln_range(kind, d)
        p = RR.grid_data(x.shape[0], d, seed=1)
        z, mean, rstd = RR.layernorm_fwd_model(x, p['gamma'], p['beta'])
        dx, dg, db = RR.layernorm_bwd_model(p['dz'], x, mean, rstd, p['gamma'])
        fr = RR.ln_range_fractions(kind, x, p['gamma'], p['beta'], p['dz'], dict(z=z, mean=mean, rstd=rstd, dx=dx, dgamma=dg))
        print('layernorm range d=%d %-16s kappa %.3g' % (d, kind, RR.kappa(x).max()), {k: round(v, 3) for k, v in fr.items()})
        worst[kind] = max(fr.values())
        assert np.isfinite(dx).all()
    assert max(worst.values()) <= HALF, worst


def test_one_pass_variance_misses_the_conditioned_bound():
    """What the bound is for: var = E[x^2] - mean^2 in float32 is far outside it (40 times at kappa = 1e3, more beyond)."""
    d = 900
    x = RR.ln_range('shift_1000_1', d)
    p = RR.grid_data(3, d, seed=1)
    mean = RR._row_sum(x) / RR.F(d)
    var = np.maximum(RR._row_sum(x * x) / RR.F(d) - mean * mean, 0)
    rstd = RR.F(1) / np.sqrt(var + RR.F(RR.EPS))
    z = p['gamma'] * ((x - mean) * rstd) + p['beta']
    ref = RR.layernorm_ref(x, p['gamma'], p['beta'], p['dz'])
    assert RR.cond_fraction(z, ref['z'], RR.TOL_Z, RR.kappa(x)) > 20


@pytest.mark.parametrize('n', RR.ONE_PER_CLASS + (1001,))
def test_softmax_models_on_range_data(n):
    x, dead = RR.softmax_range(n)
    live = np.arange(x.shape[0]) != dead
    y = RR.softmax_fwd_model(x)
    ref = RR.softmax_ref(x)
    assert np.isnan(ref[dead]).all() and np.isnan(y[dead]).all() and np.isfinite(ref[live]).all() and np.isfinite(y[live]).all()
    assert (y[live][np.isinf(x[live])] == 0).all()
    np.testing.assert_allclose(y[live].sum(axis=1, dtype=np.float64), 1.0, rtol=1e-5)
    dy = RR.softmax_data(x.shape[0], n, seed=2)[1]
    fr = dict(y=RR.fraction(y[live], ref[live], RR.TOL_SOFTMAX),
              dx=RR.fraction(RR.softmax_bwd_model(y, dy)[live], RR.softmax_bwd_ref(y, dy)[live], RR.TOL_SOFTMAX_BWD))
    print('softmax range n=%d model fractions' % n, fr)
    assert max(fr.values()) <= HALF, fr


@pytest.mark.parametrize('rows,d,blocks_per_cu', [(RR.nt_rows(256), 256, 4), (RR.nt_rows(4096), 4096, 4), (RR.ln_walk_rows(), 3076, 1),
                                                  (RR.ln_walk_rows(), 72, 1)])
def test_dgamma_dbeta_models_at_the_largest_row_counts(rows, d, blocks_per_cu):
    """The sums over the rows at the most rows the GPU tests use: the NT shapes (8 rows per wave at d = 256) and the row walk."""
    rng = np.random.default_rng(d)
    data = dict(x=rng.standard_normal((rows, d)).astype(np.float32), dz=rng.standard_normal((rows, d)).astype(np.float32),
                gamma=rng.standard_normal(d).astype(np.float32), beta=rng.standard_normal(d).astype(np.float32))
    fr = _ln_fractions(data, residual=False, grid=RR.ln_bwd_grid(rows, blocks_per_cu))
    print('rows=%d d=%d model fractions' % (rows, d), fr)
    assert max(fr.values()) <= HALF, fr


@pytest.mark.parametrize('rows,cols', [(37, 12), (1000, 64), (300, 200), (5000, 130), (63, 64), (65, 64), (1024, 2 * 3076)])
def test_colsum_model(rows, cols):
    x = np.random.default_rng(rows + cols).standard_normal((rows, cols)).astype(np.float32)
    fr = RR.fraction(RR.colsum_model(x), x.astype(np.float64).sum(axis=0), RR.TOL_COLSUM)
    assert fr <= HALF, fr
