"""GPU: every Conv2D kernel instance, K order, knob value and split seam at image edges (tests/conv_cases.py; the cells are proved
on the CPU by tests/test_conv_host.py).  Every case asserts which kernel ran (``npm_last_conv_kernel`` against ``route`` with the
device's own CU count), the values against float64 at the bounds tests/test_gpu_conv.py has always used (3e-6; 5e-6 for dw), the
bit equalities that hold by construction, and the memory around every tensor: inputs sit inside NaN, outputs are pre-filled with a
NaN pattern between guard words.  A test id carries the cases of one geometry class (or of one list): ``each`` runs them all and
names the ones that failed."""

import ctypes as C
import functools

import numpy as np
import pytest

import conv_cases as CC
from conftest import assert_close
from oracle import np_oracle as O

pytestmark = pytest.mark.gpu

TOL, TOL_DW = 3e-6, 5e-6


@pytest.fixture(scope='module')
def env():
    from np_modeling_amd import _C, device as D
    from test_gpu_rowops_paths import compute_units
    _C.lib()
    return _C, D, compute_units()


def each(cases, run):
    """One test id carries a group of cases (the suite's id count is what every later run pays for): every case of the group
    runs, whatever the ones before it did, and the id fails with the list of the cases that failed."""
    assert cases
    problems = []
    for case in cases:
        try:
            run(case)
        except AssertionError as err:
            problems.append('%s: %s' % (case.id, str(err).strip()[:600]))
    assert not problems, '%d of %d cases failed:\n%s' % (len(problems), len(cases), '\n'.join(problems))


FWD_CLASSES = [name for name, _ in CC.FWD_GEOMETRIES]
FUSED_CLASSES = [name for name, _ in CC.FUSED_GEOMETRIES]


def of_class(cases, geometry):
    return [c for c in cases if c.geometry == geometry]


# the groups leave no case out
assert all({c.geometry for c in cases} <= set(FWD_CLASSES) for cases in (CC.FWD_PLAIN, CC.FWD_DMA, CC.FWD_KNOBS, CC.FWD_PRIO, CC.FWD_MISALIGNED))
assert {c.cell for c in CC.FUSED} == set(FUSED_CLASSES)


@functools.lru_cache(maxsize=None)
def reference(shape, seed):
    """The host operands of ``ConvCall(shape, seed)`` (the same generator; ``call_for`` compares) and their float64 results,
    computed once per shape and left unchanged."""
    n, h, w, c0, c1, k = shape
    rng = np.random.default_rng([seed, n, h, w, c0, c1, k])
    x = rng.standard_normal((n, h, w, c0)).astype(np.float32)
    filt = rng.standard_normal((k, k, c0, c1)).astype(np.float32)
    bias = rng.standard_normal(c1).astype(np.float32)
    dy = rng.standard_normal((n, h, w, c1)).astype(np.float32)
    x64, f64, dy64 = x.astype(np.float64), filt.astype(np.float64), dy.astype(np.float64)
    return dict(x=x, filt=filt, bias=bias, dy=dy, y=O.conv2d_fwd(x64, f64), bias64=bias.astype(np.float64),
                dx=O.conv2d_grad_x(dy64, f64), dw=functools.partial(O.conv2d_grad_w, x=x64, k=k))


def call_for(env, shape, seed, offset=0):
    _C, D, _ = env
    call = CC.ConvCall(D, _C, shape, seed, offset)
    ref = reference(shape, seed)
    for name in ('x', 'filt', 'bias', 'dy'):
        assert np.array_equal(getattr(call, name), ref[name]), name
    return call, ref


def check_forward(call, ref, knobs, want_report, want_math, what):
    """All four epilogues; returns {epilogue: (y, pre)}."""
    out = {}
    for name, bias, relu, save in CC.EPILOGUES:
        y, pre, report, math = call.fwd(knobs, bias=bias, relu=relu, save_pre=save)
        assert report == want_report, f'{what} {name}: ran {report!r}'
        assert math == want_math, f'{what} {name}: npm_last_math says {math}'
        want = ref['y'] + ref['bias64'] if bias else ref['y']
        if save:
            assert_close(pre, want, tol=TOL, what=f'{what} {name} pre')
            assert np.array_equal(CC.bits(y), CC.bits(np.maximum(pre, np.float32(0)))), f'{what} {name}: y is not max(pre, 0)'
        elif relu:
            assert_close(y, np.maximum(want, 0), tol=TOL, what=f'{what} {name} y')
            assert (y >= 0).all()
        else:
            assert_close(y, want, tol=TOL, what=f'{what} {name} y')
        out[name] = (y, pre)
    return out


def run_fwd_case(env, case, mode='f32'):
    _C, D, cus = env
    call, ref = call_for(env, case.shape, 11, case.offset)
    want_fwd, want_bwd = case.routes(cus, mode)
    maths = [CC.CONV_MATH[mode][1] if CC.instance(r) in ('dma', 'tall') else 'f32' for r in (want_fwd, want_bwd)]
    what = f'{case.id} math={mode}'
    out = check_forward(call, ref, case.knobs, want_fwd, maths[0], what + ' fwd')
    dx, report, math = call.bwd_x(case.knobs)
    assert report == want_bwd, f'{what} bwd_x: ran {report!r}'
    assert math == maths[1], f'{what} bwd_x: npm_last_math says {math}'
    assert_close(dx, ref['dx'], tol=TOL, what=what + ' dx')
    return call, ref, out, dx


@pytest.mark.parametrize('geometry', FWD_CLASSES)
def test_forward_and_grad_x_register_staged(env, geometry):
    """The scalar and the float4 instance at every geometry: f32 whatever mode is set (checked under bf16x3 for the first pairs)."""
    _C = env[0]

    def run(case):
        run_fwd_case(env, case)
        if (case.c0, case.c1) in ((3, 5), (4, 8)):
            _C.set_math('bf16x3')
            try:
                run_fwd_case(env, case, 'bf16x3')         # reports and runs f32
            finally:
                _C.set_math('f32')

    each(of_class(CC.FWD_PLAIN, geometry), run)


@pytest.mark.parametrize('geometry', FWD_CLASSES)
def test_forward_and_grad_x_dma(env, geometry, math_mode):
    each(of_class(CC.FWD_DMA, geometry), lambda case: run_fwd_case(env, case, math_mode))


@pytest.mark.parametrize('geometry', FWD_CLASSES)
def test_forward_and_grad_x_knobs(env, geometry):
    """KORDER = 0, CONV_DMA = 0 / 2: another summation order or another kernel, so float64 only."""
    each(of_class(CC.FWD_KNOBS, geometry), lambda case: run_fwd_case(env, case))


@pytest.mark.parametrize('geometry', sorted({c.geometry for c in CC.FWD_PRIO}))
def test_wave_priority_changes_no_bit(env, geometry):
    each(of_class(CC.FWD_PRIO, geometry), lambda case: wave_priority_case(env, case))


def wave_priority_case(env, case):
    call, ref, out, dx = run_fwd_case(env, case)
    base = case._replace(knobs=CC.DEFAULT)
    for name, bias, relu, save in CC.EPILOGUES:
        y, pre, report, _ = call.fwd(base.knobs, bias=bias, relu=relu, save_pre=save)
        assert report == base.routes(env[2])[0]
        assert np.array_equal(CC.bits(y), CC.bits(out[name][0])), f'{case.id} {name}: y'
        if save:
            assert np.array_equal(CC.bits(pre), CC.bits(out[name][1])), f'{case.id} {name}: pre'
    dx0, _, _ = call.bwd_x(base.knobs)
    assert np.array_equal(CC.bits(dx0), CC.bits(dx)), f'{case.id}: dx'


@pytest.mark.parametrize('geometry', sorted({c.geometry for c in CC.FWD_MISALIGNED}))
def test_misaligned_base_takes_the_scalar_instance(env, geometry):
    def run(case):
        assert [CC.instance(r) for r in case.routes(env[2])] == ['scalar', 'scalar']
        run_fwd_case(env, case)

    each(of_class(CC.FWD_MISALIGNED, geometry), run)


# ---- filter gradient ------------------------------------------------------------------------------------------------------------------------
def run_wgrad_case(env, case, mode='f32'):
    _C, D, cus = env
    call, ref = call_for(env, case.shape, 12, case.offset)
    want = case.route(cus, mode)
    if not case.cus_dependent:
        assert want == case.route(256, mode), f'{case.id}: the route depends on the CU count and the case does not say so'
    dw, report, math = call.bwd_w(case.knobs)
    what = f'{case.id} math={mode}'
    assert report == want, f'{what}: ran {report!r}, not {want!r}'
    assert math == (CC.CONV_MATH[mode][1] if CC.instance(want) == 'dma' else 'f32'), f'{what}: npm_last_math says {math}'
    if 'dw_of_dy' not in ref:
        ref['dw_of_dy'] = ref['dw'](ref['dy'].astype(np.float64))
    assert_close(dw, ref['dw_of_dy'], tol=TOL_DW, what=what + ' dw')
    if CC.fields(want)['splits'] > 1:                      # fixed-order slab reduction: two runs, the same bits
        again, report2, _ = call.bwd_w(case.knobs)
        assert report2 == want and np.array_equal(CC.bits(again), CC.bits(dw)), f'{what}: two runs differ'


def test_filter_gradient_dma(env, math_mode):
    each(CC.WGRAD_DMA, lambda case: run_wgrad_case(env, case, math_mode))


def test_filter_gradient_register_staged(env):
    each(CC.WGRAD_PLAIN, lambda case: run_wgrad_case(env, case))


# ---- fused filter gradient --------------------------------------------------------------------------------------------------------------------
def run_fused_case(env, case, seed=13):
    _C, D, cus = env
    call, ref = call_for(env, case.shape, seed, case.offset)
    want = case.route(cus)
    if not case.cus_dependent:
        assert want == case.route(256), f'{case.id}: the route depends on the CU count and the case does not say so'
    g, dw, db, report = call.bwd_w_relu(case.knobs)
    assert report == want, f'{case.id}: ran {report!r}, not {want!r}'
    want_g = np.where(call.pre >= 0, call.dy, np.float32(0)).astype(np.float32)
    assert np.array_equal(CC.bits(g), CC.bits(want_g)), f'{case.id}: g is not where(pre >= 0, dy, 0)'
    g64 = want_g.astype(np.float64)
    assert_close(db, g64.reshape(-1, case.c1).sum(axis=0), tol=TOL, what=case.id + ' db')
    assert_close(dw, ref['dw'](g64), tol=TOL_DW, what=case.id + ' dw')
    return g, dw, db


@pytest.mark.parametrize('geometry', FUSED_CLASSES)
def test_fused_filter_gradient(env, geometry):
    each([c for c in CC.FUSED if c.cell == geometry], lambda case: run_fused_case(env, case))


def test_fused_filter_gradient_falls_back(env):
    def run(case):
        assert case.route(env[2]).startswith('two_pass ')
        run_fused_case(env, case)

    each(CC.FUSED_FALLBACK, run)


def test_small_rendezvous_changes_nothing(env):
    """The K rendezvous at 2^14 pixels (every == 2 and 4 against off): engaged on this device, dw, db and g bit-equal."""
    _C, D, cus = env
    shape = CC.RENDEZVOUS_SHAPE
    runs = {}
    for every in CC.RENDEZVOUS_KSYNC:
        case = CC.FusedCase('rendezvous', *shape, CC.Knobs(fused=3, ksync=every), cus_dependent=True)
        assert CC.fields(case.route(cus))['ksync'] == every, f'the rendezvous does not engage at {cus} CUs'
        runs[every] = run_fused_case(env, case)
    for every in CC.RENDEZVOUS_KSYNC[1:]:
        for name, got, want in zip(('g', 'dw', 'db'), runs[every], runs[0]):
            assert np.array_equal(CC.bits(got), CC.bits(want)), f'{name} with the rendezvous every {every} K tiles'


# ---- empty and refused calls ----------------------------------------------------------------------------------------------------------------
def test_empty_calls(env):
    _C, D, _ = env
    lib = _C.lib()
    call, _ = call_for(env, (2, 5, 17, 4, 8, 3), 14)
    call.fwd()                                                                     # something else than 'none' is the last report
    assert _C.last_conv_kernel() != 'none'
    y = CC.Output(D, (4, 8))
    desc = _C.npm_conv2d(n=0, h=5, w=17, c_in=4, c_out=8, ksize=3, x=None, filt=None, bias=None, y=y.ptr, pre=None, relu=1)
    _C.check(lib.npm_conv2d_fwd(C.byref(desc)))
    assert _C.last_conv_kernel() == 'none'
    y.read('y of n == 0', written=False)
    call.fwd()
    dx = CC.Output(D, (4, 8))
    _C.check(lib.npm_conv2d_bwd_x(None, None, dx.ptr, 0, 5, 17, 4, 8, 3))
    assert _C.last_conv_kernel() == 'none'
    dx.read('dx of n == 0', written=False)
    call.fwd()
    dw = CC.Output(D, (3, 3, 4, 8))
    _C.check(lib.npm_conv2d_bwd_w(None, None, dw.ptr, 0, 5, 17, 4, 8, 3))
    assert _C.last_conv_kernel() == 'none'
    assert np.array_equal(CC.bits(dw.read('dw of no pixels')), np.zeros((3, 3, 4, 8), dtype=np.uint32))
    call.fwd()
    dw, db, g = CC.Output(D, (3, 3, 4, 8)), CC.Output(D, (8,)), CC.Output(D, (4, 8))
    _C.check(lib.npm_conv2d_bwd_w_relu(None, None, None, g.ptr, dw.ptr, db.ptr, 0, 5, 17, 4, 8, 3))
    assert _C.last_conv_kernel() == 'none'
    assert not CC.bits(dw.read('dw of no pixels')).any() and not CC.bits(db.read('db of no pixels')).any()
    g.read('g of no pixels', written=False)


def test_bad_arguments_launch_nothing(env):
    _C, D, _ = env
    lib = _C.lib()
    shape = n, h, w, c0, c1, k = (2, 5, 17, 4, 8, 3)
    call, _ = call_for(env, shape, 14)
    call.fwd()
    before = _C.last_conv_kernel()
    outs = dict(y=CC.Output(D, (n, h, w, c1)), dx=CC.Output(D, (n, h, w, c0)), dw=CC.Output(D, (k, k, c0, c1)), db=CC.Output(D, (c1,)),
                g=CC.Output(D, (n, h, w, c1)))
    x, dy, pre, filt = call.d_x.ptr, call.d_dy.ptr, call.d_pre.ptr, call.d_filt.ptr

    def fwd(**change):
        fields = dict(n=n, h=h, w=w, c_in=c0, c_out=c1, ksize=k, x=x, filt=filt, bias=None, y=outs['y'].ptr, pre=None, relu=0)
        fields.update(change)
        return lib.npm_conv2d_fwd(C.byref(_C.npm_conv2d(**fields)))

    def dims(**change):
        d = dict(n=n, h=h, w=w, c_in=c0, c_out=c1, ksize=k)
        d.update(change)
        return [d[key] for key in ('n', 'h', 'w', 'c_in', 'c_out', 'ksize')]

    refused = [
        ('npm_conv2d_fwd', lambda: fwd(ksize=2)), ('npm_conv2d_fwd', lambda: fwd(h=0)), ('npm_conv2d_fwd', lambda: fwd(c_in=0)),
        ('npm_conv2d_fwd', lambda: fwd(x=None)), ('npm_conv2d_fwd', lambda: fwd(filt=None)), ('npm_conv2d_fwd', lambda: fwd(y=None)),
        ('npm_conv2d_fwd', lambda: lib.npm_conv2d_fwd(None)),
        ('npm_conv2d_bwd_x', lambda: lib.npm_conv2d_bwd_x(dy, filt, outs['dx'].ptr, *dims(ksize=4))),
        ('npm_conv2d_bwd_x', lambda: lib.npm_conv2d_bwd_x(dy, filt, outs['dx'].ptr, *dims(h=0))),
        ('npm_conv2d_bwd_x', lambda: lib.npm_conv2d_bwd_x(dy, filt, outs['dx'].ptr, *dims(c_in=0))),
        ('npm_conv2d_bwd_x', lambda: lib.npm_conv2d_bwd_x(None, filt, outs['dx'].ptr, *dims())),
        ('npm_conv2d_bwd_x', lambda: lib.npm_conv2d_bwd_x(dy, None, outs['dx'].ptr, *dims())),
        ('npm_conv2d_bwd_x', lambda: lib.npm_conv2d_bwd_x(dy, filt, None, *dims())),
        ('npm_conv2d_bwd_w', lambda: lib.npm_conv2d_bwd_w(dy, x, outs['dw'].ptr, *dims(ksize=2))),
        ('npm_conv2d_bwd_w', lambda: lib.npm_conv2d_bwd_w(dy, x, outs['dw'].ptr, *dims(h=0))),
        ('npm_conv2d_bwd_w', lambda: lib.npm_conv2d_bwd_w(dy, x, outs['dw'].ptr, *dims(c_in=0))),
        ('npm_conv2d_bwd_w', lambda: lib.npm_conv2d_bwd_w(dy, x, None, *dims())),
        ('npm_conv2d_bwd_w', lambda: lib.npm_conv2d_bwd_w(None, x, outs['dw'].ptr, *dims())),
        ('npm_conv2d_bwd_w', lambda: lib.npm_conv2d_bwd_w(dy, None, outs['dw'].ptr, *dims())),
        ('npm_conv2d_bwd_w_relu', lambda: lib.npm_conv2d_bwd_w_relu(dy, pre, x, outs['g'].ptr, outs['dw'].ptr, outs['db'].ptr, *dims(ksize=2))),
        ('npm_conv2d_bwd_w_relu', lambda: lib.npm_conv2d_bwd_w_relu(dy, pre, x, outs['g'].ptr, outs['dw'].ptr, outs['db'].ptr, *dims(h=0))),
        ('npm_conv2d_bwd_w_relu', lambda: lib.npm_conv2d_bwd_w_relu(dy, pre, x, outs['g'].ptr, outs['dw'].ptr, outs['db'].ptr, *dims(c_in=0))),
        ('npm_conv2d_bwd_w_relu', lambda: lib.npm_conv2d_bwd_w_relu(dy, pre, x, outs['g'].ptr, None, outs['db'].ptr, *dims())),
        ('npm_conv2d_bwd_w_relu', lambda: lib.npm_conv2d_bwd_w_relu(dy, pre, x, outs['g'].ptr, outs['dw'].ptr, None, *dims())),
        ('npm_conv2d_bwd_w_relu', lambda: lib.npm_conv2d_bwd_w_relu(dy, None, x, outs['g'].ptr, outs['dw'].ptr, outs['db'].ptr, *dims())),
        ('npm_conv2d_bwd_w_relu', lambda: lib.npm_conv2d_bwd_w_relu(dy, pre, x, None, outs['dw'].ptr, outs['db'].ptr, *dims())),
    ]
    for i, (entry, attempt) in enumerate(refused):
        assert attempt() == CC.E_BAD_ARGUMENT, (i, entry)
        message = lib.npm_last_error().decode()
        assert message.startswith(entry + ': bad argument'), (i, message)
        assert _C.last_conv_kernel() == before, (i, entry)                 # nothing chose a kernel
    D.synchronize()
    for name, out in outs.items():
        out.read(name + ' of refused calls', written=False)                   # and nothing was written
