"""CPU: the optimizer, loss and dropout entry points (csrc/npm_optim.hip) without a GPU.

* the cases of tests/optim_cases.py on the simulator of tests/hostsim/, so that every check of tests/test_gpu_optim.py has run
  (and its near-tie count has been asserted for every Adam case) before a GPU sees it;
* the Adam model of tests/optim_reference.py against the reference's own ``AdamOptimizer`` (where a checkout of the reference is at
  hand) and against the arrays recorded from it (tests/golden/adam_steps.npz);
* the checks themselves: five wrong Adam models, a float32 loss accumulator and a Philox with the offset's halves exchanged each fail;
* ``UpdateQueue`` keeps an Adam update's moment buffers alive when the update was enqueued through a drain.
"""

import ctypes
import gc
import importlib.util
import os
import weakref

import numpy as np
import pytest

from hostsim.fixtures import npm_fixture
import optim_cases as OC
import optim_reference as R
from conftest import load_golden
from oracle import np_oracle as O


npm = npm_fixture('training')


# ---- the same cases as on the GPU ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', OC.ADAM_CASES, ids=OC.adam_case_id)
def test_adam_cases(npm, case):
    used = OC.check_adam_case(npm, case)
    print('near ties (step, in the case, differing):', used)
    assert all(differing == 0 for _, _, differing in used)               # the simulator divides and roots as the model does


def test_near_tie_counts_at_the_largest_size():
    """Seed 20, n = 2^20 + 257: the model alone exempts a handful of elements per step (the cap is 16)."""
    case = OC.ADAM_CASES[8]
    assert case[0] == OC.EW_SEAM + 257
    used = OC.check_adam_case(None, case, stepper=lambda p, g, m, v, step, hyper: R.adam_model(p, g, m, v, step, hyper)[:3])
    print('near ties (step, in the case, differing):', used)
    assert all(exempt <= R.MAX_EXEMPT for _, exempt, _ in used)


def test_adam_golden_fixture_on_the_simulator(npm):
    OC.check_adam_golden(npm, load_golden('adam_steps'))


def test_adam_optimizer_class(npm):
    OC.check_adam_optimizer_class(npm)


def test_encoder_adam_coalesced_equals_per_parameter(npm):
    OC.check_encoder_adam_coalesced(npm)


@pytest.mark.parametrize('case', OC.LOSS_CASES, ids=lambda c: f'n{c[0]}-off{c[1][0]}{c[1][1]}')
def test_loss_sums(npm, case):
    print('error / bound:', OC.check_loss_sums(npm, case))


@pytest.mark.parametrize('case', OC.BWD_CASES, ids=lambda c: f'n{c[0]}-off{"".join(map(str, c[1]))}')
def test_loss_gradients(npm, case):
    OC.check_loss_gradients(npm, case)


def test_mask_scale(npm):
    for case in OC.MASK_SCALE_CASES:
        OC.check_mask_scale(npm, case)


def test_dropout_philox_grid(npm):
    grid = OC.philox_grid()
    assert len(grid) == 4 * 4 * 6 * 4 + 12
    for case in grid:
        OC.check_philox_case(npm, case)
    OC.check_philox_offsets_differ(npm)


def test_fill_f64_and_argument_checks(npm):
    OC.check_fill_f64(npm)
    OC.check_arguments(npm)


# ---- the model against the reference --------------------------------------------------------------------------------------------------
def _reference_optimizer():
    from oracle.make_golden import REFERENCE
    path = os.path.join(REFERENCE, 'optimizer.py')
    if not os.path.isfile(path):
        pytest.skip('no checkout of the reference here (NPM_REFERENCE)')
    spec = importlib.util.spec_from_file_location('_reference_optimizer', path)
    module = importlib.util.module_from_spec(spec)
    import sys
    sys.modules[spec.name] = module                      # dataclasses looks the module up by name
    try:
        spec.loader.exec_module(module)
    finally:
        sys.modules.pop(spec.name, None)
    return module


@pytest.mark.parametrize('hyper', [R.DEFAULT_HYPER, R.OTHER_HYPER])
def test_model_is_the_references_adam_bit_for_bit(hyper):
    """Parameters and both moments, three steps at n = 2^20 + 257, moments re-synchronised every step."""
    ref = _reference_optimizer().AdamOptimizer(*hyper)
    n = OC.EW_SEAM + 257
    rng = np.random.default_rng(OC.ADAM_SEED)
    p = rng.standard_normal(n).astype(np.float32)
    m, v = np.zeros(n), np.zeros(n)
    for step in (1, 2, 3):
        g = R.adam_gradient(rng, n)
        want = R.adam_model(p, g, m, v, step, hyper)
        with np.errstate(all='ignore'):
            got = ref.update_variable('p', p.copy(), g)
        assert got.dtype == np.float32
        assert np.array_equal(R.bits(got), R.bits(want.p))
        assert np.array_equal(R.bits(ref._momentums['p']), R.bits(want.m)) and np.array_equal(R.bits(ref._velocities['p']), R.bits(want.v))
        p, m, v = want.p, want.m, want.v


def test_model_and_oracle_equal_the_recorded_reference_steps():
    """tests/golden/adam_steps.npz was written by the reference's class: the model, ``O.adam_step`` and the package's host path
    (``AdamOptimizer._step_on_host``) each reproduce it bit for bit."""
    import np_modeling_amd
    g = load_golden('adam_steps')
    hyper = tuple(float(h) for h in g['hyper'])
    n = g['p0'].size
    p, m, v, state = g['p0'], np.zeros(n), np.zeros(n), {}
    host, mine = g['p0'].copy(), np_modeling_amd.optimizer.AdamOptimizer(*hyper)
    for step in (1, 2, 3):
        want = R.adam_model(p, g[f'g{step}'], m, v, step, hyper)
        for name, got in (('p', want.p), ('m', want.m), ('v', want.v)):
            assert np.array_equal(R.bits(got), R.bits(g[f'{name}{step}'])), (name, step)
        with np.errstate(all='ignore'):
            oracle = O.adam_step(p, g[f'g{step}'], state, hyper[0], *hyper[1:])
            host = mine.update_variable('p', host, g[f'g{step}'])
        assert np.array_equal(R.bits(oracle), R.bits(want.p)) and np.array_equal(R.bits(state['m']), R.bits(want.m))
        assert np.array_equal(R.bits(host), R.bits(want.p))
        p, m, v = want.p, want.m, want.v


def test_inplace_f32_minus_f64_rounds_once():
    """What the model's single rounding stands on: NumPy's ``f32 -= f64`` is (f64(p) - s) rounded to float32."""
    rng = np.random.default_rng(0)
    p, s = rng.standard_normal(100000).astype(np.float32), rng.standard_normal(100000) * 1e-2
    q = p.copy()
    q -= s
    assert np.array_equal(R.bits(q), R.bits((p.astype(np.float64) - s).astype(np.float32)))


# ---- wrong models must fail -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('variant', ['round_step', 'eps_outside', 'f32_moments', 'step_minus_1', 'f64_products'])
def test_a_wrong_adam_model_fails_the_check(variant):
    """On the largest case and on the one below the seam; the near-tie rule does not excuse any of them."""
    def stepper(p, g, m, v, step, hyper):
        return R.adam_model(p, g, m, v, step, hyper, variant=variant)[:3]

    for case in (OC.ADAM_CASES[8], OC.ADAM_CASES[5]):
        with pytest.raises(AssertionError, match='moment differs|no near ties|more than one ulp'):
            OC.check_adam_case(None, case, stepper=stepper)


def test_a_float32_accumulator_fails_the_sum_bound():
    case = OC.LOSS_CASES[8]
    assert case[0] == OC.SUM_SEAM + 257
    with pytest.raises(AssertionError, match='mse'):
        OC.check_loss_sums(None, case, mse=R.pairwise_f32_sum, xent=lambda terms: float(terms.sum()))
    with pytest.raises(AssertionError, match='xent'):
        OC.check_loss_sums(None, case, mse=lambda terms: float(terms.sum()), xent=R.pairwise_f32_sum)
    OC.check_loss_sums(None, case, mse=lambda terms: float(terms.sum()), xent=lambda terms: float(terms.sum()))


def test_philox_with_the_offset_halves_exchanged_fails(npm):
    def swapped(n, keep, seed, offset):
        return R.dropout_philox_mask_range(0, n, keep, seed, offset, swap_offset_halves=True)

    case = (1027, 0, 0, 0, 0.75, OC.SEEDS[0], 2 ** 32)
    OC.check_philox_case(npm, case)
    with pytest.raises(AssertionError):
        OC.check_philox_case(npm, case, mask_model=swapped)
    OC.check_philox_case(npm, case[:6] + (0,), mask_model=swapped)           # offset 0: both halves are 0, nothing to tell apart


def test_ranged_philox_equals_the_whole_mask():
    for keep, seed, offset in ((0.75, OC.SEEDS[0], 2 ** 63 + 5), (0.1, OC.SEEDS[1], 2 ** 32 - 1)):
        whole = O.dropout_philox_mask(5003, keep, seed, offset)
        for first, count in ((0, 5003), (0, 1), (1024, 2048), (4096, 907), (5000, 3)):
            assert np.array_equal(R.dropout_philox_mask_range(first, count, keep, seed, offset), whole[first:first + count])
    assert R.philox_threshold(1.0) == 2 ** 32 and R.philox_threshold(2.0 ** -33) == 0 and R.philox_threshold(0.75) == 3 * 2 ** 30


def test_mse_gradient_model_is_within_two_ulp_of_float64():
    """float32(2 / n) * (y - t) -- three roundings -- against 2 (y - t) / n in float64, in ulps of the float32 result."""
    for n in (3, 997, 1023, OC.EW_SEAM + 257):
        rng = np.random.default_rng(n + 1)
        y, t = rng.standard_normal(n).astype(np.float32), rng.standard_normal(n).astype(np.float32)
        model = np.float32(2.0 / n) * (y - t)
        exact = 2.0 * (y.astype(np.float64) - t.astype(np.float64)) / n
        ulp = np.spacing(np.abs(exact).astype(np.float32)).astype(np.float64)
        used = float((np.abs(model.astype(np.float64) - exact) / ulp).max())
        print(f'n={n}: {used:.2f} ulp')
        assert used <= 2.0


# ---- UpdateQueue keeps the moments of an update that was enqueued through a drain ---------------------------------------------------------
def test_queue_keeps_moment_buffers_of_an_update_enqueued_through_a_drain(npm, monkeypatch):
    """Two Adam updates of one parameter inside ``coalesced_updates()``: the second overlaps the pending first, so ``_enqueue``
    drains -- and ``run()`` ends with ``_keep = []``.  The optimizer is then dropped before the scope exits: the queue alone must
    keep the moment buffers of the still-pending second update alive."""
    D = npm.device
    monkeypatch.setattr(D, 'COALESCE_UPDATES', True)
    n = 300
    rng = np.random.default_rng(7)
    p0 = rng.standard_normal(n).astype(np.float32)
    g1, g2 = R.adam_gradient(rng, n), R.adam_gradient(rng, n)
    holder = type('Holder', (), {})()
    holder._w = var = npm.as_device(p0)
    d1, d2 = npm.as_device(g1), npm.as_device(g2)         # uploaded first: a library call between the two updates would drain by itself
    with D.coalesced_updates() as queue:
        adam = npm.optimizer.AdamOptimizer(*R.DEFAULT_HYPER)
        adam.update(holder, '_w', d1)
        assert queue.drains == 0 and len(queue._pending) == 1
        adam.update(holder, '_w', d2)
        assert queue.drains == 1 and queue.launches == 1 and len(queue._pending) == 1       # drained inside _enqueue
        (_, moments), = adam._state.values()
        owner = weakref.ref(moments.owner)
        first_ptr, second_ptr = moments.first_ptr, moments.second_ptr
        del adam, moments
        gc.collect()
        assert owner() is not None, 'the pending update holds its moment buffers by raw pointer only'
        read = lambda ptr: np.ctypeslib.as_array((ctypes.c_double * n).from_address(ptr)).copy()
        m1, v1 = read(first_ptr), read(second_ptr)                     # after step 1 (the drain ran it), before step 2
    one = R.adam_model(p0, g1, np.zeros(n), np.zeros(n), 1)
    assert np.array_equal(R.bits(m1), R.bits(one.m)) and np.array_equal(R.bits(v1), R.bits(one.v))
    two = R.adam_model(one.p, g2, one.m, one.v, 2)
    assert np.array_equal(R.bits(var.numpy()), R.bits(two.p))
    assert queue.launches == 2 and queue.updates == 2
    gc.collect()
    assert owner() is None                                             # and lets go of them afterwards
