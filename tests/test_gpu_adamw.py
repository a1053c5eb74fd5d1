"""GPU: npm_sumsq_ranges, npm_clip_finish, npm_adamw_step (csrc/npm_clip.hip) and ``optimizer.AdamWOptimizer`` on a small
``CausalLM``, on the cases of tests/adamw_cases.py -- the ones tests/test_adamw_host.py runs on the simulator.

Bounds (tests/adamw_reference.py; nothing in them is measured):

* the sum of squares against ``math.fsum`` of the exact fp64 squares: |got - exact| <= N 2^-53 exact, N the number of elements.
  The squares are exact and every partial sum of non-negative terms is at most the total, so this holds for any order of fp64
  additions; a float32 accumulator or a float32 square misses it by orders of magnitude (shown in the host file);
* the clip factor against the header's expression in NumPy: bit for bit;
* the step against the NumPy model: both moments bit for bit, the parameter bit for bit except at near ties of its one final
  rounding (one float32 ulp; at most 16 a case, counted from the model alone and asserted in the host file for every case).

Every test here needs the three entry points and the class: none passes on the parent commit."""

import numpy as np
import pytest

import adamw_cases as AC
import adamw_reference as AR

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def npm():
    import np_modeling_amd
    return np_modeling_amd


@pytest.mark.parametrize('kind', AC.SUMSQ_DATA)
def test_sumsq_one_range(npm, kind):
    print('worst error / bound:', AC.check_sumsq_single(npm, kind))


def test_sumsq_tables_and_arguments(npm):
    print('error / bound:', AC.check_sumsq_tables(npm))
    AC.check_sumsq_arguments(npm)


def test_thirty_three_ranges_through_the_optimizer(npm):
    class Holder:
        pass
    rng = np.random.default_rng(3)
    holders, grads = [], []
    for i in range(33):
        h = Holder()
        h._w = npm.device.zeros([5 + i])
        holders.append(h)
        grads.append(rng.standard_normal(5 + i).astype(np.float32))
    opt = npm.optimizer.AdamWOptimizer(1e-3, clip_norm=1.0)
    for h, g in zip(holders, grads):
        opt.update(h, '_w', npm.device.from_host(g))
    opt.apply()
    assert opt.last['ranges'] == 33                     # two launches of the sum: 32 ranges and 1
    print('error / bound:', AR.sumsq_check(float(AC.clip_state(opt)[0]), grads, '33 ranges'))
    norm, scale, ok = opt.last_grad_norm()
    assert ok and scale < 1.0 and all(np.asarray(h._w).any() for h in holders)


def test_clip_finish(npm):
    AC.check_clip_finish(npm)


@pytest.mark.parametrize('case', AC.STEP_CASES, ids=AC.step_case_id)
def test_step_cases(npm, case):
    used = AC.check_step_case(npm, case)
    print('near ties (step, in the case, differing):', used)


def test_step_arguments(npm):
    AC.check_step_arguments(npm)


def test_class_on_a_model(npm):
    print(AC.check_class_on_model(npm))


def test_coalesced_equals_per_parameter(npm):
    AC.check_coalesced_equals_per_parameter(npm)


def test_a_non_finite_norm_skips_the_step(npm):
    AC.check_non_finite_step_is_skipped(npm)
