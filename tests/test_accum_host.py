"""CPU: gradient accumulation without a GPU.  The cases of tests/accum_cases.py run on tests/accum_sim.py -- the host simulator with
the two entry points of csrc/npm_accum.hip restated beside it -- so that every check of tests/test_gpu_accum.py has run, and the
near-tie counts of the model fixture have been asserted from the model alone, before a GPU sees it; where noted also on the plain
simulator, which has neither entry point: ``fold()`` then takes the npm_axpy route.

Host only: the call lists (``accumulate=True`` with one backward per ``apply()`` makes exactly the calls of ``accumulate=False``;
``Trainer.train(..., micro_batches=1)`` makes the recorded calls of tests/golden/trainer_sgd_calls.json), the order of all-reduce,
wait and fold under a recording communicator, the binding, and the code-object metadata of npm_accum.o."""

import ctypes
import json
import os

import numpy as np
import pytest

import accum_cases as XC
import accum_sim
import adamw_cases as AC
import lm_cases as MC
from hostsim.fixtures import activate, built, deactivate  # noqa: F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture
def npm():
    """The package on an ``AccumSim``: both entry points present."""
    import np_modeling_amd
    from np_modeling_amd import parallel
    np_modeling_amd.sim = accum_sim.install()
    parallel.set_communicator(None)
    yield np_modeling_amd
    deactivate()


@pytest.fixture
def plain():
    """The package on the plain simulator: a library of before this feature."""
    package = activate()
    sim = package.sim  # noqa: F841
    yield package
    deactivate()


# ---- the kernels' cases ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind', XC.DATA)
def test_fold_every_length_and_phase(npm, kind):
    assert XC.check_fold_single(npm, kind) == len(XC.LENGTHS) * 16


def test_fold_tables_count_zero_and_split(npm):
    XC.check_fold_tables(npm)
    XC.check_fold_split_32_plus_1(npm)


def test_fold_refusals(npm):
    XC.check_fold_refusals(npm)


def test_clip_finish_scaled(npm):
    XC.check_clip_finish_scaled(npm)


def test_clip_finish_scaled_refusals(npm):
    XC.check_clip_finish_scaled_refusals(npm)


# ---- the class and the trainer -----------------------------------------------------------------------------------------------------------
def _calls_of_a_run(package, accumulate):
    lm = MC.make_lm(package)
    opt = XC.holding(package, XC.LR, weight_decay=XC.WEIGHT_DECAY, clip_norm=0.05, accumulate=accumulate)
    start = len(package.sim.calls)
    AC.train(package, lm, opt, 2)
    return package.sim.calls[start:]


@pytest.mark.parametrize('library', ['npm', 'plain'])
def test_accumulate_with_one_backward_per_apply_is_the_plain_optimizer(request, library):
    package = request.getfixturevalue(library)
    XC.check_accumulate_with_one_backward_equals_plain(package)
    plain_calls, accumulating_calls = _calls_of_a_run(package, False), _calls_of_a_run(package, True)
    assert plain_calls == accumulating_calls and 'npm_adamw_step' in plain_calls
    assert not {'npm_accumulate_ranges', 'npm_clip_finish_scaled', 'npm_axpy'} & set(accumulating_calls)


def test_trainer_with_one_micro_batch_makes_the_recorded_calls(npm):
    with open(os.path.join(ROOT, 'tests', 'golden', 'trainer_sgd_calls.json')) as f:
        recorded = json.load(f)['calls']
    lm = MC.make_lm(npm)
    _, inputs, targets = MC.tokens()
    start = len(npm.sim.calls)
    import contextlib
    import io
    with contextlib.redirect_stdout(io.StringIO()):
        npm.train.Trainer([lm], npm.loss.SoftmaxCrossEntropyLoss()).train(inputs, targets, 2, npm.optimizer.SGDOptimizer(0.02), micro_batches=1)
    assert npm.sim.calls[start:] == recorded and len(recorded) > 100


@pytest.mark.parametrize('library', ['npm', 'plain'])
def test_three_micro_batches_against_the_models(request, library):
    """Near ties are counted from the model alone (``adamw_check`` asserts the cap, AR.MAX_EXEMPT, per parameter): the simulator's
    step IS the model, so no parameter may differ."""
    package = request.getfixturevalue(library)
    if library == 'plain':                               # no npm_clip_finish_scaled in that library: the error names it
        with pytest.raises(package._C.NpmError, match='npm_clip_finish_scaled'):
            XC.check_three_micro_batches(package)
        return
    out = XC.check_three_micro_batches(package)
    out.pop('snapshot')
    print(out)
    assert out['differing'] == 0 and out['norm error / bound'] <= 1.0


def test_switches_agree_and_last_follows_them(npm):
    lasts = XC.check_switches_agree(npm)
    print(lasts)
    for (fused, ranges), last in lasts.items():
        assert last['fused_norm'] == (fused and ranges) and last['folds'] == XC.K - 1
    calls = npm.sim.calls
    assert 'npm_axpy' in calls and 'npm_accumulate_ranges' in calls and 'npm_clip_finish_scaled' in calls


def test_the_calls_of_an_accumulated_step(npm):
    """Fused: the fold of micro-batch 2, the fold of micro-batch 3 with the sum, the scaled finish, the steps -- and no
    npm_sumsq_ranges.  Not fused: both folds without the sum, then the calls of a plain step with npm_clip_finish_scaled in
    npm_clip_finish's place; the table of the sum is the last fold's dst table."""
    from np_modeling_amd import device as D
    saved = D.ACCUM_FUSED_NORM
    try:
        for fused in (True, False):
            D.ACCUM_FUSED_NORM = fused
            lm = MC.make_lm(npm)
            opt = XC.holding(npm, XC.LR, clip_norm=1.0, accumulate=True)
            start, tables = len(npm.sim.calls), len(npm.sim.accum_tables)
            XC.train(npm, lm, opt, 1, micro_batches=XC.K)
            calls = [c for c in npm.sim.calls[start:] if c in ('npm_accumulate_ranges', 'npm_sumsq_ranges', 'npm_clip_finish',
                                                               'npm_clip_finish_scaled', 'npm_adamw_step', 'npm_axpy')]
            steps = opt.last['launches']
            middle = [] if fused else ['npm_sumsq_ranges']
            assert calls == ['npm_accumulate_ranges'] * 2 + middle + ['npm_clip_finish_scaled'] + ['npm_adamw_step'] * steps, calls
            summed = [with_sum for _, with_sum in npm.sim.accum_tables[tables:]]
            assert summed == [False, fused]
            # the fused fold's dst table is the table of the norm
            if not fused:
                pairs = npm.sim.accum_tables[-1][0]
                assert [(d, n) for d, _, n in pairs] == [tuple(p) for p in npm.sim.sumsq_tables[-1]]
    finally:
        D.ACCUM_FUSED_NORM = saved


def test_against_the_full_batch_in_float64(npm):
    print('worst error / bound:', XC.check_against_the_full_batch_in_float64(npm))


@pytest.mark.parametrize('library', ['npm', 'plain'])
def test_a_second_update_folds_first_and_the_plain_optimizer_still_raises(request, library):
    package = request.getfixturevalue(library)
    if library == 'plain':
        with pytest.raises(package._C.NpmError, match='npm_clip_finish_scaled'):
            XC.check_second_update_folds_first_and_plain_still_raises(package)
        assert package.sim.calls.count('npm_axpy') == 2          # the folds took the yardstick route
        return
    XC.check_second_update_folds_first_and_plain_still_raises(package)


def test_thirty_three_pairs_take_two_launches(npm):
    from np_modeling_amd import device as D
    saved = D.ACCUM_FUSED_NORM
    try:
        for fused in (True, False):
            D.ACCUM_FUSED_NORM = fused
            tables = len(npm.sim.accum_tables)
            last = XC.check_thirty_three_pairs_through_the_optimizer(npm)
            assert last['fold_launches'] == 2 and last['fused_norm'] == fused
            assert [(len(p), s) for p, s in npm.sim.accum_tables[tables:]] == [(32, fused), (1, fused)]
    finally:
        D.ACCUM_FUSED_NORM = saved


def test_a_scale_without_clipping(npm):
    XC.check_unclipped_scale(npm)
    assert npm.sim.calls.count('npm_clip_finish_scaled') == 1 and 'npm_clip_finish' not in npm.sim.calls


def test_trainer_refusals(npm):
    XC.check_trainer_refusals(npm)


def test_the_printed_loss_is_the_token_mean_of_the_batch(npm):
    XC.check_printed_loss_is_the_token_mean(npm)


def test_views_are_made_once_and_nothing_goes_through_the_host(npm):
    """Micro-batch views are made once per ``train`` call: the loss counts each view's targets once (one copy of 4 bytes per row),
    not once per step."""
    lm = MC.make_lm(npm)
    opt = npm.optimizer.AdamWOptimizer(1e-3, accumulate=True)
    d2h = len(npm.sim.d2h)
    steps = 3
    XC.train(npm, lm, opt, steps, micro_batches=XC.K)
    # (the embedding's backward sorts its ids on the host, once per backward, with or without micro-batches: steps x K copies)
    assert npm.sim.d2h[d2h:] == [4 * MC.S] * (XC.K + steps * XC.K), npm.sim.d2h[d2h:]


def test_a_mean_loss_without_a_count_uses_one_over_k(npm):
    np.random.seed(2)
    dense = npm.layers.Linear(units=5)
    x, t = np.random.standard_normal([4, 3]).astype(np.float32), np.random.standard_normal([4, 5]).astype(np.float32)
    seen = []

    class Spy(npm.optimizer.AdamWOptimizer):
        def apply(self, grad_scale=1.0):
            seen.append(grad_scale)
            super().apply(grad_scale=grad_scale)
    import contextlib
    import io
    with contextlib.redirect_stdout(io.StringIO()):
        npm.train.Trainer([dense]).train(x, t, 2, Spy(1e-3, accumulate=True), micro_batches=2)
    assert seen == [0.5, 0.5]


class RecordingComm:
    """A communicator whose ``active`` is true and which only records: one rank, nothing to add."""
    active = True
    rank, size = 0, 1

    def __init__(self, sim):
        self.sim = sim

    def allreduce_async(self, flat, op):
        self.sim.calls.append('allreduce')

    def wait(self):
        self.sim.calls.append('comm_wait')

    def allreduce_scalar(self, value, op):
        return value

    def barrier(self):
        pass


def test_every_all_reduce_and_wait_of_a_micro_batch_precedes_its_fold(npm):
    from np_modeling_amd import parallel
    lm = MC.make_lm(npm)
    parallel.set_communicator(RecordingComm(npm.sim))
    opt = npm.optimizer.AdamWOptimizer(1e-2, clip_norm=1.0, accumulate=True)
    start = len(npm.sim.calls)
    XC.train(npm, lm, opt, 1, micro_batches=XC.K)
    calls = [c for c in npm.sim.calls[start:] if c in ('allreduce', 'comm_wait', 'npm_accumulate_ranges')]
    folds = [i for i, c in enumerate(calls) if c == 'npm_accumulate_ranges']
    assert len(folds) == XC.K - 1
    reduces, waits = calls.count('allreduce') // XC.K, calls.count('comm_wait') // XC.K      # per micro-batch: one scope per layer
    assert reduces >= 1 and waits >= 1 and calls.count('allreduce') == reduces * XC.K and calls.count('comm_wait') == waits * XC.K
    # micro-batch 1 is adopted; the fold of micro-batch j (j = 2 .. K) comes after all of j's exchange and before any of j + 1's
    for index, at in enumerate(folds):
        j = index + 2
        assert calls[:at].count('allreduce') == j * reduces and calls[:at].count('comm_wait') == j * waits, (j, calls)


# ---- the binding and the object ------------------------------------------------------------------------------------------------------------
def test_the_entry_points_are_declared_and_bound_outside_the_simulator():
    from np_modeling_amd import _C
    import hostsim
    P, D = ctypes.c_void_p, ctypes.c_double
    T = ctypes.POINTER(_C.npm_ranges)
    assert _C._SPECIAL['npm_accumulate_ranges'] == (ctypes.c_int, [T, T, P])
    assert _C._SPECIAL['npm_clip_finish_scaled'] == (ctypes.c_int, [P, D, D])
    assert not {'npm_accumulate_ranges', 'npm_clip_finish_scaled'} & set(_C.SIGNATURES)
    assert not hasattr(hostsim.HostSim(), 'npm_accumulate_ranges') and not isinstance(accum_sim.AccumSim(), hostsim.HostSim)
    header = open(os.path.join(ROOT, 'include', 'npm_hip.h')).read()
    assert 'int npm_accumulate_ranges(const npm_ranges *dst, const npm_ranges *src, double *sumsq_acc);' in header
    assert 'int npm_clip_finish_scaled(double *state, double max_norm, double grad_scale);' in header
    assert '#define NPM_ABI_VERSION 2 ' in header


def test_the_library_exports_them(built):
    lib = built.load_library()
    assert lib.npm_accumulate_ranges.restype is ctypes.c_int and lib.npm_clip_finish_scaled.restype is ctypes.c_int


def test_the_new_kernels_spill_nothing(built):
    """Code-object metadata of the gfx950 kernels of csrc/npm_accum.hip (tools/kernel_meta.py): no spill, no scratch -- the table of
    pairs is a kernel argument indexed at run time, which must stay scalar loads -- and no LDS in the fold without a sum."""
    import sys
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import kernel_meta
    meta = kernel_meta.kernel_metadata(os.path.join(os.path.dirname(built.LIB_PATH), 'npm_accum.o'))
    assert len(meta) == 4 and all(any(tag in name for name in meta) for tag in ('accum_tiles', 'accum_finish', 'clip_finish_scaled'))
    for name, m in meta.items():
        assert m['.vgpr_spill_count'] == 0 and m['.sgpr_spill_count'] == 0 and m['.private_segment_fixed_size'] == 0, (name, m)
        if 'accum_tiles_kernel<false>' in name.replace(' ', '') or 'ILb0E' in name:
            assert m['.group_segment_fixed_size'] == 0, (name, m)


def test_a_single_pair_without_the_sum_takes_the_yardstick_unless_forced(npm):
    """The one shape the bench measured slower than npm_axpy (README): with ``device.ACCUM_RANGES`` unset a fold of ONE joined pair
    that carries no sum goes through npm_axpy; several pairs, a fold that carries the sum, or the switch set, take the ranges."""
    from np_modeling_amd import device as D

    class Holder:
        pass
    assert D.ACCUM_RANGES is None or os.environ.get('NPM_ACCUM_RANGES')
    saved = D.ACCUM_RANGES
    try:
        for setting, clip, want in ((None, None, 'npm_axpy'), (None, 1.0, 'npm_accumulate_ranges'), (True, None, 'npm_accumulate_ranges'),
                                    (False, 1.0, 'npm_axpy')):
            D.ACCUM_RANGES = setting
            h = Holder()
            h._w = npm.device.zeros([9])
            opt = npm.optimizer.AdamWOptimizer(1e-3, clip_norm=clip, accumulate=True)
            start = len(npm.sim.calls)
            for _ in range(2):
                opt.update(h, '_w', npm.device.full([9], 1.0))
            opt.apply(grad_scale=0.5)
            folds = [c for c in npm.sim.calls[start:] if c in ('npm_axpy', 'npm_accumulate_ranges')]
            assert folds == [want], (setting, clip, folds)
            assert opt.last['fused_norm'] == (want == 'npm_accumulate_ranges' and clip is not None)
    finally:
        D.ACCUM_RANGES = saved
