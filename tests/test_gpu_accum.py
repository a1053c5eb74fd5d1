"""GPU: npm_accumulate_ranges and npm_clip_finish_scaled (csrc/npm_accum.hip), ``optimizer.AdamWOptimizer(accumulate=True)`` and
``train.Trainer.train(..., micro_batches=3)`` on a small ``CausalLM``, on the cases of tests/accum_cases.py -- the ones
tests/test_accum_host.py runs on the simulator.

No check of the kernels has a tolerance:

* the fold against NumPy's float32 ``a + b``, raw bits, at every length x dst phase x src phase (the diagonal reads src 16 bytes at
  a time, every other cell with four 4-byte loads), with +-0, subnormals, +-inf and NaN; sentinels around every buffer; src unchanged;
* the sum of squares out of the same pass against npm_sumsq_ranges on the updated buffers from the same non-zero start: 8 equal bytes;
* npm_clip_finish_scaled against the header's expression in NumPy, bit for bit, and against npm_clip_finish at grad_scale 1;
* the class: accumulators bit for bit the float32 fold of the recorded micro-gradients, moments bit for bit, parameters bit for bit
  except at near ties of their one final rounding (one ulp; at most 16 a parameter, counted from the model alone in the host file);
  fused norm on / off and ranges / axpy route: the same bits;
* the accumulated gradient against the whole batch in float64: the derived bound of tests/accum_reference.py.

Every test here needs the new entry points or the new keywords: none passes on the parent commit.  The largest buffer is two tiles
and a bit."""

import pytest

import accum_cases as XC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def npm():
    import np_modeling_amd
    return np_modeling_amd


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


def test_accumulate_with_one_backward_per_apply_is_the_plain_optimizer(npm):
    XC.check_accumulate_with_one_backward_equals_plain(npm)


def test_three_micro_batches_against_the_models(npm):
    out = XC.check_three_micro_batches(npm)
    out.pop('snapshot')
    print(out)
    assert out['last']['folds'] == XC.K - 1


def test_switches_agree_and_last_follows_them(npm):
    lasts = XC.check_switches_agree(npm)
    print(lasts)
    for (fused, ranges), last in lasts.items():
        assert last['fused_norm'] == (fused and ranges) and last['folds'] == XC.K - 1


def test_against_the_full_batch_in_float64(npm):
    print('worst error / bound:', XC.check_against_the_full_batch_in_float64(npm))


def test_a_second_update_folds_first_and_the_plain_optimizer_still_raises(npm):
    XC.check_second_update_folds_first_and_plain_still_raises(npm)


def test_thirty_three_pairs_through_the_optimizer(npm):
    from np_modeling_amd import device as D
    saved = D.ACCUM_FUSED_NORM
    try:
        for fused in (True, False):
            D.ACCUM_FUSED_NORM = fused
            last = XC.check_thirty_three_pairs_through_the_optimizer(npm)
            print(last)
            assert last['fold_launches'] == 2 and last['fused_norm'] == fused
    finally:
        D.ACCUM_FUSED_NORM = saved


def test_a_scale_without_clipping(npm):
    XC.check_unclipped_scale(npm)


def test_trainer_refusals(npm):
    XC.check_trainer_refusals(npm)


def test_the_printed_loss_is_the_token_mean_of_the_batch(npm):
    XC.check_printed_loss_is_the_token_mean(npm)
