"""GPU: beam search -- npm_beam_step through the C ABI, ``reorder`` on both caches, and ``beam.decode_step`` end to end.

Bounds.  General rows are judged against the fp64 model of tests/beam_reference.py within eps(s) = 6e-6 + V 2^-32 + 2^-23 |s|,
derived there from the kernel's arithmetic (one fp32 rounding of z - zmax, the exponential's ulps, the floors, one rounding of
the score), not measured; every case prints its worst |device - model| / eps and the last test of the family the worst of all.
Where every gap among the model's first 2 W + 1 scores exceeds 2 eps the candidate list must EQUAL the model's
(tests/test_beam_host.py asserts that this leaves out at most 5 % of the family).  Exact rows ({c, -200, -inf}, filtered away from
fp32 rounding boundaries) are bitwise the contract: scores, lists and splits; they carry the tie-breaks.  The split is integer
logic and is always compared exactly, on the device's own candidate list.  ``reorder`` is compared with ``gather`` output and
with layer outputs as bits.  End to end the hypotheses EQUAL the plain Python beam search run on the device's own logits, after
the test asserted from the reference that every decision gap is at least 100 times eps plus the decode tolerance.

Every test here needs npm_beam_step, ``reorder`` or ``beam``: none passes on the parent commit.
"""

import numpy as np
import pytest

import beam_cases as BC

pytestmark = pytest.mark.gpu

WORST = {}


@pytest.fixture(scope='module')
def npm():
    import np_modeling_amd
    return np_modeling_amd


@pytest.fixture(scope='module')
def model(npm):
    return BC.tiny_model(npm)


# ---- npm_beam_step ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', BC.GENERAL, ids=BC.general_id)
def test_general_rows_meet_the_fp64_model(npm, case):
    from np_modeling_amd import _C
    vocab, width, groups, _ = case
    logits, cum, eos = BC.general(*case)
    out = BC.run(logits, cum, groups, width, eos)
    kernel = _C.last_beam_kernel()
    assert kernel == 'beam_rows_kernel %s G=%d W=%d V=%d row=%s' % ('vec' if vocab % 4 == 0 else 'scalar', groups, width, vocab,
                                                                    'lds' if vocab <= 32768 else 'global'), kernel
    WORST[case] = None
    WORST[case] = BC.check_general(out, logits, cum, groups, width, eos, BC.Model(logits, cum, groups, width))
    print(f'{BC.general_id(case)}: worst |device - model| / eps = {WORST[case]:.3f}')


def test_the_worst_error_of_the_family_over_eps(npm):
    """Every general case stayed within eps (each asserted it); this prints the largest ratio for DESIGN.md."""
    assert WORST and None not in WORST.values(), 'a general case failed before its ratio was known'
    case = max(WORST, key=WORST.get)
    print(f'worst |s_dev - s_model| / eps over {len(WORST)} general cases: {WORST[case]:.3f} at {BC.general_id(case)}')
    assert WORST[case] <= 1


@pytest.mark.parametrize('name', [c[0] for c in BC.EXACT])
def test_exact_rows_are_bitwise_the_contract(npm, name):
    logits, cum, groups, width, eos = BC.exact(name)
    out = BC.run(logits, cum, groups, width, eos)
    BC.check_exact(out, logits, cum, groups, width, eos)
    BC.check_split(out, groups, width, eos)
    assert BC.same_bits(out, BC.run(logits, cum, groups, width, eos, pitch=logits.shape[1] + 5, offset=3))


@pytest.mark.parametrize('edge', [BC.edge_pitch_and_misaligned_base, BC.edge_fewer_candidates_than_slots, BC.edge_dead_rows_are_not_read,
                                  BC.edge_a_live_invalid_row_contributes_nothing, BC.edge_eos_positions,
                                  BC.edge_groups_are_independent_and_launches_repeat, BC.edge_bad_arguments],
                         ids=lambda f: f.__name__[5:])
def test_edge_cases(npm, edge):
    edge()


# ---- reorder -------------------------------------------------------------------------------------------------------------------------------
def test_paged_reorder_equals_release_and_fork_and_gathers_the_parents_rows(npm):
    BC.reorder_paged_equals_release_and_fork(npm.device)


@pytest.mark.parametrize('dtype', ['f32', 'f16'])
def test_contiguous_reorder_equals_numpy(npm, dtype):
    BC.reorder_contiguous_equals_numpy(npm.device, dtype)


@pytest.mark.parametrize('dtype, options, page_size', [('f32', {}, 16), ('f32', {'rope_base': 10000.0}, 64), ('f32', {'window': 16}, 16),
                                                       ('f16', {'window': 16, 'rope_base': 500.0}, 16), ('f16', {}, 16), ('f32', {}, None)],
                         ids=['plain', 'rope-page64', 'window', 'f16-window-rope', 'f16', 'contiguous'])
def test_reordered_sequences_equal_sequences_filled_on_their_own(npm, monkeypatch, dtype, options, page_size):
    monkeypatch.setattr(npm.device, 'SHARED_PREFIX', False)
    BC.reordered_sequences_equal_sequences_filled_on_their_own(npm, dtype, options, page_size)


# ---- end to end ------------------------------------------------------------------------------------------------------------------------------
def test_width_one_is_the_greedy_loop(npm, model):
    greedy = BC.greedy_tokens(npm, model, 3, 6)
    search, _, seen = BC.beam_flow(npm, model, 3, 1, None, 6)
    assert len(seen) == 6
    for g in range(3):
        (tokens, score), = search.hypotheses(g)
        assert tokens == greedy[:, g].tolist() and np.isfinite(score)


@pytest.mark.parametrize('kwargs, steps', [({}, None), (dict(early_stopping=False, length_penalty=0.7), 8)], ids=['early', 'patient'])
def test_width_three_equals_the_python_beam_search(npm, model, kwargs, steps):
    eos = int(BC.greedy_tokens(npm, model, 2, 3)[2, 0])
    search, reference, seen = BC.beam_flow(npm, model, 2, 3, eos, 8, **kwargs)
    ratio = BC.least_decision_gap(reference, seen, BC.VOCAB)
    print(f'least decision gap / (100 (eps + decode tolerance)) = {ratio:.2f}, eos {eos}, {len(seen)} steps')
    assert ratio >= 1, 'the fixture has a near-tie'
    assert steps is None or len(seen) == steps
    finished = 0
    for g in range(2):
        got, want = search.hypotheses(g), reference.hypotheses(g)
        assert [t for t, _ in got] == [t for t, _ in want] and len(got) == 3
        assert np.allclose([s for _, s in got], [s for _, s in want], rtol=0, atol=1e-4)
        finished += sum(t[-1] == eos for t, _ in got)
    assert finished > 0, 'eos never occurred'
    assert search.done.all() and (search.scores() == -np.inf).all()
