"""CPU: beam search without a GPU, on the simulator of tests/hostsim/ (profile 'beam').

* the reference alone: at most 5 % of the general family is ambiguous (a gap among the model's first 2 W + 1 scores within
  2 eps), the exact family passes its filter, and the contract restated in tests/beam_reference.py meets its own fp64 model;
* npm_beam_step through ``np_modeling_amd._C`` on the simulator: general rows, exact rows, every edge case and every refusal of
  tests/beam_cases.py -- the very functions tests/test_gpu_beam.py runs on the device;
* ``PagedKVCache.reorder`` against ``release`` / ``fork`` through a spare slot, ``KVCache.reorder`` against NumPy,
  ``DecodeState.reorder``, reordered sequences against sequences filled on their own;
* ``beam.BeamSearch`` and ``beam.decode_step`` end to end: width 1 is the greedy loop, width 3 equals the plain Python beam search;
* header, bindings and Makefile name the entry point.

Every test names ``beam``, ``reorder`` or npm_beam_step: none passes without this feature.
"""

import os
import re

import numpy as np
import pytest

import beam_cases as BC
import beam_reference as BR
from hostsim.fixtures import npm_fixture

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST_GENERAL = [c for c in BC.GENERAL if c[0] <= 4099 or (c[0], c[1], c[2]) in ((32768, 3, 1), (32769, 2, 3), (65537, 8, 1))]


npm = npm_fixture('beam')


# ---- the reference alone --------------------------------------------------------------------------------------------------------------
def test_at_most_five_percent_of_the_general_family_is_ambiguous():
    """Where every gap among the model's first C + 1 scores exceeds 2 eps the device's list must EQUAL the model's; this counts
    the groups for which that cannot be asked."""
    groups = ambiguous = 0
    per_width = {}
    for case in BC.GENERAL:
        logits, cum, _ = BC.general(*case)
        model = BC.Model(logits, cum, case[2], case[1])
        groups += len(model.ambiguous)
        ambiguous += sum(model.ambiguous)
        per_width[case[1]] = per_width.get(case[1], 0) + sum(model.ambiguous)
    print(f'ambiguous groups: {ambiguous} of {groups} ({100.0 * ambiguous / groups:.2f} %), per width {per_width}')
    assert ambiguous <= 0.05 * groups


def test_the_exact_family_passes_its_filter_and_covers_the_tie_breaks():
    for name, *_ in BC.EXACT:
        logits, cum, groups, width, eos = BC.exact(name)
        want = BR.step(logits, cum, groups, width, eos, weights=BR.exact_weights)
        assert (want['cand_slot'] >= 0).any(), name
    # equal scores across beams: the smaller beam first; inside a row: the lower index first
    logits, cum, groups, width, eos = BC.exact('ties-across-beams')
    want = BR.step(logits, cum, groups, width, eos, weights=BR.exact_weights)
    assert len(set(want['cand_score'][0].tolist())) == 1
    assert want['cand_slot'][0].tolist() == [0, 0, 1, 1, 2, 2]
    assert all(a < b for a, b in zip(want['cand_token'][0][0::2], want['cand_token'][0][1::2]))
    # the quota of equal keys at the cut: C = 2 of seven maxima, the two lowest indices
    logits, cum, groups, width, eos = BC.exact('seven-max-quota')
    want = BR.step(logits, cum, groups, width, eos, weights=BR.exact_weights)
    for g in range(groups):
        assert want['cand_token'][g].tolist() == np.nonzero(logits[g] == logits[g].max())[0][:2].tolist()
    logits, cum, groups, width, eos = BC.exact('cut-inside-the-ties')
    want = BR.step(logits, cum, groups, width, eos, weights=BR.exact_weights)
    assert sorted(want['cand_token'][0].tolist()) != want['cand_token'][0].tolist()      # several beams interleave
    assert not BC._off_boundary(np.float64(np.float32(1.0)) + 2.0 ** -24)                # a tie of the fp32 rounding is refused


def test_eps_is_what_the_docstring_derives():
    assert BR.eps(0.0, 0) == 6e-6 and BR.eps(-8.0, 1 << 20) == 6e-6 + 2.0 ** -12 + 2.0 ** -20
    assert 88 * 2.0 ** -24 + 3e-7 < 6e-6


# ---- npm_beam_step on the simulator ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', HOST_GENERAL, ids=BC.general_id)
def test_general_rows_meet_the_fp64_model(npm, case):
    vocab, width, groups, _ = case
    logits, cum, eos = BC.general(*case)
    out = BC.run(logits, cum, groups, width, eos)
    worst = BC.check_general(out, logits, cum, groups, width, eos, BC.Model(logits, cum, groups, width))
    print(f'{BC.general_id(case)}: worst |simulator - model| / eps = {worst:.3f}')
    assert npm.sim.beams[-1] == dict(groups=groups, width=width, vocab=vocab, pitch=vocab, eos=eos)


@pytest.mark.parametrize('name', [c[0] for c in BC.EXACT])
def test_exact_rows_are_bitwise_the_contract(npm, name):
    logits, cum, groups, width, eos = BC.exact(name)
    out = BC.run(logits, cum, groups, width, eos)
    BC.check_exact(out, logits, cum, groups, width, eos)
    BC.check_split(out, groups, width, eos)


@pytest.mark.parametrize('edge', [BC.edge_pitch_and_misaligned_base, BC.edge_fewer_candidates_than_slots, BC.edge_dead_rows_are_not_read,
                                  BC.edge_a_live_invalid_row_contributes_nothing, BC.edge_eos_positions,
                                  BC.edge_groups_are_independent_and_launches_repeat, BC.edge_bad_arguments],
                         ids=lambda f: f.__name__[5:])
def test_edge_cases(npm, edge):
    edge()


# ---- reorder -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kwargs', [{}, dict(window=24), dict(dtype='f16')], ids=['plain', 'window', 'f16'])
def test_paged_reorder_equals_release_and_fork_through_a_spare_slot(npm, kwargs):
    calls = []
    real = npm.device.PagedKVCache.reorder

    def counted(cache, parents):
        before = len(npm.sim.calls)
        real(cache, parents)
        calls.append(len(npm.sim.calls) - before)

    npm.device.PagedKVCache.reorder = counted
    try:
        BC.reorder_paged_equals_release_and_fork(npm.device, **kwargs)
    finally:
        npm.device.PagedKVCache.reorder = real
    assert calls and not any(calls), 'PagedKVCache.reorder launches nothing'


def test_an_identity_reorder_and_a_child_in_its_parents_slot_cost_nothing(npm):
    D = npm.device
    cache = D.PagedKVCache(4, 64, 2, 16, page_size=16)
    BC.cache_append(D, cache, [BC.cache_rows(b, 20) for b in range(3)] + [None])
    cache._device_table()
    uploads, state = cache.table_uploads, BC.cache_state(cache)
    for parents in ([0, 1, 2, 3], [0, 1, 2, -1]):                                      # slot 3 is empty either way
        cache.reorder(parents)
        cache._device_table()
        assert cache.table_uploads == uploads and all(np.array_equal(x, y) for x, y in zip(state, BC.cache_state(cache)))
    cache.reorder([0, 1, 1, -1])
    cache._device_table()
    assert cache.table_uploads == uploads + 1 and cache.refcount[:6].tolist() == [1, 1, 2, 2, 0, 0] and cache.pages_free == 12
    assert cache.page_copies == 0


@pytest.mark.parametrize('dtype', ['f32', 'f16'])
def test_contiguous_reorder_equals_numpy(npm, dtype):
    BC.reorder_contiguous_equals_numpy(npm.device, dtype)
    assert 'O(L)' in npm.device.KVCache.reorder.__doc__


def test_a_bad_vector_raises_with_nothing_changed(npm):
    BC.reorder_bad_vectors(npm.device, pytest)


@pytest.mark.parametrize('page_size', [16, 64, None], ids=['page16', 'page64', 'contiguous'])
@pytest.mark.parametrize('dtype, options', [('f32', {}), ('f32', {'rope_base': 10000.0}), ('f32', {'window': 16}),
                                            ('f16', {'window': 16, 'rope_base': 500.0}), ('f16', {})],
                         ids=['plain', 'rope', 'window', 'f16-window-rope', 'f16'])
def test_reordered_sequences_equal_sequences_filled_on_their_own(npm, monkeypatch, dtype, options, page_size):
    monkeypatch.setattr(npm.device, 'SHARED_PREFIX', False)
    BC.reordered_sequences_equal_sequences_filled_on_their_own(npm, dtype, options, page_size)


def test_decode_state_reorder_shares_or_copies_the_memory(npm):
    import decode_cases as DC
    f = 64
    dec, _ = DC.make_decoder(npm, f, 4, 2, 96, True, True, seed=5, batch=4)
    rng = np.random.default_rng(2)
    kv = rng.standard_normal([4, 7, f]).astype(np.float32)
    kv[2:] = kv[0]                                                                     # slots 0, 2, 3: beams of one prompt
    state = dec.start_decoding(kv, 48, page_size=16, kv_lengths=[7, 5, 7, 7])
    q = rng.standard_normal([4, 20, f]).astype(np.float32)
    dec.decode(q, state, new_lengths=[20, 9, 0, 0])
    before = (BC.cache_state(state.self_cache), state.cross_cache.lengths.copy())
    for bad, error in (([1, 1, 0, 0], ValueError), ([0, 0, 0, 0], ValueError), ([0, 1, 2], ValueError), ([0, 1, 2, 4], IndexError)):
        with pytest.raises(error):
            state.reorder(bad)
    with pytest.raises(ValueError, match='memory'):
        state.reorder([0, 1, 2, 3], memory='none')
    assert all(np.array_equal(x, y) for x, y in zip(before[0], BC.cache_state(state.self_cache)))
    assert np.array_equal(before[1], state.cross_cache.lengths)
    calls = len(npm.sim.calls)
    dec.reorder(state, [0, -1, 0, 0])
    assert len(npm.sim.calls) == calls, "memory='shared' launches nothing"
    assert state.positions.tolist() == [20, 0, 20, 20] and state.cross_cache.lengths.tolist() == [7, 0, 7, 7]
    assert state.self_cache.refcount[:2].tolist() == [3, 3] and state.self_cache.pages_in_use == 2
    # 'copy': the cross-attention rows follow
    state = dec.start_decoding(kv, 48, page_size=16, kv_lengths=[7, 5, 7, 7])
    dec.decode(q, state, new_lengths=[20, 9, 0, 0])
    rows = [np.asarray(x).copy() for x in state.cross_cache.gather(7)]
    state.reorder([1, 0, 1, -1], memory='copy')
    assert state.positions.tolist() == [9, 20, 9, 0] and state.cross_cache.lengths.tolist() == [5, 7, 5, 0]
    for x, was in zip(state.cross_cache.gather(7), rows):
        assert np.array_equal(np.asarray(x)[[0, 1, 2]], was[[1, 0, 1]]) and (np.asarray(x)[3] == 0).all()


# ---- end to end ------------------------------------------------------------------------------------------------------------------------------
def test_width_one_is_the_greedy_loop(npm):
    model = BC.tiny_model(npm)
    greedy = BC.greedy_tokens(npm, model, 3, 6)
    search, _, seen = BC.beam_flow(npm, model, 3, 1, None, 6)
    assert len(seen) == 6
    for g in range(3):
        (tokens, score), = search.hypotheses(g)
        assert tokens == greedy[:, g].tolist() and np.isfinite(score)
    # one launch and ONE copy to the host per search: 4 bytes each of parent, ids, lse and 3 x 2 W candidates
    assert npm.sim.calls.count('npm_beam_step') == 6 and npm.sim.d2h.count(4 * (3 * 3 + 3 * 3 * 2)) >= 6


def test_width_three_equals_the_python_beam_search(npm):
    model = BC.tiny_model(npm)
    eos = int(BC.greedy_tokens(npm, model, 2, 3)[2, 0])
    search, reference, seen = BC.beam_flow(npm, model, 2, 3, eos, 6)
    ratio = BC.least_decision_gap(reference, seen, BC.VOCAB)
    print(f'least decision gap / (100 (eps + decode tolerance)) = {ratio:.2f}, eos {eos}, {len(seen)} steps')
    assert ratio >= 1, 'the fixture has a near-tie: pick another eos or length'
    finished = 0
    for g in range(2):
        got, want = search.hypotheses(g), reference.hypotheses(g)
        assert [t for t, _ in got] == [t for t, _ in want] and len(got) == 3
        assert np.allclose([s for _, s in got], [s for _, s in want], rtol=0, atol=1e-4)
        assert [s for _, s in got] == sorted((s for _, s in got), reverse=True)
        finished += sum(t[-1] == eos for t, _ in got)
    assert finished > 0, 'eos never occurred'
    assert search.done.all() and (search.scores() == -np.inf).all()


def test_a_group_without_early_stopping_and_a_reset(npm):
    model = BC.tiny_model(npm)
    eos = int(BC.greedy_tokens(npm, model, 2, 3)[2, 0])
    search, reference, seen = BC.beam_flow(npm, model, 2, 3, eos, 8, early_stopping=False, length_penalty=0.7)
    ratio = BC.least_decision_gap(reference, seen, BC.VOCAB)
    print(f'least decision gap / (100 (eps + decode tolerance)) = {ratio:.2f}, eos {eos}, {len(seen)} steps')
    assert ratio >= 1 and len(seen) == 8
    for g in range(2):
        assert [t for t, _ in search.hypotheses(g)] == [t for t, _ in reference.hypotheses(g)]
    search.reset(1)
    assert search.scores().tolist() == [-np.inf] * 3 + [0.0, -np.inf, -np.inf] and search.hypotheses(1) == [] and not search.done[1]
    assert search.done[0] and search.tokens[1] == [[], None, None]
    with pytest.raises(ValueError):
        npm.beam.BeamSearch(1, 33)
    with pytest.raises(ValueError):
        npm.beam.BeamSearch(0, 2)
    with pytest.raises(ValueError):
        search.search(np.zeros([6, 50], dtype=np.float32))


# ---- the entry point ------------------------------------------------------------------------------------------------------------------------
def test_the_entry_point_is_declared_bound_and_built():
    import ctypes
    from np_modeling_amd import _C
    text = open(os.path.join(ROOT, 'include', 'npm_hip.h')).read()
    assert re.search(r'#define\s+NPM_ABI_VERSION\s+2\b', text)
    assert int(re.search(r'#define\s+NPM_BEAM_MAX_WIDTH\s+(\d+)', text).group(1)) == _C.BEAM_MAX_WIDTH == 32
    assert _C.SIGNATURES['npm_beam_step'] == [ctypes.POINTER(_C.npm_beam)]
    body = re.search(r'typedef struct npm_beam \{(.*?)\} npm_beam;', text, flags=re.S).group(1)
    body = re.sub(r'/\*.*?\*/', '', body, flags=re.S)
    names = []
    for decl in body.split(';'):
        decl = re.sub(r'^\s*(const\s+)?(float|int32_t|int64_t|void)\s*\*?', '', decl.strip())
        names += [n.strip().lstrip('*') for n in decl.split(',') if n.strip()]
    assert names == [f[0] for f in _C.npm_beam._fields_]
    assert ctypes.sizeof(_C.npm_beam) == 8 * 2 + 4 * 4 + 8 * 9
    for groups, width in ((1, 1), (3, 8), (7, 32)):
        assert _C.beam_workspace_bytes(groups, width) == 4 * groups * width * (1 + 2 * 2 * width)
    makefile = open(os.path.join(ROOT, 'np_modeling_amd', 'csrc', 'Makefile')).read()
    assert 'npm_beam.hip' in re.search(r'SRCS\s*:=(.*)', makefile).group(1)
    if not os.path.exists(_C.LIB_PATH):
        import __graft_entry__ as entry
        entry.build()
    bound = _C.load_library()
    count = ctypes.c_int(0)
    bound.npm_device_count(ctypes.byref(count))
    if count.value == 0:
        assert bound.npm_beam_step(ctypes.byref(_C.npm_beam())) == 10001
        assert bound.npm_last_beam_kernel() == b''
