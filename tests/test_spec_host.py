"""CPU: speculative decoding on the host simulator (tests/hostsim/ (profile 'spec')) and its references (tests/spec_reference.py).

* the draft rule on hand-worked histories (tests/spec_cases.py HAND: the expected n, j and m are written out there);
* ``KVCache.truncate`` / ``PagedKVCache.truncate`` / ``DecodeState.truncate``: lengths, page accounting, windows, refusals;
* ``speculative.decode_step`` emits the tokens of the one-token loop, greedy and sampled; counters, cache lengths, host copies
  (one per step while the same slots decode, never more than two);
* the fixture of tests/test_gpu_spec.py has what that test needs of it;
* header against bindings for npm_verify and the two entry points.

Every test names npm_verify_rows, npm_ngram_draft, truncate, NgramDrafter or speculative: none passes on the parent commit.
"""

import ctypes
import os
import re

import numpy as np
import pytest

from hostsim.fixtures import npm_fixture
import spec_cases as XC
import spec_reference as XR


npm = npm_fixture('spec')


# ---- the draft rule --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', sorted(XC.HAND))
def test_spec_reference_draft_on_hand_worked_histories(name):
    history, t, limit, (nmax, nmin), (n, j, m), chunk = XC.HAND[name]
    got_chunk, n_new, found = XR.draft(history, t, limit, nmax, nmin)
    assert found == (n, j, m) and got_chunk == chunk
    assert n_new == (0 if not history or limit < 0 else 1 + m)


def test_ngram_drafter_proposes_the_hand_worked_drafts_and_checks_its_arguments(npm):
    for name, (history, t, limit, ngram, _, chunk) in sorted(XC.HAND.items()):
        drafter = npm.sampling.NgramDrafter(2, 16, t, ngram=ngram)
        drafter.admit(1, history)
        got, n_new = drafter.propose(np.array([t, limit]))
        assert got.shape == (2, t + 1) and got.numpy()[1].tolist() == chunk, name
        assert n_new.tolist() == [0, XR.draft(history, t, limit, *ngram)[1]] and (got.numpy()[0] == -1).all()
        assert drafter.lengths.tolist() == [0, len(history)] == drafter.device_lengths().tolist()
    drafter.release(1)
    assert drafter.propose()[1].tolist() == [0, 0] and drafter.device_lengths().tolist() == [0, 0]
    for bad in (dict(batch=0), dict(capacity=0), dict(max_draft=0), dict(max_draft=64), dict(ngram=(2, 3)), dict(ngram=(9, 1)),
                dict(ngram=(1, 0))):
        with pytest.raises(ValueError):
            npm.sampling.NgramDrafter(**{**dict(batch=2, capacity=8, max_draft=2), **bad})
    drafter = npm.sampling.NgramDrafter(2, 4, 2)
    for b, ids in ((2, [1]), (0, [1, 2, 3, 4, 5]), (0, [-1]), (0, [2 ** 31]), (0, [[1]]), (0, [1.5]), (True, [1])):
        with pytest.raises(ValueError):
            drafter.admit(b, ids)
    with pytest.raises(ValueError):
        drafter.propose([1, 2, 3])
    assert drafter.lengths.tolist() == [0, 0]
    lib = npm.sim
    ok = dict(history=drafter._history.ptr, history_pitch=4, history_cap=4, history_len=drafter._lengths.ptr, limit=None, batch=2,
              max_draft=2, nmax=3, nmin=1, chunk=drafter._history.ptr, n_new=drafter._lengths.ptr)
    for change in (dict(batch=0), dict(max_draft=64), dict(nmin=0), dict(nmax=9), dict(nmax=1, nmin=2), dict(history_pitch=3),
                   dict(history=None), dict(chunk=None), dict(n_new=None), dict(history_len=None)):
        assert lib.npm_ngram_draft(**{**ok, **change}) == 10002, change


# ---- truncate --------------------------------------------------------------------------------------------------------------------------
def _snapshot(cache):
    return (cache.lengths.copy(), cache.block_table.copy(), sorted(cache._free), cache.dropped.copy()) if cache.paged else (cache.lengths.copy(),)


def _same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


def _rows(batch, tokens, width):
    from np_modeling_amd import device as D
    return D.Mat(D.zeros([batch, tokens, width]), width)


def test_truncate_makes_a_contiguous_cache_ragged_and_refuses_what_it_cannot_do(npm):
    from np_modeling_amd import device as D
    cache = D.KVCache(3, 16, 2, 16)
    cache.append(_rows(3, 5, 32), _rows(3, 5, 32), 5)
    cache.truncate(0)
    assert cache.length == 5
    cache.truncate([0, 2, 5])
    assert cache.ragged and cache.lengths.tolist() == [5, 3, 0] and cache.max_length == 5
    cache.truncate(np.array([1, 1, 0]))
    assert cache.lengths.tolist() == [4, 2, 0]
    before = _snapshot(cache)
    for bad in (-1, [0, 3, 0], [1, 1], [1.0, 1.0, 0.0], 1.0, True, [[1, 1, 0]], 'x'):
        with pytest.raises(ValueError):
            cache.truncate(bad)
        assert _same(before, _snapshot(cache))
    cache.truncate(np.int64(0))
    cache.frozen = True
    with pytest.raises(ValueError, match='frozen'):
        cache.truncate(0)
    launched = [c for c in npm.sim.calls if c.startswith('npm_kv')]
    assert len(launched) == 2                                          # the append's two; truncate launches nothing


def _check_pages(cache):
    held = cache.block_table[cache.block_table >= 0]
    assert len(set(held.tolist())) == held.size and not set(held.tolist()) & set(cache._free)          # no page owned twice
    assert held.size + cache.pages_free == cache.pages and held.size == cache.pages_in_use
    first = cache.dropped // cache.page_size
    last = -(-cache.lengths // cache.page_size)
    for b in range(cache.batch):
        slots = np.nonzero(cache.block_table[b] >= 0)[0].tolist()
        assert slots == list(range(int(first[b]), int(last[b]))), (b, slots, cache.lengths, cache.dropped)


@pytest.mark.parametrize('seed', range(4))
def test_paged_truncate_keeps_the_page_invariants_over_a_seeded_schedule(npm, seed):
    from np_modeling_amd import device as D
    rng = np.random.default_rng(seed)
    batch, capacity, page = 4, 80, 16
    cache = D.PagedKVCache(batch, capacity, 1, 16, page_size=page, pages=12)
    uploads = cache.table_uploads
    for step in range(60):
        action = rng.integers(0, 4)
        if action == 0:                                                # release one, admit it again with the next append
            cache.release(int(rng.integers(0, batch)))
        elif action == 1:
            rows = rng.integers(0, cache.lengths + 1)
            before = -(-cache.lengths // page)
            cache.truncate(rows)
            if ((-(-cache.lengths // page)) < before).any():
                assert cache._table_dirty
        else:
            n = np.minimum(rng.integers(0, 20, size=batch), capacity - cache.lengths)
            try:
                cache.append(_rows(batch, 19, 16), _rows(batch, 19, 16), 19, new_lengths=n)
            except ValueError:
                assert int(cache._pages_needed(n).sum()) > cache.pages_free
        _check_pages(cache)
        assert (cache.lengths >= 0).all() and (cache.block_table >= -1).all()
    assert cache.table_uploads > uploads
    before = _snapshot(cache)
    for bad in (-1, cache.lengths + 1, [0] * 3, 0.5):
        with pytest.raises(ValueError):
            cache.truncate(bad)
        assert _same(before, _snapshot(cache))
    cache.truncate(cache.lengths)
    assert cache.pages_in_use == 0 and (cache.block_table == -1).all()


def test_windowed_paged_truncate_inside_the_last_chunk_and_not_below_the_window(npm):
    from np_modeling_amd import device as D
    cache = D.PagedKVCache(2, 128, 1, 16, page_size=16, window=8)
    cache.append(_rows(2, 40, 16), _rows(2, 40, 16), 40)
    cache.append(_rows(2, 5, 16), _rows(2, 5, 16), 5)                  # reclaims from length 40: rows below 33 -> 32 dropped
    assert cache.dropped.tolist() == [32, 32] and cache.lengths.tolist() == [45, 45]
    _check_pages(cache)
    cache.truncate([4, 0])                                             # inside the chunk just appended: always allowed
    assert cache.lengths.tolist() == [41, 45] and cache.dropped.tolist() == [32, 32]
    _check_pages(cache)
    before = _snapshot(cache)
    with pytest.raises(ValueError, match='window'):
        cache.truncate([3, 0])                                         # 38 - 8 + 1 = 31 < 32: a key it needs is gone
    with pytest.raises(ValueError, match='window'):
        cache.truncate([0, 20])
    assert _same(before, _snapshot(cache))
    cache.truncate([2, 6])                                             # 39 - 7 = 32: the lowest length that still has its window
    assert cache.lengths.tolist() == [39, 39]
    _check_pages(cache)
    cache.append(_rows(2, 5, 16), _rows(2, 5, 16), 5, new_lengths=np.array([5, 0]))
    _check_pages(cache)
    cache.truncate([0, 39])                                            # an emptied sequence starts over
    assert cache.lengths.tolist() == [44, 0] and cache.dropped.tolist() == [32, 0]
    _check_pages(cache)


def test_decode_state_truncate_forwards_to_the_self_cache_only(npm):
    model = XC.make_model(npm)
    dec, _, _, kv, _ = model
    state = dec.start_decoding(kv, 32, page_size=16)
    dec.decode(np.zeros([3, 5, XC.F], dtype=np.float32), state)
    cross = state.cross_cache.lengths.copy()
    state.truncate([0, 1, 4])
    assert state.positions.tolist() == [5, 4, 1] and np.array_equal(state.cross_cache.lengths, cross)
    with pytest.raises(ValueError):
        state.truncate([0, 5, 0])
    with pytest.raises(ValueError, match='frozen'):
        state.cross_cache.truncate(0)


# ---- Sampler.verify --------------------------------------------------------------------------------------------------------------------
def test_verify_on_the_simulator_is_the_reference_and_advances_counters_and_history(npm):
    from np_modeling_amd import device as D
    rng = np.random.default_rng(5)
    batch, rows, vocab = 3, 4, 40
    z = rng.standard_normal([batch * rows, vocab]).astype(np.float32)
    z[2 * rows:] = np.nan                                              # slot 2 is inactive: its logits do not matter
    logits = D.from_host(z)
    sampler, one = npm.sampling.Sampler(batch), npm.sampling.Sampler(batch)
    for b in range(batch):
        sampler.set(b, temperature=0.8, top_k=10, seed=50 + b)
        one.set(b, temperature=0.8, top_k=10, seed=50 + b)
    # what the one-token loop samples from the same rows, counter for counter
    want = np.full([batch, rows], -1)
    for r in range(rows):
        want[:2, r] = one(D.from_host(np.where(np.isnan(z[r::rows]), 0, z[r::rows])), active=[1, 1, 0]).numpy()[:2]
    draft = np.full([batch, rows - 1], -1)
    draft[0] = want[0, :rows - 1]                                      # slot 0: everything confirmed
    draft[1] = [want[1, 0], (want[1, 1] + 1) % vocab, want[1, 2]]      # slot 1: the second drafted token is wrong
    drafter = npm.sampling.NgramDrafter(batch, 8, rows - 1)
    drafter.admit(0, [1, 2])
    drafter.admit(1, [3])
    result = sampler.verify(logits, draft, [rows - 1, rows - 1, -1], history=drafter)
    assert result.accepted.tolist() == [3, 1, 0] and result.ids.shape == (batch, rows)
    assert result.numpy().tolist() == [want[0].tolist(), want[1, :2].tolist() + [-1, -1], [-1] * rows]
    assert np.array_equal(result.ids.numpy(), result.numpy()) and (result.kept[result.numpy() < 0] == 0).all()
    assert ((result.prob > 0) == (result.numpy() >= 0)).all() and result.kept.shape == result.prob.shape == (batch, rows)
    assert sampler.draw.tolist() == [4, 2, 0] == sampler.device_draw().tolist()
    assert drafter.lengths.tolist() == [6, 3, 0] == drafter.device_lengths().tolist()
    assert drafter.numpy()[0, :6].tolist() == [1, 2] + want[0].tolist() and drafter.numpy()[1, :3].tolist() == [3] + want[1, :2].tolist()
    assert npm._C.last_sample_kernel() == 'hostsim npm_verify_rows' and npm.sim.verifies[-1]['history'] != 0
    with pytest.raises(ValueError, match='history capacity'):          # slot 0 holds 6 of 8 and may emit 4
        sampler.verify(logits, draft, [rows - 1, 0, -1], history=drafter)
    for args in ((logits, draft, [rows, 0, 0]), (logits, draft, [0, 0]), (logits, draft[:, :2], [0, 0, 0]), (logits, draft[:2], [0, 0, 0]),
                 (D.from_host(z[:4]), draft, [0, 0, 0]), (z, draft, [0, 0, 0]), (logits, draft, [0.0, 0.0, 0.0])):
        with pytest.raises(ValueError):
            sampler.verify(*args)
    assert sampler.draw.tolist() == [4, 2, 0] and npm.sim.calls.count('npm_verify_rows') == 1


def test_the_simulated_verify_refuses_bad_arguments(npm):
    from np_modeling_amd import _C, device as D
    buf = D.zeros([64])
    ok = dict(logits=buf.ptr, pitch=4, batch=2, rows=2, vocab=4, history_cap=4, temperature=buf.ptr, top_k=buf.ptr, top_p=buf.ptr,
              seed=buf.ptr, draw=buf.ptr, draft=buf.ptr, draft_pitch=1, n_draft=buf.ptr, token=buf.ptr, accepted=buf.ptr,
              history=buf.ptr, history_pitch=4, history_len=buf.ptr)
    for change in (dict(batch=0), dict(rows=0), dict(rows=65), dict(vocab=0), dict(vocab=(1 << 20) + 1), dict(pitch=3), dict(logits=None),
                   dict(draw=None), dict(n_draft=None), dict(token=None), dict(accepted=None), dict(draft=None), dict(draft_pitch=0),
                   dict(history_len=None), dict(history_cap=0), dict(history_pitch=3)):
        assert npm.sim.npm_verify_rows(ctypes.byref(_C.npm_verify(**{**ok, **change}))) == 10002, change


# ---- decode_step -----------------------------------------------------------------------------------------------------------------------
def _samplers(npm, sampled):
    out = []
    for _ in range(2):
        sampler = npm.sampling.Sampler(3)
        if sampled:
            for b in range(3):
                sampler.set(b, temperature=0.8, top_k=10, seed=100 + b)
        out.append(sampler)
    return out


@pytest.mark.parametrize('sampled', [False, True], ids=['greedy', 'sampled'])
@pytest.mark.parametrize('setting', [dict(), dict(cache_dtype='f16'), dict(window=8)], ids=['f32', 'f16', 'window8'])
def test_speculative_decode_step_emits_the_tokens_of_the_one_token_loop(npm, sampled, setting):
    model = XC.make_model(npm, window=setting.get('window'))
    dtype = setting.get('cache_dtype', 'f32')
    one, spec = _samplers(npm, sampled)
    want, _, pages, lengths = XC.plain(npm, model, one, cache_dtype=dtype)
    got, log, state, drafter = XC.speculative(npm, model, spec, cache_dtype=dtype, probe=lambda: len(npm.sim.d2h))
    assert [g[:XC.EMIT] for g in got] == want
    emitted = np.array([len(g) for g in got])
    assert spec.draw.tolist() == emitted.tolist() == spec.device_draw().tolist()             # one draw per token, the first included
    assert state.positions.tolist() == (np.array(XC.PROMPT_LENGTHS) + emitted - 1).tolist()
    assert drafter.lengths.tolist() == (np.array(XC.PROMPT_LENGTHS) + emitted).tolist() == drafter.device_lengths().tolist()
    assert all(copies <= 2 for _, _, copies in log) and len(log) < XC.EMIT - 1               # two host copies a step; fewer steps
    same_slots = [i for i in range(1, len(log)) if np.array_equal(log[i][0] >= 0, log[i - 1][0] >= 0)]
    assert log[0][2] == 2 and same_slots and all(log[i][2] == 1 for i in same_slots)         # one, while the same slots decode
    state.truncate(emitted - XC.EMIT)                                  # stop at the budget: the caches of both loops agree
    assert state.positions.tolist() == lengths.tolist() and state.self_cache.pages_in_use == pages
    calls = npm.sim.calls
    assert calls.count('npm_verify_rows') == len(log) < calls.count('npm_ngram_draft') <= 2 * len(log)


def test_speculative_decode_step_shortens_its_drafts_at_the_capacity_and_stops_there(npm):
    """A cache of 21 rows: sequence 0 (9 prompt rows, 12 tokens) is one row short of it when the loop ends.  The drafts shrink to
    what still fits -- ``limit = capacity - length - 1`` -- the tokens stay those of the plain loop, and a full sequence emits
    nothing more."""
    model = XC.make_model(npm)
    one, spec = _samplers(npm, True)
    want, _, _, lengths = XC.plain(npm, model, one, capacity=21)
    got, log, state, drafter = XC.speculative(npm, model, spec, capacity=21, probe=lambda: len(npm.sim.d2h))
    assert [g[:XC.EMIT] for g in got] == want and lengths.max() == 20
    assert (state.positions <= 21).all() and all(copies <= 2 for _, _, copies in log)
    length = 9
    for n, a, _ in log:                                                # slot 0: never more drafted tokens than rows left
        if n[0] >= 0:
            assert n[0] <= 21 - length - 1
            length += a[0] + 1
    dec, emb, head = model[:3]
    while state.positions[0] < 21:
        before = int(state.positions[0])
        out = npm.speculative.decode_step(dec, state, emb, head, spec, drafter)
        assert len(out[0]) >= 1 and state.positions[0] == before + len(out[0])
    draws = spec.draw.copy()
    out = npm.speculative.decode_step(dec, state, emb, head, spec, drafter)
    assert out[0] == [] and state.positions[0] == 21 and spec.draw[0] == draws[0]


def test_speculative_decode_step_of_a_slot_alone_and_with_nothing_to_do(npm):
    model = XC.make_model(npm)
    _, spec = _samplers(npm, True)
    got, _, _, _ = XC.speculative(npm, model, spec)
    alone = npm.sampling.Sampler(1)
    alone.set(0, temperature=0.8, top_k=10, seed=101)
    tokens, _, state, drafter = XC.speculative(npm, model, alone, rows=[1])
    assert tokens[0][:XC.EMIT] == got[1][:XC.EMIT]
    before = (state.positions.copy(), drafter.lengths.copy(), alone.draw.copy())
    dec, emb, head = model[:3]
    assert npm.speculative.decode_step(dec, state, emb, head, alone, drafter, active=[False]) == [[]]
    assert (state.positions == before[0]).all() and (drafter.lengths == before[1]).all() and (alone.draw == before[2]).all()
    with pytest.raises(ValueError):
        npm.speculative.decode_step(dec, state, emb, head, npm.sampling.Sampler(2), drafter)


@pytest.mark.parametrize('setting', [dict(), dict(cache_dtype='f16'), dict(window=8)], ids=['f32', 'f16', 'window8'])
def test_the_speculative_fixture_has_a_gap_and_both_accepts_and_rejects(npm, setting):
    """What tests/test_gpu_spec.py asserts of its own runs holds for the seed on the simulator, with room: the least top-2 gap of
    the plain run is five times the bound the GPU test asks for, and drafts were both accepted and rejected."""
    model = XC.make_model(npm, window=setting.get('window'))
    dtype = setting.get('cache_dtype', 'f32')
    _, logits, _, _ = XC.plain(npm, model, npm.sampling.Sampler(3), cache_dtype=dtype)
    assert XC.least_gap(logits) >= 5 * XC.GAP
    _, log, _, _ = XC.speculative(npm, model, npm.sampling.Sampler(3), cache_dtype=dtype)
    assert XC.accepts_and_rejects(log) >= (3, 2)


# ---- the entry points ------------------------------------------------------------------------------------------------------------------
def test_spec_header_bindings_and_exports():
    from np_modeling_amd import _C
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, 'include', 'npm_hip.h')).read()
    body = re.search(r'typedef struct npm_verify \{(.*?)\} npm_verify;', text, flags=re.S).group(1)
    body = re.sub(r'/\*.*?\*/', '', body, flags=re.S)
    names = [n.strip().lstrip('*') for decl in body.split(';') if decl.strip()
             for n in re.sub(r'^\s*(const\s+)?(float|int32_t|int64_t|uint64_t)\s*\*?', '', decl.strip()).split(',')]
    assert names == [f[0] for f in _C.npm_verify._fields_]
    assert int(re.search(r'#define NPM_VERIFY_MAX_ROWS (\d+)', text).group(1)) == _C.VERIFY_MAX_ROWS
    assert int(re.search(r'#define NPM_DRAFT_MAX_NGRAM (\d+)', text).group(1)) == _C.DRAFT_MAX_NGRAM
    proto = re.search(r'int npm_ngram_draft\((.*?)\);', text, flags=re.S).group(1)
    kinds = [_C._P if '*' in arg else {'int64_t': _C._I64, 'int32_t': _C._I32}[arg.split()[0]] for arg in proto.split(',')]
    assert kinds == _C.SIGNATURES['npm_ngram_draft'] and _C.SIGNATURES['npm_verify_rows'] == [ctypes.POINTER(_C.npm_verify)]
    assert _C._SPECIAL['npm_last_draft_kernel'] == (ctypes.c_char_p, [])
    if os.path.exists(_C.LIB_PATH):
        lib = ctypes.CDLL(_C.LIB_PATH)
        for name in ('npm_verify_rows', 'npm_ngram_draft', 'npm_last_draft_kernel'):
            assert hasattr(lib, name)
        lib.npm_verify_rows.argtypes, lib.npm_ngram_draft.argtypes = _C.SIGNATURES['npm_verify_rows'], _C.SIGNATURES['npm_ngram_draft']
        count = ctypes.c_int(0)
        lib.npm_device_count(ctypes.byref(count))
        if count.value == 0:                                           # no compute without a GPU: NOT_INITIALIZED, not a crash
            assert lib.npm_verify_rows(ctypes.byref(_C.npm_verify())) == 10001
            assert lib.npm_ngram_draft(None, 0, 0, None, None, 0, 0, 0, 0, None, None) == 10001
