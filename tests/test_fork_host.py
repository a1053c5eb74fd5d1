"""CPU: shared key / value prefixes without a GPU, on the simulator of tests/hostsim/kvcache.py.

* ``device.PagedKVCache.fork``: reference counts, free list and table after fork / append / truncate / release; copy-on-write of a
  partly filled shared page exactly once per appender but the last owner; a full shared page never copied; ``room`` refusing with
  nothing changed when copy-on-write would need the last page; the window's reclaim under sharing; refusals of ``fork``;
* ``shared_prefix_rows``; the entry points a layer calls, in order, with ``SHARED_PREFIX`` on and off;
* ``KVCache.fork`` and ``TransformerDecoder.fork`` against every sequence decoded alone in float64;
* the new entry points: header against bindings, and the split rule of the built library against its restatement.

Every test names ``fork``, ``refcount``, ``shared_prefix_rows``, ``SHARED_PREFIX`` or an entry point that does not exist without
this feature.
"""

import ctypes
import os
import re

import numpy as np
import pytest

import decode_cases as DC
import hostsim
from hostsim.fixtures import npm_fixture
import varlen_reference as VR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROW = 32                                   # Hkv * D of the bare caches below: 2 heads of 16


npm = npm_fixture('prefix')


def _rows(seed, count):
    return np.random.default_rng(seed).standard_normal([count, ROW]).astype(np.float32)


def _append(D, cache, mirror, new_rows):
    """``new_rows``: per sequence an array [n_b, ROW] (or None); one ragged append, mirrored on the host."""
    n = np.array([0 if r is None else len(r) for r in new_rows], dtype=np.int64)
    t = max(int(n.max()), 1)
    x = np.zeros([cache.batch, t, ROW], dtype=np.float32)
    for b, r in enumerate(new_rows):
        if r is not None:
            x[b, :len(r)] = r
    dev = D.from_host(x)
    cache.append(D.Mat(dev, ROW), D.Mat(dev, ROW), t, new_lengths=n)
    for b, r in enumerate(new_rows):
        if r is not None:
            mirror[b] = np.concatenate([mirror[b], r])


def _check(cache, mirror):
    """Counts, free list and rows: refcount is the number of table entries naming a page, a page is free exactly at 0, every
    sequence gathers to its own rows."""
    named = np.bincount(cache.block_table[cache.block_table >= 0], minlength=cache.pages)
    assert np.array_equal(cache.refcount, named), (cache.refcount, named)
    assert sorted(cache._free) == np.nonzero(named == 0)[0].tolist()
    assert cache.pages_in_use == int((named > 0).sum()) and cache.pages_in_use + cache.pages_free == cache.pages
    if not cache.dropped.any() and cache.max_length:
        k, v = cache.gather(cache.max_length)
        got = np.asarray(k).reshape(cache.batch, cache.max_length, ROW)
        assert np.array_equal(np.asarray(v), np.asarray(k))
        for b, rows in enumerate(mirror):
            assert np.array_equal(got[b, :len(rows)], rows), b


def _state(cache):
    return cache.lengths.copy(), cache.block_table.copy(), cache.refcount.copy(), sorted(cache._free), cache.dropped.copy()


def _same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


def _prompt(D, batch, rows, page_size, **kwargs):
    cache = D.PagedKVCache(batch, 256, 2, 16, page_size=page_size, **kwargs)
    mirror = [np.zeros([0, ROW], dtype=np.float32) for _ in range(batch)]
    _append(D, cache, mirror, [_rows(0, rows)] + [None] * (batch - 1))
    return cache, mirror


def _fork(cache, mirror, src, dst):
    cache.fork(src, dst)
    mirror[dst] = mirror[src].copy()


# ---- fork and copy-on-write ---------------------------------------------------------------------------------------------------------
def test_a_partly_filled_shared_page_is_copied_once_per_appender_and_written_in_place_by_the_last_owner(npm):
    D = npm.device
    cache, mirror = _prompt(D, 3, 40, 16)                                  # pages 0, 1 full, page 2 holds 8 rows
    calls = len(npm.sim.calls)
    _fork(cache, mirror, 0, 1)
    _fork(cache, mirror, 0, 2)
    assert len(npm.sim.calls) == calls, 'fork launches nothing'
    assert cache.refcount[:3].tolist() == [3, 3, 3] and cache.pages_in_use == 3 and cache.lengths.tolist() == [40, 40, 40]
    assert np.array_equal(cache.block_table[1], cache.block_table[0]) and np.array_equal(cache.block_table[2], cache.block_table[0])
    _check(cache, mirror)

    calls = len(npm.sim.calls)
    _append(D, cache, mirror, [_rows(1, 1), _rows(2, 1), _rows(3, 1)])
    # sequences 0 and 1 took pages 3 and 4 and the 8 valid rows; sequence 2, the last owner, wrote into page 2
    assert npm.sim.copy_calls == [2, 2], 'one launch per tensor for all sequences of the call'
    assert npm.sim.page_copies == [(2, 3, 8), (2, 4, 8)] * 2 and cache.page_copies == 2
    assert cache.block_table[:, 2].tolist() == [3, 4, 2] and cache.refcount[:5].tolist() == [3, 3, 1, 1, 1]
    span = npm.sim.calls[calls:]
    assert span == ['npm_kv_copy_pages'] * 2 + ['npm_kv_append_paged'] * 2, span
    _check(cache, mirror)

    _append(D, cache, mirror, [_rows(4, 3), None, _rows(5, 9)])            # private pages now: nothing more is copied
    assert npm.sim.copy_calls == [2, 2] and cache.pages_in_use == 6
    _check(cache, mirror)
    cache.release(2)
    assert cache.refcount[:3].tolist() == [2, 2, 0] and cache.pages_in_use == 4
    _check(cache, mirror[:2] + [np.zeros([0, ROW], dtype=np.float32)])


def test_a_full_shared_page_is_never_copied(npm):
    D = npm.device
    cache, mirror = _prompt(D, 2, 32, 16)
    _fork(cache, mirror, 0, 1)
    _append(D, cache, mirror, [_rows(1, 5), _rows(2, 1)])
    assert 'npm_kv_copy_pages' not in npm.sim.calls and cache.page_copies == 0
    assert cache.block_table[:, :3].tolist() == [[0, 1, 2], [0, 1, 3]] and cache.refcount[:4].tolist() == [2, 2, 1, 1]
    _check(cache, mirror)


def test_truncate_into_a_shared_page_changes_no_page_and_the_next_append_copies(npm):
    D = npm.device
    cache, mirror = _prompt(D, 2, 40, 16)
    _fork(cache, mirror, 0, 1)
    cache.truncate([0, 12])                                                # sequence 1 back to 28 rows: inside shared page 1
    mirror[1] = mirror[1][:28]
    assert cache.lengths.tolist() == [40, 28] and cache.refcount[:3].tolist() == [2, 2, 1] and cache.block_table[1, 2] == -1
    assert 'npm_kv_copy_pages' not in npm.sim.calls
    _check(cache, mirror)
    _append(D, cache, mirror, [None, _rows(7, 2)])
    assert npm.sim.page_copies == [(1, 3, 12)] * 2 and cache.block_table[1, :2].tolist() == [0, 3]
    assert cache.refcount[:4].tolist() == [2, 1, 1, 1]
    _check(cache, mirror)                                                  # sequence 0 still reads its own rows 16 .. 31 from page 1


def test_room_counts_the_pages_of_copy_on_write_and_refuses_with_nothing_changed(npm):
    D = npm.device
    cache, mirror = _prompt(D, 2, 40, 16, pages=3)
    _fork(cache, mirror, 0, 1)
    before, calls = _state(cache), len(npm.sim.calls)
    one = D.from_host(np.zeros([2, 1, ROW], dtype=np.float32))
    for n in ([1, 0], [0, 1], [1, 1]):
        with pytest.raises(ValueError, match=r'need 1 more pages.* 0 of 3 are free'):
            cache.append(D.Mat(one, ROW), D.Mat(one, ROW), 1, new_lengths=n)
        with pytest.raises(ValueError, match='need 1 more pages'):
            cache.room(1, n)
    assert _same(before, _state(cache)) and len(npm.sim.calls) == calls
    cache.release(0)                                                       # the last owner writes in place: no page needed
    mirror[0] = mirror[0][:0]
    _append(D, cache, mirror, [None, _rows(3, 1)])
    assert 'npm_kv_copy_pages' not in npm.sim.calls and cache.pages_in_use == 3
    _check(cache, mirror)


def test_a_windowed_reclaim_under_sharing_only_decrements(npm):
    D = npm.device
    cache, mirror = _prompt(D, 2, 40, 16, window=8)
    cache.fork(0, 1)
    assert cache.dropped.tolist() == [0, 0] and cache.refcount[:3].tolist() == [2, 2, 2]
    cache.truncate([0, 20])                                                # sequence 1 keeps rows 0 .. 19: pages 0 and 1
    assert cache.refcount[:3].tolist() == [2, 2, 1] and cache.pages_free == cache.pages - 3
    assert cache._reclaim_frees() == 0, 'the pages sequence 0 gives up are still named by sequence 1'
    _append(D, cache, mirror, [_rows(1, 1), None])
    assert cache.dropped.tolist() == [32, 0] and cache.block_table[0, :3].tolist() == [-1, -1, 2]
    assert cache.refcount[:3].tolist() == [1, 1, 1] and cache.pages_free == cache.pages - 3
    assert 'npm_kv_copy_pages' not in npm.sim.calls
    _check(cache, mirror)
    # a fork of a sequence that dropped rows carries ``dropped``
    cache.release(1)
    assert cache.refcount[:3].tolist() == [0, 0, 1] and sorted(cache._free)[:2] == [0, 1]
    cache.fork(0, 1)
    assert cache.dropped.tolist() == [32, 32] and cache.lengths.tolist() == [41, 41] and cache.refcount[2] == 2
    _append(D, cache, mirror, [None, _rows(2, 1)])
    assert npm.sim.page_copies == [(2, 0, 9)] * 2 and cache.block_table[1, 2] == 0
    _check(cache, mirror)


def test_fork_into_an_occupied_slot_or_onto_itself_is_refused(npm):
    D = npm.device
    cache, mirror = _prompt(D, 3, 20, 16)
    _append(D, cache, mirror, [None, _rows(1, 3), None])
    before = _state(cache)
    with pytest.raises(ValueError, match='still holds 3 rows'):
        cache.fork(0, 1)
    with pytest.raises(ValueError, match='onto itself'):
        cache.fork(0, 0)
    for src, dst in ((0, 3), (-1, 2), (3, 2)):
        with pytest.raises(IndexError):
            cache.fork(src, dst)
    assert _same(before, _state(cache))
    cache.fork(0, 2)
    assert cache.lengths.tolist() == [20, 3, 20]


def test_pages_in_use_after_forking_a_prompt_seven_times(npm):
    D = npm.device
    cache, mirror = _prompt(D, 8, 100, 16)                                 # 6 full pages and one with 4 rows
    for dst in range(1, 8):
        _fork(cache, mirror, 0, dst)
    assert cache.pages_in_use == 7 and cache.refcount[:7].tolist() == [8] * 7
    _append(D, cache, mirror, [_rows(10 + b, 1) for b in range(8)])
    assert cache.pages_in_use == 7 + 7 and npm.sim.copy_calls == [7, 7]     # the last owner keeps page 6
    _append(D, cache, mirror, [_rows(20 + b, 16) for b in range(8)])
    assert cache.pages_in_use == 7 + 7 + 8 and npm.sim.copy_calls == [7, 7]
    assert 8 * -(-117 // 16) == 64, 'eight prompts filled on their own hold 64 pages'
    _check(cache, mirror)


def test_two_runs_build_the_same_table(npm):
    D = npm.device
    tables = []
    for _ in range(2):
        cache, mirror = _prompt(D, 4, 50, 16, pages=20)
        rng = np.random.default_rng(5)
        for step in range(40):
            kind = rng.integers(4)
            b = int(rng.integers(4))
            if kind == 0 and cache.lengths[b] == 0:
                src = int(np.argmax(cache.lengths))
                if src != b:
                    _fork(cache, mirror, src, b)
            elif kind == 1 and cache.lengths[b]:
                cache.release(b)
                mirror[b] = mirror[b][:0]
            elif kind == 2 and cache.lengths[b]:
                cut = int(rng.integers(0, min(cache.lengths[b], 20)))
                cache.truncate(np.eye(4, dtype=np.int64)[b] * cut)
                mirror[b] = mirror[b][:len(mirror[b]) - cut]
            else:
                rows = [(_rows(step * 4 + i, int(rng.integers(1, 20))) if cache.lengths[i] else None) for i in range(4)]
                try:
                    cache.room(max(len(r) for r in rows if r is not None) if any(r is not None for r in rows) else 0,
                               [0 if r is None else len(r) for r in rows])
                except ValueError:
                    continue
                if any(r is not None for r in rows):
                    _append(D, cache, mirror, rows)
            _check(cache, mirror)
        tables.append(cache.block_table.copy())
    assert np.array_equal(*tables)


# ---- shared_prefix_rows ---------------------------------------------------------------------------------------------------------------
def test_shared_prefix_rows(npm):
    D = npm.device
    cache, mirror = _prompt(D, 5, 100, 16)
    for dst in (1, 2):
        _fork(cache, mirror, 0, dst)
    _append(D, cache, mirror, [None, None, None, _rows(9, 70), None])      # sequence 3: its own prompt; 4 stays released
    one = np.array([1, 1, 1, 0, 0])
    _append(D, cache, mirror, [_rows(1, 1), _rows(2, 1), _rows(3, 1), None, None])
    assert cache.shared_prefix_rows(one) == 96                             # six full pages; the page of rows 96 .. 100 is private
    assert cache.shared_prefix_rows([1, 0, 1, 0, 0]) == 96                 # inactive and released slots are ignored
    assert cache.shared_prefix_rows([1, 0, 0, 0, 0]) == 0                  # one active sequence
    assert cache.shared_prefix_rows([0, 0, 0, 0, 0]) == 0
    assert cache.shared_prefix_rows([1, 1, 1, 1, 0]) == 0                  # sequence 3 names other pages from slot 0 on
    # a prefix page that still holds a new row: with 6 new tokens of 101 rows, row 95 is new and page 5 is not all old
    assert cache.shared_prefix_rows([6, 6, 1, 0, 0]) == 80
    assert cache.shared_prefix_rows([101, 1, 1, 0, 0]) == 0
    # it stops at the first differing slot: sequence 1 rolls back into page 3 and grows again
    cache.truncate([0, 45, 0, 0, 0])
    mirror[1] = mirror[1][:56]
    _append(D, cache, mirror, [None, _rows(4, 50), None, None, None])
    assert cache.block_table[1, 3] != cache.block_table[0, 3] and cache.block_table[1, 2] == cache.block_table[0, 2]
    assert cache.shared_prefix_rows(one) == 48 and cache.shared_prefix_rows([1, 0, 1, 0, 0]) == 96
    _check(cache, mirror)
    windowed, _ = _prompt(D, 2, 40, 16, window=64)
    windowed.fork(0, 1)
    assert windowed.shared_prefix_rows([1, 1]) == 0                        # a window
    assert D.KVCache(2, 64, 2, 16).attend_prefix_rows(np.array([1, 1]), True) == 0


# ---- the layer: which entry points, in which order ------------------------------------------------------------------------------------
PREFIX_CALLS = ('npm_mha_prefix_fwd', 'npm_attn_combine')


def _forked_layer_run(npm, dtype, tokens, steps=3, rope=False):
    """One prompt of 70 rows into slot 0 of a batch of 4, forked into slots 1 and 2 (slot 3 stays empty), then ``steps`` calls of
    ``tokens`` rows each for the three sequences.  Returns per step (output, path, calls) and the float64 reference rows."""
    f, heads, kv_heads = 128, 8, 1
    att, p = DC.make_mha(npm, f, heads, kv_heads, seed=3, batch=4)
    rng = np.random.default_rng(1)
    prompt = rng.standard_normal([70, f]).astype(np.float32)
    tails = [rng.standard_normal([steps * tokens, f]).astype(np.float32) for _ in range(3)]
    cache = att.make_cache(4, 70 + steps * tokens, page_size=16, dtype=dtype)
    x = np.zeros([4, 70, f], dtype=np.float32)
    x[0] = prompt
    att(x, cache=cache, new_lengths=[70, 0, 0, 0])
    cache.fork(0, 1)
    cache.fork(0, 2)
    out = []
    for s in range(steps):
        x = np.zeros([4, tokens, f], dtype=np.float32)
        for b in range(3):
            x[b] = tails[b][s * tokens:(s + 1) * tokens]
        first, uploads = len(npm.sim.calls), len(npm.sim.uploads)
        y = np.asarray(att(x, cache=cache, new_lengths=[tokens] * 3 + [0]))
        out.append((y, att._cached_path, npm.sim.calls[first:], npm.sim.uploads[uploads:]))
    rows = [np.concatenate([prompt, tail]) for tail in tails]
    schedule = [[70] * 3] + [[tokens] * 3] * steps
    want = [r[70:] for r in VR.layer_alone(p, rows, schedule)]
    return out, want, cache


@pytest.mark.parametrize('dtype', ['f32', 'f16'])
@pytest.mark.parametrize('tokens, path', [(1, 'decode'), (5, 'prefill')])
def test_the_entry_points_called_with_the_switch_on_and_off(npm, monkeypatch, dtype, tokens, path):
    D = npm.device
    monkeypatch.setattr(D, 'PREFILL_KERNEL', True)
    monkeypatch.setattr(D, 'PREFILL_KERNEL_F16', True)
    monkeypatch.setattr(D, 'SHARED_PREFIX_MIN_ROWS', 16)
    suffix_call = {('decode', 'f32'): 'npm_mha_decode_fwd_paged', ('prefill', 'f32'): 'npm_mha_prefill_fwd'}.get(
        (path, dtype), f'npm_mha_{path}_fwd_f16')
    runs = {}
    for on in (False, True):
        monkeypatch.setattr(D, 'SHARED_PREFIX', on)
        prefix_calls = len(npm.sim.prefix_calls)
        out, want, cache = _forked_layer_run(npm, dtype, tokens)
        runs[on] = out
        for step, (y, got_path, calls, uploads) in enumerate(out):
            attention = [c for c in calls if c.startswith('npm_mha_') or c in PREFIX_CALLS]
            if on:
                assert got_path == path + '_shared' and attention == [suffix_call, 'npm_mha_prefix_fwd', 'npm_attn_combine'], (got_path, calls)
                # behind the append's lengths: the table when copy-on-write changed it, and ONE vector of shifted lengths
                assert uploads.count(4 * 3 * 4) == 2, uploads
            else:
                assert got_path == path and attention == [suffix_call] and not any(c in PREFIX_CALLS for c in calls), (got_path, calls)
            assert calls.count('npm_kv_copy_pages') == (2 if step == 0 else 0)
        seen = npm.sim.prefix_calls[prefix_calls:]
        assert len(seen) == (3 if on else 0)
        for call in seen:
            assert call['prefix'] == 64 and call['rows'] == 4 * tokens and call['f16'] == (dtype == 'f16')
            assert call['pages'] == cache.block_table[0, :4].tolist()
            assert call['splits'] == hostsim.kvcache.auto_splits(4 * tokens, 8, 1, 64) == 1
        if dtype == 'f32':
            for step in range(3):
                for b in range(3):
                    got = np.concatenate([o[0][b] for o in out])
                    assert np.abs(got - want[b]).max() <= 2e-5 * (1 + np.abs(want[b]).max())
    for (a, *_), (b, *_) in zip(runs[False], runs[True]):                  # both restated in float64: they differ by roundings
        assert np.abs(a[:3] - b[:3]).max() <= 4e-6 * (1 + np.abs(a[:3]).max())
    assert 'mha_prefix_kernel D=16 R=%d rows=64 prefix=64 splits=1 paged=16' % (4 * tokens) in npm.sim.npm_last_prefix_kernel().decode()


def test_sequences_that_do_not_share_and_short_prefixes_take_the_ordinary_path(npm, monkeypatch):
    D = npm.device
    monkeypatch.setattr(D, 'SHARED_PREFIX', True)
    monkeypatch.setattr(D, 'SHARED_PREFIX_MIN_ROWS', 128)                  # the forked prefix of 64 rows is below the minimum
    out, _, _ = _forked_layer_run(npm, 'f32', 1)
    assert [o[1] for o in out] == ['decode'] * 3 and not npm.sim.prefix_calls
    monkeypatch.setattr(D, 'SHARED_PREFIX_MIN_ROWS', 16)
    att, _ = DC.make_mha(npm, 128, 8, 2, seed=3, batch=3)
    cache = att.make_cache(3, 64, page_size=16)
    x = np.random.default_rng(0).standard_normal([3, 40, 128]).astype(np.float32)
    att(x, cache=cache)                                                    # three prompts filled on their own
    att(x[:, :1], cache=cache)
    assert att._cached_path == 'decode' and not npm.sim.prefix_calls and cache.shared_prefix_rows([1, 1, 1]) == 0


def test_the_split_knob_reaches_the_prefix_pass(npm, monkeypatch):
    from np_modeling_amd import _C
    D = npm.device
    monkeypatch.setattr(D, 'SHARED_PREFIX', True)
    monkeypatch.setattr(D, 'SHARED_PREFIX_MIN_ROWS', 16)
    assert _C.TUNE_PREFIX_SPLITS == 24
    _C.check(_C.lib().npm_set_tuning(_C.TUNE_PREFIX_SPLITS, 3), 'npm_set_tuning')
    out, want, _ = _forked_layer_run(npm, 'f32', 1, steps=1)
    assert [c['splits'] for c in npm.sim.prefix_calls] == [3]
    assert np.abs(out[0][0][0] - want[0]).max() <= 2e-5 * (1 + np.abs(want[0]).max())
    assert hostsim.kvcache.split_ranges(64, 3) == [(0, 32), (32, 64), (64, 64)]        # an empty split is allowed


# ---- the contiguous cache and the decoder ----------------------------------------------------------------------------------------------
def test_a_contiguous_cache_forks_by_copying_its_rows(npm):
    D = npm.device
    for dtype in ('f32', 'f16'):
        cache = D.KVCache(3, 48, 2, 16, dtype=dtype)
        x = np.random.default_rng(0).standard_normal([3, 20, ROW]).astype(np.float32)
        dev = D.from_host(x)
        cache.append(D.Mat(dev, ROW), D.Mat(dev, ROW), 20, new_lengths=[20, 7, 0])
        copies = len(npm.sim.calls)
        cache.fork(0, 2)
        cache.fork(1, 0)                                                   # an occupied slot is replaced, as by write_slot
        assert cache.lengths.tolist() == [7, 7, 20]
        k, v = cache.gather(20)
        got = np.asarray(k).reshape(3, 20, ROW)
        stored = x.astype(np.float16).astype(np.float32) if dtype == 'f16' else x
        assert np.array_equal(got[2], stored[0]) and np.array_equal(got[0, :7], stored[1, :7]) and (got[0, 7:] == 0).all()
        with pytest.raises(ValueError, match='onto itself'):
            cache.fork(1, 1)
        with pytest.raises(IndexError):
            cache.fork(0, 3)
        assert len(npm.sim.calls) >= copies
    frozen = D.KVCache(2, 8, 2, 16)
    frozen.frozen = True
    frozen.lengths[:] = [5, 0]
    frozen.fork(0, 1)                                                      # a frozen cross-attention cache may be forked
    assert frozen.lengths.tolist() == [5, 5] and frozen.frozen


@pytest.mark.parametrize('norm_first', [True, False])
@pytest.mark.parametrize('shared', [False, True])
def test_decoder_fork_then_decode_equals_every_sequence_alone(npm, monkeypatch, norm_first, shared):
    D = npm.device
    monkeypatch.setattr(D, 'SHARED_PREFIX', shared)
    monkeypatch.setattr(D, 'SHARED_PREFIX_MIN_ROWS', 16)
    f, heads, kv_heads = 64, 4, 2
    dec, p = DC.make_decoder(npm, f, heads, kv_heads, 96, norm_first, True, seed=5, batch=3)
    rng = np.random.default_rng(2)
    kv = rng.standard_normal([3, 7, f]).astype(np.float32)
    prompt = rng.standard_normal([37, f]).astype(np.float32)
    tails = [rng.standard_normal([4, f]).astype(np.float32) for _ in range(3)]
    state = dec.start_decoding(kv, 48, page_size=16)
    weights = state.weights
    q = np.zeros([3, 37, f], dtype=np.float32)
    q[0] = prompt
    dec.decode(q, state, new_lengths=[37, 0, 0])
    with pytest.raises(ValueError, match='still holds 37 rows'):
        state.fork(1, 0)
    with pytest.raises(ValueError, match='onto itself'):
        dec.fork(state, 0, 0)
    calls = len(npm.sim.calls)
    dec.fork(state, 0, 1)
    state.fork(0, 2)
    assert state.weights is weights and state.positions.tolist() == [37, 37, 37] and state.cross_cache.lengths.tolist() == [7, 7, 7]
    assert [c for c in npm.sim.calls[calls:] if c != 'npm_d2d'] == []       # the cross-attention rows are copied, nothing else runs
    assert state.self_cache.pages_in_use == 3 and state.self_cache.refcount[:3].tolist() == [3, 3, 3]
    outs, paths = [], []
    for s in range(4):
        x = np.stack([t[s:s + 1] for t in tails])
        outs.append(np.asarray(dec.decode(x, state)))
        paths.append(dec._self_attention._cached_path)
    assert paths == ['decode_shared' if shared else 'decode'] * 4
    assert state.self_cache.page_copies == 2 and state.self_cache.pages_in_use == 5
    rows = [np.concatenate([prompt, t]) for t in tails]
    want = VR.decoder_alone(p, rows, [[37] * 3] + [[1] * 3] * 4, np.repeat(kv[:1], 3, axis=0), [7] * 3, norm_first)
    for b in range(3):
        got = np.concatenate([o[b] for o in outs])
        assert np.abs(got - want[b][37:]).max() <= 1e-4 * (1 + np.abs(want[b]).max()), b


# ---- the entry points --------------------------------------------------------------------------------------------------------------------
def test_prefix_entry_points_are_declared_bound_exported_and_refuse_without_a_device():
    from np_modeling_amd import _C
    text = open(os.path.join(ROOT, 'include', 'npm_hip.h')).read()
    assert re.search(r'#define\s+NPM_ABI_VERSION\s+2\b', text)              # additions: the version stays
    assert int(re.search(r'NPM_TUNE_PREFIX_SPLITS\s*=\s*(\d+)', text).group(1)) == _C.TUNE_PREFIX_SPLITS
    assert int(re.search(r'#define\s+NPM_PREFIX_MAX_SPLITS\s+(\d+)', text).group(1)) == _C.PREFIX_MAX_SPLITS == hostsim.kvcache.MAX_SPLITS
    ctype = {'const npm_mha_decode *': ctypes.POINTER(_C.npm_mha_decode), 'const int32_t *': ctypes.c_void_p, 'int32_t': ctypes.c_int32,
             'int64_t': ctypes.c_int64, 'int': ctypes.c_int, 'float *': ctypes.c_void_p, 'const float *': ctypes.c_void_p,
             'void *': ctypes.c_void_p}
    for name, count in (('npm_kv_copy_pages', 7), ('npm_mha_prefix_fwd', 9), ('npm_mha_prefix_splits', 4), ('npm_attn_combine', 12),
                        ('npm_mha_prefix_supported', 1)):
        proto = re.search(r'int %s\((.*?)\);' % name, text, flags=re.S).group(1)
        args = [re.sub(r'\s*\w+$', '', a.strip()).strip() for a in proto.split(',')]
        assert len(args) == count and _C.SIGNATURES[name] == [ctype[a] for a in args], (name, args)
    makefile = open(os.path.join(ROOT, 'np_modeling_amd', 'csrc', 'Makefile')).read()
    assert 'npm_prefix.hip' in re.search(r'SRCS\s*:=(.*)', makefile).group(1)
    if not os.path.exists(_C.LIB_PATH):
        import __graft_entry__ as entry
        entry.build()
    bound = _C.load_library()
    assert bound.npm_last_prefix_kernel() == b''
    assert [bound.npm_mha_prefix_supported(d) for d in (16, 32, 64, 128, 24, 256)] == [1, 1, 1, 1, 0, 0]
    # the split rule: a function of the shape only, restated in tests/hostsim/kvcache.py
    for shape in ((64, 64, 8, 8192), (8, 64, 8, 2048), (1, 8, 8, 512), (256, 8, 1, 8192), (4, 6, 3, 2112), (2, 8, 8, 16), (64, 128, 1, 8192)):
        assert bound.npm_mha_prefix_splits(*shape) == hostsim.kvcache.auto_splits(*shape), shape
    assert bound.npm_mha_prefix_splits(64, 64, 8, 8192) == 8 and bound.npm_mha_prefix_splits(1, 8, 8, 512) == 4
    assert bound.npm_mha_prefix_splits(0, 8, 8, 512) == 1 and bound.npm_mha_prefix_splits(4, 6, 4, 512) == 1
    count = ctypes.c_int(0)
    bound.npm_device_count(ctypes.byref(count))
    if count.value == 0:
        d = ctypes.byref(_C.npm_mha_decode())
        assert bound.npm_mha_prefix_fwd(d, None, None, 16, 16, 1, None, None, 0) == 10001
        assert bound.npm_attn_combine(None, None, 1, None, 0, None, 1, 1, 1, 16, None, 0) == 10001
        assert bound.npm_kv_copy_pages(None, 0, 0, None, None, None, 0) == 10001
