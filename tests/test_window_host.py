"""CPU: sliding-window attention for decoding without a GPU, on the simulator of tests/hostsim/ (profile 'window').

* the page reclaim of ``PagedKVCache(window=W)`` is exact: after every call the table slots in use are the pages that hold a row
  the window can still reach or a row of the call, ``dropped`` is a multiple of the page size, the free list stays a heap and the
  same schedule builds the same table twice; ``room()`` counts the pages about to come back; ``gather()`` raises once rows are
  gone; ``release`` / ``reset`` clear ``dropped``; the table is uploaded only when it changed;
* routing: a windowed cache calls ``npm_mha_decode_fwd_window`` / ``npm_mha_prefill_fwd_window`` and nothing else for its
  self-attention, f32 and f16, whatever the prefill switches say; ``causal=False`` raises; ``window`` without ``causal`` raises;
* ``window=None`` changes no call: the trace of a schedule is that of the classes used without the keyword;
* results: the layer and the decoder fed in chunks equal tests/decode_reference.py with the band mask;
* the entry points: header against bindings and exports, the windowed instances of the built objects do not spill.
"""

import ctypes
import heapq
import os
import re

import numpy as np
import pytest

import decode_cases as DC
import decode_reference as DR
from hostsim.fixtures import npm_fixture
import window_cases as WC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WINDOW_CALLS = ('npm_mha_decode_fwd_window', 'npm_mha_prefill_fwd_window')
OTHER_ATTENTION = ('npm_mha_decode_fwd', 'npm_mha_decode_fwd_varlen', 'npm_mha_decode_fwd_paged', 'npm_mha_decode_fwd_f16',
                   'npm_mha_prefill_fwd', 'npm_mha_prefill_fwd_f16', 'npm_mha_core_fwd', 'npm_mha_core_fwd_grouped', 'npm_mha_mask_summary',
                   'npm_kv_gather_varlen', 'npm_kv_gather_paged', 'npm_kv_gather_f16', 'npm_softmax_fwd')


npm = npm_fixture('window')


# ---- page reclaim ---------------------------------------------------------------------------------------------------------------
def _schedule(rng, batch, capacity, most):
    """Calls n [B] (0 .. most tokens each, some sequences riding along) until the first sequence is about to pass ``capacity``."""
    total, calls = np.zeros(batch, dtype=np.int64), []
    while True:
        n = rng.integers(0, most + 1, size=batch)
        n[rng.integers(0, batch)] = most                                  # T of the call
        if (total + n > capacity).any():
            return calls
        calls.append(n)
        total += n


def _append(npm, cache, n, seed):
    D = npm.device
    t, row = int(n.max()), cache.kv_heads * cache.key_dim
    x = np.random.default_rng(seed).standard_normal([cache.batch, t, row]).astype(np.float32)
    k, v = D.from_host(x), D.from_host(-x)
    cache.append(D.Mat(k, row), D.Mat(v, row), t, n)


def _is_heap(free):
    return all(free[i] <= free[c] for i in range(len(free)) for c in (2 * i + 1, 2 * i + 2) if c < len(free))


@pytest.mark.parametrize('seed', range(6))
def test_window_reclaim_holds_exactly_the_pages_a_row_can_still_reach(npm, seed):
    D = npm.device
    rng = np.random.default_rng(seed)
    window, page, most = int(rng.choice([1, 5, 16, 17, 40, 100])), int(rng.choice([16, 32, 64])), int(rng.choice([1, 4, 33]))
    batch, capacity = 3, 400
    calls = _schedule(rng, batch, capacity, most)
    tables = []
    for run in range(2):
        cache = D.PagedKVCache(batch, capacity, 2, 16, page_size=page, window=window)
        assert cache.window == window and cache.dropped.tolist() == [0] * batch
        history = []
        for step, n in enumerate(calls):
            before, uploads, old = cache.lengths.copy(), cache.table_uploads, cache.block_table.copy()
            _append(npm, cache, n, step)
            assert (cache.lengths == before + n).all()
            for b in range(batch):
                held = WC.held_slots(int(before[b]), int(cache.lengths[b]), window, page, cache.pages_per_sequence)
                assert ((cache.block_table[b] >= 0) == held).all(), (step, b, before, n, cache.block_table[b])
                assert cache.dropped[b] % page == 0 and cache.dropped[b] == np.argmax(held) * page if held.any() else cache.dropped[b] % page == 0
                assert held.sum() <= WC.max_pages(window, most, page)
            used = cache.block_table[cache.block_table >= 0]
            assert len(set(used.tolist())) == len(used) and sorted(used.tolist() + list(cache._free)) == list(range(cache.pages))
            assert _is_heap(cache._free) and cache.pages_in_use == len(used)
            assert cache.table_uploads - uploads == int(not np.array_equal(old, cache.block_table))     # append uploads the table once
            history.append(cache.block_table.copy())
        tables.append(history)
        assert cache.dropped.any() or window > capacity // 2
    for a, b in zip(*tables):
        assert np.array_equal(a, b)                                       # lowest-numbered free page first, both runs


def test_window_room_counts_the_pages_about_to_come_back(npm):
    """A pool of exactly B (ceil((W - 1 + T) / page) + 1) pages decodes to the capacity; without the window it runs out.  Then
    ``room`` against first principles: it raises exactly when free + reclaimable pages do not cover the need."""
    D = npm.device
    batch, page, window, capacity = 2, 16, 24, 200
    pages = batch * WC.max_pages(window, 1, page)
    cache = D.PagedKVCache(batch, capacity, 2, 16, page_size=page, pages=pages, window=window)
    plain = D.PagedKVCache(batch, capacity, 2, 16, page_size=page, pages=pages)
    assert plain.window is None
    raised = None
    for step in range(capacity):
        n = np.ones(batch, dtype=np.int64)
        cache.room(1)
        _append(npm, cache, n, step)
        assert cache.pages_in_use <= pages
        if raised is None:
            try:
                _append(npm, plain, n, step)
            except ValueError as e:
                raised = (step, str(e))
    assert cache.lengths.tolist() == [capacity] * batch and cache.dropped.tolist() == [(capacity - 1 - window + 1) // page * page] * batch
    assert raised is not None and re.search(r'need \d+ more pages', raised[1]) and raised[0] == pages // batch * page
    with pytest.raises(ValueError, match='do not fit the capacity'):
        cache.room(1)
    # first principles, ragged: a pool that is too small by one page for some calls
    rng = np.random.default_rng(0)
    for trial in range(40):
        window, page = int(rng.choice([3, 20, 50])), int(rng.choice([16, 32]))
        small = D.PagedKVCache(3, 300, 1, 16, page_size=page, pages=int(rng.integers(4, 9)), window=window)
        for step in range(30):
            n = rng.integers(0, 40, size=3)
            lengths = small.lengths
            need = int((-(-(lengths + n) // page) - -(-lengths // page)).sum())
            bound = np.maximum(lengths - window + 1, 0) // page
            reclaimable = int((bound - small.dropped // page).clip(min=0).sum())
            fits = need <= small.pages_free + reclaimable and (lengths + n <= small.capacity).all()
            state = (small.lengths.copy(), small.block_table.copy(), list(small._free), small.dropped.copy())
            if fits:
                small.room(int(n.max()), n)
                _append(npm, small, n, step)
            else:
                with pytest.raises(ValueError):
                    small.room(int(n.max()), n)
                with pytest.raises(ValueError):
                    _append(npm, small, n, step)
                assert (small.lengths == state[0]).all() and np.array_equal(small.block_table, state[1])      # nothing was touched
                assert small._free == state[2] and (small.dropped == state[3]).all()
                break


def test_window_gather_raises_once_rows_are_dropped_and_release_and_reset_clear_dropped(npm):
    D = npm.device
    cache = D.PagedKVCache(2, 128, 2, 16, page_size=16, window=8)
    _append(npm, cache, np.array([20, 3]), 0)
    k, _ = cache.gather(20)                                               # nothing dropped yet: the reclaim is the next append's
    assert np.asarray(k).shape == (2, 20, 2, 16) and cache.dropped.tolist() == [0, 0]
    _append(npm, cache, np.array([1, 1]), 1)
    assert cache.dropped.tolist() == [0, 0]                               # 20 - 8 + 1 = 13 < 16: page 0 still holds a live row
    _append(npm, cache, np.array([10, 1]), 2)                             # 21 - 8 + 1 = 14: still page 0
    _append(npm, cache, np.array([1, 1]), 3)                              # 31 - 8 + 1 = 24: page 0 goes
    assert cache.dropped.tolist() == [16, 0] and cache.block_table[0, 0] == -1 and cache.lengths.tolist() == [32, 6]
    with pytest.raises(ValueError, match='given back'):
        cache.gather(32)
    free = cache.pages_free
    cache.release(0)
    assert cache.dropped.tolist() == [0, 0] and cache.lengths.tolist() == [0, 6] and cache.pages_free == free + 1
    assert np.asarray(cache.gather(6)[0]).shape == (2, 6, 2, 16)
    _append(npm, cache, np.array([40, 0]), 4)
    _append(npm, cache, np.array([1, 0]), 5)
    assert cache.dropped.tolist() == [32, 0]
    cache.reset()
    assert cache.dropped.tolist() == [0, 0] and cache.pages_free == cache.pages and (cache.block_table == -1).all()
    with pytest.raises(ValueError, match='window'):
        D.PagedKVCache(2, 128, 2, 16, page_size=16, window=0)
    with pytest.raises(ValueError, match='window'):
        D.KVCache(2, 128, 2, 16, window=2.5)
    assert D.KVCache(2, 128, 2, 16).window is None and D.KVCache(2, 128, 2, 16, window=7).window == 7


# ---- routing --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', ['f32', 'f16'])
@pytest.mark.parametrize('page_size', [None, 16])
@pytest.mark.parametrize('switches', [False, True])
def test_window_layer_calls_only_the_windowed_entry_points_and_equals_the_band(npm, monkeypatch, dtype, page_size, switches):
    """MultiHeadAttention(8, num_kv_heads=2, window=24): chunks 40 (from empty), 1, 4, 40, 1 ..., the decode kernel up to 32 score
    rows per K / V head and the prefill kernel above, with the prefill switches on or off; against float64 with the band."""
    monkeypatch.setattr(npm.device, 'PREFILL_KERNEL', switches)
    monkeypatch.setattr(npm.device, 'PREFILL_KERNEL_F16', switches)
    window, f, heads, kv_heads = 24, 128, 8, 2
    att, p = WC.make_mha(npm, f, heads, kv_heads, seed=3, window=window, batch=3)
    sizes = [40, 1, 4, 40, 1, 8, 9, 1, 1, 1]
    x = np.random.default_rng(2).standard_normal([3, sum(sizes), f]).astype(np.float32)
    cache = att.make_cache(3, sum(sizes), page_size=page_size, dtype=dtype)
    assert cache.window == window and cache.paged == (page_size is not None)
    outs = []
    for piece in DC.split(x, sizes):
        first, reads = len(npm.sim.calls), len(npm.sim.window_reads)
        before = cache.lengths.copy()
        outs.append(np.asarray(att(np.ascontiguousarray(piece), cache=cache)))
        t = piece.shape[1]
        want = 'decode' if heads // kv_heads * t <= 32 else 'prefill'
        span = npm.sim.calls[first:]
        assert att._cached_path == want and span.count(f'npm_mha_{want}_fwd_window') == 1, (t, att._cached_path, span)
        assert not any(c in OTHER_ATTENTION for c in span) and sum(span.count(c) for c in WINDOW_CALLS) == 1, span
        tail = f' window={window}'
        last = (npm.sim.npm_last_decode_kernel if want == 'decode' else npm.sim.npm_last_prefill_kernel)().decode()
        assert last.endswith(tail) and ('kv=f16' in last) == (dtype == 'f16') and ('paged=16' in last) == (page_size == 16), last
        for _, b, lo, hi in npm.sim.window_reads[reads:]:                 # nothing below the first token's floor was looked at
            assert lo == max(0, int(before[b]) + 1 - window) and hi == int(before[b]) + t
    got = np.concatenate(outs, axis=1)
    if dtype == 'f32':
        want_out, _ = DR.att_fwd(p, x.astype(np.float64), mask=WC.band(sum(sizes), window)[None, None])
        np.testing.assert_allclose(got, want_out, rtol=2e-6, atol=2e-6)
    if page_size is not None:
        assert cache.dropped.tolist() == [(sum(sizes) - sizes[-1] - window + 1) // 16 * 16] * 3
        assert cache.pages_in_use <= 3 * WC.max_pages(window, max(sizes), 16)
    with pytest.raises(ValueError, match='causal'):
        cache.attend(npm.device.Mat(npm.device.zeros([3, 1, f]), f), heads, 1, 0.25, causal=False)


def test_window_layer_paged_equals_contiguous_and_ragged_batches_equal_each_sequence_alone(npm):
    import varlen_reference as VR
    window, f, heads, kv_heads = 24, 128, 8, 2
    att, p = WC.make_mha(npm, f, heads, kv_heads, seed=5, window=window, batch=3)
    schedule = [np.array(n) for n in ([5, 40, 0], [1, 1, 33], [4, 0, 1], [1, 1, 1], [30, 1, 1], [1, 1, 0])]
    total = VR.schedule_rows(schedule)
    rng = np.random.default_rng(4)
    x_rows = [rng.standard_normal([int(s), f]).astype(np.float32) for s in total]
    runs = []
    for page_size in (None, 16):
        cache = att.make_cache(3, int(total.max()), page_size=page_size)
        runs.append([np.asarray(att(xc, cache=cache, new_lengths=n)) for xc, n in VR.padded_calls(x_rows, schedule)])
    for a, b in zip(*runs):
        assert np.array_equal(a, b)
    for got, rows in zip(VR.collect(runs[1], schedule, 3), x_rows):
        want, _ = DR.att_fwd(p, rows[None].astype(np.float64), mask=WC.band(len(rows), window)[None, None])
        np.testing.assert_allclose(got, want[0], rtol=2e-6, atol=2e-6)


def test_window_needs_the_kernels_head_sizes_and_causal(npm):
    att, _ = WC.make_mha(npm, 96, 4, 4, seed=1, window=8)                # head size 24
    with pytest.raises(ValueError, match='windowed cache needs head sizes'):
        att.make_cache(2, 32)
    with pytest.raises(ValueError, match='window'):
        npm.layers.MultiHeadAttention(4, window=0)
    with pytest.raises(ValueError, match='causal=True'):
        npm.layers.TransformerDecoder(num_heads=4, hidden_units=32, norm_first=True, window=8)
    with pytest.raises(ValueError, match='causal=True'):
        npm.layers.TransformerDecoder(num_heads=4, hidden_units=32, norm_first=True, causal=False, window=8)


@pytest.mark.parametrize('norm_first', [True, False])
@pytest.mark.parametrize('options', [{}, {'page_size': 16}, {'cache_dtype': 'f16'}, {'page_size': 64, 'cache_dtype': 'f16'}])
def test_window_decoder_trace_names_only_the_windowed_entry_points_for_self_attention(npm, norm_first, options):
    window, f = 24, 128
    dec, p = WC.make_decoder(npm, f, 8, 2, 64, norm_first, seed=7, window=window)
    assert dec._cross_attention._window is None and dec._self_attention._window == window
    rng = np.random.default_rng(1)
    sizes = [40, 1, 1, 5, 33, 1, 15]
    q = rng.standard_normal([2, sum(sizes), f]).astype(np.float32)
    kv = rng.standard_normal([2, 7, f]).astype(np.float32)
    state = dec.start_decoding(kv, sum(sizes) + 8, **options)
    assert state.self_cache.window == window and state.cross_cache.window is None
    first = len(npm.sim.calls)
    outs = [np.asarray(dec.decode(np.ascontiguousarray(piece), state)) for piece in DC.split(q, sizes)]
    calls = npm.sim.calls[first:]
    attention = [c for c in calls if c.startswith('npm_mha_') and c != 'npm_mha_mask_summary']
    assert sum(attention.count(c) for c in WINDOW_CALLS) == len(sizes)
    # every other attention call is the cross-attention's over its frozen, unwindowed cache (7 rows: no call is ragged or paged)
    rest = [c for c in attention if c not in WINDOW_CALLS]
    assert len(rest) >= len(sizes) and not any('varlen' in c or 'paged' in c or 'prefill' in c for c in rest), rest
    if options.get('cache_dtype') == 'f16':                              # the only gathers are the frozen cross cache's (40 rows over 7)
        assert calls.count('npm_kv_gather_f16') == 2 * sum(1 for t in sizes if 4 * t > 32)
    assert attention.count('npm_mha_prefill_fwd_window') == 3 and 'npm_kv_gather_paged' not in calls and 'npm_kv_gather_varlen' not in calls
    if not options.get('cache_dtype'):
        want, _ = DR.decoder_fwd(p, q.astype(np.float64), kv.astype(np.float64), norm_first, mask=WC.band(sum(sizes), window)[None, None])
        np.testing.assert_allclose(np.concatenate(outs, axis=1), want, rtol=1e-5, atol=1e-5)
        # training: forward runs the band through the mask path and equals the same reference
        np.testing.assert_allclose(np.asarray(dec(q, kv)), want, rtol=1e-5, atol=1e-5)
        mask = dec._self_mask(2, sum(sizes))
        assert np.array_equal(np.asarray(mask.full(2, 8, sum(sizes), sum(sizes)))[0, 0].astype(bool), WC.band(sum(sizes), window))
    if 'page_size' in options:
        state.release(0)
        gone = (sum(sizes) - sizes[-1] - window + 1) // options['page_size'] * options['page_size']
        assert state.self_cache.dropped.tolist() == [0, gone]
        dec.admit(state, 0, kv[:1])
        out = np.asarray(dec.decode(np.ascontiguousarray(q[:, :3]), state, new_lengths=np.array([3, 1])))
        assert np.isfinite(out).all() and state.self_cache.lengths.tolist() == [3, sum(sizes) + 1]


def _trace(npm, make, decode):
    obj = make()
    first, uploads = len(npm.sim.calls), len(npm.sim.uploads)
    outs = decode(obj)
    return npm.sim.calls[first:], npm.sim.uploads[uploads:], outs


@pytest.mark.parametrize('page_size', [None, 16])
@pytest.mark.parametrize('dtype', ['f32', 'f16'])
def test_window_none_changes_no_library_call(npm, page_size, dtype):
    """The same ragged schedule through a layer made without the keyword and through one made with window=None, and through
    caches made either way: the same calls in the same order, the same uploads, the same bits."""
    import varlen_reference as VR
    f = 128
    schedule = [np.array(n) for n in ([5, 40, 0], [1, 1, 33], [4, 0, 1], [1, 1, 1])]
    total = VR.schedule_rows(schedule)
    rng = np.random.default_rng(4)
    x_rows = [rng.standard_normal([int(s), f]).astype(np.float32) for s in total]
    uniform = rng.standard_normal([3, 9, f]).astype(np.float32)

    def decode(att):
        cache = att.make_cache(3, int(total.max()), page_size=page_size, dtype=dtype)
        outs = [np.asarray(att(xc, cache=cache, new_lengths=n)) for xc, n in VR.padded_calls(x_rows, schedule)]
        cache = att.make_cache(3, 16, page_size=page_size, dtype=dtype)
        return outs + [np.asarray(att(np.ascontiguousarray(piece), cache=cache)) for piece in DC.split(uniform, [5, 1, 1, 2])]

    def without():
        np.random.seed(11)
        att = npm.layers.MultiHeadAttention(8, num_kv_heads=2)
        att(np.zeros([3, 2, f], dtype=np.float32))
        return att

    def with_none():
        np.random.seed(11)
        att = npm.layers.MultiHeadAttention(8, num_kv_heads=2, window=None)
        att(np.zeros([3, 2, f], dtype=np.float32))
        return att

    a, b = _trace(npm, without, decode), _trace(npm, with_none, decode)
    assert a[0] == b[0] and a[1] == b[1] and not any('window' in c for c in a[0])
    for x, y in zip(a[2], b[2]):
        assert np.array_equal(x, y)
    D = npm.device
    kw = dict(page_size=16) if page_size else {}
    cls = D.PagedKVCache if page_size else D.KVCache
    plain, none = cls(2, 64, 2, 16, dtype=dtype, **kw), cls(2, 64, 2, 16, dtype=dtype, window=None, **kw)
    traces = []
    for cache in (plain, none):
        first = len(npm.sim.calls)
        for step, n in enumerate(([20, 3], [1, 1], [30, 0], [1, 1])):
            _append(npm, cache, np.array(n), step)
        traces.append((npm.sim.calls[first:], cache.lengths.tolist(), np.asarray(cache.gather(51)[0])))
    assert traces[0][0] == traces[1][0] and traces[0][1] == traces[1][1] and np.array_equal(traces[0][2], traces[1][2])
    if page_size:
        assert np.array_equal(plain.block_table, none.block_table) and plain.dropped.tolist() == [0, 0] and plain.pages_in_use == 5


# ---- the entry points -------------------------------------------------------------------------------------------------------------
def test_window_entry_points_are_declared_bound_exported_and_refuse_without_a_device():
    from np_modeling_amd import _C
    text = open(os.path.join(ROOT, 'include', 'npm_hip.h')).read()
    assert re.search(r'#define\s+NPM_ABI_VERSION\s+2\b', text)
    ctype = {'const npm_mha_decode *': ctypes.POINTER(_C.npm_mha_decode), 'const int32_t *': ctypes.c_void_p, 'int32_t': ctypes.c_int32,
             'int': ctypes.c_int}
    for name, count in (('npm_mha_decode_fwd_window', 8), ('npm_mha_prefill_fwd_window', 8), ('npm_mha_decode_window_splits', 5)):
        proto = re.search(r'int %s\((.*?)\);' % name, text, flags=re.S).group(1)
        args = [re.sub(r'\s*\w+$', '', a.strip()).strip() for a in proto.split(',')]
        assert len(args) == count and _C.SIGNATURES[name] == [ctype[a] for a in args], (name, args)
    if not os.path.exists(_C.LIB_PATH):
        import __graft_entry__ as entry
        entry.build()
    bound = _C.load_library()
    count = ctypes.c_int(0)
    bound.npm_device_count(ctypes.byref(count))
    assert bound.npm_mha_decode_window_splits(64, 8, 8192, 1, 512) == bound.npm_mha_decode_splits(64, 8, 512)
    assert bound.npm_mha_decode_window_splits(2, 2, 100, 4, 1000) == bound.npm_mha_decode_splits(2, 2, 100)
    assert bound.npm_mha_decode_window_splits(1, 1, 8192, 4, 2 ** 31 - 1) == bound.npm_mha_decode_splits(1, 1, 8192)
    if count.value == 0:
        d = ctypes.byref(_C.npm_mha_decode())
        assert bound.npm_mha_decode_fwd_window(d, None, None, None, 0, 0, 4, 0) == 10001
        assert bound.npm_mha_prefill_fwd_window(d, None, None, None, 0, 0, 4, 1) == 10001


def test_window_instances_exist_under_their_own_names_and_do_not_spill():
    import sys
    from np_modeling_amd import _C
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import kernel_meta
    if not os.path.exists(_C.LIB_PATH):
        import __graft_entry__ as entry
        entry.build()
    lib_dir = os.path.dirname(_C.LIB_PATH)
    for obj, tag, count in (('npm_decode.o', 'mha_decode_window_kernel', 64), ('npm_prefill.o', 'mha_prefill_window_kernel', 8),
                            ('npm_prefill.o', 'mha_prefill_window_f16_kernel', 8)):      # (an fp16 instance's name may stay mangled)
        meta = {n: m for n, m in kernel_meta.kernel_metadata(os.path.join(lib_dir, obj)).items() if tag in n}
        assert len(meta) == count, (tag, sorted(meta))
        for name, m in meta.items():
            assert m['.vgpr_spill_count'] == 0 and m['.sgpr_spill_count'] == 0 and m['.private_segment_fixed_size'] == 0, (name, m)
