"""CPU: the paged key / value cache without a GPU, on the simulator of tests/hostsim/ (profile 'paged').

* ``device.PagedKVCache``: page sizes it takes, the pool (not batch x capacity) as the limit -- an append that needs more pages
  than are free raises before any call is recorded and leaves lengths, table and free list as they were; ``release`` gives the
  pages back; a seeded random schedule of append / release / admit keeps the invariants (no page owned twice, in use + free ==
  pages, ``gather`` returns each sequence's rows exactly, the same seed builds the same table);
* the table's device mirror goes up only when the table changed;
* ``MultiHeadAttention`` and ``TransformerDecoder.decode`` with a paged cache give outputs array_equal to the same calls with a
  ``KVCache`` (the simulator restates both in float64 from the same rows), on the three paths that remain;
* continuous batching: four sequences decode, one is released (its pages are filled with NaN), a fifth is admitted into its slot;
  every sequence equals the float64 reference of that sequence alone at the bounds tests/test_varlen_host.py uses;
* the three new entry points: header against bindings.

Every test names npm_*_paged, ``PagedKVCache``, ``page_size``, ``release`` or ``admit``: none exists without this feature.
"""

import ctypes
import os
import re

import numpy as np
import pytest

import decode_cases as DC
from hostsim.fixtures import built, npm_fixture
import paged_cases as PC
import varlen_reference as VR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


npm = npm_fixture('paged')


def _owned(cache):
    return [cache.block_table[b][cache.block_table[b] >= 0].tolist() for b in range(cache.batch)]


def _check_invariants(cache):
    owned = _owned(cache)
    flat = [p for row in owned for p in row]
    assert len(flat) == len(set(flat)), 'a page is owned twice'
    assert cache.pages_in_use == len(flat) and cache.pages_in_use + cache.pages_free == cache.pages
    assert sorted(flat + sorted(cache._free)) == list(range(cache.pages))
    for b, row in enumerate(owned):
        assert len(row) == PC.pages_of(cache.lengths[b], cache.page_size)
        assert (cache.block_table[b, :len(row)] >= 0).all()                # a sequence's pages are the first entries of its row


# ---- PagedKVCache ----------------------------------------------------------------------------------------------------------------
def test_page_size_must_be_a_power_of_two_of_at_least_16(npm):
    D = npm.device
    for bad in (0, 8, 24, 48, -16):
        with pytest.raises(ValueError, match='page_size'):
            D.PagedKVCache(2, 64, 2, 16, page_size=bad)
    with pytest.raises(TypeError):
        D.PagedKVCache(2, 64, 2, 16)                                       # no default
    cache = D.PagedKVCache(3, 100, 2, 16, 32, page_size=32)
    assert (cache.pages, cache.pages_per_sequence, cache.pages_free, cache.pages_in_use) == (12, 4, 12, 0)
    assert cache.k.shape == (12, 32, 2, 16) and cache.v.shape == (12, 32, 2, 32)
    assert cache.block_table.shape == (3, 4) and cache.block_table.dtype == np.int32 and (cache.block_table == -1).all()
    assert cache.lengths.tolist() == [0, 0, 0] and cache.length == 0 and not cache.ragged and not cache.frozen


def test_the_pool_is_the_limit_not_batch_times_capacity(npm):
    D = npm.device
    cache = D.PagedKVCache(4, 256, 2, 16, page_size=16, pages=24)         # a contiguous cache would be 64 pages
    rng = np.random.default_rng(0)
    src = rng.standard_normal([4, 256, 32]).astype(np.float32)
    rows = D.from_host(src)
    cache.append(D.Mat(rows, 32), D.Mat(rows, 32), 256, new_lengths=[256, 16, 40, 8])
    assert cache.lengths.tolist() == [256, 16, 40, 8] and cache.pages_in_use == 16 + 1 + 3 + 1 and cache.pages_free == 3
    assert npm.sim.calls.count('npm_kv_append_paged') == 2 and not any('varlen' in c or c == 'npm_kv_append' for c in npm.sim.calls)
    one = D.from_host(src[:, :1])
    cache.append(D.Mat(one, 32), D.Mat(one, 32), 1, new_lengths=[0, 1, 1, 1])   # only the sequence at 16 needs a page
    assert cache.lengths.tolist() == [256, 17, 41, 9] and cache.pages_in_use == 22 and cache.pages_free == 2
    _check_invariants(cache)

    chunk = D.from_host(src[:, :48])
    calls, lengths, table, free = len(npm.sim.calls), cache.lengths.copy(), cache.block_table.copy(), sorted(cache._free)
    with pytest.raises(ValueError, match=r'need 3 more pages.* 2 of 24 are free'):
        cache.append(D.Mat(chunk, 32), D.Mat(chunk, 32), 48, new_lengths=[0, 0, 48, 0])
    with pytest.raises(ValueError, match=r'need 3 more pages'):
        cache.room(48, [0, 0, 48, 0])
    assert len(npm.sim.calls) == calls and np.array_equal(cache.lengths, lengths) and np.array_equal(cache.block_table, table)
    assert sorted(cache._free) == free and cache.pages_free == 2
    with pytest.raises(ValueError, match='do not fit'):
        cache.room(1, [1, 0, 0, 0])                                        # and capacity still bounds ONE sequence
    cache.release(0)
    assert cache.pages_free == 18 and cache.lengths.tolist() == [0, 17, 41, 9] and len(npm.sim.calls) == calls   # nothing launched
    cache.append(D.Mat(chunk, 32), D.Mat(chunk, 32), 48, new_lengths=[0, 0, 48, 0])
    assert cache.lengths.tolist() == [0, 17, 89, 9] and cache.pages_in_use == 2 + 6 + 1
    _check_invariants(cache)
    k, v = cache.gather(89)
    got = np.asarray(k).reshape(4, 89, 32)
    assert np.array_equal(got[2], np.concatenate([src[2, :40], src[2, :1], src[2, :48]])) and (got[0] == 0).all()
    assert np.array_equal(got[1, :17], np.concatenate([src[1, :16], src[1, :1]])) and (got[1, 17:] == 0).all()
    assert np.array_equal(np.asarray(v), np.asarray(k))
    assert 'npm_kv_gather_paged' in npm.sim.calls
    cache.reset()
    assert cache.pages_free == 24 and cache.max_length == 0 and (cache.block_table == -1).all()


def _random_schedule(D, seed, steps=300):
    """append / release / admit at random; returns the table history's digest and checks gather against a host mirror."""
    rng = np.random.default_rng(seed)
    batch, capacity, size, pages, row = 5, 96, 16, 17, 16
    cache = D.PagedKVCache(batch, capacity, 1, row, page_size=size, pages=pages)
    mirror = [np.zeros([0, row], dtype=np.float32) for _ in range(batch)]
    tables, refused = [], 0
    for step in range(steps):
        kind = rng.integers(0, 24)
        if kind == 0:                                                     # a sequence (or two) ends
            gone = rng.choice(batch, size=rng.integers(1, 3), replace=False)
            cache.release(gone if len(gone) > 1 else int(gone[0]))
            for b in gone:
                mirror[b] = mirror[b][:0]
        else:                                                             # single tokens, or a prompt into every empty slot
            tokens = 1 if kind < 18 else int(rng.integers(2, 40))
            n = np.where(cache.lengths == 0, rng.integers(0, tokens + 1, batch), rng.integers(0, 3, batch))
            n = np.minimum(n, tokens)
            src = rng.standard_normal([batch, tokens, row]).astype(np.float32)
            dev = D.from_host(src)
            try:
                cache.append(D.Mat(dev, row), D.Mat(dev, row), tokens, new_lengths=n)
            except ValueError as e:                                       # the capacity of one sequence, or the pool
                assert 'do not fit' in str(e) or 'more pages' in str(e)
                refused += 1
            else:
                for b in range(batch):
                    mirror[b] = np.concatenate([mirror[b], src[b, :n[b]]])
        _check_invariants(cache)
        assert cache.lengths.tolist() == [len(m) for m in mirror]
        tables.append(cache.block_table.copy())
        if step % 25 == 24 and cache.max_length:
            k, _ = cache.gather(cache.max_length)
            got = np.asarray(k).reshape(batch, cache.max_length, row)
            for b in range(batch):
                assert np.array_equal(got[b, :len(mirror[b])], mirror[b]) and (got[b, len(mirror[b]):] == 0).all()
    return np.stack(tables), refused


def test_random_append_release_admit_schedule_keeps_the_invariants(npm):
    D = npm.device
    first, refused = _random_schedule(D, seed=11)
    again, _ = _random_schedule(D, seed=11)
    other, _ = _random_schedule(D, seed=12)
    assert refused > 0, 'the schedule never ran the pool dry'
    assert np.array_equal(first, again) and not np.array_equal(first, other)             # the same seed builds the same table
    assert (first >= 0).any() and (first == -1).any()


def test_release_takes_an_index_or_several_and_allocation_is_lowest_page_first(npm):
    D = npm.device
    cache = D.PagedKVCache(3, 64, 1, 16, page_size=16, pages=8)
    rows = D.from_host(np.zeros([3, 33, 16], dtype=np.float32))
    cache.append(D.Mat(rows, 16), D.Mat(rows, 16), 33, new_lengths=[33, 1, 17])
    assert _owned(cache) == [[0, 1, 2], [3], [4, 5]]
    cache.release([0, 2])
    assert _owned(cache) == [[], [3], []] and cache.lengths.tolist() == [0, 1, 0] and cache.pages_free == 7
    cache.append(D.Mat(rows, 16), D.Mat(rows, 16), 33, new_lengths=[0, 0, 20])
    assert _owned(cache) == [[], [3], [0, 1]]
    with pytest.raises(IndexError):
        cache.release(3)
    with pytest.raises(ValueError, match='cannot be assigned'):
        cache.length = 4


def test_single_token_steps_inside_their_pages_upload_the_table_once(npm):
    att, _ = DC.make_mha(npm, 64, 4, 2, seed=1, batch=3)
    cache = att.make_cache(3, 64, page_size=16)
    rng = np.random.default_rng(0)
    att(rng.standard_normal([3, 5, 64]).astype(np.float32), cache=cache, new_lengths=[5, 2, 3])
    assert cache.table_uploads == 1
    table_bytes = cache.block_table.nbytes
    assert table_bytes != 3 * 3 * 4                                       # the lengths mirror [3, B] has another size
    first = len(npm.sim.uploads)
    for _ in range(10):                                                   # lengths reach 15, 12, 13: every step stays in its page
        att(rng.standard_normal([3, 1, 64]).astype(np.float32), cache=cache, new_lengths=[1, 1, 1])
    assert cache.table_uploads == 1 and table_bytes not in npm.sim.uploads[first:]
    assert npm.sim.uploads[first:].count(3 * 3 * 4) == 10                 # the lengths: one upload per step, shared by append and attend
    att(rng.standard_normal([3, 1, 64]).astype(np.float32), cache=cache, new_lengths=[1, 0, 0])   # row 15: the page's last
    assert cache.table_uploads == 1 and cache.lengths.tolist() == [16, 12, 13]
    att(rng.standard_normal([3, 1, 64]).astype(np.float32), cache=cache, new_lengths=[1, 0, 0])   # sequence 0 takes a second page
    assert cache.table_uploads == 2 and npm.sim.uploads[first:].count(table_bytes) == 1
    assert npm.sim.npm_last_decode_kernel().decode().endswith('causal=1 varlen=1 paged=16')


# ---- layers: a paged cache against the contiguous one ------------------------------------------------------------------------------
def _layer_run(att, x_rows, schedule, capacity, **paged):
    cache = att.make_cache(len(x_rows), capacity, **paged)
    outs, paths = [], []
    for x, n in VR.padded_calls(x_rows, schedule):
        outs.append(np.asarray(att(x, cache=cache, new_lengths=n)))
        paths.append(att._cached_path)
    assert cache.lengths.tolist() == VR.schedule_rows(schedule).tolist()
    return outs, paths, cache


@pytest.mark.parametrize('heads,kv_heads,f', [(4, 4, 64), (8, 2, 128), (4, 1, 64)])
@pytest.mark.parametrize('page_size', [16, 64])
def test_layer_with_a_paged_cache_equals_the_contiguous_cache(npm, heads, kv_heads, f, page_size):
    """A ragged prompt (the fused forward on the fresh projection), single tokens (the decode kernel), a second chunk too large
    for the decode kernel (the fused forward on gathered rows), more single tokens."""
    att, p = DC.make_mha(npm, f, heads, kv_heads, seed=heads, batch=3)
    g = heads // kv_heads
    schedule = [np.array(n) for n in ([3, 37, 20], [1, 1, 1], [1, 0, 1], [40, 2, 33], [1, 1, 0], [1, 1, 1])]
    total = VR.schedule_rows(schedule)
    rng = np.random.default_rng(1)
    x_rows = [rng.standard_normal([s, f]).astype(np.float32) for s in total]
    want, want_paths, _ = _layer_run(att, x_rows, schedule, int(total.max()) + 2)
    first = len(npm.sim.calls)
    got, paths, cache = _layer_run(att, x_rows, schedule, int(total.max()) + 2, page_size=page_size, pages=3 * PC.pages_of(total.max(), page_size))
    calls = npm.sim.calls[first:]
    assert paths == want_paths == ['fused_masked', 'decode', 'decode', 'fused_masked', 'decode', 'decode']
    assert isinstance(cache, npm.device.PagedKVCache) and cache.page_size == page_size
    assert calls.count('npm_mha_decode_fwd_paged') == 4 and calls.count('npm_kv_gather_paged') == 2
    assert calls.count('npm_kv_append_paged') == 12
    assert not any(c in ('npm_mha_decode_fwd', 'npm_mha_decode_fwd_varlen', 'npm_kv_append', 'npm_kv_append_varlen',
                         'npm_kv_gather_varlen', 'npm_d2d') for c in calls)
    for a, b in zip(got, want):
        assert np.array_equal(a, b)
    for a, b in zip(VR.collect(got, schedule, 3), VR.layer_alone(p, x_rows, schedule)):
        np.testing.assert_allclose(a, b, rtol=2e-6, atol=2e-6)
    _check_invariants(cache)


def test_uniform_lengths_on_a_paged_cache_still_take_the_paged_calls(npm):
    att, _ = DC.make_mha(npm, 64, 4, 2, seed=1)
    x = np.random.default_rng(0).standard_normal([2, 3, 64]).astype(np.float32)
    plain, paged = att.make_cache(2, 40), att.make_cache(2, 40, page_size=32)
    for chunk in (x, x[:, :1], x[:, :2]):
        first = len(npm.sim.calls)
        want = np.asarray(att(np.ascontiguousarray(chunk), cache=plain))
        middle = len(npm.sim.calls)
        got = np.asarray(att(np.ascontiguousarray(chunk), cache=paged))
        assert np.array_equal(got, want) and att._cached_path == 'decode'
        assert 'npm_mha_decode_fwd' in npm.sim.calls[first:middle] and 'npm_mha_decode_fwd_paged' in npm.sim.calls[middle:]
        assert 'npm_mha_decode_fwd' not in npm.sim.calls[middle:]
    assert paged.length == plain.length == 6 and not paged.ragged
    wide = np.random.default_rng(1).standard_normal([2, 20, 64]).astype(np.float32)        # 2 x 20 rows: the fused forward, gathered
    want = np.asarray(att(wide, cache=plain))
    first = len(npm.sim.calls)
    got = np.asarray(att(wide, cache=paged))
    assert att._cached_path == 'fused_masked' and npm.sim.calls[first:].count('npm_kv_gather_paged') == 2
    np.testing.assert_allclose(got, want, rtol=2e-6, atol=2e-6)          # the contiguous cache took its b == 1 / full-cache shortcut or a copy


def test_make_cache_refuses_what_a_paged_cache_cannot_serve(npm):
    att12, _ = DC.make_mha(npm, 48, 4, 2, seed=6)                        # head size 12: only the GEMM composition
    with pytest.raises(NotImplementedError, match='16, 32, 64, 128'):
        att12.make_cache(2, 8, page_size=16)
    att, _ = DC.make_mha(npm, 64, 4, 2, seed=6)
    with pytest.raises(ValueError, match='page_size'):
        att.make_cache(2, 8, pages=4)
    with pytest.raises(ValueError, match='page_size'):
        att.make_cache(2, 8, page_size=24)
    assert type(att.make_cache(2, 8)) is npm.device.KVCache               # without page_size: today's cache


def test_cross_attention_fills_a_paged_cache_too(npm):
    att, p = DC.make_mha(npm, 64, 4, 2, seed=8, batch=3)
    rng = np.random.default_rng(4)
    kv = rng.standard_normal([3, 9, 64]).astype(np.float32)
    kv_lengths = np.array([9, 2, 5])
    cache = att.fill_cache(att.make_cache(3, 9, page_size=16), kv, lengths=kv_lengths)
    assert cache.frozen and cache.lengths.tolist() == [9, 2, 5] and cache.pages_in_use == 3
    n = np.array([4, 0, 2])
    x_rows = [rng.standard_normal([s, 64]).astype(np.float32) for s in n]
    (x, _), = VR.padded_calls(x_rows, [n])
    out = np.asarray(att(x, cache=cache, new_lengths=n))
    assert att._cached_path == 'decode' and npm.sim.npm_last_decode_kernel().decode().endswith('causal=0 varlen=1 paged=16')
    for got, want in zip(VR.collect([out], [n], 3), VR.cross_alone(p, x_rows, kv, kv_lengths)):
        np.testing.assert_allclose(got, want, rtol=2e-6, atol=2e-6)


# ---- TransformerDecoder ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('norm_first', [True, False])
@pytest.mark.parametrize('kv_heads', [None, 2])
def test_decoder_decode_with_a_paged_self_cache_equals_the_contiguous_one(npm, norm_first, kv_heads):
    f = 64
    dec, p = DC.make_decoder(npm, f, 4, kv_heads, 96, norm_first, True, seed=9, batch=3)
    schedule = [np.array(n) for n in ([11, 2, 6], [1, 1, 1], [1, 1, 0], [1, 0, 0], [1, 0, 1])]
    total = VR.schedule_rows(schedule)
    rng = np.random.default_rng(5)
    q_rows = [rng.standard_normal([s, f]).astype(np.float32) for s in total]
    kv = rng.standard_normal([3, 7, f]).astype(np.float32)
    kv_lengths = np.array([7, 3, 1])
    runs = []
    for kwargs in ({}, dict(page_size=16, pages=4)):
        state = dec.start_decoding(kv, 32, kv_lengths=kv_lengths, **kwargs)
        runs.append([np.asarray(dec.decode(x, state, new_lengths=n)) for x, n in VR.padded_calls(q_rows, schedule)])
        assert state.positions.tolist() == total.tolist()
    assert isinstance(state.self_cache, npm.device.PagedKVCache) and type(state.cross_cache) is npm.device.KVCache
    assert state.self_cache.pages_in_use == 3 and state.self_cache.pages_free == 1
    for a, b in zip(*runs):
        assert np.array_equal(a, b)
    for got, ref in zip(VR.collect(runs[1], schedule, 3), VR.decoder_alone(p, q_rows, schedule, kv, kv_lengths, norm_first)):
        np.testing.assert_allclose(got, ref, rtol=1e-5, atol=1e-5)
    before = len(npm.sim.calls)
    with pytest.raises(ValueError, match='more pages'):
        dec.decode(np.zeros([3, 13, f], dtype=np.float32), state, new_lengths=[0, 13, 10])   # 2 pages wanted, 1 free
    assert len(npm.sim.calls) == before and state.positions.tolist() == total.tolist()
    plain = dec.start_decoding(kv, 8)
    with pytest.raises(ValueError, match='not paged'):
        plain.release(0)


# ---- continuous batching -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('heads,kv_heads,f', [(4, 4, 64), (8, 2, 128)])
def test_layer_release_and_admit_while_the_others_decode(npm, heads, kv_heads, f):
    att, p = DC.make_mha(npm, f, heads, kv_heads, seed=heads + 1, batch=4)
    total = PC.plan_rows()
    rng = np.random.default_rng(7)
    x_rows = [rng.standard_normal([s, f]).astype(np.float32) for s in total]
    cache = att.make_cache(4, 32, page_size=16, pages=6)                  # 2 + 1 + 1 + 1 pages, then 1 for the fifth
    got = PC.run_continuous(lambda x, n: att(x, cache=cache, new_lengths=n), cache.release, lambda slot: None, cache, x_rows)
    assert cache.lengths.tolist() == [int(total[0]), int(total[4]), int(total[2]), int(total[3])]
    for a, b in zip(got, VR.layer_alone(p, x_rows, PC.PLAN)):
        np.testing.assert_allclose(a, b, rtol=2e-6, atol=2e-6)
    _check_invariants(cache)


@pytest.mark.parametrize('norm_first', [True, False])
def test_decoder_release_and_admit_with_a_longer_memory(npm, norm_first):
    f = 64
    dec, p = DC.make_decoder(npm, f, 4, 2, 96, norm_first, True, seed=13, batch=4)
    total = PC.plan_rows()
    rng = np.random.default_rng(8)
    q_rows = [rng.standard_normal([s, f]).astype(np.float32) for s in total]
    kv = rng.standard_normal([5, 11, f]).astype(np.float32)              # the fifth sequence's memory is the longest
    kv_lengths = np.array([7, 3, 1, 5, 11])
    state = dec.start_decoding(kv[:4, :7], 32, kv_lengths=kv_lengths[:4], page_size=16, pages=6, memory_capacity=12)
    assert state.cross_cache.capacity == 12 and state.cross_cache.lengths.tolist() == [7, 3, 1, 5]
    def admit(slot):
        assert state.cross_cache.lengths[slot] == 0 and state.self_cache.lengths[slot] == 0
        with pytest.raises(ValueError, match='do not fit'):
            dec.admit(state, slot, np.zeros([1, 13, f], dtype=np.float32))
        dec.admit(state, slot, kv[4:5], kv_length=11)
        assert state.cross_cache.lengths.tolist() == [7, 11, 1, 5]

    got = PC.run_continuous(lambda x, n: dec.decode(x, state, new_lengths=n), state.release, admit, state.self_cache, q_rows)
    assert state.positions.tolist() == [int(total[0]), int(total[4]), int(total[2]), int(total[3])]
    for a, b in zip(got, VR.decoder_alone(p, q_rows, PC.PLAN, kv, kv_lengths, norm_first)):
        np.testing.assert_allclose(a, b, rtol=1e-5, atol=1e-5)
    with pytest.raises(ValueError, match='release'):
        dec.admit(state, 0, kv[4:5])                                      # the slot is in use


# ---- the C ABI -------------------------------------------------------------------------------------------------------------------
def test_paged_entry_points_header_against_bindings(built):
    _C = built
    text = open(os.path.join(ROOT, 'include', 'npm_hip.h')).read()
    text = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    ctype = {'const npm_mha_decode *': ctypes.POINTER(_C.npm_mha_decode), 'const int32_t *': ctypes.c_void_p,
             'const float *': ctypes.c_void_p, 'float *': ctypes.c_void_p, 'int64_t': ctypes.c_int64, 'int32_t': ctypes.c_int32}
    lib = ctypes.CDLL(_C.LIB_PATH)
    for name, count in (('npm_mha_decode_fwd_paged', 6), ('npm_kv_append_paged', 13), ('npm_kv_gather_paged', 11)):
        args = re.search(r'\bint %s\((.*?)\);' % name, text, flags=re.S).group(1)
        want = []
        for arg in (a.strip() for a in args.split(',')):
            kind = re.match(r'(.*?)(\w+)$', arg).group(1).strip()
            want.append(ctype[kind])
        assert len(want) == count and _C.SIGNATURES[name] == want, (name, want, _C.SIGNATURES[name])
        assert hasattr(lib, name), f'{name} not exported'
    bound = _C.load_library()
    assert bound.npm_abi_version() == 2
    assert ctypes.sizeof(_C.npm_mha_decode) == 120                       # the descriptor keeps its layout
    count = ctypes.c_int(-1)
    bound.npm_device_count(ctypes.byref(count))
    if count.value == 0:                                                  # no compute without a GPU, as every entry point
        assert bound.npm_mha_decode_fwd_paged(ctypes.byref(_C.npm_mha_decode()), None, None, None, 0, 16) in (10001, 10002)
        assert bound.npm_kv_gather_paged(None, 0, 0, None, 1, 1, 4, None, None, 0, 16) == 10001
        assert bound.npm_kv_append_paged(None, 0, None, 0, 0, 1, 1, 4, None, None, None, 0, 16) == 10001
