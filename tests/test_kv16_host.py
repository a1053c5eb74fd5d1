"""CPU: the half-precision key / value cache without a GPU, on the simulator of tests/hostsim/ (profile 'kv16').

* what an append stores is NumPy's ``astype(np.float16)``: the row of edge values of tests/kv16_reference.py against bit patterns
  worked out by hand (IEEE round to nearest even, overflow to inf at 65520, subnormal results kept);
* the derived distance bound is a worst case: a float64 model of attention over rounded K / V uses a small fraction of it;
* the grid of the GPU's bitwise comparison covers every value of every axis;
* routing: ``dtype=`` validation, ``nbytes`` halved, which entry points a cached forward calls, ``_cached_path`` ('decode' where the
  decode kernel takes the call, else 'fused_masked' on ``cache.gather``: never the fresh projection, ``_valid_rows`` / npm_d2d, the
  prefill kernel or the cache tensors themselves), ``write_slot``'s byte offsets, and that an fp32 cache makes exactly the calls it
  made before;
* the three entry points: header against bindings and exports.

Every test names ``dtype=``, ``cache_dtype=``, an ``_f16`` entry point or tests/kv16_reference.py: none exists without the feature.
"""

import ctypes
import os
import re

import numpy as np
import pytest

import decode_cases as DC
import decode_reference as DR
from hostsim.fixtures import activate, built, deactivate, npm_fixture
import kv16_reference as K16
import varlen_reference as VR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32_CACHE_CALLS = ('npm_kv_append', 'npm_kv_append_varlen', 'npm_kv_append_paged', 'npm_kv_gather_varlen', 'npm_kv_gather_paged',
                   'npm_mha_decode_fwd', 'npm_mha_decode_fwd_varlen', 'npm_mha_decode_fwd_paged', 'npm_mha_prefill_fwd')


npm = npm_fixture('kv16')


# ---- the references themselves ------------------------------------------------------------------------------------------------------
def test_edge_values_round_as_ieee_says():
    assert np.array_equal(K16.to_f16(K16.EDGE_VALUES).view(np.uint16), K16.EDGE_BITS)
    assert np.isinf(K16.to_f16(np.float32(65520.0))) and K16.to_f16(np.float32(65519.996)) == np.float16(65504.0)
    assert K16.to_f16(np.float32(1 + 2.0 ** -11)) == 1.0 and K16.to_f16(np.float32(1 + 3 * 2.0 ** -11)) == np.float16(1 + 2.0 ** -9)
    assert K16.rounded(np.float32(6e-8)) == np.float32(2.0 ** -24) and K16.rounded(np.float32(2.9e-8)) == 0.0
    assert np.signbit(K16.to_f16(np.float32(-0.0)))


def test_case_grid_covers_every_axis_value():
    cases = K16.bitwise_cases()
    assert 150 <= len(cases) <= 400 and len({K16.case_id(c) for c in cases}) == len(cases)
    assert {c[0] for c in cases} == set(K16.HEAD_DIMS) == {16, 32, 64, 128}
    assert {c[1] // c[2] * c[3] for c in cases} == set(K16.GROUP_ROWS) == {1, 3, 16, 17, 32}
    assert {c[1:4] for c in cases} == set(K16.GROUPS)
    assert {1, 15, 16, 17, 100, 529} <= {c[4] for c in cases} and all(c[4] >= c[3] for c in cases)
    assert {c[5] for c in cases} == {0, 1} and {c[6] for c in cases} == {'one', 'auto', 'many'}
    assert {c[7] for c in cases} == {1, 2} and {c[8] for c in cases} == {1, 3}
    assert {c[9] for c in cases} == {'uniform', 'varlen', 'paged16', 'paged64'}
    for d in K16.HEAD_DIMS:                                               # every head size meets every layout, split mode and row block count
        mine = [c for c in cases if c[0] == d]
        assert {c[9] for c in mine} == set(K16.LAYOUTS) and {c[6] for c in mine} == set(K16.SPLITS) and {c[7] for c in mine} == {1, 2}
        assert {c[1] // c[2] * c[3] > 16 for c in mine} == {False, True} and {c[4] for c in mine} >= {15, 16, 17, 100, 529}


@pytest.mark.parametrize('d', [16, 64, 128])
def test_derived_bound_is_a_worst_case_for_a_float64_model(d):
    rng = np.random.default_rng(d)
    q = rng.standard_normal([2, 3, 8, d])
    k, v = rng.standard_normal([2, 200, 2, d]), rng.standard_normal([2, 200, 2, d])
    scale = 1.0 / np.sqrt(d)
    want, _ = DR.decode_attention(q, k, v, 200, scale, True)
    got, _ = DR.decode_attention(q, K16.rounded(k).astype(np.float64), K16.rounded(v).astype(np.float64), 200, scale, True)
    bound, eps = K16.derived_bound(q, k, v, scale, 0.0)
    used = float(np.abs(got - want).max() / bound)
    print(f'D={d}: eps {eps:.3e}, {100 * used:.2f} % of the derived bound')
    assert 0 < used < 0.05


# ---- the cache classes --------------------------------------------------------------------------------------------------------------
def test_dtype_is_validated_and_reported(npm):
    D = npm.device
    for bad in ('bf16', 'fp16', None, 16):
        with pytest.raises(ValueError, match='dtype'):
            D.KVCache(2, 8, 2, 16, dtype=bad)
        with pytest.raises(ValueError, match='dtype'):
            D.PagedKVCache(2, 32, 2, 16, page_size=16, dtype=bad)
    plain, half = D.KVCache(2, 24, 2, 16), D.KVCache(2, 24, 2, 16, dtype='f16')
    assert (plain.dtype, plain.itemsize, half.dtype, half.itemsize) == ('f32', 4, 'f16', 2)
    assert plain.nbytes == 2 * 4 * 2 * 24 * 2 * 16 and half.nbytes * 2 == plain.nbytes
    assert isinstance(half.k, D.HalfBuffer) and half.k.shape == (2, 24, 2, 16) and not hasattr(half.k, '__array__')
    assert half.layout(half.k) == D.KVLayout(32, 24 * 32, dtype='f16') and plain.layout(plain.k) == D.KVLayout(32, 24 * 32)
    pp, ph = D.PagedKVCache(2, 40, 2, 16, page_size=16, pages=5), D.PagedKVCache(2, 40, 2, 16, page_size=16, pages=5, dtype='f16')
    assert (pp.dtype, ph.dtype, ph.itemsize) == ('f32', 'f16', 2) and ph.nbytes * 2 == pp.nbytes == 2 * 4 * 5 * 16 * 32
    assert ph.layout(ph.k)[:2] == (32, 16 * 32) and ph.layout(ph.k).dtype == 'f16' and ph.layout(ph.k).page_rows == 16


def test_append_gather_and_attend_take_the_f16_entry_points(npm):
    D = npm.device
    rng = np.random.default_rng(0)
    b, cap, hkv, d, hq = 3, 40, 2, 16, 4
    k, v = (rng.standard_normal([b, 5, hkv, d]).astype(np.float32) * 300 for _ in range(2))
    k[0, 0, 0, :K16.EDGE_VALUES.size] = K16.EDGE_VALUES
    for cache in (D.KVCache(b, cap, hkv, d, dtype='f16'), D.PagedKVCache(b, cap, hkv, d, page_size=16, dtype='f16')):
        first = len(npm.sim.calls)
        cache.append(D.Mat(D.from_host(k), hkv * d), D.Mat(D.from_host(v), hkv * d), 5)
        cache.append(D.Mat(D.from_host(k), hkv * d), D.Mat(D.from_host(v), hkv * d), 5, new_lengths=[2, 0, 5])
        assert cache.lengths.tolist() == [7, 5, 10]
        gk, gv = (np.asarray(x) for x in cache.gather(12))
        for got, src in ((gk, k), (gv, v)):
            want = np.zeros([b, 12, hkv, d], dtype=np.float32)
            want[:, :5] = K16.rounded(src)
            want[0, 5:7], want[2, 5:10] = K16.rounded(src[0, :2]), K16.rounded(src[2])
            assert np.array_equal(got.view(np.uint32), want.view(np.uint32))           # exact, -0.0 and inf included
        q = rng.standard_normal([b, 2, hq, d]).astype(np.float32)
        ctx, lse = cache.attend(D.Mat(D.from_host(q), hq * d), hq, 2, 0.25, False, want_lse=True)
        assert npm.sim.npm_last_decode_kernel().decode().endswith(' kv=f16')
        with pytest.raises(ValueError, match='prefill'):
            cache.attend(D.Mat(D.from_host(q), hq * d), hq, 2, 0.25, False, kernel='prefill')
        calls = npm.sim.calls[first:]
        assert calls.count('npm_kv_append_f16') == 4 and calls.count('npm_kv_gather_f16') == 2 and calls.count('npm_mha_decode_fwd_f16') == 1
        assert not any(c in F32_CACHE_CALLS for c in calls)
        reads = [r for r in npm.sim.f16_reads if r[0] == 'decode'][-2 * b:]
        assert [r[2] for r in reads] == [7, 7, 5, 5, 10, 10]              # nothing at or past a length is looked at


def test_write_slot_offsets_count_bytes_of_the_storage_type(npm):
    D = npm.device
    rng = np.random.default_rng(1)
    b, cap, hkv, d = 3, 9, 2, 16
    rows = rng.standard_normal([4, hkv, d]).astype(np.float32)
    for dtype in ('f32', 'f16'):
        cache = D.KVCache(b, cap, hkv, d, dtype=dtype)
        base = rng.standard_normal([b, 2, hkv, d]).astype(np.float32)
        cache.append(D.Mat(D.from_host(base), hkv * d), D.Mat(D.from_host(base), hkv * d), 2)
        cache.write_slot(1, D.Mat(D.from_host(rows), hkv * d), D.Mat(D.from_host(2 * rows), hkv * d), 4)
        assert cache.lengths.tolist() == [2, 4, 2]
        gk, gv = (np.asarray(x) for x in cache.gather(4))
        conv = K16.rounded if dtype == 'f16' else (lambda x: x)
        assert np.array_equal(gk[1], conv(rows)) and np.array_equal(gv[1], conv(2 * rows))
        for i in (0, 2):                                                  # the neighbours keep their rows
            assert np.array_equal(gk[i, :2], conv(base[i])) and not gk[i, 2:].any()
    with pytest.raises(NotImplementedError):
        D.PagedKVCache(b, 32, hkv, d, page_size=16, dtype='f16').write_slot(0, None, None, 1)


# ---- layers -------------------------------------------------------------------------------------------------------------------------
def test_make_cache_validates_dtype_and_head_size(npm):
    att, _ = DC.make_mha(npm, 64, 4, 2, seed=6)
    with pytest.raises(ValueError, match='dtype'):
        att.make_cache(2, 8, dtype='f8')
    half = att.make_cache(2, 8, dtype='f16')
    assert type(half) is npm.device.KVCache and half.dtype == 'f16' and att.make_cache(2, 8).dtype == 'f32'
    paged = att.make_cache(2, 40, page_size=16, pages=5, dtype='f16')
    assert type(paged) is npm.device.PagedKVCache and paged.dtype == 'f16' and paged.nbytes == 2 * 2 * 5 * 16 * 2 * 16
    att12, _ = DC.make_mha(npm, 48, 4, 2, seed=6)                        # head size 12
    with pytest.raises(NotImplementedError, match='16, 32, 64, 128'):
        att12.make_cache(2, 8, dtype='f16')
    assert att12.make_cache(2, 8).dtype == 'f32'                          # the fp32 cache still serves it


def _chunks(att, x, sizes, cache, new_lengths=None):
    outs, paths, spans = [], [], []
    for i, piece in enumerate(DC.split(x, sizes)):
        first = len(att_sim(att).calls)
        outs.append(np.asarray(att(np.ascontiguousarray(piece), cache=cache, new_lengths=None if new_lengths is None else new_lengths[i])))
        paths.append(att._cached_path)
        spans.append(att_sim(att).calls[first:])
    return outs, paths, spans


def att_sim(att):
    import np_modeling_amd
    return np_modeling_amd.sim


def _stored_reference(p, x, sizes, cache_rows, heads, kv_heads):
    """Attention in float64 over K / V AS STORED (``cache_rows``: (k, v) gathered after the last call), per chunk."""
    k, v = (np.asarray(r, dtype=np.float64) for r in cache_rows)
    outs, at = [], 0
    for piece in DC.split(x, sizes):
        t = piece.shape[1]
        q = DR._project(piece.astype(np.float64), p['wq'], p['bq'])
        ctx, _ = DR.decode_attention(q, k, v, at + t, 1.0 / np.sqrt(q.shape[3]), True)
        outs.append(np.einsum('...abc,...dbc->...ad', ctx, p['wo']) + p['bo'])
        at += t
    return outs


@pytest.mark.parametrize('heads,kv_heads,f', [(8, 8, 128), (8, 2, 128), (4, 1, 256)])
@pytest.mark.parametrize('switch', [False, True])
def test_layer_attends_to_the_rows_as_stored(npm, monkeypatch, heads, kv_heads, f, switch):
    """Chunks 40 (from empty: the fp32 cache would use the fresh projection), 1, 3, 40 (on cached rows), 1: the decode kernel where
    it takes the call, else the fused masked forward on gathered rows -- with the prefill switch on or off."""
    monkeypatch.setattr(npm.device, 'PREFILL_KERNEL', switch)
    att, p = DC.make_mha(npm, f, heads, kv_heads, seed=3)
    sizes = [40, 1, 3, 40, 1]
    x = np.random.default_rng(2).standard_normal([2, sum(sizes), f]).astype(np.float32)
    monkeypatch.setattr(type(att), '_valid_rows', staticmethod(lambda *a: pytest.fail('_valid_rows on an fp16 cache')))
    cache = att.make_cache(2, sum(sizes) + 3, dtype='f16')
    copies = len(npm.sim.copies)
    outs, paths, spans = _chunks(att, x, sizes, cache)
    g = heads // kv_heads
    want_paths = ['fused_masked', 'decode', 'decode' if 3 * g <= 32 else 'fused_masked', 'fused_masked', 'decode']
    assert paths == want_paths
    for path, calls in zip(paths, spans):
        assert calls.count('npm_kv_append_f16') == 2 and not any(c in F32_CACHE_CALLS for c in calls)
        if path == 'decode':
            assert calls.count('npm_mha_decode_fwd_f16') == 1 and 'npm_kv_gather_f16' not in calls
        else:
            assert calls.count('npm_kv_gather_f16') == 2 and 'npm_mha_decode_fwd_f16' not in calls
            assert 'npm_mha_core_fwd' in calls or 'npm_mha_core_fwd_grouped' in calls
    assert len(npm.sim.copies) == copies                                  # no npm_d2d: neither _valid_rows nor a per-sequence copy
    stored = cache.gather(sum(sizes))
    assert np.array_equal(np.asarray(stored[0]), K16.rounded(np.asarray(stored[0])))          # halves, exactly
    for got, want in zip(outs, _stored_reference(p, x, sizes, stored, heads, kv_heads)):
        np.testing.assert_allclose(got, want, rtol=2e-6, atol=2e-6)
    # and the stored rows are the rounded projection: a fresh-projection path would have shown fp32 K / V to the first chunk
    kproj = DR._project(x.astype(np.float64), p['wk'], p['bk'])
    assert np.abs(np.asarray(stored[0]) - kproj).max() <= K16.U * np.abs(kproj).max() * 1.01 + 1e-5
    assert np.abs(np.asarray(stored[0]) - kproj).max() > 1e-5             # (not the unrounded projection)


def test_ragged_and_paged_f16_caches_route_the_same_way(npm):
    att, p = DC.make_mha(npm, 64, 4, 2, seed=4, batch=3)
    schedule = [np.array(n) for n in ([3, 37, 20], [1, 1, 1], [1, 0, 1], [40, 2, 33], [1, 1, 0])]
    total = VR.schedule_rows(schedule)
    rng = np.random.default_rng(1)
    x_rows = [rng.standard_normal([s, 64]).astype(np.float32) for s in total]
    runs = []
    for kwargs in ({}, dict(page_size=16)):
        cache = att.make_cache(3, int(total.max()) + 2, dtype='f16', **kwargs)
        first, copies = len(npm.sim.calls), len(npm.sim.copies)
        outs, paths = [], []
        for x, n in VR.padded_calls(x_rows, schedule):
            outs.append(np.asarray(att(x, cache=cache, new_lengths=n)))
            paths.append(att._cached_path)
        calls = npm.sim.calls[first:]
        assert paths == ['fused_masked', 'decode', 'decode', 'fused_masked', 'decode']
        assert calls.count('npm_kv_append_f16') == 10 and calls.count('npm_kv_gather_f16') == 4 and calls.count('npm_mha_decode_fwd_f16') == 3
        assert not any(c in F32_CACHE_CALLS for c in calls) and len(npm.sim.copies) == copies
        assert cache.lengths.tolist() == total.tolist()
        runs.append(outs)
    for a, b in zip(*runs):
        assert np.array_equal(a, b)                                       # paged == contiguous on the simulator too
    cache.release(1)                                                      # paged growth, release and re-admit work on top
    assert cache.lengths.tolist() == [int(total[0]), 0, int(total[2])]
    out = np.asarray(att(np.zeros([3, 2, 64], dtype=np.float32), cache=cache, new_lengths=[1, 2, 0]))
    assert att._cached_path == 'decode' and np.isfinite(out[0, :1]).all() and np.isfinite(out[1]).all()


def test_split_math_mode_runs_the_fused_forward_on_stored_rows(npm):
    from np_modeling_amd import _C
    att, _ = DC.make_mha(npm, 64, 4, 2, seed=5)
    cache = att.make_cache(2, 16, dtype='f16')
    x = np.random.default_rng(3).standard_normal([2, 4, 64]).astype(np.float32)
    att(x[:, :3], cache=cache)
    assert att._cached_path == 'decode'
    _C.set_math('bf16x3')
    try:
        first = len(npm.sim.calls)
        out = np.asarray(att(x[:, 3:], cache=cache))
        assert att._cached_path == 'fused_masked' and npm.sim.calls[first:].count('npm_kv_gather_f16') == 2
        assert 'npm_mha_decode_fwd_f16' not in npm.sim.calls[first:] and np.isfinite(out).all()
    finally:
        _C.set_math('f32')


def test_fill_cache_and_cross_attention_over_an_f16_cache(npm):
    att, p = DC.make_mha(npm, 64, 4, 2, seed=8, batch=3)
    rng = np.random.default_rng(4)
    kv = rng.standard_normal([3, 9, 64]).astype(np.float32)
    cache = att.fill_cache(att.make_cache(3, 9, dtype='f16'), kv, lengths=np.array([9, 2, 5]))
    assert cache.frozen and cache.lengths.tolist() == [9, 2, 5] and cache.dtype == 'f16'
    first = len(npm.sim.calls)
    out = np.asarray(att(rng.standard_normal([3, 4, 64]).astype(np.float32), cache=cache))
    assert att._cached_path == 'decode' and npm.sim.npm_last_decode_kernel().decode().endswith('causal=0 varlen=1 kv=f16')
    assert 'npm_kv_append_f16' not in npm.sim.calls[first:] and np.isfinite(out).all()
    # a uniform frozen cache shorter than the query: the uniform decode call does not take it, the gathered rows do
    short = att.fill_cache(att.make_cache(3, 9, dtype='f16'), kv[:, :2])
    out = np.asarray(att(rng.standard_normal([3, 4, 64]).astype(np.float32), cache=short))
    assert att._cached_path == 'fused_masked' and np.isfinite(out).all()


def test_start_decoding_builds_both_caches_in_f16(npm):
    f = 64
    dec, _ = DC.make_decoder(npm, f, 4, 2, 96, True, True, seed=9, batch=2)
    rng = np.random.default_rng(5)
    kv = rng.standard_normal([2, 7, f]).astype(np.float32)
    with pytest.raises(ValueError, match='cache_dtype'):
        dec.start_decoding(kv, 16, cache_dtype='half')
    sizes = {}
    for dtype in ('f32', 'f16'):
        for kwargs in ({}, dict(page_size=16)):
            state = dec.start_decoding(kv, 32, cache_dtype=dtype, **kwargs)
            assert state.self_cache.dtype == state.cross_cache.dtype == dtype
            assert state.self_cache.paged == bool(kwargs) and not state.cross_cache.paged
            sizes[dtype, bool(kwargs)] = (state.self_cache.nbytes, state.cross_cache.nbytes)
    for paged in (False, True):
        assert all(2 * half == full for half, full in zip(sizes['f16', paged], sizes['f32', paged]))
    state = dec.start_decoding(kv, 32, cache_dtype='f16')
    first = len(npm.sim.calls)
    q = rng.standard_normal([2, 6, f]).astype(np.float32)
    outs = [np.asarray(dec.decode(np.ascontiguousarray(piece), state)) for piece in DC.split(q, [3, 1, 1, 1])]
    calls = npm.sim.calls[first:]
    assert calls.count('npm_mha_decode_fwd_f16') == 8 and calls.count('npm_kv_append_f16') == 8
    assert not any(c in F32_CACHE_CALLS for c in calls) and state.position == 6
    whole = np.asarray(dec.decode(q, dec.start_decoding(kv, 32, cache_dtype='f16')))
    np.testing.assert_allclose(np.concatenate(outs, axis=1), whole, rtol=2e-5, atol=2e-5)


def _fp32_schedule(npm):
    """Ragged, uniform, paged and decoder calls with every new keyword left at its default: (calls, outputs).  Every device
    object dies here, before the simulator that owns its memory is uninstalled."""
    att, _ = DC.make_mha(npm, 64, 4, 2, seed=4, batch=3)
    dec, _ = DC.make_decoder(npm, 64, 4, 2, 96, True, True, seed=9, batch=3)
    first = len(npm.sim.calls)
    rng = np.random.default_rng(1)
    outs = []
    for kwargs in ({}, dict(page_size=16)):
        cache = att.make_cache(3, 50, **kwargs)
        for t, n in ((20, [3, 20, 7]), (1, None), (12, None), (1, [1, 0, 1])):
            outs.append(np.asarray(att(rng.standard_normal([3, t, 64]).astype(np.float32), cache=cache, new_lengths=n)))
        outs.extend(np.asarray(x) for x in cache.gather(int(cache.max_length)))
        state = dec.start_decoding(rng.standard_normal([3, 7, 64]).astype(np.float32), 32, **kwargs)
        for t in (5, 1, 1):
            outs.append(np.asarray(dec.decode(rng.standard_normal([3, t, 64]).astype(np.float32), state)))
    return list(npm.sim.calls[first:]), outs


def test_an_fp32_cache_makes_exactly_the_calls_it_made_before():
    """The same schedule on the simulator WITHOUT the new entry points and, with the keyword left at its default, on the one with
    them: the recorded call lists and the results are identical."""
    records = []
    for profile in ('prefill', 'kv16'):
        npm = activate(profile)
        try:
            assert hasattr(npm.sim, 'npm_kv_append_f16') == (profile == 'kv16')
            records.append(_fp32_schedule(npm))
        finally:
            deactivate()
    assert records[0][0] == records[1][0] and len(records[0][0]) > 50 and not any(c.endswith('_f16') for c in records[1][0])
    for a, b in zip(records[0][1], records[1][1]):
        assert np.array_equal(a, b, equal_nan=True)


# ---- the C ABI ------------------------------------------------------------------------------------------------------------------------
def test_f16_entry_points_header_against_bindings(built):
    _C = built
    text = open(os.path.join(ROOT, 'include', 'npm_hip.h')).read()
    assert 'NPM_ABI_VERSION 2' in re.sub(r'\s+', ' ', text)
    text = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    ctype = {'const npm_mha_decode *': ctypes.POINTER(_C.npm_mha_decode), 'const int32_t *': ctypes.c_void_p, 'const void *': ctypes.c_void_p,
             'void *': ctypes.c_void_p, 'const float *': ctypes.c_void_p, 'float *': ctypes.c_void_p, 'int64_t': ctypes.c_int64,
             'int32_t': ctypes.c_int32}
    lib = ctypes.CDLL(_C.LIB_PATH)
    for name, count in (('npm_mha_decode_fwd_f16', 6), ('npm_kv_append_f16', 14), ('npm_kv_gather_f16', 11)):
        args = re.search(r'\bint %s\((.*?)\);' % name, text, flags=re.S).group(1)
        want = [ctype[re.match(r'(.*?)(\w+)$', a.strip()).group(1).strip()] for a in args.split(',')]
        assert len(want) == count and _C.SIGNATURES[name] == want, (name, want, _C.SIGNATURES[name])
        assert hasattr(lib, name), f'{name} not exported'
    bound = _C.load_library()
    assert bound.npm_abi_version() == 2 and ctypes.sizeof(_C.npm_mha_decode) == 120
    count = ctypes.c_int(-1)
    bound.npm_device_count(ctypes.byref(count))
    if count.value == 0:                                                  # no compute without a GPU, as every entry point
        assert bound.npm_mha_decode_fwd_f16(ctypes.byref(_C.npm_mha_decode()), None, None, None, 0, 16) in (10001, 10002)
        assert bound.npm_kv_gather_f16(None, 0, 0, None, 1, 1, 8, None, None, 0, 16) == 10001
        assert bound.npm_kv_append_f16(None, 0, None, 0, 0, 1, 1, 8, 0, None, None, None, 0, 16) == 10001
