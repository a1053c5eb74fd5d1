"""CPU: ragged batches in the key / value cache (per-sequence lengths) without a GPU.

* the float64 restatement of tests/varlen_reference.py: a ragged batch equals every sequence run alone at batch 1, exactly;
* a float32 model of the split / combine rule with the partition taken from Lmax and per-sequence early exit stays under HALF of
  the bound tests/test_gpu_varlen.py applies (tests/test_gpu_decode.py's: ctx 2e-6 (1 + |ref|), lse 3e-6, grown by
  attn_range_data.exponent_tol) at every (lengths, D, splits) of that test's grid;
* the product's host logic on the simulator (tests/hostsim/ (profile 'varlen')): ``KVCache.lengths`` over ragged calls, overflow of one
  sequence raised before any call, ``length`` raising once ragged, ``reset``, a frozen cache with ``lengths``, the path each shape
  selects, uniform input recording exactly the scalar calls, NotImplementedError where only the GEMM composition is left, and
  ``TransformerDecoder.decode`` with ragged prompts followed by single-token steps;
* the three new entry points: header against bindings.

Every test names npm_*_varlen, ``lengths``, ``new_lengths``, ``kv_lengths`` or ``positions``: none exists without this feature.
"""

import ctypes
import os
import re

import numpy as np
import pytest

import attn_range_data as R
import decode_cases as DC
import decode_reference as DR
from hostsim.fixtures import built, npm_fixture
import varlen_reference as VR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the restatement ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('causal', [0, 1])
def test_ragged_batch_equals_every_sequence_alone_exactly(causal):
    rng = np.random.default_rng(causal)
    lengths, t = np.array([0 if not causal else 2, 1, 17, 40]), 5
    n = VR.new_lengths(t, lengths, causal, 0)
    q = rng.standard_normal([4, t, 6, 16])
    k, v = rng.standard_normal([4, 44, 3, 16]), rng.standard_normal([4, 44, 3, 16])
    k[np.arange(44)[None, :] >= lengths[:, None]] = np.nan                # nothing at or past a sequence's length is looked at
    v[np.arange(44)[None, :] >= lengths[:, None]] = np.nan
    q[np.arange(t)[None, :] >= n[:, None]] = np.nan                       # nor a padded query row
    ctx, lse = VR.decode_attention(q, k, v, lengths, n, 0.25, causal)
    seen = VR.valid_rows(t, lengths, n)
    assert seen.sum() and (~seen).sum()
    for b in range(4):
        rows = int(seen[b].sum())
        assert (ctx[b, rows:] == 0).all() and np.isneginf(lse[b, :, rows:]).all()
        if rows:
            alone_q = np.ascontiguousarray(q[b, :rows])[None]             # its own arrays: batch 1, no padding, its own capacity
            alone_k, alone_v = (np.ascontiguousarray(x[b, :lengths[b]])[None] for x in (k, v))
            want_ctx, want_lse = DR.decode_attention(alone_q, alone_k, alone_v, int(lengths[b]), 0.25, causal)
            assert np.array_equal(ctx[b, :rows], want_ctx[0]) and np.array_equal(lse[b, :, :rows], want_lse[0])
    assert np.isfinite(ctx).all()


def test_uniform_lengths_restate_the_uniform_reference():
    rng = np.random.default_rng(2)
    q, k, v = rng.standard_normal([3, 2, 4, 16]), rng.standard_normal([3, 9, 2, 16]), rng.standard_normal([3, 9, 2, 16])
    want = DR.decode_attention(q, k, v, 7, 0.25, True)
    got = VR.decode_attention(q, k, v, [7, 7, 7], None, 0.25, True)
    np.testing.assert_allclose(got[0], want[0], rtol=1e-14, atol=1e-14)
    np.testing.assert_allclose(got[1], want[1], rtol=1e-14, atol=1e-14)
    f32 = [x.astype(np.float32) for x in (q, k, v)]
    for splits in (1, 3):                                                 # and the float32 model is the uniform model, bit for bit
        a = VR.split_model(*f32, [7, 7, 7], None, 0.25, True, splits, 7)
        b = DR.split_model(*f32, 7, 0.25, True, splits)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


# ---- the split / combine rule in float32, partition from Lmax ------------------------------------------------------------------
def test_varlen_split_model_stays_under_half_of_the_gpu_bound():
    """Unit-normal inputs at every (lengths, n, D, splits, T, causal) of the GPU grid, Hq = 2 over Hkv = 1 (the error depends on
    neither the head count nor the pitch layout).  Bound: 2e-6 (1 + |ref|) on ctx, 3e-6 on lse, grown by tol(X)."""
    worst_ctx = worst_lse = 0.0
    done = set()
    for d, hq, hkv, t, causal, lengths, n, _, mode in VR.kernel_cases():
        lmax = int(lengths.max())
        for splits in {VR.split_count(mode, lmax, len(lengths), hkv), VR.split_count(mode, lmax, len(lengths), 1)}:
            key = (d, t, causal, tuple(lengths), tuple(n), splits)
            if key in done:
                continue
            done.add(key)
            rng = np.random.default_rng(d + t + splits + lmax)
            q = rng.standard_normal([len(lengths), t, 2, d]).astype(np.float32)
            k, v = (rng.standard_normal([len(lengths), max(lmax, 1), 1, d]).astype(np.float32) for _ in range(2))
            scale = 1.0 / np.sqrt(d)
            ctx, lse = VR.split_model(q, k, v, lengths, n, scale, causal, splits, lmax)
            want_ctx, want_lse = VR.decode_attention(q, k, v, lengths, n, scale, causal)
            seen = VR.valid_rows(t, lengths, n)
            assert (ctx[~seen] == 0).all() and np.isneginf(lse.transpose(0, 2, 1)[~seen]).all()
            for b in np.nonzero(seen.any(axis=1))[0]:
                rows = seen[b]
                x = R.exponent_magnitude(q[b:b + 1, rows], k[b:b + 1, :lengths[b]], scale, want_lse[b:b + 1, :, rows])
                frac_ctx = float((np.abs(ctx[b, rows] - want_ctx[b, rows]) / (R.exponent_tol(2e-6, x) * (1 + np.abs(want_ctx[b, rows])))).max())
                frac_lse = float(np.abs(lse[b][:, rows] - want_lse[b][:, rows]).max() / R.exponent_tol(3e-6, x))
                assert frac_ctx < 0.5 and frac_lse < 0.5, (key, b, frac_ctx, frac_lse)
                worst_ctx, worst_lse = max(worst_ctx, frac_ctx), max(worst_lse, frac_lse)
    print(f'varlen split model over {len(done)} cases: worst {worst_ctx:.3f} of the ctx bound, {worst_lse:.3f} of the lse bound')
    assert len(done) >= 100


def test_kernel_case_grid_covers_what_it_must():
    cases = VR.kernel_cases()
    assert {c[0] for c in cases} == set(VR.HEAD_DIMS) and {c[3] for c in cases} == set(VR.TOKENS) and {c[4] for c in cases} == {0, 1}
    assert {(c[1], c[2]) for c in cases} == set(VR.HEADS) and {c[8] for c in cases} == set(VR.SPLIT_MODES)
    lengths = set().union(*(set(c[5].tolist()) for c in cases))
    assert {0, 1, 15, 16, 17, 255, 256, 257} <= lengths and max(lengths) >= 2049
    assert any(0 in c[5] for c in cases if not c[4]) and not any(0 in c[5] for c in cases if c[4])
    for d, hq, hkv, t, causal, lens, n, _, _ in cases:
        assert (n >= 0).all() and (n <= t).all() and (not causal or (n <= lens).all())
    assert any({0, 1, c[3]} <= set(c[6].tolist()) for c in cases if c[3] > 1)
    assert any(c[5].max() >= 2049 and c[5].min() <= 1 for c in cases)


# ---- host logic on the simulator -----------------------------------------------------------------------------------------------
npm = npm_fixture('varlen')


def test_cache_lengths_bookkeeping_overflow_and_reset(npm):
    D = npm.device
    cache = D.KVCache(3, 6, 2, 16)
    assert cache.lengths.tolist() == [0, 0, 0] and cache.length == 0 and cache.max_length == 0 and not cache.ragged
    src = np.arange(3 * 4 * 32, dtype=np.float32).reshape(3, 4, 32)
    rows = D.from_host(src)
    cache.append(D.Mat(rows, 32), D.Mat(rows, 32), 4, new_lengths=[4, 1, 0])
    assert cache.lengths.tolist() == [4, 1, 0] and cache.max_length == 4 and cache.ragged
    assert npm.sim.calls.count('npm_kv_append_varlen') == 2 and 'npm_kv_append' not in npm.sim.calls
    with pytest.raises(ValueError, match='different numbers of rows'):
        cache.length
    got = np.asarray(cache.k).reshape(3, 6, 32)
    assert np.array_equal(got[0, :4], src[0]) and np.array_equal(got[1, :1], src[1, :1])
    assert np.isnan(got[1, 1:]).all() and np.isnan(got[2]).all()         # the simulator's poison: nothing else was written
    cache.append(D.Mat(rows, 32), D.Mat(rows, 32), 2, new_lengths=[0, 2, 1])
    assert cache.lengths.tolist() == [4, 3, 1]
    got = np.asarray(cache.k).reshape(3, 6, 32)
    flat = src.reshape(12, 32)                                           # read as [B * 2, 32]: sequence b's rows are 2 b, 2 b + 1
    assert np.array_equal(got[1, 1:3], flat[2:4]) and np.array_equal(got[2, :1], flat[4:5]) and np.isnan(got[2, 1:]).all()
    before = len(npm.sim.calls)
    with pytest.raises(ValueError, match='do not fit'):
        cache.append(D.Mat(rows, 32), D.Mat(rows, 32), 3, new_lengths=[3, 1, 1])       # 4 + 3 > 6 for sequence 0 alone
    with pytest.raises(ValueError, match='do not fit'):
        cache.append(D.Mat(rows, 32), D.Mat(rows, 32), 3)                               # the scalar form: sequence 0 again
    for bad in ([1, 1], [1, 1, 4], [-1, 0, 0], [0.5, 1, 1]):
        with pytest.raises(ValueError, match='new_lengths'):
            cache.room(3, bad)
    assert len(npm.sim.calls) == before and cache.lengths.tolist() == [4, 3, 1]        # raised before any call
    cache.append(D.Mat(rows, 32), D.Mat(rows, 32), 2)                    # a ragged cache takes a uniform chunk through the varlen call
    assert cache.lengths.tolist() == [6, 5, 3] and npm.sim.calls.count('npm_kv_append_varlen') == 6
    cache.reset()
    assert cache.lengths.tolist() == [0, 0, 0] and cache.length == 0 and not cache.frozen
    cache.length = 2                                                     # the scalar attribute still assigns
    assert cache.lengths.tolist() == [2, 2, 2] and cache.length == 2


def test_uniform_input_records_exactly_the_scalar_calls(npm):
    att, _ = DC.make_mha(npm, 64, 4, 2, seed=1)
    x = np.random.default_rng(0).standard_normal([2, 3, 64]).astype(np.float32)
    runs = []
    for kwargs in ({}, dict(new_lengths=[3, 3]), dict(new_lengths=np.array([3, 3]))):
        cache = att.make_cache(2, 8)
        first = len(npm.sim.calls)
        out = np.asarray(att(x, cache=cache, **kwargs))
        out2 = np.asarray(att(x[:, :1], cache=cache, **({} if not kwargs else dict(new_lengths=[1, 1]))))
        runs.append((npm.sim.calls[first:], out, out2, att._cached_path))
        assert cache.length == 4 and not cache.ragged
        assert npm.sim.npm_last_decode_kernel().decode().endswith('causal=1')
    assert 'npm_mha_decode_fwd' in runs[0][0] and not any('varlen' in c for r in runs for c in r[0])
    for other in runs[1:]:
        assert other[0] == runs[0][0] and np.array_equal(other[1], runs[0][1]) and np.array_equal(other[2], runs[0][2])
    with pytest.raises(ValueError, match='cache='):
        att(x, new_lengths=[3, 3])


def _ragged_layer_run(att, x_rows, schedule, capacity, pad=0.0):
    cache = att.make_cache(len(x_rows), capacity)
    outs, paths = [], []
    for x, n in VR.padded_calls(x_rows, schedule, pad):
        out = np.asarray(att(x, cache=cache, new_lengths=n))
        assert np.isfinite(out).all()
        outs.append(out)
        paths.append(att._cached_path)
    assert cache.lengths.tolist() == VR.schedule_rows(schedule).tolist()
    return VR.collect(outs, schedule, len(x_rows)), paths, cache


@pytest.mark.parametrize('heads,kv_heads,f', [(4, 4, 64), (8, 2, 128), (4, 1, 64)])
def test_layer_with_ragged_lengths_equals_every_sequence_alone(npm, heads, kv_heads, f):
    att, p = DC.make_mha(npm, f, heads, kv_heads, seed=heads, batch=3)
    schedule = [np.array(n) for n in ([3, 37, 20], [1, 1, 1], [1, 0, 1], [2, 0, 5], [1, 1, 0])]
    total = VR.schedule_rows(schedule)
    rng = np.random.default_rng(1)
    x_rows = [rng.standard_normal([s, f]).astype(np.float32) for s in total]
    want = VR.layer_alone(p, x_rows, schedule)
    g = heads // kv_heads
    for pad in (0.0, 7.5):                                               # what the padding holds does not matter
        got, paths, _ = _ragged_layer_run(att, x_rows, schedule, int(total.max()) + 2, pad)
        assert paths == ['decode' if g * int(n.max()) <= 32 else 'fused_masked' for n in schedule], paths
        assert paths[0] == 'fused_masked'
        for a, b in zip(got, want):
            np.testing.assert_allclose(a, b, rtol=2e-6, atol=2e-6)
    assert 'npm_mha_decode_fwd_varlen' in npm.sim.calls and 'npm_kv_append_varlen' in npm.sim.calls
    assert npm.sim.npm_last_decode_kernel().decode().endswith('causal=1 varlen=1')


def test_ragged_fused_path_gathers_zeros_behind_the_valid_rows(npm):
    """A second ragged chunk too large for the decode kernel: K / V come from npm_kv_gather_varlen, and what lies past a
    sequence's length in the cache (the simulator's NaN poison) reaches nothing."""
    att, p = DC.make_mha(npm, 64, 4, 1, seed=3, batch=2)                 # 4 T rows: T = 9 is too many
    schedule = [np.array(n) for n in ([2, 6], [9, 3], [1, 1])]
    rng = np.random.default_rng(2)
    x_rows = [rng.standard_normal([s, 64]).astype(np.float32) for s in VR.schedule_rows(schedule)]
    got, paths, cache = _ragged_layer_run(att, x_rows, schedule, 16)
    assert paths == ['decode', 'fused_masked', 'decode'] and npm.sim.calls.count('npm_kv_gather_varlen') == 2
    assert np.isnan(np.asarray(cache.k)[0, 12:]).all()
    for a, b in zip(got, VR.layer_alone(p, x_rows, schedule)):
        np.testing.assert_allclose(a, b, rtol=2e-6, atol=2e-6)


def test_ragged_lengths_on_the_gemm_path_are_not_implemented(npm):
    att12, _ = DC.make_mha(npm, 48, 4, 2, seed=6)                        # head size 12: the GEMM composition
    x = np.zeros([2, 3, 48], dtype=np.float32)
    cache = att12.make_cache(2, 8)
    before = len(npm.sim.calls)
    with pytest.raises(NotImplementedError, match='16, 32, 64, 128'):
        att12(x, cache=cache, new_lengths=[3, 1])
    assert len(npm.sim.calls) == before and cache.lengths.tolist() == [0, 0]
    att12(x, cache=cache, new_lengths=[3, 3])                            # uniform: the existing route
    assert att12._cached_path == 'gemm' and cache.length == 3


def test_frozen_cross_cache_with_memory_lengths(npm):
    att, p = DC.make_mha(npm, 64, 4, 2, seed=8, batch=3)
    rng = np.random.default_rng(4)
    kv = rng.standard_normal([3, 9, 64]).astype(np.float32)
    kv_lengths = np.array([9, 2, 5])
    cache = att.fill_cache(att.make_cache(3, 9), kv, lengths=kv_lengths)
    assert cache.frozen and cache.lengths.tolist() == [9, 2, 5] and cache.max_length == 9
    assert np.isnan(np.asarray(cache.k)[1, 2:]).all()                    # the padded memory rows were not stored
    for n in ([1, 1, 1], [4, 0, 2], [17, 3, 17]):                         # the last: 17 x 2 rows > 32, the fused masked forward
        n = np.array(n)
        x_rows = [rng.standard_normal([s, 64]).astype(np.float32) for s in n]
        (x, _), = VR.padded_calls(x_rows, [n])
        out = np.asarray(att(x, cache=cache, new_lengths=n))
        assert np.isfinite(out).all() and att._cached_path == ('decode' if n.max() <= 4 else 'fused_masked')
        assert cache.lengths.tolist() == [9, 2, 5]
        for got, want in zip(VR.collect([out], [n], 3), VR.cross_alone(p, x_rows, kv, kv_lengths)):
            np.testing.assert_allclose(got, want, rtol=2e-6, atol=2e-6)
    with pytest.raises(ValueError):
        att.fill_cache(att.make_cache(3, 4), kv, lengths=[4, 2, 5])       # 5 rows of sequence 2 do not fit 4
    with pytest.raises(ValueError, match='new_lengths'):
        att.fill_cache(att.make_cache(3, 9), kv, lengths=[10, 2, 5])      # more rows than the memory has
    same = att.fill_cache(att.make_cache(3, 9), kv, lengths=[9, 9, 9])    # uniform: the scalar route
    assert same.length == 9


@pytest.mark.parametrize('norm_first', [True, False])
@pytest.mark.parametrize('kv_heads', [None, 2])
def test_decoder_decode_with_ragged_prompts_then_single_tokens(npm, norm_first, kv_heads):
    f = 64
    dec, p = DC.make_decoder(npm, f, 4, kv_heads, 96, norm_first, True, seed=9, batch=3)
    schedule = [np.array(n) for n in ([11, 2, 6], [1, 1, 1], [1, 1, 0], [1, 0, 0], [1, 0, 1])]
    total = VR.schedule_rows(schedule)
    rng = np.random.default_rng(5)
    q_rows = [rng.standard_normal([s, f]).astype(np.float32) for s in total]
    kv = rng.standard_normal([3, 7, f]).astype(np.float32)
    kv_lengths = np.array([7, 3, 1])
    want = VR.decoder_alone(p, q_rows, schedule, kv, kv_lengths, norm_first)
    state = dec.start_decoding(kv, int(total.max()), kv_lengths=kv_lengths)
    assert state.positions.tolist() == [0, 0, 0] and state.position == 0
    outs = []
    for x, n in VR.padded_calls(q_rows, schedule):
        outs.append(np.asarray(dec.decode(x, state, new_lengths=n)))
        assert np.isfinite(outs[-1]).all()
    assert state.positions.tolist() == total.tolist() and state.cross_cache.lengths.tolist() == [7, 3, 1]
    with pytest.raises(ValueError, match='different numbers of rows'):
        state.position
    for got, ref in zip(VR.collect(outs, schedule, 3), want):
        np.testing.assert_allclose(got, ref, rtol=1e-5, atol=1e-5)
    before = len(npm.sim.calls)
    with pytest.raises(ValueError, match='do not fit'):
        dec.decode(np.zeros([3, 1, f], dtype=np.float32), state, new_lengths=[1, 0, 0])   # sequence 0 is full
    assert len(npm.sim.calls) == before and state.positions.tolist() == total.tolist()


# ---- the C ABI -----------------------------------------------------------------------------------------------------------------
def test_varlen_entry_points_header_against_bindings(built):
    _C = built
    text = open(os.path.join(ROOT, 'include', 'npm_hip.h')).read()
    text = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    ctype = {'const npm_mha_decode *': ctypes.POINTER(_C.npm_mha_decode), 'const int32_t *': ctypes.c_void_p,
             'const float *': ctypes.c_void_p, 'float *': ctypes.c_void_p, 'int64_t': ctypes.c_int64, 'int32_t': ctypes.c_int32}
    lib = ctypes.CDLL(_C.LIB_PATH)
    for name, count in (('npm_mha_decode_fwd_varlen', 3), ('npm_kv_append_varlen', 10), ('npm_kv_gather_varlen', 8)):
        args = re.search(r'\bint %s\((.*?)\);' % name, text, flags=re.S).group(1)
        want = []
        for arg in (a.strip() for a in args.split(',')):
            kind = re.match(r'(.*?)(\w+)$', arg).group(1).strip()
            want.append(ctype[kind])
        assert len(want) == count and _C.SIGNATURES[name] == want, (name, want, _C.SIGNATURES[name])
        assert hasattr(lib, name), f'{name} not exported'
    bound = _C.load_library()
    assert bound.npm_abi_version() == 2
    count = ctypes.c_int(-1)
    bound.npm_device_count(ctypes.byref(count))
    if count.value == 0:                                                  # no compute without a GPU, as every entry point
        assert bound.npm_mha_decode_fwd_varlen(ctypes.byref(_C.npm_mha_decode()), None, None) in (10001, 10002)
        assert bound.npm_kv_gather_varlen(None, 0, 0, None, 1, 1, 4, None) == 10001
