"""CPU: the half-precision weight copies (device.HalfWeights, npm_sgemm_skinny_w16) without a GPU, on the simulator of
tests/hostsim/ (profile 'w16').

* the ABI version is still 2; header, exports, ``_C.SIGNATURES`` and the simulator's support rule agree;
* a snapshot keeps adjacent sources adjacent: the packed q / k / v projection is ONE ``npm_sgemm_skinny_w16`` call over one half
  matrix, and a decode step is the six w16 products of tests/skinny_cases.py ``decode_products``;
* M > 64, ``SKINNY_GEMM`` off, a split math mode and a library without the entry point take ``npm_cvt_f16_f32`` + ``npm_sgemm``
  with array_equal outputs: the model with the rounded matrices at every M;
* a rebound parameter raises RuntimeError and ``refresh()`` repairs it; ``weights='bf16'`` and ``weights=`` without ``cache=``
  raise ValueError;
* without the keyword the call trace is, call for call, the trace on tests/hostsim/ (profile 'skinny');
* ``state.release`` / ``dec.admit`` leave the snapshot alone.
"""

import ctypes
import os
import re

import numpy as np
import pytest

import decode_cases as DC
import hostsim
from hostsim.fixtures import built, npm_fixture
import skinny_cases as SC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIX = (('_self_attention', '_wq'), ('_self_attention', '_wk'), ('_self_attention', '_wv'), ('_self_attention', '_wo'),
       ('_cross_attention', '_wq'), ('_cross_attention', '_wo'), ('_dense1._linear', '_w'), ('_dense2', '_w'))


npm = npm_fixture('w16')


def _gemms(calls):
    return [c for c in calls if c.startswith('npm_sgemm') or c.startswith('npm_cvt')]


def _round_six(dec):
    """The six matrices of a decode step replaced, in place, by their fp16-rounded values."""
    for path, attr in SIX:
        arr = getattr(DC.sub(dec, path), attr)
        arr.set(np.asarray(arr).astype(np.float16).astype(np.float32))


def _decode(npm, dec, q, kv, sizes, capacity=32, **kwargs):
    state = dec.start_decoding(kv, capacity, **kwargs)
    first = len(npm.sim.calls)
    outs = [np.asarray(dec.decode(np.ascontiguousarray(piece), state)) for piece in DC.split(q, sizes)]
    return outs, npm.sim.calls[first:], state


def _inputs(batch, tokens, f, seed, seq_kv=7):
    rng = np.random.default_rng(seed)
    return rng.standard_normal([batch, tokens, f]).astype(np.float32), rng.standard_normal([batch, seq_kv, f]).astype(np.float32)


def test_a_snapshot_keeps_packed_qkv_adjacent_and_the_projection_is_one_call(npm):
    f, heads, kv_heads = 64, 4, 2
    att, _ = DC.make_mha(npm, f, heads, kv_heads, seed=1, batch=2)
    assert att._params_adjacent()
    first = len(npm.sim.calls)
    hw = att.half_weights()
    assert all((att, name) in hw for name in ('_wq', '_wk', '_wv', '_wo')) and (att, '_bq') not in hw
    views = [hw.view(att, name) for name in ('_wq', '_wk', '_wv', '_wo')]
    assert views[1].ptr == views[0].ptr + 2 * att._wq.size and views[2].ptr == views[1].ptr + 2 * att._wk.size
    assert views[0]._keep is views[1]._keep is views[2]._keep and all(v.ptr % 16 == 0 for v in views)
    for name in ('_wq', '_wk', '_wv', '_wo'):
        assert np.array_equal(hw.numpy(att, name).view(np.uint16), np.asarray(getattr(att, name)).astype(np.float16).view(np.uint16))
    made = npm.sim.calls[first:]
    assert set(made) <= {'npm_cvt_f32_f16', 'npm_malloc', 'npm_d2h'} and 1 <= made.count('npm_cvt_f32_f16') <= 2
    x = np.random.default_rng(2).standard_normal([2, 3, f]).astype(np.float32)
    cache = att.make_cache(2, 8)
    first, before = len(npm.sim.calls), len(npm.sim.w16)
    got = np.asarray(att(x, cache=cache, weights=hw))
    assert _gemms(npm.sim.calls[first:]) == ['npm_sgemm_skinny_w16'] * 2
    width = f + 2 * (f // heads * kv_heads)
    assert npm.sim.w16[before:] == [('NT', 6, width, f, SC.EPI_BIAS, views[0].ptr), ('NT', 6, f, f, SC.EPI_BIAS, views[3].ptr)]
    assert npm._C.last_skinny_kernel().endswith(' w=f16')
    # the same layer with the four matrices rounded, without the keyword: the same numbers from the fp32 route
    twin, _ = DC.make_mha(npm, f, heads, kv_heads, seed=1, batch=2)
    for name in ('_wq', '_wk', '_wv', '_wo'):
        getattr(twin, name).set(np.asarray(getattr(twin, name)).astype(np.float16).astype(np.float32))
    want = np.asarray(twin(x, cache=twin.make_cache(2, 8)))
    assert np.array_equal(got, want) and not np.array_equal(got, np.asarray(att(x, cache=att.make_cache(2, 8))))
    assert not npm._C.last_skinny_kernel().endswith(' w=f16')


@pytest.mark.parametrize('packed', [True, False])
@pytest.mark.parametrize('norm_first', [True, False])
def test_a_decode_step_with_half_weights_is_six_w16_products_on_the_rounded_model(npm, monkeypatch, packed, norm_first):
    D = npm.device
    monkeypatch.setattr(D, 'PACK_QKV', packed)
    f, hidden, heads, kv_heads, batch = 64, 96, 4, 2, 3
    dec, _ = DC.make_decoder(npm, f, heads, kv_heads, hidden, norm_first, True, seed=3, batch=batch)
    q, kv = _inputs(batch, 6, f, seed=0)
    before = len(npm.sim.w16)
    got, calls, state = _decode(npm, dec, q, kv, [5, 1], weights='f16')
    count = 6 if packed else 8
    assert _gemms(calls) == ['npm_sgemm_skinny_w16'] * (2 * count) and isinstance(state.weights, D.HalfWeights)
    shapes = [c[:5] for c in npm.sim.w16[before:]]
    assert shapes == SC.decode_products(f, hidden, heads, kv_heads, batch * 5, packed) + SC.decode_products(f, hidden, heads, kv_heads, batch, packed)
    assert npm.sim.npm_last_skinny_kernel().decode().startswith('sgemm_skinny_kernel NN M=3 N=64 K=96 ')
    plain, plain_calls, plain_state = _decode(npm, dec, q, kv, [5, 1])
    assert plain_state.weights is None and _gemms(plain_calls) == ['npm_sgemm_skinny'] * (2 * count)
    _round_six(dec)
    want, _, _ = _decode(npm, dec, q, kv, [5, 1])
    for a, b, c in zip(got, want, plain):
        assert np.array_equal(a, b) and not np.array_equal(a, c)


def test_large_m_the_switch_a_split_math_mode_and_an_old_library_take_cvt_and_npm_sgemm(npm, monkeypatch):
    D = npm.device
    f = 64
    dec, _ = DC.make_decoder(npm, f, 4, 2, 96, True, True, seed=4, batch=5)
    q, kv = _inputs(5, 13, f, seed=1)
    assert 5 * 13 > 64 >= D.SKINNY_MAX_M
    twin, _ = DC.make_decoder(npm, f, 4, 2, 96, True, True, seed=4, batch=5)
    _round_six(twin)
    want_big, _, _ = _decode(npm, twin, q, kv, [13])
    want_small, _, _ = _decode(npm, twin, q[:2], kv[:2], [4, 1])

    def converted(outs, calls, want, steps):
        assert _gemms(calls) == ['npm_cvt_f16_f32', 'npm_sgemm'] * (6 * steps), _gemms(calls)
        assert all(np.array_equal(a, b) for a, b in zip(outs, want))

    first = len(npm.sim.cvt)
    outs, calls, state = _decode(npm, dec, q, kv, [13], weights='f16')            # M = 65
    converted(outs, calls, want_big, 1)
    back = npm.sim.cvt[first:]
    assert [c[0] for c in back] == ['npm_cvt_f32_f16'] * (len(back) - 6) + ['npm_cvt_f16_f32'] * 6
    assert back[-6][1:3] == (64 + 2 * 32, 64) and back[-6][3] == state.weights.view(dec._self_attention, '_wq').ptr    # packed: one conversion
    assert back[-2][1:3] == (64, 96) and back[-1][1:3] == (96, 64)                # dense1 [K, N], dense2 [K, N]
    with monkeypatch.context() as m:
        m.setattr(D, 'SKINNY_GEMM', False)
        converted(*_decode(npm, dec, q[:2], kv[:2], [4, 1], weights='f16')[:2], want_small, 2)
    npm.set_math('bf16x3')
    converted(*_decode(npm, dec, q[:2], kv[:2], [4, 1], weights='f16')[:2], want_small, 2)
    npm.set_math('f32')
    with monkeypatch.context() as m:                                              # a library with the conversions but no w16 GEMM
        m.setattr(D, '_w16_entry_points', lambda lib: False)
        converted(*_decode(npm, dec, q[:2], kv[:2], [4, 1], weights='f16')[:2], want_small, 2)
    outs, calls, _ = _decode(npm, dec, q[:2], kv[:2], [4, 1], weights='f16')
    assert _gemms(calls) == ['npm_sgemm_skinny_w16'] * 12 and all(np.array_equal(a, b) for a, b in zip(outs, want_small))
    # a shape the w16 kernel does not take (K = 40): the predicate says no, nothing is attempted, the halves are still what is used
    att40, _ = DC.make_mha(npm, 40, 2, 2, seed=8)
    hw = att40.half_weights()
    x = np.random.default_rng(9).standard_normal([2, 3, 40]).astype(np.float32)
    first = len(npm.sim.calls)
    got = np.asarray(att40(x, cache=att40.make_cache(2, 8), weights=hw))
    assert _gemms(npm.sim.calls[first:])[:2] == ['npm_cvt_f16_f32', 'npm_sgemm'] and 'npm_sgemm_skinny_w16' not in npm.sim.calls[first:]
    for name in ('_wq', '_wk', '_wv', '_wo'):
        getattr(att40, name).set(np.asarray(getattr(att40, name)).astype(np.float16).astype(np.float32))
    assert np.array_equal(got, np.asarray(att40(x, cache=att40.make_cache(2, 8))))
    assert npm.sim.npm_sgemm_skinny_w16(ctypes.byref(npm._C.npm_gemm())) == 10003


def test_a_rebound_parameter_raises_and_refresh_repairs_it(npm):
    D = npm.device
    f = 64
    dec, _ = DC.make_decoder(npm, f, 4, 2, 96, False, True, seed=5, batch=2)
    q, kv = _inputs(2, 3, f, seed=2)
    state = dec.start_decoding(kv, 16, weights='f16')
    dec.decode(q[:, :1], state)
    lin2 = dec._dense2
    values = np.asarray(lin2._w) * np.float32(0.5)
    lin2._w = values                                                     # a weight binder: a host array, moved to the device on use
    with pytest.raises(RuntimeError, match=r'Linear\._w was rebound'):
        dec.decode(q[:, 1:2], state)
    assert state.weights.refresh() is state.weights
    assert np.array_equal(state.weights.numpy(lin2, '_w'), values.astype(np.float16))
    dec.decode(q[:, 1:2], state)
    att = dec._self_attention
    hw = att.half_weights()
    att._wk = D.from_host(np.asarray(att._wk))                           # same values, another address; q / k / v no longer adjacent
    with pytest.raises(RuntimeError, match=r'MultiHeadAttention\._wk was rebound'):
        att(q, cache=att.make_cache(2, 8), weights=hw)
    hw.refresh()
    first = len(npm.sim.calls)
    att(q, cache=att.make_cache(2, 8), weights=hw)
    assert _gemms(npm.sim.calls[first:]) == ['npm_sgemm_skinny_w16'] * 4        # q, k, v on their own, and the output projection
    # a value change in place is not seen: the snapshot is of the weights as they were
    before = hw.numpy(att, '_wo').copy()
    att._wo.set(np.asarray(att._wo) * np.float32(2.0))
    hw.view(att, '_wo')
    assert np.array_equal(hw.numpy(att, '_wo'), before)
    assert np.array_equal(hw.refresh().numpy(att, '_wo'), np.asarray(att._wo).astype(np.float16))


def test_bad_keywords_raise_before_anything_is_launched(npm):
    f = 64
    dec, _ = DC.make_decoder(npm, f, 4, 2, 96, True, True, seed=6, batch=2)
    q, kv = _inputs(2, 3, f, seed=3)
    first = len(npm.sim.calls)
    for bad in ('bf16', 'f32', 16, True):
        with pytest.raises(ValueError, match='weights must be None or'):
            dec.start_decoding(kv, 16, weights=bad)
    att = dec._self_attention
    hw = att.half_weights()
    mark = len(npm.sim.calls)
    with pytest.raises(ValueError, match='needs cache='):
        att(q, weights=hw)
    assert len(npm.sim.calls) == mark and 'npm_sgemm' not in npm.sim.calls[first:]
    fresh = npm.layers.MultiHeadAttention(4)
    with pytest.raises(RuntimeError, match='no parameters yet'):
        fresh.half_weights()


def test_without_the_keyword_the_trace_is_the_one_of_the_skinny_simulator(npm):
    def trace(profile, **kwargs):
        sim = hostsim.install(profile)
        npm.sim = sim
        dec, _ = DC.make_decoder(npm, 64, 4, 2, 96, True, True, seed=7, batch=3)
        q, kv = _inputs(3, 9, 64, seed=4)
        att, _ = DC.make_mha(npm, 64, 4, 2, seed=8, batch=3)
        first = len(sim.calls)
        state = dec.start_decoding(kv, 32, page_size=16, **kwargs)
        outs = [np.asarray(dec.decode(np.ascontiguousarray(p), state)) for p in DC.split(q, [5, 1, 1, 2])]
        cache = att.make_cache(3, 16)
        outs.append(np.asarray(att(q[:, :4], cache=cache)))
        outs.append(np.asarray(att(q[:, 4:5], cache=cache)))
        return sim.calls[first:], outs

    old_calls, old_outs = trace('skinny')
    new_calls, new_outs = trace('w16')
    none_calls, none_outs = trace('w16', weights=None)
    assert new_calls == old_calls == none_calls and not any('w16' in c or 'cvt' in c for c in new_calls)
    assert all(np.array_equal(a, b) and np.array_equal(a, c) for a, b, c in zip(old_outs, new_outs, none_outs))
    assert npm.sim.w16 == [] and npm.sim.cvt == []


def test_release_and_admit_leave_the_snapshot_alone_and_the_memory_projection_stays_fp32(npm):
    f = 64
    dec, _ = DC.make_decoder(npm, f, 4, 2, 96, True, True, seed=9, batch=2)
    q, kv = _inputs(2, 3, f, seed=5)
    first = len(npm.sim.calls)
    state = dec.start_decoding(kv, 16, page_size=16, pages=4, weights='f16')
    started = npm.sim.calls[first:]
    assert started.count('npm_sgemm') == 2 and 'npm_sgemm_skinny_w16' not in started and 'npm_cvt_f16_f32' not in started   # wk, wv of the memory
    hw = state.weights
    assert (dec._cross_attention, '_wk') not in hw and (dec._cross_attention, '_wv') not in hw and (dec._norm1, '_gamma') not in hw
    snapshot = {key: (v.ptr, v._keep, hw.numpy(DC.sub(dec, key[0]), key[1]).copy()) for key in SIX for v in [hw.view(DC.sub(dec, key[0]), key[1])]}
    dec.decode(q[:, :2], state)
    state.release(1)
    mark = len(npm.sim.calls)
    dec.admit(state, 1, kv[:1, :4])
    admitted = npm.sim.calls[mark:]
    assert admitted.count('npm_sgemm') == 2 and not any('w16' in c or 'cvt' in c for c in admitted)
    dec.decode(q[:, 2:3], state, new_lengths=[1, 1])
    assert state.weights is hw
    for key in SIX:
        v = hw.view(DC.sub(dec, key[0]), key[1])
        assert (v.ptr, v._keep) == snapshot[key][:2] and np.array_equal(hw.numpy(DC.sub(dec, key[0]), key[1]), snapshot[key][2])


def test_a_snapshot_is_converted_with_the_pitched_conversions(npm):
    """device.HalfWeights through the simulator's conversions: what a snapshot stores is astype(float16) of its source, values that
    overflow or underflow included, and the conversions themselves are pitched and write nothing outside their columns."""
    sim = npm.sim
    lin = npm.layers.Linear(24)
    lin(np.zeros([2, 16], dtype=np.float32))
    values = (np.random.default_rng(1).standard_normal([16, 24]) * 300.0).astype(np.float32)
    values[0, :4] = (65504.0, 65519.99, 65520.0, 1e-8)
    lin._w.set(values)
    hw = npm.device.HalfWeights([(lin, '_w')])
    with np.errstate(over='ignore'):
        assert np.array_equal(hw.numpy(lin, '_w').view(np.uint16), values.astype(np.float16).view(np.uint16))
    assert sim.cvt[-1][:3] == ('npm_cvt_f32_f16', 16, 24)
    # the conversions: pitched, nothing outside the columns is written, empty calls are fine
    src = np.random.default_rng(0).standard_normal([5, 24]).astype(np.float32) * np.float32(300.0)
    src[0, :4] = (65504.0, 65519.99, 65520.0, 1e-8)
    dev = npm.device.from_host(src)
    half = npm.device.HalfBuffer([5, 16])
    assert sim.npm_cvt_f32_f16(dev.ptr, 24, half.ptr, 16, 5, 12) == 0
    with np.errstate(over='ignore'):
        assert np.array_equal(half.numpy()[:, :12].view(np.uint16), src[:, :12].astype(np.float16).view(np.uint16))
    back = npm.device.full([5, 20], 7.0)
    assert sim.npm_cvt_f16_f32(half.ptr, 16, back.ptr, 20, 5, 12) == 0
    host = np.asarray(back)
    assert np.array_equal(host[:, :12], half.numpy()[:, :12].astype(np.float32)) and (host[:, 12:] == 7.0).all()
    assert sim.npm_cvt_f32_f16(None, 0, None, 0, 0, 0) == 0 and sim.npm_cvt_f16_f32(None, 8, None, 8, 4, 0) == 0
    assert sim.npm_cvt_f32_f16(dev.ptr, 8, half.ptr, 16, 5, 12) == 10002 and sim.npm_cvt_f16_f32(None, 16, back.ptr, 20, 5, 12) == 10002


# ---- the C ABI -------------------------------------------------------------------------------------------------------------------
def test_w16_entry_points_header_against_bindings(built):
    _C = built
    text = open(os.path.join(ROOT, 'include', 'npm_hip.h')).read()
    assert int(re.search(r'#define\s+NPM_ABI_VERSION\s+(\d+)', text).group(1)) == 2
    code = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    gemm = ctypes.POINTER(_C.npm_gemm)
    p, i64 = ctypes.c_void_p, ctypes.c_int64
    for name, decl, want in (
            ('npm_sgemm_skinny_w16', r'int npm_sgemm_skinny_w16\(const npm_gemm \*g\);', [gemm]),
            ('npm_sgemm_skinny_w16_supported', r'int npm_sgemm_skinny_w16_supported\(const npm_gemm \*g\);', [gemm]),
            ('npm_cvt_f32_f16', r'int npm_cvt_f32_f16\(const float \*src, int64_t src_pitch, void \*dst, int64_t dst_pitch, int64_t rows, '
                                r'int64_t cols\);', [p, i64, p, i64, i64, i64]),
            ('npm_cvt_f16_f32', r'int npm_cvt_f16_f32\(const void \*src, int64_t src_pitch, float \*dst, int64_t dst_pitch, int64_t rows, '
                                r'int64_t cols\);', [p, i64, p, i64, i64, i64])):
        assert re.search(decl, code), name
        assert _C.SIGNATURES[name] == want
    lib = ctypes.CDLL(_C.LIB_PATH)
    for name in ('npm_sgemm_skinny_w16', 'npm_sgemm_skinny_w16_supported', 'npm_cvt_f32_f16', 'npm_cvt_f16_f32'):
        assert hasattr(lib, name), f'{name} not exported'
        assert name in hostsim.PROFILES['w16'] and name not in hostsim.PROFILES['skinny']
    bound = _C.load_library()
    assert bound.npm_abi_version() == 2
    assert bound.npm_sgemm_skinny_w16_supported(None) == 0 and bound.npm_sgemm_skinny_w16_supported(ctypes.byref(_C.npm_gemm())) == 0
    # the rule itself needs no device: the library and the simulator's restatement agree on every field the rule reads, one field
    # changed at a time from a call both take, for both layouts
    sim = hostsim.HostSim('w16')
    spare = 32768

    def base(trans_b):
        g = _C.npm_gemm()
        g.trans_a, g.trans_b, g.m, g.n, g.k, g.batch0, g.batch1 = 0, trans_b, 8, 32, 48, 1, 1
        g.a, g.lda, g.b, g.ldb, g.c, g.ldc = 4096, 48, 8192, 48, 16384, 32
        g.alpha, g.epilogue, g.bias, g.residual, g.ldr, g.aux, g.ldaux = 1.0, 0, spare, spare, 32, spare, 32
        return g

    changes = [('ldb', v) for v in (52, 56, 40, 32, 24, 44)] + [('b', 8192 + v) for v in (2, 4, 8, 16)] + [('b', None)] + \
        [('m', v) for v in (0, 1, 64, 65)] + [('n', v) for v in (16, 24, 40, 48, 0)] + [('k', v) for v in (16, 8, 24, 40, 64, 0)] + \
        [('lda', v) for v in (44, 50, 52, 56)] + [('ldc', v) for v in (28, 30, 34, 36)] + [('a', 4096 + 4), ('a', None), ('c', 16384 + 8), ('c', None)] + \
        [('epilogue', v) for v in (1, 2, 3, 4, 5, 7, 8, 16, 17, 19, 20, 32, 64, 128)] + [('trans_a', 1), ('trans_b', 2), ('batch0', 2), ('batch1', 0)] + \
        [('split_k', 2), ('colsum', spare), ('bsum', spare), ('asum', spare), ('rowdot', spare)]
    seen = set()
    for trans_b in (0, 1):
        g = base(trans_b)
        assert bound.npm_sgemm_skinny_w16_supported(ctypes.byref(g)) == sim.npm_sgemm_skinny_w16_supported(ctypes.byref(g)) == 1
        for field, value in changes:
            g = base(trans_b)
            setattr(g, field, value)
            for epilogue_field, bad in ((None, None), ('bias', spare + 4), ('bias', None), ('residual', spare + 8), ('ldr', 30), ('ldr', 28),
                                        ('aux', spare + 4), ('aux', None), ('ldaux', 34)):
                if epilogue_field is not None:
                    if field != 'epilogue':
                        continue
                    g = base(trans_b)
                    g.epilogue = value
                    setattr(g, epilogue_field, bad)
                says = bound.npm_sgemm_skinny_w16_supported(ctypes.byref(g))
                assert says == sim.npm_sgemm_skinny_w16_supported(ctypes.byref(g)), (trans_b, field, value, epilogue_field, bad)
                seen.add(says)
    assert seen == {0, 1}
    count = ctypes.c_int(-1)
    bound.npm_device_count(ctypes.byref(count))
    if count.value == 0:                                                  # no compute without a GPU, as every entry point
        assert bound.npm_sgemm_skinny_w16(ctypes.byref(_C.npm_gemm())) == 10001
        assert bound.npm_cvt_f32_f16(None, 0, None, 0, 0, 0) == 10001
