"""GPU: incremental decoding -- npm_mha_decode_fwd / npm_kv_append (csrc/npm_decode.hip) through the C ABI against the float64
reference of tests/decode_reference.py, then MultiHeadAttention with a cache and TransformerDecoder(causal=True) / decode.

Bounds.  Kernel: those tests/test_gpu_attn.py holds the fused forward to on unit-scale inputs -- ctx |got - ref| <= 2e-6 (1 + |ref|),
lse within 3e-6 -- grown by tests/attn_range_data.py's rule tol(X) = tol0 max(1, X / 32) for large scores (X: magnitude, in log2
units, of the operands of the kernel's exponents).  tests/test_decode_host.py shows that a float32 model of the split / combine
rule stays under half of these at the same (L, D, splits).  Every element of every case is compared, behind every output lies
a guard region that must keep its sentinel, and every case asserts through npm_last_decode_kernel() which kernel, row count and
split count ran.

Every test here touches npm_mha_decode_fwd, npm_kv_append, KVCache, ``cache=``, ``causal=`` or ``decode``: none of them exists
without this feature, so all of them fail on the parent commit.
"""

import ctypes as C
import itertools

import numpy as np
import pytest

import attn_range_data as R
import decode_gpu
import decode_reference as DR
import gqa_reference as G
from decode_gpu import GUARD, NT_KNOB, SENTINEL, SPLITS_KNOB
from decode_gpu import guarded as _guarded, layer_close as _layer_close
from oracle import np_oracle as O

pytestmark = pytest.mark.gpu

HEAD_DIMS = (16, 32, 64, 128)
HEADS = ((8, 8), (8, 4), (8, 2), (8, 1), (6, 3), (1, 1))
TOKENS = (1, 2, 5, 16)
MAX_ROWS = 32
# (L, B): the long caches with one sequence, the large batch with short ones; L < T becomes T
LENGTHS = ((0, 1), (7, 3), (127, 64), (128, 1), (129, 3), (2049, 1), (16405, 1), (0, 64), (7, 1), (127, 3), (128, 64), (129, 1),
           (2049, 3), (0, 3), (7, 64), (129, 64), (128, 3), (127, 1))
SPLIT_MODES = ('one', 'auto', 'many', 2, 'auto', 32)


@pytest.fixture(scope='module')
def npm():
    import np_modeling_amd
    return np_modeling_amd


@pytest.fixture(autouse=True)
def _defaults_afterwards(npm):
    yield
    decode_gpu.reset_knobs()


def _set_splits(mode, length):
    """Applies a split mode; returns the split count the call must report (None: automatic, read back through the ABI)."""
    from np_modeling_amd import _C
    tiles = (length + 15) // 16
    value = {'one': 1, 'auto': 0, 'many': min(tiles + 3, 1024)}.get(mode, mode)
    _C.check(_C.lib().npm_set_tuning(SPLITS_KNOB, int(value)), 'npm_set_tuning')
    return int(value) or None


def _run(q, k, v, length, scale, causal, packed=False, want_lse=True, expect=0):
    """q [B, T, Hq, D], k / v [B, capacity, Hkv, D] host arrays (float32) -> ctx, lse, kernel string.  ``packed``: q sits in a
    [B, T, Hq + 2 Hkv, D] buffer (pitch of the layer's packed projection) and the cache rows carry 4 floats of padding."""
    from np_modeling_amd import _C, device as D
    b, t, hq, d = q.shape
    cap, hkv = k.shape[1], k.shape[2]
    if packed:
        qp = hq * d + 2 * hkv * d
        qbuf = np.full([b, t, qp], np.nan, dtype=np.float32)
        qbuf[:, :, :hq * d] = q.reshape(b, t, hq * d)
        kp = hkv * d + 4
        kbuf, vbuf = (np.full([b, cap, kp], np.nan, dtype=np.float32) for _ in range(2))
        kbuf[:, :, :hkv * d], vbuf[:, :, :hkv * d] = k.reshape(b, cap, hkv * d), v.reshape(b, cap, hkv * d)
    else:
        qp, kp, qbuf, kbuf, vbuf = hq * d, hkv * d, q, k, v
    qd, kd, vd = D.from_host(qbuf), D.from_host(kbuf), D.from_host(vbuf)
    ctx = D.full([b * t * hq * d + GUARD], SENTINEL)
    lse = D.full([b * hq * t + GUARD], SENTINEL)
    c = _C.npm_mha_decode()
    c.batch, c.heads, c.kv_heads, c.new_tokens, c.kv_len, c.head_dim = b, hq, hkv, t, length, d
    c.causal, c.scale = int(causal), scale
    c.q, c.q_pitch = qd.ptr, qp
    c.k, c.k_pitch, c.k_stride_b = kd.ptr, kp, cap * kp
    c.v, c.v_pitch, c.v_stride_b = vd.ptr, kp, cap * kp
    c.ctx, c.ctx_pitch = ctx.ptr, hq * d
    c.lse = lse.ptr if want_lse else None
    rc = _C.lib().npm_mha_decode_fwd(C.byref(c))
    if expect:
        assert rc == expect, (rc, _C.lib().npm_last_error())
        assert b'npm_mha_decode_fwd:' in _C.lib().npm_last_error(), 'the error names the entry point that was called'
        return None
    _C.check(rc, 'npm_mha_decode_fwd')
    out_ctx = _guarded(ctx, b * t * hq * d).reshape(b, t, hq, d)
    out_lse = _guarded(lse, b * hq * t).reshape(b, hq, t) if want_lse else None
    if not want_lse:
        np.testing.assert_array_equal(lse.numpy(), SENTINEL)
    return out_ctx, out_lse, _C.last_decode_kernel()


def _check(got_ctx, got_lse, q, k, v, length, scale, causal, what, grow=1.0):
    """Every element of ctx and lse against float64 at tol(X); prints the fraction of the bound used."""
    want_ctx, want_lse = DR.decode_attention(q, k, v, length, scale, causal)
    x = R.exponent_magnitude(q, k[:, :length], scale, want_lse)
    tol_ctx, tol_lse = R.exponent_tol(2e-6, x) * grow, R.exponent_tol(3e-6, x) * grow
    assert np.isfinite(got_ctx).all() and np.isfinite(got_lse).all(), f'{what}: not finite'
    frac_ctx = float((np.abs(got_ctx.astype(np.float64) - want_ctx) / (tol_ctx * (1.0 + np.abs(want_ctx)))).max())
    frac_lse = float(np.abs(got_lse.astype(np.float64) - want_lse).max() / tol_lse)
    print(f'{what}: X={x:.1f} ctx {frac_ctx:.3f} of {tol_ctx:.2e}(1+|ref|), lse {frac_lse:.3f} of {tol_lse:.2e}')
    assert frac_ctx <= 1.0, f'{what}: ctx {frac_ctx:.3g} of the bound {tol_ctx:.3g}'
    assert frac_lse <= 1.0, f'{what}: lse {frac_lse:.3g} of the bound {tol_lse:.3g}'


def _data(seed, b, t, hq, hkv, d, cap):
    rng = np.random.default_rng(seed)
    q = rng.standard_normal([b, t, hq, d]).astype(np.float32)
    k = rng.standard_normal([b, cap, hkv, d]).astype(np.float32)
    v = rng.standard_normal([b, cap, hkv, d]).astype(np.float32)
    return q, k, v


def _cases():
    """Every (D, heads, T, causal) the kernel takes, each with a cache length / batch, a pitch layout and a split mode drawn
    round robin, so that every value of every axis meets every other axis' values many times."""
    out, i = [], 0
    for d, (hq, hkv), t, causal in itertools.product(HEAD_DIMS, HEADS, TOKENS, (0, 1)):
        if hq // hkv * t > MAX_ROWS:
            continue
        length, b = LENGTHS[(i * 7 + i // len(LENGTHS)) % len(LENGTHS)]
        out.append(pytest.param(d, hq, hkv, t, causal, max(length, t), b, bool((i // 2) % 2), SPLIT_MODES[(i * 5 + i // 6) % 6],
                                id=f'D{d}-H{hq}/{hkv}-T{t}-c{causal}-L{max(length, t)}-B{b}-{"packed" if (i // 2) % 2 else "plain"}-'
                                   f'{SPLIT_MODES[(i * 5 + i // 6) % 6]}'))
        i += 1
    return out


def test_case_grid_covers_every_axis_value():
    seen = [set() for _ in range(9)]
    for case in _cases():
        for axis, value in zip(seen, case.values):
            axis.add(value)
    assert seen[0] == set(HEAD_DIMS) and seen[3] == set(TOKENS) and seen[4] == {0, 1}
    assert {(hq, hkv) for hq, hkv in HEADS} == {(c.values[1], c.values[2]) for c in _cases()}
    assert {7, 127, 128, 129, 2049, 16405} <= seen[5] and seen[6] == {1, 3, 64} and seen[7] == {False, True}
    assert seen[8] == set(SPLIT_MODES)


@pytest.mark.parametrize('d,hq,hkv,t,causal,length,b,packed,mode', _cases())
def test_kernel_against_float64(npm, d, hq, hkv, t, causal, length, b, packed, mode):
    from np_modeling_amd import _C
    cap = length + 3
    q, k, v = _data(d * 1000 + hq * 100 + t * 10 + causal + length, b, t, hq, hkv, d, cap)
    k[:, length:], v[:, length:] = np.nan, np.nan                        # nothing past the valid length may matter
    scale = 1.0 / np.sqrt(d)
    forced = _set_splits(mode, length)
    splits = forced or _C.lib().npm_mha_decode_splits(b, hkv, length)
    assert forced or splits == DR.auto_splits(b, hkv, length)
    ctx, lse, kernel = _run(q, k, v, length, scale, causal, packed=packed)
    assert kernel == f'mha_decode_kernel D={d} rows={hq // hkv * t} splits={splits} causal={causal}'
    _check(ctx, lse, q, k, v, length, scale, causal, kernel + f' L={length} B={b}')


@pytest.mark.parametrize('hq,hkv,t', [(8, 1, 5), (8, 2, 16), (8, 1, 16), (64, 1, 1)])
def test_more_rows_than_the_kernel_takes_is_unsupported(npm, hq, hkv, t):
    from np_modeling_amd import _C
    assert hq // hkv * t > MAX_ROWS and not _C.lib().npm_mha_decode_supported(64, hq // hkv * t)
    q, k, v = _data(1, 1, t, hq, hkv, 64, 40)
    _run(q, k, v, 40, 0.125, 1, expect=10003)


def test_unsupported_head_size_and_bad_arguments(npm):
    from np_modeling_amd import _C
    lib = _C.lib()
    assert [d for d in range(1, 200) if lib.npm_mha_decode_supported(d, 1)] == list(HEAD_DIMS)
    assert lib.npm_mha_decode_supported(128, MAX_ROWS) and not lib.npm_mha_decode_supported(128, 0)
    q, k, v = _data(2, 1, 2, 4, 2, 24, 8)
    _run(q, k, v, 8, 0.2, 1, expect=10003)                             # head size 24
    q, k, v = _data(3, 1, 4, 4, 2, 32, 8)
    _run(q, k, v, 3, 0.2, 1, expect=10002)                             # kv_len < new_tokens
    q, k, v = _data(4, 1, 1, 6, 4, 32, 8)
    _run(q, k, v, 8, 0.2, 1, expect=10002)                             # heads % kv_heads


@pytest.mark.parametrize('poison', [np.nan, 1e30])
@pytest.mark.parametrize('d,hq,hkv,t,length,mode', [(128, 8, 2, 1, 129, 'auto'), (64, 8, 8, 5, 2049, 'auto'), (32, 6, 3, 2, 7, 'one'),
                                                    (16, 8, 1, 2, 127, 'many'), (128, 8, 1, 4, 300, 4)])
def test_rows_past_the_valid_length_never_matter(npm, d, hq, hkv, t, length, mode, poison):
    """Cache rows at and past L filled with NaN / 1e30: finite output, bitwise equal to the run with zeros there and to the run
    on a cache of a larger capacity."""
    q, k, v = _data(5 + d + t, 3, t, hq, hkv, d, length + 37)
    scale = 1.0 / np.sqrt(d)
    runs = []
    for fill, extra in ((0.0, 37), (poison, 37), (poison, 5)):
        kk, vv = k[:, :length + extra].copy(), v[:, :length + extra].copy()
        kk[:, length:], vv[:, length:] = fill, fill
        _set_splits(mode, length)
        runs.append(_run(q, kk, vv, length, scale, 1))
    assert np.isfinite(runs[1][0]).all() and np.isfinite(runs[1][1]).all()
    for other in runs[1:]:
        assert np.array_equal(runs[0][0], other[0]) and np.array_equal(runs[0][1], other[1]) and runs[0][2] == other[2]
    _check(runs[1][0], runs[1][1], q, k, v, length, scale, 1, f'poison {poison} D={d}')


@pytest.mark.parametrize('nt', [0, 1, 2])
@pytest.mark.parametrize('d,hq,hkv,t,length,b', [(128, 8, 2, 1, 8192, 2), (64, 8, 4, 2, 2049, 3), (16, 8, 8, 16, 129, 64)])
def test_same_call_twice_is_bitwise_equal_and_load_policy_does_not_change_results(npm, d, hq, hkv, t, length, b, nt):
    from np_modeling_amd import _C
    q, k, v = _data(9 + d, b, t, hq, hkv, d, length)
    _C.check(_C.lib().npm_set_tuning(NT_KNOB, 2), 'npm_set_tuning')            # plain loads
    base = _run(q, k, v, length, 1.0 / np.sqrt(d), 1)
    _C.check(_C.lib().npm_set_tuning(NT_KNOB, nt), 'npm_set_tuning')
    for _ in range(2):
        again = _run(q, k, v, length, 1.0 / np.sqrt(d), 1)
        assert np.array_equal(base[0], again[0]) and np.array_equal(base[1], again[1])


@pytest.mark.parametrize('mode', ['one', 'auto', 'many', 3])
@pytest.mark.parametrize('d,hq,hkv,t', [(128, 8, 2, 4), (64, 8, 8, 16), (32, 6, 3, 5), (16, 8, 1, 1)])
def test_shifted_and_saturated_scores(npm, d, hq, hkv, t, mode):
    """attn_range_data's +-200 shift and its saturated (nearly one-hot) scores; rows whose maximum sits in the last split; rows
    whose maximum sits in keys a causal row cannot see."""
    length, b = 700, 2
    scale = 1.0 / np.sqrt(d)
    q, _, v, _, _, ku, _ = R.shift_problem(b, hq, hkv, t, length, d, seed=d + t)
    _set_splits(mode, length)
    ctx, lse, kernel = _run(q, ku, v, length, scale, 1)
    _check(ctx, lse, q, ku, v, length, scale, 1, f'shift {kernel}')
    q, k, v, _, _ = R.saturated_problem(b, hq, hkv, t, length, d, seed=d + t + 1)
    k[:, -2] = 3.0 * np.sign(q[:, 0, :hkv])                              # the largest scores of token 0 sit in the last split, at keys
    k[:, -1] = 6.0 * np.sign(q[:, 0, :hkv])                              # that (causal, T > 1) token 0 cannot see
    _set_splits(mode, length)
    for causal in (0, 1):
        ctx, lse, kernel = _run(q, k, v, length, scale, causal)
        _check(ctx, lse, q, k, v, length, scale, causal, f'saturated {kernel}')


def test_lse_is_optional(npm):
    q, k, v = _data(11, 2, 2, 8, 4, 64, 300)
    for mode in ('one', 5):
        _set_splits(mode, 300)
        with_lse = _run(q, k, v, 300, 0.125, 1)
        without = _run(q, k, v, 300, 0.125, 1, want_lse=False)
        assert np.array_equal(with_lse[0], without[0])


# ---- npm_kv_append -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('b,t,hkv,d,cap,at', [(3, 5, 2, 16, 40, 0), (3, 5, 2, 16, 40, 35), (1, 1, 8, 128, 9, 4), (64, 7, 1, 32, 7, 0),
                                              (2, 129, 3, 64, 300, 171)])
@pytest.mark.parametrize('packed', [False, True])
def test_kv_append_is_exact(npm, b, t, hkv, d, cap, at, packed):
    from np_modeling_amd import _C, device as D
    rng = np.random.default_rng(b + t + at)
    row = hkv * d
    pitch = 3 * row + 8 * d if packed else row                           # the K part of a packed [B, T, Hq + 2 Hkv, D] projection
    offset = 8 * d if packed else 0
    src = rng.standard_normal([b * t, pitch]).astype(np.float32)
    before = rng.standard_normal([b, cap, row]).astype(np.float32)
    sd = D.from_host(src)
    cache = D.full([b * cap * row + GUARD], SENTINEL)
    cache.flat_view(0, [b * cap * row]).set(before.ravel())
    _C.check(_C.lib().npm_kv_append(sd.ptr + 4 * offset, pitch, cache.ptr, row, cap * row, b, t, row, at), 'npm_kv_append')
    got = _guarded(cache, b * cap * row).reshape(b, cap, row)
    want = before.copy()
    want[:, at:at + t] = src.reshape(b, t, pitch)[:, :, offset:offset + row]
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


def test_kv_append_rejects_misaligned_arguments(npm):
    from np_modeling_amd import _C, device as D
    src, cache = D.zeros([64]), D.zeros([256])
    lib = _C.lib()
    assert lib.npm_kv_append(src.ptr, 16, cache.ptr, 16, 64, 1, 2, 14, 0) == 10002        # row_len % 4
    assert lib.npm_kv_append(src.ptr + 4, 16, cache.ptr, 16, 64, 1, 2, 16, 0) == 10002     # pointer alignment
    assert lib.npm_kv_append(src.ptr, 18, cache.ptr, 16, 64, 1, 2, 16, 0) == 10002         # pitch % 4
    assert lib.npm_kv_append(src.ptr, 16, cache.ptr, 16, 64, 1, 2, 16, 0) == 0


# ---- MultiHeadAttention with a cache -----------------------------------------------------------------------------------------
# A float32 evaluation of attention + the two projections at O(1) activations stays within 1e-5 (|ref| + max |ref|) of float64:
# the bound tests/test_gpu_gqa.py and tests/test_gpu_attn.py hold the layer's forward to.  Comparing two float32 evaluations
# (the cached path and the fused forward on the whole sequence) allows the sum of the two.
LAYER_TOL = 1e-5


@pytest.mark.parametrize('heads,kv_heads,f', [(8, 8, 1024), (8, 2, 1024), (8, 1, 512), (4, 4, 64), (6, 3, 192), (4, 2, 48)])
def test_layer_with_cache_against_float64_and_the_fused_causal_forward(npm, heads, kv_heads, f):
    """Chunked cached self-attention against (a) the float64 reference and (b) the existing fused forward with a causal mask on
    the whole sequence; head sizes 128, 64, 16, 32 and one fallback size (Dk 12: the GEMM composition)."""
    import decode_cases as DC
    from np_modeling_amd import _C
    att, p = DC.make_mha(npm, f, heads, kv_heads, seed=heads + f)
    s, dk, g = 37, f // heads, heads // kv_heads
    x = np.random.default_rng(f).standard_normal([2, s, f]).astype(np.float32)
    want, _ = DR.att_fwd(p, x.astype(np.float64), mask=DR.causal_mask(s))
    fused = None
    if dk in HEAD_DIMS:
        fused = np.asarray(att(x, mask=DR.causal_mask(s)))
        assert _C.last_attn_kernel().startswith('mha_fwd') and 'mask=1' in _C.last_attn_kernel()
        _layer_close(fused, want, LAYER_TOL, f'fused causal forward H{heads}/{kv_heads} D{dk}')
    for sizes in DC.chunkings(s):
        got, paths = DC.run_mha_chunks(att, x, sizes, capacity=s + 11)
        expect = ['gemm' if dk not in HEAD_DIMS else 'decode' if g * t <= MAX_ROWS else 'fused_masked' for t in sizes]
        assert paths == expect, (paths, expect)
        if paths[-1] == 'decode':
            assert _C.last_decode_kernel().startswith(f'mha_decode_kernel D={dk} rows={g * sizes[-1]} ') and \
                _C.last_decode_kernel().endswith('causal=1')
        _layer_close(got, want, LAYER_TOL, f'cached H{heads}/{kv_heads} D{dk} chunks {sizes[:4]}')
        if fused is not None:
            _layer_close(got, fused, 2 * LAYER_TOL, f'cached vs fused H{heads}/{kv_heads} D{dk} chunks {sizes[:4]}')
    with pytest.raises(RuntimeError, match='inference only'):
        att(x, backprop=True, learning_rate=1e-3)


def test_layer_cross_attention_over_a_frozen_cache(npm):
    import decode_cases as DC
    att, p = DC.make_mha(npm, 256, 8, 2, seed=3)
    rng = np.random.default_rng(8)
    kv = rng.standard_normal([3, 50, 256]).astype(np.float32)
    cache = att.fill_cache(att.make_cache(3, 64), kv)                     # capacity larger than what is filled
    for t in (1, 4, 70):                                                   # 70 > L: not the decode kernel's contract
        x = rng.standard_normal([3, t, 256]).astype(np.float32)
        got = np.asarray(att(x, cache=cache))
        want, _ = DR.att_fwd(p, x.astype(np.float64), kv.astype(np.float64), kv.astype(np.float64))
        assert att._cached_path == ('decode' if t <= 50 and 4 * t <= MAX_ROWS else 'fused_masked') and cache.length == 50
        _layer_close(got, want, LAYER_TOL, f'cross T={t}')


def test_layer_cache_overflow_raises_before_any_launch(npm):
    import decode_cases as DC
    att, _ = DC.make_mha(npm, 64, 4, 2, seed=4)
    cache = att.make_cache(2, 5)
    att(np.zeros([2, 4, 64], dtype=np.float32), cache=cache)
    before = np.asarray(cache.k).copy()
    with pytest.raises(ValueError):
        att(np.ones([2, 2, 64], dtype=np.float32), cache=cache)
    assert cache.length == 4 and np.array_equal(np.asarray(cache.k)[:, :4], before[:, :4])


# ---- TransformerDecoder: causal=True, decode -----------------------------------------------------------------------------------
@pytest.mark.parametrize('norm_first', [True, False])
@pytest.mark.parametrize('kv_heads', [None, 2])
def test_causal_decoder_forward_backward_and_decode(npm, norm_first, kv_heads):
    """causal=True forward and backward against the float64 restatement (output, both input gradients, all 26 parameter
    gradients) at the bound tests/test_gpu_encoder.py holds the unmasked decoder to (1e-4); fused equals unfused at that file's
    3e-6 / 1e-5; then ``decode`` in chunks against ``forward``."""
    import decode_cases as DC
    from np_modeling_amd import parallel
    from conftest import assert_close
    D = npm.device
    f, s = 256, 45
    dec, p = DC.make_decoder(npm, f, 4, kv_heads, 384, norm_first, True, seed=11, batch=3, seq_kv=23)
    rng = np.random.default_rng(12)
    q, kv, dy = (rng.standard_normal(shape).astype(np.float32) for shape in ([3, s, f], [3, 23, f], [3, s, f]))
    want, c = DR.decoder_fwd(p, q.astype(np.float64), kv.astype(np.float64), norm_first, mask=DR.causal_mask(s))
    (want_dq, want_dkv), want_g = DR.decoder_bwd(p, c, dy.astype(np.float64), norm_first)
    unmasked, _ = DR.decoder_fwd(p, q.astype(np.float64), kv.astype(np.float64), norm_first)
    assert np.abs(unmasked - want).max() > 1e-2                            # the mask matters
    out = np.asarray(dec(q, kv))
    assert dec._fused and dec._self_attention._mask is dec._causal_masks[(3, s)]
    assert_close(out, want, tol=1e-4, what='out')
    rec = DC.GradRecorder()
    dq, dkv = (np.asarray(g) for g in dec(dy, backprop=True, optimizer_=rec))
    assert_close(dq, want_dq, tol=1e-4, what='dq')
    assert_close(dkv, want_dkv, tol=1e-4, what='dkv')
    grads = rec.named(dec)
    assert len(grads) == 26
    for name, grad in grads.items():
        if name.endswith('_bk'):              # exactly zero in real arithmetic (rows of datt sum to 0): rounding noise
            assert np.abs(grad).max() < 1e-4 and np.abs(want_g[name]).max() < 1e-9
            continue
        assert_close(grad, want_g[name], tol=1e-4, what=name)
    ref = np.asarray(dec._forward_unfused(D.as_device(q), D.as_device(kv)))
    assert_close(out, ref, tol=3e-6, what='fused vs unfused')
    rec2 = DC.GradRecorder()
    with parallel.grad_scope(0) as scope:
        dq2, dkv2 = (np.asarray(g) for g in dec._backward_unfused(D.as_device(dy), rec2, scope))
    assert_close(dq, dq2, tol=1e-5, what='dq fused vs unfused')
    assert_close(dkv, dkv2, tol=1e-5, what='dkv fused vs unfused')
    out = np.asarray(dec(q, kv))
    for sizes in DC.chunkings(s):
        got = DC.run_decoder_chunks(dec, q, kv, sizes, capacity=s + 3)
        _layer_close(got, out, 2 * LAYER_TOL, f'decode chunks {sizes[:4]} vs forward')
        _layer_close(got, want, 1e-4, f'decode chunks {sizes[:4]} vs float64')
    with pytest.raises(RuntimeError, match='inference only'):
        dec(dy, backprop=True, learning_rate=1e-3)


def test_decoder_default_is_not_causal_and_odd_head_sizes_raise(npm):
    import decode_cases as DC
    from conftest import assert_close
    dec, p = DC.make_decoder(npm, 128, 4, None, 96, True, False, seed=13)
    rng = np.random.default_rng(14)
    q, kv = rng.standard_normal([2, 9, 128]).astype(np.float32), rng.standard_normal([2, 7, 128]).astype(np.float32)
    want, _ = O.decoder_fwd(p, q.astype(np.float64), kv.astype(np.float64), True)
    assert_close(np.asarray(dec(q, kv)), want, tol=1e-4)
    assert dec._self_attention._mask is None and not dec._causal_masks
    np.random.seed(1)
    odd = npm.layers.TransformerDecoder(num_heads=4, hidden_units=32, norm_first=True, causal=True)
    with pytest.raises(NotImplementedError):
        odd(np.zeros([1, 3, 48], dtype=np.float32), np.zeros([1, 3, 48], dtype=np.float32))       # head size 12
