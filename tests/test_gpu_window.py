"""GPU: sliding-window attention for decoding -- npm_mha_decode_fwd_window, npm_mha_prefill_fwd_window,
npm_mha_decode_window_splits, ``KVCache`` / ``PagedKVCache(window=)``, ``MultiHeadAttention(window=)`` and
``TransformerDecoder(causal=True, window=)``.

Bounds.  The kernels are held against float64 attention of every sequence alone over the rows its window reaches
(tests/window_cases.py) at the bounds of tests/test_gpu_varlen.py: ctx 2e-6 (1 + |ref|), lse 3e-6, both grown by
attn_range_data.exponent_tol(X).  Layers: LAYER_TOL = 1e-5 in decode_gpu.layer_close's metric against float64, 2 LAYER_TOL between
two runs of the product on the same model, the decoder 1e-4 against float64 (tests/test_gpu_paged.py).  A half-precision cache
rounds K / V when it stores them and ``forward`` does not, so its chunked decode is held to the one-call decode over the same
stored halves (as tests/test_gpu_kv16.py does); half-precision weights are exact copies here because the test first rounds the
six matrices to fp16-representable values, so ``forward`` is the same model.

Poison.  NaN fills every cache row below the smallest floor of its sequence, every row at and past its length, every unused page
and the padded query rows; reclaimed and out-of-range table entries name an all-NaN page that is in range.  A wrong read shows up
as NaN, never as a fault.  ctx and lse are followed by guard regions that must keep their sentinel.

Every test names a keyword or an entry point of this feature: none passes on the parent commit.
"""

import ctypes as C
import itertools

import numpy as np
import pytest

import attn_range_data as R
import decode_cases as DC
import decode_gpu
import decode_reference as DR
import varlen_reference as VR
import window_cases as WC
from decode_gpu import GUARD, SENTINEL

pytestmark = pytest.mark.gpu

LAYER_TOL = 1e-5
BAD = 10002


@pytest.fixture(scope='module')
def npm():
    import np_modeling_amd
    return np_modeling_amd


@pytest.fixture(autouse=True)
def _knobs(npm):
    decode_gpu.reset_knobs()
    yield
    decode_gpu.reset_knobs()


def _lib():
    from np_modeling_amd import _C
    return _C.lib()


# ---- one call through the C ABI ---------------------------------------------------------------------------------------------------
def _call(entry, q, k, v, lmax, scale, kv_lens, new_lens, window=None, paged=None, f16=False, causal=1, expect=0, null_lens=False,
          page_rows=None):
    """``entry`` 'decode' or 'prefill', windowed when ``window`` is given, else the unwindowed entry point of the same layout and
    storage type.  k / v [B, capacity, Hkv, D] or, with ``paged = (table, page_rows)``, pools [pages, page_rows, Hkv, D]; ``f16``:
    uploaded as halves (pitches then count halves).  -> ctx [B, T, Hq, D], lse [B, Hq, T], kernel string; ``expect``: the call
    must return that code and leave ctx and lse at their sentinel."""
    from np_modeling_amd import _C, device as D
    b, t, hq, d = q.shape
    rows, hkv = k.shape[1], k.shape[2]
    qd = D.from_host(q)
    with np.errstate(over='ignore'):
        kd, vd = (D.bytes_from_host(np.ascontiguousarray(x.astype(np.float16))) if f16 else D.from_host(x) for x in (k, v))
    ctx = D.full([b * t * hq * d + GUARD], SENTINEL)
    lse = D.full([b * hq * t + GUARD], SENTINEL)
    c = _C.npm_mha_decode()
    c.batch, c.heads, c.kv_heads, c.new_tokens, c.kv_len, c.head_dim = b, hq, hkv, t, lmax, d
    c.causal, c.scale = int(causal), scale
    c.q, c.q_pitch = qd.ptr, hq * d
    c.k, c.k_pitch, c.k_stride_b = kd.ptr, hkv * d, rows * hkv * d
    c.v, c.v_pitch, c.v_stride_b = vd.ptr, hkv * d, rows * hkv * d
    c.ctx, c.ctx_pitch, c.lse = ctx.ptr, hq * d, lse.ptr
    lens = None if null_lens else decode_gpu.ints(kv_lens)
    new = None if new_lens is None else decode_gpu.ints(new_lens)
    lens_ptr, new_ptr = (None if x is None else x.ptr for x in (lens, new))
    table, table_pitch, prows = None, 0, 0
    if paged is not None:
        assert paged[0].min() >= 0 and paged[0].max() < k.shape[0], 'every table entry must name a page of the pool'
        table, table_pitch, prows = decode_gpu.ints(paged[0]), paged[0].shape[1], paged[1] if page_rows is None else page_rows
    table_ptr = None if table is None else table.ptr
    lib = _lib()
    if window is not None:
        name = f'npm_mha_{entry}_fwd_window'
        rc = getattr(lib, name)(C.byref(c), lens_ptr, new_ptr, table_ptr, table_pitch, prows, int(window), int(f16))
    elif entry == 'prefill':
        name = 'npm_mha_prefill_fwd_f16' if f16 else 'npm_mha_prefill_fwd'
        rc = getattr(lib, name)(C.byref(c), lens_ptr, new_ptr, table_ptr, table_pitch, prows)
    elif f16:
        name = 'npm_mha_decode_fwd_f16'
        rc = lib.npm_mha_decode_fwd_f16(C.byref(c), lens_ptr, new_ptr, table_ptr, table_pitch, prows)
    elif paged is not None:
        name = 'npm_mha_decode_fwd_paged'
        rc = lib.npm_mha_decode_fwd_paged(C.byref(c), lens_ptr, new_ptr, table_ptr, table_pitch, prows)
    else:
        name = 'npm_mha_decode_fwd_varlen'
        rc = lib.npm_mha_decode_fwd_varlen(C.byref(c), lens_ptr, new_ptr)
    if expect:
        assert rc == expect, (rc, lib.npm_last_error())
        assert name.encode() in lib.npm_last_error(), 'the error names the entry point that was called'
        np.testing.assert_array_equal(ctx.numpy(), SENTINEL)              # nothing was launched
        np.testing.assert_array_equal(lse.numpy(), SENTINEL)
        return None
    _C.check(rc, name)
    last = _C.last_decode_kernel() if entry == 'decode' else _C.last_prefill_kernel()
    return decode_gpu.guarded(ctx, b * t * hq * d).reshape(b, t, hq, d), decode_gpu.guarded(lse, b * hq * t).reshape(b, hq, t), last


def _bits_equal(a, b, what):
    assert np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32)), f'{what}: ctx differs'
    assert np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32)), f'{what}: lse differs'


def _check(got_ctx, got_lse, q, k, v, kv_lens, new_lens, scale, window, what):
    """Every valid element against float64 of its sequence alone over the rows its window reaches, at tol(X) of that sequence; rows
    without a visible key are ctx == 0, lse == -inf.  Prints the largest fraction of the bound used."""
    b, t = q.shape[:2]
    want_ctx, want_lse = WC.attention(q, k, v, kv_lens, new_lens, scale, window)
    seen = VR.valid_rows(t, kv_lens, new_lens)
    first = WC.smallest_floor(kv_lens, new_lens, window)
    assert (got_ctx[~seen] == 0).all(), f'{what}: ctx of a row without a visible key is not 0'
    assert np.isneginf(got_lse.transpose(0, 2, 1)[~seen]).all(), f'{what}: lse of a row without a visible key is not -inf'
    worst_ctx = worst_lse = 0.0
    for i in np.nonzero(seen.any(axis=1))[0]:
        rows = seen[i]
        g_ctx, g_lse = got_ctx[i, rows].astype(np.float64), got_lse[i][:, rows].astype(np.float64)
        assert np.isfinite(g_ctx).all() and np.isfinite(g_lse).all(), f'{what}: sequence {i} not finite'
        x = R.exponent_magnitude(q[i:i + 1, rows], k[i:i + 1, first[i]:kv_lens[i]], scale, want_lse[i:i + 1, :, rows])
        worst_ctx = max(worst_ctx, float((np.abs(g_ctx - want_ctx[i, rows]) / (R.exponent_tol(2e-6, x) * (1.0 + np.abs(want_ctx[i, rows])))).max()))
        worst_lse = max(worst_lse, float(np.abs(g_lse - want_lse[i][:, rows]).max() / R.exponent_tol(3e-6, x)))
    print(f'{what}: ctx {worst_ctx:.3f} of the bound, lse {worst_lse:.3f} of the bound')
    assert worst_ctx <= 1.0, f'{what}: ctx {worst_ctx:.3g} of the bound'
    assert worst_lse <= 1.0, f'{what}: lse {worst_lse:.3g} of the bound'


def _data(seed, kv_lens, new_lens, t, hq, hkv, d, window):
    """q, k, v with finite values only where a windowed call may look (the rest NaN: ``WC.poison``)."""
    rng = np.random.default_rng(seed)
    b, cap = len(kv_lens), max(int(np.max(kv_lens)), 1)
    q = rng.standard_normal([b, t, hq, d]).astype(np.float32)
    k, v = (np.full([b, cap, hkv, d], np.nan, dtype=np.float32) for _ in range(2))
    first = WC.smallest_floor(kv_lens, new_lens, window)
    for i in range(b):
        lo, hi = int(first[i]), int(kv_lens[i])
        k[i, lo:hi] = rng.standard_normal([hi - lo, hkv, d])
        v[i, lo:hi] = rng.standard_normal([hi - lo, hkv, d])
    return WC.poison(q, k, v, kv_lens, new_lens, window)


# ---- 1. the decode kernel against float64, poisoned ---------------------------------------------------------------------------------
HEADS = ((8, 8, 1), (8, 2, 4), (5, 1, 4), (6, 3, 5))                     # (Hq, Hkv, T); (5, 1, 4): 20 rows, two row blocks
WINDOWS = (1, 5, 16, 17, 100)
LAYOUTS = ('contiguous', 'paged16-identity', 'paged16-random', 'paged64-identity', 'paged64-random')
MODES = ('one', 'auto', 'many')


def _lengths(window, t, shift):
    """Lengths around the window, 300 and 2049, L - W + 1 at a multiple of 16 and one either side, and one empty sequence; the new
    tokens mix 0, 1 and T."""
    base = [1, window - 1, window, window + 1, 300, 2049, 48 + window - 2, 48 + window - 1, 48 + window]
    kv = np.maximum(np.array(base, dtype=np.int64), 1)
    pattern = (t, 1, t, 0, 1, t)
    n = np.minimum(np.array([pattern[(i + shift) % len(pattern)] for i in range(len(kv))], dtype=np.int64), kv)
    kv, n = kv[kv >= t], n[kv >= t]                                      # L >= T
    return np.append(kv, 0), np.append(n, 0)                              # ... and L_b = 0


def _decode_cases():
    """D x (Hq, Hkv, T) x W; every case runs the whole product of split modes and layouts on one set of data."""
    return [(d, hq, hkv, t, window, i) for i, (d, (hq, hkv, t), window) in enumerate(itertools.product((16, 32, 64, 128), HEADS, WINDOWS))]


def _layout(k, v, kv_lens, new_lens, window, layout, seed):
    if layout == 'contiguous':
        return k, v, None
    page_rows, order = int(layout[5:7]), layout[8:]
    pk, pv, table = WC.build_pool(k, v, kv_lens, new_lens, window, page_rows, order, seed)
    return pk, pv, (table, page_rows)


@pytest.mark.parametrize('case', _decode_cases(), ids=lambda c: f'D{c[0]}-H{c[1]}/{c[2]}-T{c[3]}-W{c[4]}')
def test_npm_mha_decode_fwd_window_against_float64_with_poison(npm, case):
    """Every split mode (one / auto / many) x every layout (contiguous, paged 16 and 64, identity and random tables) on the data
    of the case: the contiguous result of each mode against float64, each paged result bit for bit against the contiguous one of
    its mode (a stronger statement than the bound) with its own kernel string and split count."""
    d, hq, hkv, t, window, seed = case
    kv_lens, new_lens = _lengths(window, t, seed)
    lmax, b, scale = int(kv_lens.max()), len(kv_lens), 1.0 / np.sqrt(d)
    q, k, v = _data(seed, kv_lens, new_lens, t, hq, hkv, d, window)
    bound = min(lmax, window + t - 1)
    pools = {layout: _layout(k, v, kv_lens, new_lens, window, layout, seed) for layout in LAYOUTS}
    for mode in MODES:
        forced = decode_gpu.set_splits(mode, bound)                      # 'many': more splits than the window has tiles
        splits = _lib().npm_mha_decode_window_splits(b, hkv, lmax, t, window)
        assert splits == (forced or DR.auto_splits(b, hkv, bound))
        flat = None
        for layout in LAYOUTS:
            pk, pv, paged = pools[layout]
            got = _call('decode', q, pk, pv, lmax, scale, kv_lens, new_lens, window, paged)
            tail = '' if paged is None else f' paged={paged[1]}'
            assert got[2] == f'mha_decode_kernel D={d} rows={hq // hkv * t} splits={splits} causal=1 varlen=1{tail} window={window}', got[2]
            if paged is None:
                flat = got
                _check(got[0], got[1], q, k, v, kv_lens, new_lens, scale, window, f'decode window {case[:5]} splits {mode}')
            else:
                _bits_equal(got, flat, f'decode window {case[:5]} splits {mode}: {layout} vs contiguous')


# ---- 2. the decode kernel's bitwise identities ---------------------------------------------------------------------------------------
@pytest.mark.parametrize('d', [16, 32, 64, 128])
@pytest.mark.parametrize('hq,hkv,t', HEADS)
def test_npm_mha_decode_fwd_window_bitwise_identities(npm, d, hq, hkv, t):
    """(a) a covering window is the unwindowed entry point of the same layout and storage type, bit for bit, at every split mode;
    (b) paged equals contiguous, fp16 equals fp32 on the rounded values, either load policy gives the same bits."""
    from np_modeling_amd import _C
    seed = d + hq + t
    # (a): lengths up to 1025 so that the automatic rule splits; nothing is poisoned below a floor (there is none)
    kv_lens = np.array([1025, 300, 17, max(t, 1), 0, 1024], dtype=np.int64)
    new_lens = np.minimum(np.array([t, 1, t, t, 0, 0], dtype=np.int64), kv_lens)
    lmax, b, scale = 1025, len(kv_lens), 1.0 / np.sqrt(d)
    q, k, v = decode_gpu.data(seed, b, t, hq, hkv, d, lmax)
    q, k, v = decode_gpu.poison(q, k, v, kv_lens, new_lens)
    import paged_cases as PC
    pk, pv, table = PC.build_pool(k, v, kv_lens, 16, 'random', seed)
    for mode in MODES:
        forced = decode_gpu.set_splits(mode, lmax)
        for window in (lmax, 5000, 2 ** 31 - 1):
            assert _lib().npm_mha_decode_window_splits(b, hkv, lmax, t, window) == _lib().npm_mha_decode_splits(b, hkv, lmax)
        for name, args, f16 in (('contiguous', (k, v), False), ('paged', (pk, pv), False), ('contiguous f16', (k, v), True), ('paged f16', (pk, pv), True)):
            paged = (table, 16) if name.startswith('paged') else None
            plain = _call('decode', q, *args, lmax, scale, kv_lens, new_lens, None, paged, f16)
            for window in ((lmax, 2 ** 31 - 1) if mode == 'auto' else (lmax,)):
                got = _call('decode', q, *args, lmax, scale, kv_lens, new_lens, window, paged, f16)
                _bits_equal(got, plain, f'covering window {window} vs unwindowed, {name}, splits {mode}')
                assert got[2] == plain[2] + f' window={window}', (got[2], plain[2])
    # (b): a real window, poisoned below the floors
    window = 100
    decode_gpu.reset_knobs()
    kv_lens = np.array([2049, 300, window + 47, max(t, 1), 0, 1024], dtype=np.int64)
    new_lens = np.minimum(np.array([t, 1, t, t, 0, 0], dtype=np.int64), kv_lens)
    lmax = 2049
    q, k, v = _data(seed, kv_lens, new_lens, t, hq, hkv, d, window)
    rk, rv = (x.astype(np.float16).astype(np.float32) for x in (k, v))
    for mode in ('auto', 'many'):
        decode_gpu.set_splits(mode, min(lmax, window + t - 1))
        flat = _call('decode', q, k, v, lmax, scale, kv_lens, new_lens, window)
        for page_rows, order in ((16, 'random'), (64, 'identity')):
            pk, pv, table = WC.build_pool(k, v, kv_lens, new_lens, window, page_rows, order, seed)
            _bits_equal(_call('decode', q, pk, pv, lmax, scale, kv_lens, new_lens, window, (table, page_rows)), flat,
                        f'paged {page_rows} {order} vs contiguous, splits {mode}')
        half = _call('decode', q, k, v, lmax, scale, kv_lens, new_lens, window, f16=True)
        _bits_equal(half, _call('decode', q, rk, rv, lmax, scale, kv_lens, new_lens, window), f'fp16 vs fp32 on the rounded values, splits {mode}')
        pk, pv, table = WC.build_pool(k, v, kv_lens, new_lens, window, 16, 'random', seed)
        _bits_equal(_call('decode', q, pk, pv, lmax, scale, kv_lens, new_lens, window, (table, 16), f16=True), half, f'paged fp16 vs contiguous fp16, splits {mode}')
        policies = []
        for nt in (1, 2):
            _C.check(_lib().npm_set_tuning(decode_gpu.NT_KNOB, nt), 'npm_set_tuning')
            policies.append(_call('decode', q, k, v, lmax, scale, kv_lens, new_lens, window))
        _C.check(_lib().npm_set_tuning(decode_gpu.NT_KNOB, 0), 'npm_set_tuning')
        _bits_equal(policies[0], policies[1], 'nontemporal vs plain loads')
        _bits_equal(policies[0], flat, 'a forced load policy vs the automatic one')


# ---- 3. the prefill kernel ------------------------------------------------------------------------------------------------------------
def _prefill_cases():
    out = []
    for i, (t, window, before, d) in enumerate(itertools.product((33, 64, 65, 130), (1, 16, 40, 64, 200), (0, 7, 300), (16, 128))):
        out.append((d, ((8, 2), (6, 3), (4, 1), (8, 8))[i % 4], t, window, before, i))
    return out


@pytest.mark.parametrize('case', _prefill_cases(), ids=lambda c: f'D{c[0]}-H{c[1][0]}/{c[1][1]}-T{c[2]}-W{c[3]}-before{c[4]}')
def test_npm_mha_prefill_fwd_window_against_float64_and_its_bitwise_identities(npm, case):
    d, (hq, hkv), t, window, before, seed = case
    new_lens = np.array([t, max(t - 5, 1), 0, 1, t - 32], dtype=np.int64)                 # ragged; one sequence rides along
    kv_lens = np.array([before + t, before + new_lens[1], before, before + 1, before + 3 + new_lens[4]], dtype=np.int64)
    lmax, b, scale = int(kv_lens.max()), len(kv_lens), 1.0 / np.sqrt(d)
    q, k, v = _data(seed, kv_lens, new_lens, t, hq, hkv, d, window)
    got = _call('prefill', q, k, v, lmax, scale, kv_lens, new_lens, window)
    assert got[2] == f'mha_prefill_kernel D={d} T={t} rows=64 causal=1 varlen=1 window={window}', got[2]
    _check(got[0], got[1], q, k, v, kv_lens, new_lens, scale, window, f'prefill window {case[:5]}')
    # paged is contiguous
    page_rows = (16, 64)[seed % 2]
    pk, pv, table = WC.build_pool(k, v, kv_lens, new_lens, window, page_rows, ('identity', 'random')[(seed // 2) % 2], seed)
    paged = _call('prefill', q, pk, pv, lmax, scale, kv_lens, new_lens, window, (table, page_rows))
    _bits_equal(paged, got, 'paged vs contiguous')
    assert paged[2] == f'mha_prefill_kernel D={d} T={t} rows=64 causal=1 varlen=1 paged={page_rows} window={window}', paged[2]
    # a sequence in a batch is that sequence alone (the same new_tokens)
    for i in (0, 4):
        rows = max(int(kv_lens[i]), 1)
        alone = _call('prefill', q[i:i + 1], k[i:i + 1, :rows], v[i:i + 1, :rows], int(kv_lens[i]), scale, kv_lens[i:i + 1], new_lens[i:i + 1], window)
        n = int(new_lens[i])
        assert np.array_equal(alone[0][0, :n].view(np.uint32), got[0][i, :n].view(np.uint32)), f'sequence {i} alone: ctx differs'
        assert np.array_equal(alone[1][0, :, :n].view(np.uint32), got[1][i, :, :n].view(np.uint32)), f'sequence {i} alone: lse differs'
    # fp16 is fp32 on the rounded values
    rk, rv = (x.astype(np.float16).astype(np.float32) for x in (k, v))
    half = _call('prefill', q, k, v, lmax, scale, kv_lens, new_lens, window, f16=True)
    _bits_equal(half, _call('prefill', q, rk, rv, lmax, scale, kv_lens, new_lens, window), 'fp16 vs fp32 on the rounded values')
    assert half[2].endswith(f' kv=f16 window={window}')
    # a covering window is npm_mha_prefill_fwd[_f16]: rows below the floors must be real for the unwindowed call
    fq, fk, fv = decode_gpu.poison(*decode_gpu.data(seed, b, t, hq, hkv, d, max(lmax, 1)), kv_lens, new_lens)
    for f16 in (False, True):
        plain = _call('prefill', fq, fk, fv, lmax, scale, kv_lens, new_lens, None, f16=f16)
        for cover in (max(lmax, 1), 2 ** 31 - 1):
            _bits_equal(_call('prefill', fq, fk, fv, lmax, scale, kv_lens, new_lens, cover, f16=f16), plain, f'covering window {cover}, f16 {f16}')


# ---- 4. refusals ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('entry', ['decode', 'prefill'])
def test_window_entry_points_refuse_bad_arguments_and_launch_nothing(npm, entry):
    import paged_cases as PC
    kv_lens, new_lens = np.array([40, 17], dtype=np.int64), np.array([4, 1], dtype=np.int64)
    q, k, v = decode_gpu.data(1, 2, 4, 8, 2, 64, 40)
    pk, pv, table = PC.build_pool(k, v, kv_lens, 16, 'identity')
    args = (q, k, v, 40, 0.125, kv_lens, new_lens)
    for f16 in (False, True):
        _call(entry, *args, window=0, f16=f16, expect=BAD)
        _call(entry, *args, window=-3, f16=f16, expect=BAD)
        _call(entry, *args, window=8, f16=f16, causal=0, expect=BAD)
        _call(entry, *args, window=8, f16=f16, null_lens=True, expect=BAD)
        for page_rows in (0, 8, 24):
            _call(entry, q, pk, pv, 40, 0.125, kv_lens, new_lens, window=8, paged=(table, 16), f16=f16, page_rows=page_rows, expect=BAD)
    assert _call(entry, *args, window=8) is not None                      # the same arguments with nothing wrong


# ---- 5. the layer ---------------------------------------------------------------------------------------------------------------------
def _layer_run(att, x, sizes, capacity, want_paths=True, **cache_args):
    cache = att.make_cache(x.shape[0], capacity, **cache_args)
    outs = []
    for piece in DC.split(x, sizes):
        outs.append(np.asarray(att(np.ascontiguousarray(piece), cache=cache)))
        if want_paths:
            assert att._cached_path == ('decode' if att._num_heads // att._num_kv_heads * piece.shape[1] <= 32 else 'prefill')
    return np.concatenate(outs, axis=1), cache


def test_layer_window_24_chunked_cached_calls_equal_the_banded_forward(npm, monkeypatch):
    """MultiHeadAttention(8, num_kv_heads=2, window=24) at B 3, F 128, page 16: token by token and in chunks of 1, 4 and 40, f32
    and f16 caches, with both prefill switches off."""
    D = npm.device
    monkeypatch.setattr(D, 'PREFILL_KERNEL', False)
    monkeypatch.setattr(D, 'PREFILL_KERNEL_F16', False)
    window, f, s = 24, 128, 96
    att, p = WC.make_mha(npm, f, 8, 2, seed=3, window=window, batch=3)
    x = np.random.default_rng(5).standard_normal([3, s, f]).astype(np.float32)
    band = WC.band(s, window)
    want, _ = DR.att_fwd(p, x.astype(np.float64), mask=band[None, None])
    whole = np.asarray(att(x, mask=D.AttnMask(band, 3, 8, s, s)))          # the uncached forward with the band mask
    decode_gpu.layer_close(whole, want, LAYER_TOL, 'uncached forward with the band vs float64')
    for sizes in ([1] * s, [40, 1, 4, 1, 40, 4, 1, 1, 4]):
        flat, _ = _layer_run(att, x, sizes, s)
        paged, cache = _layer_run(att, x, sizes, s, page_size=16)
        assert np.array_equal(flat, paged), f'paged vs contiguous windowed cache, chunks {sizes[:4]}'
        decode_gpu.layer_close(flat, want, LAYER_TOL, f'window chunks {sizes[:4]} vs float64 with the band')
        decode_gpu.layer_close(flat, whole, 2 * LAYER_TOL, f'window chunks {sizes[:4]} vs the uncached forward with the band')
        assert cache.dropped.tolist() == [(s - sizes[-1] - window + 1) // 16 * 16] * 3
    one, _ = _layer_run(att, x, [s], s, dtype='f16')
    half, _ = _layer_run(att, x, [40, 1, 4, 1, 40, 4, 1, 1, 4], s, dtype='f16', page_size=16)
    decode_gpu.layer_close(half, one, 2 * LAYER_TOL, 'f16 windowed cache in chunks vs one call')
    decode_gpu.layer_close(half, want, 2e-3, 'f16 windowed cache vs float64 (fp16 rounding of K / V: 2^-11 relative)')


@pytest.mark.parametrize('tokens', [1, 4, 40])
def test_layer_window_pages_in_use_stay_bounded_and_a_pool_of_that_size_suffices(npm, tokens):
    window, f, page, capacity, b = 24, 128, 16, 208, 3
    att, _ = WC.make_mha(npm, f, 8, 2, seed=4, window=window, batch=b)
    bound = b * WC.max_pages(window, tokens, page)
    x = np.random.default_rng(6).standard_normal([b, tokens, f]).astype(np.float32)
    cache = att.make_cache(b, capacity, page_size=page, pages=bound)
    plain_att, _ = WC.make_mha(npm, f, 8, 2, seed=4, window=None, batch=b)
    plain = plain_att.make_cache(b, capacity, page_size=page, pages=bound)
    raised = False
    for step in range(capacity // tokens):                                # 200 tokens and more
        out = np.asarray(att(x, cache=cache))
        assert cache.pages_in_use <= bound
        if not raised:
            try:
                plain_att(x, cache=plain)
            except ValueError as e:
                assert 'more pages' in str(e)
                raised = True
    assert np.isfinite(out).all() and cache.max_length == capacity // tokens * tokens >= 200 and raised


# ---- 6. the decoder -------------------------------------------------------------------------------------------------------------------
def _round_six_matrices(dec):
    for path, attrs in (('_self_attention', ('_wq', '_wk', '_wv', '_wo')), ('_cross_attention', ('_wq', '_wo')),
                        ('_dense1._linear', ('_w',)), ('_dense2', ('_w',))):
        for attr in attrs:
            arr = getattr(DC.sub(dec, path), attr)
            arr.set(np.asarray(arr).astype(np.float16).astype(np.float32))


@pytest.mark.parametrize('norm_first,options', [(True, {}), (False, {}), (True, {'rope_base': 10000.0}), (False, {'cache_dtype': 'f16'}),
                                                (True, {'weights': 'f16'}), (False, {'page_size': 16})],
                         ids=['pre', 'post', 'pre-rope', 'post-kv16', 'pre-w16', 'post-paged'])
def test_decoder_causal_window_24_decode_equals_forward_and_backward_equals_the_mask_path(npm, norm_first, options):
    D = npm.device
    window, f, b, s = 24, 128, 2, 96
    build = {k: v for k, v in options.items() if k == 'rope_base'}
    start = {k: v for k, v in options.items() if k != 'rope_base'}
    dec, _ = WC.make_decoder(npm, f, 8, 2, 256, norm_first, seed=9, window=window, batch=b, **build)
    twin, _ = WC.make_decoder(npm, f, 8, 2, 256, norm_first, seed=9, window=None, batch=b, **build)     # the band through the mask path
    if 'weights' in start:
        _round_six_matrices(dec)
        _round_six_matrices(twin)
    p = DC.decoder_params(dec)
    band = WC.band(s, window)
    twin._causal_masks[(b, s)] = D.AttnMask(band, b, 8, s, s)
    rng = np.random.default_rng(2)
    q = rng.standard_normal([b, s, f]).astype(np.float32)
    kv = rng.standard_normal([b, 7, f]).astype(np.float32)
    dy = rng.standard_normal([b, s, f]).astype(np.float32)
    out = np.asarray(dec(q, kv))
    assert np.array_equal(out, np.asarray(twin(q, kv)))
    grads = []
    for layer in (dec, twin):
        dq, dkv = (np.asarray(g) for g in layer(dy, backprop=True, optimizer_=DC.GradRecorder()))
        grads.append((dq, dkv))
    assert np.array_equal(grads[0][0], grads[1][0]) and np.array_equal(grads[0][1], grads[1][1]) and np.isfinite(grads[0][0]).all()
    if not build:
        want, _ = DR.decoder_fwd(p, q.astype(np.float64), kv.astype(np.float64), norm_first, mask=band[None, None])
        unwindowed, _ = DR.decoder_fwd(p, q.astype(np.float64), kv.astype(np.float64), norm_first, mask=DR.causal_mask(s)[None, None])
        assert np.abs(unwindowed - want).max() > 1e-2                     # the window matters
        decode_gpu.layer_close(out, want, 1e-4, 'windowed forward vs float64 with the band')
    out = np.asarray(dec(q, kv))
    runs = {}
    for sizes in ([s], [40, 1, 1, 4, 33, 1, 16], [1] * s):
        state = dec.start_decoding(kv, s + 8, **start)
        assert state.self_cache.window == window and state.cross_cache.window is None
        got = np.concatenate([np.asarray(dec.decode(np.ascontiguousarray(piece), state)) for piece in DC.split(q, sizes)], axis=1)
        runs[len(sizes)] = got
        if start.get('cache_dtype') != 'f16':
            decode_gpu.layer_close(got, out, 2 * LAYER_TOL, f'windowed decode chunks {sizes[:4]} vs forward')
        decode_gpu.layer_close(got, runs[1], 2 * LAYER_TOL, f'windowed decode chunks {sizes[:4]} vs one call')
    if 'page_size' in start:
        cache = state.self_cache
        assert cache.dropped.tolist() == [(s - 1 - window + 1) // 16 * 16] * b and cache.pages_in_use <= b * WC.max_pages(window, 1, 16)
        # release and admit beside a running windowed sequence: slot 0 starts again at position 0 with nothing dropped
        state.release(0)
        assert cache.dropped.tolist()[0] == 0 and cache.lengths.tolist() == [0, s]
        dec.admit(state, 0, kv[:1])
        fresh = np.asarray(dec.decode(np.ascontiguousarray(q[:, :5]), state, new_lengths=np.array([5, 1])))
        assert cache.lengths.tolist() == [5, s + 1] and cache.dropped[0] == 0
        decode_gpu.layer_close(fresh[0], out[0, :5], 2 * LAYER_TOL, 'the admitted sequence starts at position 0')


def test_decoder_window_without_causal_raises(npm):
    with pytest.raises(ValueError, match='causal=True'):
        npm.layers.TransformerDecoder(num_heads=8, hidden_units=64, norm_first=True, window=24)
