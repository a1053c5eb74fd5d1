"""CPU: incremental decoding without a GPU.

* the float64 restatements of tests/decode_reference.py: the causal decoder with an all-true mask IS the oracle's decoder;
  decoding in chunks with a cache equals the full causal forward, for multi-head and grouped-query attention;
* a float32 model of the kernel's split / combine rule against float64 at every (L, D, splits) tests/test_gpu_decode.py uses:
  its error stays under HALF of the bound the GPU test applies there, so the bound is one the method can meet;
* the product's host logic on the simulator (tests/hostsim/ (profile 'decode')): cache bookkeeping, capacity overflow raised before any
  call, reset, backward after a cached forward, the frozen cross-attention cache, which path a cached forward selects, the
  causal decoder and ``decode`` against the restatements;
* the new struct's layout and the new entry points against the header.
"""

import ctypes
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

import attn_range_data as R
import decode_cases as DC
import decode_reference as DR
import gqa_reference as G
from hostsim.fixtures import built, npm_fixture
from oracle import np_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the restatements ----------------------------------------------------------------------------------------------------
def _decoder_problem(seed, heads, kv_heads, f=12, hidden=20, b=2, s=9, skv=5):
    rng = np.random.default_rng(seed)
    p = {}
    for tag in ('sa', 'ca'):
        for n, a in G.init_params(rng, f, f, heads, kv_heads, scale=0.4).items():
            p[f'{tag}_{n}'] = a
    for n in ('n1', 'n2', 'n3'):
        p[n + '_gamma'], p[n + '_beta'] = 1 + 0.1 * rng.standard_normal(f), 0.1 * rng.standard_normal(f)
    p['d1_w'], p['d1_b'] = 0.4 * rng.standard_normal([f, hidden]), 0.1 * rng.standard_normal(hidden)
    p['d2_w'], p['d2_b'] = 0.4 * rng.standard_normal([hidden, f]), 0.1 * rng.standard_normal(f)
    return p, rng.standard_normal([b, s, f]), rng.standard_normal([b, skv, f]), rng.standard_normal([b, s, f])


@pytest.mark.parametrize('norm_first', [True, False])
def test_restated_decoder_with_all_true_mask_is_the_oracle_decoder(norm_first):
    p, q, kv, dy = _decoder_problem(1, 3, 3)
    want, cache = O.decoder_fwd(p, q, kv, norm_first)
    (want_dq, want_dkv), want_g = O.decoder_bwd(p, cache, dy, norm_first)
    for mask in (None, np.ones([9, 9], dtype=bool)):
        got, c = DR.decoder_fwd(p, q, kv, norm_first, mask=mask)
        (dq, dkv), g = DR.decoder_bwd(p, c, dy, norm_first)
        assert np.array_equal(got, want) and np.array_equal(dq, want_dq) and np.array_equal(dkv, want_dkv)
        assert g.keys() == want_g.keys() and all(np.array_equal(g[k], want_g[k]) for k in g)


@pytest.mark.parametrize('heads,kv_heads', [(4, 4), (4, 2), (6, 1)])
def test_restated_cached_attention_equals_the_full_causal_forward(heads, kv_heads):
    rng = np.random.default_rng(heads + kv_heads)
    f, s = 2 * heads, 11
    p = G.init_params(rng, f, f, heads, kv_heads, scale=0.5)
    x = rng.standard_normal([2, s, f])
    want, _ = DR.att_fwd(p, x, mask=DR.causal_mask(s))
    for sizes in DC.chunkings(s):
        got = DR.mha_cached(p, DC.split(x, sizes))
        np.testing.assert_allclose(got, want, rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize('norm_first', [True, False])
@pytest.mark.parametrize('heads,kv_heads', [(3, 3), (4, 2)])
def test_restated_cached_decoder_equals_the_full_causal_forward(heads, kv_heads, norm_first):
    p, q, kv, _ = _decoder_problem(2, heads, kv_heads, f=12)
    want, _ = DR.decoder_fwd(p, q, kv, norm_first, mask=DR.causal_mask(q.shape[1]))
    for sizes in DC.chunkings(q.shape[1]):
        np.testing.assert_allclose(DR.decoder_cached(p, DC.split(q, sizes), kv, norm_first), want, rtol=1e-11, atol=1e-11)
    full, _ = DR.decoder_fwd(p, q, kv, norm_first)
    assert np.abs(full - want).max() > 1e-3          # the mask matters: the unmasked decoder is a different function


def test_causal_rows_place_the_new_tokens_last():
    rows = DR.causal_rows(3, 7)
    assert rows.sum(axis=1).tolist() == [5, 6, 7] and rows[0, :5].all() and not rows[0, 5:].any()
    assert np.array_equal(DR.causal_rows(4, 4), DR.causal_mask(4))


# ---- the split / combine rule in float32 -----------------------------------------------------------------------------------
def _gpu_lengths():
    import test_gpu_decode as T
    out = set()
    for case in T._cases():
        d, _, _, t, causal, length, b, _, mode = case.values
        tiles = (length + 15) // 16
        splits = {'one': 1, 'many': min(tiles + 3, 1024), 'auto': DR.auto_splits(b, 1, length)}.get(mode, mode)
        out.add((length, d, int(splits), t, causal))
        if mode == 'auto':
            out.add((length, d, DR.auto_splits(b, 8, length), t, causal))
    return sorted(out)


def test_split_model_stays_under_half_of_the_gpu_bound():
    """Unit-normal inputs, every (L, D, splits, T, causal) of the GPU grid (one sequence, Hq = 2 over Hkv = 1: the error does not
    depend on the batch or the head count).  The GPU bound is 2e-6 (1 + |ref|) on ctx and 3e-6 on lse, grown by tol(X)."""
    worst_ctx = worst_lse = 0.0
    for length, d, splits, t, causal in _gpu_lengths():
        rng = np.random.default_rng(length + d + splits)
        q = rng.standard_normal([1, t, 2, d]).astype(np.float32)
        k, v = (rng.standard_normal([1, length, 1, d]).astype(np.float32) for _ in range(2))
        scale = 1.0 / np.sqrt(d)
        ctx, lse = DR.split_model(q, k, v, length, scale, causal, splits)
        want_ctx, want_lse = DR.decode_attention(q, k, v, length, scale, causal)
        x = R.exponent_magnitude(q, k, scale, want_lse)
        frac_ctx = float((np.abs(ctx - want_ctx) / (R.exponent_tol(2e-6, x) * (1 + np.abs(want_ctx)))).max())
        frac_lse = float(np.abs(lse - want_lse).max() / R.exponent_tol(3e-6, x))
        assert np.isfinite(ctx).all() and frac_ctx < 0.5 and frac_lse < 0.5, (length, d, splits, t, causal, frac_ctx, frac_lse)
        worst_ctx, worst_lse = max(worst_ctx, frac_ctx), max(worst_lse, frac_lse)
    print(f'split model: worst {worst_ctx:.3f} of the ctx bound, {worst_lse:.3f} of the lse bound')


def test_split_model_gives_empty_splits_weight_zero():
    rng = np.random.default_rng(3)
    q = rng.standard_normal([1, 3, 2, 16]).astype(np.float32)
    k, v = (rng.standard_normal([1, 40, 1, 16]).astype(np.float32) for _ in range(2))
    ranges = DR.split_ranges(40, 7)
    assert any(lo == hi for lo, hi in ranges) and ranges[0] == (0, 16) and max(hi for _, hi in ranges) == 40
    one = DR.split_model(q, k, v, 40, 0.25, True, 1)
    many = DR.split_model(q, k, v, 40, 0.25, True, 7)
    assert np.isfinite(many[0]).all() and np.isfinite(many[1]).all()
    np.testing.assert_allclose(many[0], one[0], rtol=1e-5, atol=1e-6)
    assert [DR.auto_splits(*a) for a in ((1, 1, 100), (1, 1, 8192), (64, 8, 8192), (8, 2, 2048), (1, 8, 1 << 20))] == [1, 32, 1, 8, 64]


# ---- host logic on the simulator -------------------------------------------------------------------------------------------
npm = npm_fixture('decode')


def test_cache_bookkeeping_overflow_and_reset(npm):
    D = npm.device
    cache = D.KVCache(2, 6, 3, 16)
    assert (cache.k.shape, cache.v.shape, cache.length) == ((2, 6, 3, 16), (2, 6, 3, 16), 0)
    rows = D.from_host(np.arange(2 * 4 * 48, dtype=np.float32).reshape(2, 4, 48))
    cache.append(D.Mat(rows, 48), D.Mat(rows, 48), 4)
    assert cache.length == 4
    np.testing.assert_array_equal(np.asarray(cache.k)[:, :4].reshape(2, 4, 48), np.asarray(rows))
    before = len(npm.sim.calls)
    with pytest.raises(ValueError):
        cache.append(D.Mat(rows, 48), D.Mat(rows, 48), 3)               # 4 + 3 > 6
    assert len(npm.sim.calls) == before and cache.length == 4          # raised before any call
    cache.append(D.Mat(rows, 48), D.Mat(rows, 48), 2)
    assert cache.length == 6
    cache.reset()
    assert cache.length == 0 and not cache.frozen
    with pytest.raises(ValueError):
        D.KVCache(2, 0, 3, 16)


def test_write_slot_replaces_one_sequence(npm):
    D = npm.device
    b, cap, hkv, d, length = 3, 8, 2, 16, 6
    row = hkv * d
    rng = np.random.default_rng(0)
    cache = D.KVCache(b, cap, hkv, d)
    for x in (cache.k, cache.v):                                          # rows past the lengths included: they must stay too
        x.set(rng.standard_normal([b, cap, hkv, d]).astype(np.float32))
    filled = D.from_host(rng.standard_normal([b, length, row]).astype(np.float32))
    cache.append(D.Mat(filled, row), D.Mat(filled, row), length)
    before_k, before_v = np.asarray(cache.k).copy(), np.asarray(cache.v).copy()
    new_k, new_v = (rng.standard_normal([5, row + 4]).astype(np.float32) for _ in range(2))   # a row pitch larger than the row
    calls = len(npm.sim.calls)
    cache.write_slot(1, D.Mat(D.from_host(new_k), row + 4), D.Mat(D.from_host(new_v), row + 4), 5)
    assert npm.sim.calls[calls:] == ['npm_kv_append', 'npm_kv_append']
    assert cache.lengths.tolist() == [length, 5, length] and cache.ragged
    got_k, got_v = np.asarray(cache.k), np.asarray(cache.v)
    assert np.array_equal(got_k[1, :5].reshape(5, row), new_k[:, :row]) and np.array_equal(got_v[1, :5].reshape(5, row), new_v[:, :row])
    for i in (0, 2):
        assert np.array_equal(got_k[i].view(np.uint32), before_k[i].view(np.uint32))
        assert np.array_equal(got_v[i].view(np.uint32), before_v[i].view(np.uint32))
    assert np.array_equal(got_k[1, 5:].view(np.uint32), before_k[1, 5:].view(np.uint32))    # nor a row behind the new ones
    calls = len(npm.sim.calls)
    too_many = D.Mat(D.from_host(np.zeros([cap + 1, row], dtype=np.float32)), row)
    with pytest.raises(ValueError):
        cache.write_slot(1, too_many, too_many, cap + 1)
    with pytest.raises(IndexError):
        cache.write_slot(3, too_many, too_many, 1)
    assert len(npm.sim.calls) == calls and cache.lengths.tolist() == [length, 5, length]
    with pytest.raises(NotImplementedError):
        D.PagedKVCache(b, cap, hkv, d, page_size=16).write_slot(1, too_many, too_many, 1)


@pytest.mark.parametrize('heads,kv_heads,f', [(4, 4, 64), (8, 2, 128), (4, 1, 64)])
def test_layer_with_cache_equals_the_full_causal_forward(npm, heads, kv_heads, f):
    att, p = DC.make_mha(npm, f, heads, kv_heads, seed=heads)
    s = 13
    x = np.random.default_rng(0).standard_normal([2, s, f]).astype(np.float32)
    want, _ = DR.att_fwd(p, x.astype(np.float64), mask=DR.causal_mask(s))
    for sizes in DC.chunkings(s):
        got, paths = DC.run_mha_chunks(att, x, sizes, capacity=s + 2)
        assert paths == ['decode' if heads // kv_heads * t <= 32 else 'fused_masked' for t in sizes]
        np.testing.assert_allclose(got, want, rtol=2e-6, atol=2e-6)
    assert npm.sim.npm_last_decode_kernel().decode().startswith(f'mha_decode_kernel D={f // heads} rows=')


def test_fallback_selection(npm):
    """More rows than the decode kernel takes -> the fused forward with a causal mask; other head sizes -> the GEMM composition;
    a split math mode -> not the decode kernel.  Same results to rounding."""
    s = 40
    att, p = DC.make_mha(npm, 64, 4, 1, seed=5)                       # 4 heads on 1 K / V head: 4 T rows, 32 at T = 8
    x = np.random.default_rng(1).standard_normal([2, s, 64]).astype(np.float32)
    want, _ = DR.att_fwd(p, x.astype(np.float64), mask=DR.causal_mask(s))
    got, paths = DC.run_mha_chunks(att, x, [20, 8, 9, 3], capacity=s)
    assert paths == ['fused_masked', 'decode', 'fused_masked', 'decode']
    np.testing.assert_allclose(got, want, rtol=2e-6, atol=2e-6)
    assert 'npm_mha_core_fwd_grouped' in npm.sim.calls
    att12, p12 = DC.make_mha(npm, 48, 4, 2, seed=6)                   # head size 12
    x = np.random.default_rng(2).standard_normal([2, 9, 48]).astype(np.float32)
    want, _ = DR.att_fwd(p12, x.astype(np.float64), mask=DR.causal_mask(9))
    for sizes in DC.chunkings(9):
        got, paths = DC.run_mha_chunks(att12, x, sizes, capacity=12)
        assert set(paths) == {'gemm'}
        np.testing.assert_allclose(got, want, rtol=2e-6, atol=2e-6)
    npm.set_math('bf16x3')
    try:
        _, paths = DC.run_mha_chunks(att, x[:, :, :48].repeat(2, axis=2)[:, :, :64], [4, 1], capacity=8)
        assert paths == ['fused_masked', 'fused_masked']
    finally:
        npm.set_math('f32')


def test_backward_after_a_cached_forward_raises(npm):
    att, _ = DC.make_mha(npm, 64, 4, 2, seed=7)
    x = np.random.default_rng(3).standard_normal([2, 3, 64]).astype(np.float32)
    att(x, cache=att.make_cache(2, 8))
    with pytest.raises(RuntimeError, match='inference only'):
        att(x, backprop=True, learning_rate=1e-3)
    att(x)                                                             # a forward without a cache saves its activations again
    att(x, backprop=True, learning_rate=1e-3)
    with pytest.raises(ValueError):
        att(x, x, cache=att.make_cache(2, 8))                          # keys go through fill_cache


def test_frozen_cross_cache_never_grows(npm):
    att, p = DC.make_mha(npm, 64, 4, 2, seed=8)
    rng = np.random.default_rng(4)
    kv = rng.standard_normal([2, 6, 64]).astype(np.float32)
    cache = att.fill_cache(att.make_cache(2, 6), kv)
    assert cache.frozen and cache.length == 6
    for t in (1, 3):
        x = rng.standard_normal([2, t, 64]).astype(np.float32)
        got = np.asarray(att(x, cache=cache))
        want, _ = DR.att_fwd(p, x.astype(np.float64), kv.astype(np.float64), kv.astype(np.float64))
        np.testing.assert_allclose(got, want, rtol=2e-6, atol=2e-6)
        assert cache.length == 6
    with pytest.raises(ValueError):
        att.fill_cache(att.make_cache(2, 5), kv)                       # 6 rows do not fit 5
    with pytest.raises(ValueError):
        cache.append(None, None, 0)                                    # a frozen cache takes no rows
    empty = att.make_cache(2, 4)
    empty.frozen = True
    with pytest.raises(ValueError):
        att(np.zeros([2, 1, 64], dtype=np.float32), cache=empty)       # frozen but never filled


@pytest.mark.parametrize('norm_first', [True, False])
@pytest.mark.parametrize('kv_heads', [None, 2])
def test_causal_decoder_and_decode_on_the_simulator(npm, norm_first, kv_heads):
    f, s = 64, 11
    dec, p = DC.make_decoder(npm, f, 4, kv_heads, 96, norm_first, True, seed=9)
    rng = np.random.default_rng(5)
    q, kv, dy = (rng.standard_normal(shape).astype(np.float32) for shape in ([2, s, f], [2, 7, f], [2, s, f]))
    want, c = DR.decoder_fwd(p, q.astype(np.float64), kv.astype(np.float64), norm_first, mask=DR.causal_mask(s))
    (want_dq, want_dkv), want_g = DR.decoder_bwd(p, c, dy.astype(np.float64), norm_first)
    out = np.asarray(dec(q, kv))
    np.testing.assert_allclose(out, want, rtol=1e-5, atol=1e-5)
    made = dec._causal_masks[(2, s)]
    dec(q, kv)
    assert dec._causal_masks[(2, s)] is made and dec._self_attention._mask is made                   # made once per (B, Sq)
    rec = DC.GradRecorder()
    dq, dkv = dec(dy, backprop=True, optimizer_=rec)
    np.testing.assert_allclose(np.asarray(dq), want_dq, rtol=1e-4, atol=1e-5)
    np.testing.assert_allclose(np.asarray(dkv), want_dkv, rtol=1e-4, atol=1e-5)
    for name, grad in rec.named(dec).items():
        np.testing.assert_allclose(grad, want_g[name], rtol=1e-4, atol=2e-5 * max(1.0, np.abs(want_g[name]).max()), err_msg=name)
    for sizes in DC.chunkings(s):
        got = DC.run_decoder_chunks(dec, q, kv, sizes, capacity=s)
        np.testing.assert_allclose(got, out, rtol=1e-5, atol=1e-5)
    with pytest.raises(RuntimeError, match='inference only'):
        dec(dy, backprop=True, learning_rate=1e-3)
    state = dec.start_decoding(kv, 4)
    before = len(npm.sim.calls)
    with pytest.raises(ValueError):
        dec.decode(q[:, :5], state)                                    # 5 tokens do not fit 4
    assert len(npm.sim.calls) == before and state.position == 0


def test_default_decoder_passes_no_mask(npm):
    dec, p = DC.make_decoder(npm, 64, 4, None, 96, True, False, seed=10)
    rng = np.random.default_rng(6)
    q, kv = rng.standard_normal([2, 9, 64]).astype(np.float32), rng.standard_normal([2, 7, 64]).astype(np.float32)
    want, _ = O.decoder_fwd(p, q.astype(np.float64), kv.astype(np.float64), True)
    np.testing.assert_allclose(np.asarray(dec(q, kv)), want, rtol=1e-5, atol=1e-5)
    assert dec._self_attention._mask is None and not dec._causal_masks
    with pytest.raises(RuntimeError):
        npm.layers.TransformerDecoder(num_heads=4, hidden_units=8, norm_first=True).start_decoding(kv, 4)


# ---- the C ABI ---------------------------------------------------------------------------------------------------------------
def test_decode_struct_layout_matches_header(built):
    """npm_mha_decode: field order of the ctypes mirror equals the C declaration; size and offsets as a C compiler sees them."""
    _C = built
    text = open(os.path.join(ROOT, 'include', 'npm_hip.h')).read()
    body = re.search(r'typedef struct npm_mha_decode \{(.*?)\} npm_mha_decode;', text, flags=re.S).group(1)
    body = re.sub(r'/\*.*?\*/', '', body, flags=re.S)
    fields = []
    for decl in filter(None, (d.strip() for d in body.split(';'))):
        decl = re.sub(r'^(const\s+)?(float|int32_t|int64_t|uint8_t)\s*\*?', '', decl)
        fields += [n.strip().lstrip('*') for n in decl.split(',')]
    assert fields == [f[0] for f in _C.npm_mha_decode._fields_]
    names = ('kv_len', 'causal', 'scale', 'q', 'k_stride_b', 'v', 'ctx', 'lse')
    prog = ('#include <stdio.h>\n#include <stddef.h>\n#include "npm_hip.h"\nint main(void){printf("%zu", sizeof(npm_mha_decode));'
            + ''.join('printf(" %%zu", offsetof(npm_mha_decode, %s));' % n for n in names)
            + 'printf(" %d %d %d %d\\n", NPM_ABI_VERSION, NPM_TUNE_DECODE_SPLITS, NPM_DECODE_MAX_ROWS, NPM_DECODE_MAX_SPLITS);return 0;}\n')
    with tempfile.TemporaryDirectory() as tmp:
        src = os.path.join(tmp, 'probe.c')
        with open(src, 'w') as f:
            f.write(prog)
        exe = os.path.join(tmp, 'probe')
        subprocess.run(['gcc', '-std=c99', '-I', os.path.join(ROOT, 'include'), src, '-o', exe], check=True)
        got = [int(x) for x in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split()]
    want = [ctypes.sizeof(_C.npm_mha_decode)] + [getattr(_C.npm_mha_decode, n).offset for n in names]
    assert got == want + [2, _C.TUNE_DECODE_SPLITS, 32, 1024]


def test_decode_entry_points_are_exported_and_bound(built):
    _C = built
    lib = ctypes.CDLL(_C.LIB_PATH)
    for name in ('npm_mha_decode_supported', 'npm_mha_decode_fwd', 'npm_mha_decode_splits', 'npm_kv_append', 'npm_last_decode_kernel'):
        assert hasattr(lib, name), f'{name} not exported'
        assert name in _C.SIGNATURES or name in _C._SPECIAL
    assert _C.SIGNATURES['npm_mha_decode_fwd'] == [ctypes.POINTER(_C.npm_mha_decode)]
    bound = _C.load_library()
    assert bound.npm_last_decode_kernel.restype is ctypes.c_char_p and bound.npm_last_decode_kernel() == b''
    assert bound.npm_mha_decode_supported(128, 32) == 1 and bound.npm_mha_decode_supported(128, 33) == 0
    assert bound.npm_mha_decode_supported(12, 1) == 0
    assert [bound.npm_mha_decode_splits(*a) for a in ((1, 1, 100), (1, 1, 8192), (64, 8, 8192), (8, 2, 2048))] == \
        [DR.auto_splits(*a) for a in ((1, 1, 100), (1, 1, 8192), (64, 8, 8192), (8, 2, 2048))]
