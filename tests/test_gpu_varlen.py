"""GPU: ragged batches in the key / value cache -- npm_mha_decode_fwd_varlen / npm_kv_append_varlen / npm_kv_gather_varlen
(csrc/npm_decode.hip) through the C ABI, then MultiHeadAttention(cache=, new_lengths=) and TransformerDecoder.decode(new_lengths=).

Reference.  Float64, every sequence ALONE with its own unpadded rows (tests/varlen_reference.py on tests/decode_reference.py).
Bounds.  No new one: the kernel is held to what tests/test_gpu_decode.py holds npm_mha_decode_fwd to -- ctx |got - ref| <=
2e-6 (1 + |ref|), lse within 3e-6, grown by tests/attn_range_data.py's tol(X) -- per sequence; tests/test_varlen_host.py shows
that a float32 model of the split / combine rule with the partition taken from Lmax stays under half of it on this grid.  Layers
and the decoder: the bounds of that file's layer and decoder tests (1e-5 (|ref| + max |ref|) against float64, twice that between
two float32 evaluations, 1e-4 for the decoder).  Every valid element is compared; padded rows must be finite (ctx == 0 and
lse == -inf at the kernel level); guard regions keep their sentinel.

Every test names an entry point or keyword that does not exist without this feature.
"""

import numpy as np
import pytest

import decode_cases as DC
import decode_gpu
import varlen_reference as VR
from decode_gpu import GUARD, NT_KNOB, SENTINEL
from decode_gpu import check as _check, data as _data, guarded as _guarded, ints as _ints, layer_close as _layer_close
from decode_gpu import poison as _poison, run as _run, set_splits as _set_splits

pytestmark = pytest.mark.gpu

LAYER_TOL = 1e-5


@pytest.fixture(scope='module')
def npm():
    import np_modeling_amd
    return np_modeling_amd


@pytest.fixture(autouse=True)
def _defaults_afterwards(npm):
    yield
    decode_gpu.reset_knobs()


# ---- npm_mha_decode_fwd_varlen ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', VR.kernel_cases(), ids=VR.case_id)
def test_varlen_kernel_against_float64(npm, case):
    from np_modeling_amd import _C
    d, hq, hkv, t, causal, lengths, n, packed, mode = case
    b, lmax = len(lengths), int(lengths.max())
    q, k, v = _data(d * 1000 + hq * 100 + t * 10 + causal + lmax, b, t, hq, hkv, d, lmax + 3)
    qn, kn, vn = _poison(q, k, v, lengths, n)                              # NaN wherever nothing may be looked at
    scale = 1.0 / np.sqrt(d)
    forced = _set_splits(mode, lmax)
    splits = forced or _C.lib().npm_mha_decode_splits(b, hkv, lmax)
    assert splits == VR.split_count(mode, lmax, b, hkv)
    ctx, lse, kernel = _run(qn, kn, vn, lmax, scale, causal, lengths, n, packed=packed)
    assert kernel == f'mha_decode_kernel D={d} rows={hq // hkv * t} splits={splits} causal={causal} varlen=1'
    _check(ctx, lse, q, k, v, lengths, n, scale, causal, kernel + f' L={lengths.tolist()} n={n.tolist()}')


@pytest.mark.parametrize('mode', ['one', 'auto', 'many'])
@pytest.mark.parametrize('d,hq,hkv,t,length,b,causal', [(128, 8, 2, 1, 8192, 2, 1), (64, 8, 8, 2, 2049, 3, 1), (16, 8, 1, 4, 129, 64, 0),
                                                        (32, 6, 3, 5, 700, 3, 1), (128, 8, 1, 4, 300, 5, 0)])
def test_uniform_lengths_are_bitwise_the_uniform_entry_point(npm, d, hq, hkv, t, length, b, causal, mode):
    q, k, v = _data(7 + d + t, b, t, hq, hkv, d, length + 5)
    scale = 1.0 / np.sqrt(d)
    _set_splits(mode, length)
    base = _run(q, k, v, length, scale, causal)
    for new_lens in (None, [t] * b):                                      # NULL new_lens: every sequence brings all T
        got = _run(q, k, v, length, scale, causal, [length] * b, new_lens)
        assert np.array_equal(base[0].view(np.uint32), got[0].view(np.uint32)), 'ctx differs in bits'
        assert np.array_equal(base[1].view(np.uint32), got[1].view(np.uint32)), 'lse differs in bits'
        assert got[2] == base[2] + ' varlen=1'


@pytest.mark.parametrize('mode', ['one', 'auto', 37])
@pytest.mark.parametrize('d,hq,hkv,t,causal,lengths,n', [(128, 8, 2, 2, 1, (2049, 17, 1, 600), (2, 1, 0, 2)),
                                                         (64, 8, 8, 4, 0, (0, 300, 16, 5000), (4, 0, 1, 3)),
                                                         (16, 8, 1, 4, 1, (33, 32, 31, 4), (4, 1, 0, 4))])
def test_same_ragged_call_twice_is_bitwise_equal_and_the_unseen_never_matters(npm, d, hq, hkv, t, causal, lengths, n, mode):
    """The same call twice: identical bits (no atomics).  Zeros, NaN or 1e30 past the lengths and in the padded query rows, a larger
    capacity, either load policy: identical bits."""
    from np_modeling_amd import _C
    lengths, n = np.array(lengths), np.array(n)
    lmax = int(lengths.max())
    q, k, v = _data(3 + d, len(lengths), t, hq, hkv, d, lmax + 37)
    scale = 1.0 / np.sqrt(d)
    runs = []
    for fill, extra, nt in ((0.0, 37, 2), (0.0, 37, 2), (np.nan, 37, 2), (1e30, 5, 1)):
        qq, kk, vv = _poison(q, k[:, :lmax + extra], v[:, :lmax + extra], lengths, n, fill)
        _set_splits(mode, lmax)
        _C.check(_C.lib().npm_set_tuning(NT_KNOB, nt), 'npm_set_tuning')
        runs.append(_run(qq, kk, vv, lmax, scale, causal, lengths, n))
    for other in runs[1:]:
        assert np.array_equal(runs[0][0].view(np.uint32), other[0].view(np.uint32))
        assert np.array_equal(runs[0][1].view(np.uint32), other[1].view(np.uint32)) and runs[0][2] == other[2]
    _check(runs[2][0], runs[2][1], q, k, v, lengths, n, scale, causal, f'poisoned {runs[2][2]}')


def test_varlen_bad_arguments(npm):
    q, k, v = _data(2, 2, 2, 4, 2, 32, 8)
    _run(q, k, v, 8, 0.2, 1, null_lens=True, expect=10002)                # kv_lens == NULL
    q, k, v = _data(2, 1, 2, 4, 2, 24, 8)
    _run(q, k, v, 8, 0.2, 1, [8], expect=10003)                           # head size 24
    q, k, v = _data(4, 1, 1, 6, 4, 32, 8)
    _run(q, k, v, 8, 0.2, 1, [8], expect=10002)                           # heads % kv_heads
    q, k, v = _data(5, 2, 4, 4, 2, 32, 8)
    ctx, lse, _ = _run(q, k, v, 3, 0.2, 1, [3, 1], [3, 1])                # d->kv_len < new_tokens is fine: the rule is per sequence
    _check(ctx, lse, q, k, v, np.array([3, 1]), np.array([3, 1]), 0.2, 1, 'kv_len < T')


# ---- npm_kv_append_varlen / npm_kv_gather_varlen -----------------------------------------------------------------------------------
@pytest.mark.parametrize('b,t,hkv,d,cap,at,n', [(3, 5, 2, 16, 40, (0, 35, 7), (5, 5, 0)), (1, 1, 8, 128, 9, (4,), (1,)),
                                                (64, 7, 1, 32, 9, None, None), (2, 129, 3, 64, 300, (171, 0), (129, 1)),
                                                (4, 3, 2, 32, 6, (0, 3, 6, 5), (3, 3, 0, 1))])
@pytest.mark.parametrize('packed', [False, True])
def test_kv_append_varlen_is_exact(npm, b, t, hkv, d, cap, at, n, packed):
    from np_modeling_amd import _C, device as D
    rng = np.random.default_rng(b + t)
    at = rng.integers(0, cap - t + 1, b) if at is None else np.array(at)
    n = rng.integers(0, t + 1, b) if n is None else np.array(n)
    row = hkv * d
    pitch = 3 * row + 8 * d if packed else row                           # the K part of a packed [B, T, Hq + 2 Hkv, D] projection
    offset = 8 * d if packed else 0
    src = rng.standard_normal([b * t, pitch]).astype(np.float32)
    before = rng.standard_normal([b, cap, row]).astype(np.float32)
    want = before.copy()
    for i in range(b):
        want[i, at[i]:at[i] + n[i]] = src.reshape(b, t, pitch)[i, :n[i], offset:offset + row]
    for new in (n, None):
        sd = D.from_host(src)
        cache = D.full([b * cap * row + GUARD], SENTINEL)
        cache.flat_view(0, [b * cap * row]).set(before.ravel())
        at_dev, n_dev = _ints(at), _ints(n)
        if new is None:                                                   # NULL new_lens: every token
            if (at + t > cap).any():
                continue
            want = before.copy()
            for i in range(b):
                want[i, at[i]:at[i] + t] = src.reshape(b, t, pitch)[i, :, offset:offset + row]
        _C.check(_C.lib().npm_kv_append_varlen(sd.ptr + 4 * offset, pitch, cache.ptr, row, cap * row, b, t, row, at_dev.ptr,
                                               None if new is None else n_dev.ptr), 'npm_kv_append_varlen')
        got = _guarded(cache, b * cap * row).reshape(b, cap, row)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


@pytest.mark.parametrize('b,hkv,d,cap,rows,lens', [(3, 2, 16, 40, 37, (3, 37, 0)), (1, 8, 128, 9, 9, (4,)), (64, 1, 32, 9, 8, None),
                                                   (2, 3, 64, 300, 129, (129, 40))])
def test_kv_gather_varlen_is_exact_and_its_tail_is_zero(npm, b, hkv, d, cap, rows, lens):
    from np_modeling_amd import _C, device as D
    rng = np.random.default_rng(b + rows)
    lens = rng.integers(0, rows + 1, b) if lens is None else np.array(lens)
    row = hkv * d
    cache = rng.standard_normal([b, cap, row]).astype(np.float32)
    want = np.where((np.arange(rows)[None, :] < lens[:, None])[:, :, None], cache[:, :rows], np.float32(0))
    cache[np.arange(cap)[None, :] >= lens[:, None]] = np.nan              # the rows past a length are not even read
    out = D.full([b * rows * row + GUARD], SENTINEL)
    lens_dev = _ints(lens)
    _C.check(_C.lib().npm_kv_gather_varlen(D.from_host(cache).ptr, row, cap * row, out.ptr, b, rows, row, lens_dev.ptr),
             'npm_kv_gather_varlen')
    got = _guarded(out, b * rows * row).reshape(b, rows, row)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    lib = _C.lib()
    assert lib.npm_kv_gather_varlen(out.ptr, row, cap * row, out.ptr, b, rows, row, None) == 10002          # lens == NULL
    assert lib.npm_kv_append_varlen(out.ptr, row, out.ptr, row, cap * row, b, 1, row, None, None) == 10002   # at_lens == NULL
    assert lib.npm_kv_append_varlen(out.ptr, row, out.ptr, row, cap * row, b, 1, 14, lens_dev.ptr, None) == 10002   # row_len % 4


# ---- MultiHeadAttention with a cache and per-sequence lengths ------------------------------------------------------------------
def _poison_cache(cache):
    """NaN into every row at and past each sequence's length."""
    for arr in (cache.k, cache.v):
        host = np.asarray(arr).copy()
        host[np.arange(cache.capacity)[None, :] >= cache.lengths[:, None]] = np.nan
        arr.set(host)


def _ragged_run(att, x_rows, schedule, capacity, expect_paths, pad=0.0, poison=False):
    from np_modeling_amd import _C
    cache = att.make_cache(len(x_rows), capacity)
    outs = []
    for (x, n), path in zip(VR.padded_calls(x_rows, schedule, pad), expect_paths):
        if poison:
            _poison_cache(cache)
        out = np.asarray(att(x, cache=cache, new_lengths=n))
        assert np.isfinite(out).all() and att._cached_path == path, (att._cached_path, path, n)
        if path == 'decode':
            assert _C.last_decode_kernel().endswith('causal=1 varlen=1')
        outs.append(out)
    assert cache.lengths.tolist() == VR.schedule_rows(schedule).tolist()
    return VR.collect(outs, schedule, len(x_rows))


@pytest.mark.parametrize('heads,kv_heads,f', [(8, 8, 1024), (8, 2, 1024), (8, 1, 512), (4, 4, 64), (6, 3, 192)])
def test_layer_ragged_prefill_then_steps_against_each_sequence_alone(npm, heads, kv_heads, f):
    """Ragged prefill (3, 37, 64 tokens: the fused masked forward), then single tokens with sequence 1 stopping early, a chunk of
    two, and more single tokens; head sizes 128, 64, 16, 32."""
    att, p = DC.make_mha(npm, f, heads, kv_heads, seed=heads + f, batch=3)
    schedule = [np.array(n) for n in ([3, 37, 64], [1, 1, 1], [1, 1, 1], [1, 0, 1], [2, 0, 1], [1, 0, 0], [1, 0, 1])]
    total = VR.schedule_rows(schedule)
    g = heads // kv_heads
    paths = ['decode' if g * int(n.max()) <= 32 else 'fused_masked' for n in schedule]
    assert paths[0] == 'fused_masked' and paths[1] == 'decode'
    rng = np.random.default_rng(f)
    x_rows = [rng.standard_normal([s, f]).astype(np.float32) for s in total]
    want = VR.layer_alone(p, x_rows, schedule)
    got = _ragged_run(att, x_rows, schedule, int(total.max()) + 5, paths)
    poisoned = _ragged_run(att, x_rows, schedule, int(total.max()) + 5, paths, pad=3.0, poison=True)
    for i in range(3):
        sizes = [int(n[i]) for n in schedule if n[i]]
        alone, _ = DC.run_mha_chunks(att, x_rows[i][None], sizes, capacity=int(total[i]))     # the same layer, batch 1, no padding
        _layer_close(got[i], want[i], LAYER_TOL, f'ragged H{heads}/{kv_heads} sequence {i} vs float64')
        _layer_close(got[i], alone[0], 2 * LAYER_TOL, f'ragged H{heads}/{kv_heads} sequence {i} vs alone')
        assert np.array_equal(got[i], poisoned[i]), f'sequence {i}: NaN past the lengths / other padding changed valid rows'


def test_layer_ragged_chunk_behind_a_ragged_cache_gathers(npm):
    """A second chunk too large for the decode kernel on a cache that is already ragged: npm_kv_gather_varlen feeds the fused
    forward, and NaN past the lengths reaches nothing."""
    att, p = DC.make_mha(npm, 256, 8, 1, seed=21, batch=3)               # 8 T rows per K / V head: T = 5 is too many
    schedule = [np.array(n) for n in ([2, 4, 1], [9, 3, 40], [1, 1, 1], [0, 6, 2])]
    paths = ['decode', 'fused_masked', 'decode', 'fused_masked']
    total = VR.schedule_rows(schedule)
    rng = np.random.default_rng(3)
    x_rows = [rng.standard_normal([s, 256]).astype(np.float32) for s in total]
    want = VR.layer_alone(p, x_rows, schedule)
    got = _ragged_run(att, x_rows, schedule, int(total.max()) + 9, paths)
    poisoned = _ragged_run(att, x_rows, schedule, int(total.max()) + 9, paths, poison=True)
    for i in range(3):
        _layer_close(got[i], want[i], LAYER_TOL, f'gathered sequence {i} vs float64')
        assert np.array_equal(got[i], poisoned[i])


def test_layer_cross_attention_over_padded_memory(npm):
    att, p = DC.make_mha(npm, 256, 8, 2, seed=3, batch=3)
    rng = np.random.default_rng(8)
    kv = rng.standard_normal([3, 50, 256]).astype(np.float32)
    kv_lengths = np.array([50, 1, 23])
    cache = att.fill_cache(att.make_cache(3, 64), kv, lengths=kv_lengths)
    _poison_cache(cache)
    assert cache.frozen and cache.lengths.tolist() == [50, 1, 23]
    for n in ([1, 1, 1], [4, 0, 2], [70, 9, 33]):                         # the last: more rows than the decode kernel takes
        n = np.array(n)
        x_rows = [rng.standard_normal([s, 256]).astype(np.float32) for s in n]
        (x, _), = VR.padded_calls(x_rows, [n], pad=-2.0)
        out = np.asarray(att(x, cache=cache, new_lengths=n))
        assert np.isfinite(out).all() and att._cached_path == ('decode' if 4 * n.max() <= 32 else 'fused_masked')
        assert cache.lengths.tolist() == [50, 1, 23]
        for i, (got, want) in enumerate(zip(VR.collect([out], [n], 3), VR.cross_alone(p, x_rows, kv, kv_lengths))):
            if n[i]:                                                      # a sequence that only rides along has no valid row
                _layer_close(got, want, LAYER_TOL, f'cross n={n.tolist()} sequence {i}')


def test_layer_overflow_of_one_sequence_raises_before_any_launch(npm):
    att, _ = DC.make_mha(npm, 64, 4, 2, seed=4)
    cache = att.make_cache(2, 5)
    att(np.zeros([2, 4, 64], dtype=np.float32), cache=cache, new_lengths=[4, 1])
    before = np.asarray(cache.k).copy()
    with pytest.raises(ValueError):
        att(np.ones([2, 2, 64], dtype=np.float32), cache=cache, new_lengths=[2, 2])      # 4 + 2 > 5 for sequence 0 alone
    assert cache.lengths.tolist() == [4, 1] and np.array_equal(np.asarray(cache.k)[0, :4], before[0, :4])
    att(np.ones([2, 2, 64], dtype=np.float32), cache=cache, new_lengths=[1, 2])
    assert cache.lengths.tolist() == [5, 3]


# ---- TransformerDecoder.decode ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('norm_first', [True, False])
@pytest.mark.parametrize('kv_heads', [None, 2])
def test_decoder_decode_ragged_end_to_end(npm, norm_first, kv_heads):
    f = 256
    dec, p = DC.make_decoder(npm, f, 4, kv_heads, 384, norm_first, True, seed=11, batch=3, seq_kv=23)
    schedule = [np.array(n) for n in ([45, 2, 17], [1, 1, 1], [1, 1, 0], [1, 0, 0], [3, 0, 1], [1, 0, 1])]
    total = VR.schedule_rows(schedule)
    rng = np.random.default_rng(12)
    q_rows = [rng.standard_normal([s, f]).astype(np.float32) for s in total]
    kv = rng.standard_normal([3, 23, f]).astype(np.float32)
    kv_lengths = np.array([23, 4, 11])
    want = VR.decoder_alone(p, q_rows, schedule, kv, kv_lengths, norm_first)
    state = dec.start_decoding(kv, int(total.max()) + 3, kv_lengths=kv_lengths)
    outs = []
    for x, n in VR.padded_calls(q_rows, schedule):
        outs.append(np.asarray(dec.decode(x, state, new_lengths=n)))
        assert np.isfinite(outs[-1]).all()
    assert state.positions.tolist() == total.tolist() and state.cross_cache.lengths.tolist() == kv_lengths.tolist()
    got = VR.collect(outs, schedule, 3)
    for i in range(3):
        alone_state = dec.start_decoding(kv[i:i + 1, :kv_lengths[i]], int(total[i]))
        alone = np.concatenate([np.asarray(dec.decode(np.ascontiguousarray(c), alone_state))
                                for c in VR.DR_split(q_rows[i][None], [int(n[i]) for n in schedule])], axis=1)[0]
        _layer_close(got[i], alone, 2 * LAYER_TOL, f'decode ragged sequence {i} vs alone')
        _layer_close(got[i], want[i], 1e-4, f'decode ragged sequence {i} vs float64')
