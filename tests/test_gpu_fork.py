"""GPU: forks of a paged key / value cache and their copy-on-write -- npm_kv_copy_pages (csrc/npm_decode.hip) through the C ABI,
then ``PagedKVCache.fork`` under MultiHeadAttention and ``TransformerDecoder.fork`` with ``device.SHARED_PREFIX`` off.

The copy is held to byte equality: rows below rows[i] of the destination page are the source's, everything else of the pool --
the rows at and past rows[i], other pages, the guard region -- keeps its sentinel.  A fork shares pages and changes no
arithmetic, so with the switch off the outputs of forked sequences that then diverge are array_equal to the same calls on a cache
in which every sequence was filled on its own; the decoder is held to every sequence decoded alone in float64 at
tests/test_gpu_paged.py's decoder bound (1e-4).

Every test names ``fork``, ``refcount`` or npm_kv_copy_pages: none exists without this feature.
"""

import numpy as np
import pytest

import decode_cases as DC
import varlen_reference as VR
import window_cases as WC
from decode_gpu import GUARD, SENTINEL
from decode_gpu import ints as _ints, layer_close as _layer_close

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def npm():
    import np_modeling_amd
    return np_modeling_amd


# ---- npm_kv_copy_pages --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', [np.float32, np.float16])
@pytest.mark.parametrize('n', [1, 70])
@pytest.mark.parametrize('page_rows,row_len', [(16, 32), (64, 1024), (16, 8)])
def test_kv_copy_pages_copies_the_valid_rows_and_nothing_else(npm, dtype, n, page_rows, row_len):
    """rows 0, 1, page_rows - 1 and a whole page, round robin over the pairs; f32 and f16 pools through the same entry point."""
    from np_modeling_amd import _C, device as D
    rng = np.random.default_rng(n + page_rows)
    pages = 2 * n + 3
    size = np.dtype(dtype).itemsize
    order = rng.permutation(pages)
    src, dst = order[:n], order[n:2 * n]
    rows = np.array([(0, 1, page_rows - 1, page_rows)[(i + n) % 4] for i in range(n)])
    guard = GUARD * 4 // size
    host = np.full([pages * page_rows * row_len + guard], SENTINEL, dtype=dtype)
    pool = host[:pages * page_rows * row_len].reshape(pages, page_rows, row_len)
    pool[src] = rng.standard_normal([n, page_rows, row_len]).astype(dtype)
    want = host.copy()
    wpool = want[:pages * page_rows * row_len].reshape(pages, page_rows, row_len)
    for s, d, r in zip(src, dst, rows):
        wpool[d, :r] = pool[s, :r]
    dev = D.bytes_from_host(host)
    pairs = _ints(np.stack([src, dst, rows]))
    _C.check(_C.lib().npm_kv_copy_pages(dev.ptr, page_rows * row_len * size, row_len * size, pairs.ptr, pairs.ptr + 4 * n,
                                        pairs.ptr + 8 * n, n), 'npm_kv_copy_pages')
    got = dev.numpy().view(dtype)
    bits = {2: np.uint16, 4: np.uint32}[size]
    assert np.array_equal(got.view(bits), want.view(bits))


def test_kv_copy_pages_empty_and_bad_arguments(npm):
    from np_modeling_amd import _C, device as D
    lib = _C.lib()
    buf = D.full([4096], SENTINEL)
    idx = _ints([0, 1, 5])
    p, i = buf.ptr, idx.ptr
    assert lib.npm_kv_copy_pages(None, 1024, 64, None, None, None, 0) == 0          # nothing to copy: NPM_OK whatever the pointers are
    assert lib.npm_kv_copy_pages(p, 1024, 0, i, i + 4, i + 8, 1) == 0
    for args in ((p, 1024, 64, i, i + 4, i + 8, -1), (None, 1024, 64, i, i + 4, i + 8, 1), (p, 1024, 64, None, i + 4, i + 8, 1),
                 (p, 1024, 64, i, None, i + 8, 1), (p, 1024, 64, i, i + 4, None, 1), (p, 1024, 24, i, i + 4, i + 8, 1),
                 (p, 1000, 64, i, i + 4, i + 8, 1), (p + 4, 1024, 64, i, i + 4, i + 8, 1), (p, 32, 64, i, i + 4, i + 8, 1),
                 (p, 1024, -16, i, i + 4, i + 8, 1)):
        assert lib.npm_kv_copy_pages(*args) == 10002, args
    np.testing.assert_array_equal(buf.numpy(), SENTINEL)


# ---- MultiHeadAttention over forked sequences, the switch off --------------------------------------------------------------------------
def _diverge(att, f, cache, tails, schedule):
    outs = []
    at = np.zeros(3, dtype=np.int64)
    for n in schedule:
        n = np.asarray(n)
        t = int(n.max())
        x = np.full([3, t, f], 2.5, dtype=np.float32)
        for i in range(3):
            x[i, :n[i]] = tails[i][at[i]:at[i] + n[i]]
        at += n
        y = np.asarray(att(x, cache=cache, new_lengths=n))
        outs.append([y[i, :n[i]] for i in range(3)])
    return outs


@pytest.mark.parametrize('dtype', ['f32', 'f16'])
@pytest.mark.parametrize('options', [{}, {'rope_base': 10000.0}, {'window': 48}, {'window': 48, 'rope_base': 500.0}],
                         ids=['plain', 'rope', 'window', 'window-rope'])
@pytest.mark.parametrize('page_size', [16, 64])
def test_forked_sequences_that_diverge_equal_sequences_filled_on_their_own(npm, monkeypatch, dtype, options, page_size):
    """A prompt of 100 rows (6 full pages and 4 rows at page 16, 1 and 36 at page 64), forked twice; then single tokens, a chunk
    of two and three, a sequence that pauses.  Copy-on-write happens at the first append of each fork but the last."""
    D = npm.device
    monkeypatch.setattr(D, 'SHARED_PREFIX', False)
    f, heads, kv_heads = 256, 8, 2
    options = dict(options)
    window = options.pop('window', None)
    att, p = WC.make_mha(npm, f, heads, kv_heads, seed=9, window=window, batch=3, **options)
    rng = np.random.default_rng(page_size)
    prompt = rng.standard_normal([100, f]).astype(np.float32)
    schedule = [[1, 1, 1], [1, 0, 1], [2, 1, 2], [3, 3, 0], [1, 1, 1]]
    tails = [rng.standard_normal([8, f]).astype(np.float32) for _ in range(3)]

    own = att.make_cache(3, 112, page_size=page_size, dtype=dtype)
    att(np.repeat(prompt[None], 3, axis=0), cache=own)
    want = _diverge(att, f, own, tails, schedule)

    forked = att.make_cache(3, 112, page_size=page_size, dtype=dtype)
    x = np.zeros([3, 100, f], dtype=np.float32)
    x[0] = prompt
    att(x, cache=forked, new_lengths=[100, 0, 0])
    held = forked.pages_in_use
    forked.fork(0, 1)
    forked.fork(0, 2)
    assert forked.pages_in_use == held and forked.lengths.tolist() == [100, 100, 100]
    got = _diverge(att, f, forked, tails, schedule)
    assert forked.page_copies == 2
    assert forked.pages_in_use < own.pages_in_use                         # the full pages of the prompt are held once
    named = np.bincount(forked.block_table[forked.block_table >= 0], minlength=forked.pages)
    assert np.array_equal(forked.refcount, named)
    for step, (a, b) in enumerate(zip(got, want)):
        for i in range(3):
            assert np.array_equal(a[i].view(np.uint32), b[i].view(np.uint32)), f'step {step} sequence {i} differs from the cache filled on its own'
    if dtype == 'f32' and window is None and not options:
        rows = [np.concatenate([prompt, tail]) for tail in tails]
        ref = VR.layer_alone(p, rows, [[100] * 3] + schedule)
        for i in range(3):
            _layer_close(np.concatenate([o[i] for o in got]), ref[i][100:], 1e-5, f'forked sequence {i} vs float64')


def test_contiguous_fork_copies_rows_and_then_diverges(npm):
    """``KVCache.fork``: the same API without sharing; the rows are copied on the device."""
    f, heads, kv_heads = 128, 4, 2
    att, p = DC.make_mha(npm, f, heads, kv_heads, seed=2, batch=3)
    rng = np.random.default_rng(1)
    prompt = rng.standard_normal([37, f]).astype(np.float32)
    tails = [rng.standard_normal([8, f]).astype(np.float32) for _ in range(3)]
    schedule = [[1, 1, 1], [2, 1, 2], [1, 0, 1]]
    own = att.make_cache(3, 48)
    att(np.repeat(prompt[None], 3, axis=0), cache=own)
    want = _diverge(att, f, own, tails, schedule)
    cache = att.make_cache(3, 48)
    x = np.zeros([3, 37, f], dtype=np.float32)
    x[0] = prompt
    att(x, cache=cache, new_lengths=[37, 0, 0])
    cache.fork(0, 1)
    cache.fork(0, 2)
    assert cache.lengths.tolist() == [37, 37, 37]
    got = _diverge(att, f, cache, tails, schedule)
    for a, b in zip(got, want):
        for i in range(3):
            assert np.array_equal(a[i].view(np.uint32), b[i].view(np.uint32))


# ---- TransformerDecoder.fork ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('norm_first', [True, False])
@pytest.mark.parametrize('options', [dict(page_size=16), dict(page_size=64), {}], ids=['page16', 'page64', 'contiguous'])
def test_decoder_fork_then_decode_against_every_sequence_alone(npm, monkeypatch, norm_first, options):
    D = npm.device
    monkeypatch.setattr(D, 'SHARED_PREFIX', False)
    f = 256
    dec, p = DC.make_decoder(npm, f, 4, 2, 384, norm_first, True, seed=11, batch=3, seq_kv=23)
    rng = np.random.default_rng(12)
    kv = rng.standard_normal([3, 23, f]).astype(np.float32)
    prompt = rng.standard_normal([45, f]).astype(np.float32)
    tails = [rng.standard_normal([4, f]).astype(np.float32) for _ in range(3)]
    state = dec.start_decoding(kv, 56, kv_lengths=np.array([17, 23, 5]), **options)
    q = np.zeros([3, 45, f], dtype=np.float32)
    q[0] = prompt
    dec.decode(q, state, new_lengths=[45, 0, 0])
    dec.fork(state, 0, 1)
    dec.fork(state, 0, 2)
    assert state.positions.tolist() == [45, 45, 45] and state.cross_cache.lengths.tolist() == [17, 17, 17]
    with pytest.raises(ValueError, match='still holds 45 rows'):
        dec.fork(state, 1, 2)
    outs = [np.asarray(dec.decode(np.stack([tail[s:s + 1] for tail in tails]), state)) for s in range(4)]
    rows = [np.concatenate([prompt, tail]) for tail in tails]
    want = VR.decoder_alone(p, rows, [[45] * 3] + [[1] * 3] * 4, np.repeat(kv[:1], 3, axis=0), [17] * 3, norm_first)
    for i in range(3):
        _layer_close(np.concatenate([o[i] for o in outs]), want[i][45:], 1e-4, f'forked decode {options} sequence {i} vs float64')
