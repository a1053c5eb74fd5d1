"""GPU: the paged key / value cache -- npm_mha_decode_fwd_paged / npm_kv_append_paged / npm_kv_gather_paged
(csrc/npm_decode.hip) through the C ABI, then MultiHeadAttention and TransformerDecoder.decode with a ``device.PagedKVCache``,
release and re-admission included.

The criterion of the kernel is BITWISE equality with npm_mha_decode_fwd_varlen on a contiguous cache holding the same rows at the
same d->kv_len (and with npm_mha_decode_fwd when all lengths are equal): paging is one table lookup per 16-key tile in front of
arithmetic that does not change.  No new tolerance.  The kernel is also held directly to the float64 reference (every sequence
alone, tests/varlen_reference.py) at the bound tests/test_gpu_varlen.py states for npm_mha_decode_fwd_varlen: ctx |got - ref| <=
2e-6 (1 + |ref|), lse within 3e-6, grown by tests/attn_range_data.py's tol(X).  Layers and the decoder: array_equal to the same
calls with a ``KVCache``; continuous batching against every sequence alone at that file's layer / decoder bounds (1e-5
(|ref| + max |ref|) against float64, twice that between two float32 evaluations, 1e-4 for the decoder against float64).

NaN fills every pool row past a sequence's length, every unused page, and the table entries past a sequence's last page name an
all-NaN page: a kernel that forms an address from such an entry or reads past a length shows up as NaN or a mismatch, never as
a fault -- every table entry is in range.  Guard regions keep their sentinel.

Every test names an entry point, class or keyword that does not exist without this feature.
"""

import numpy as np
import pytest

import decode_cases as DC
import decode_gpu
import paged_cases as PC
import varlen_reference as VR
from decode_gpu import GUARD, NT_KNOB, SENTINEL
from decode_gpu import check as _check, data as _data, guarded as _guarded, ints as _ints, layer_close as _layer_close
from decode_gpu import poison as _poison, run as _run, set_splits as _set_splits

pytestmark = pytest.mark.gpu

LAYER_TOL = 1e-5
BAD = 10002


@pytest.fixture(scope='module')
def npm():
    import np_modeling_amd
    return np_modeling_amd


@pytest.fixture(autouse=True)
def _defaults_afterwards(npm):
    yield
    decode_gpu.reset_knobs()


def _bits_equal(a, b, what):
    assert np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32)), f'{what}: ctx differs in bits'
    assert np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32)), f'{what}: lse differs in bits'


def _one_page(lmax):
    """A power of two above lmax: one page per sequence."""
    return max(16, 1 << int(lmax).bit_length())


# ---- npm_mha_decode_fwd_paged ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', VR.kernel_cases() + PC.extra_kernel_cases(), ids=VR.case_id)
def test_paged_kernel_is_bitwise_the_contiguous_ragged_kernel(npm, case):
    from np_modeling_amd import _C
    d, hq, hkv, t, causal, lengths, n, packed, mode = case
    b, lmax = len(lengths), int(lengths.max())
    q, k, v = _data(d * 1000 + hq * 100 + t * 10 + causal + lmax, b, t, hq, hkv, d, lmax + 3)
    qn, kn, vn = _poison(q, k, v, lengths, n)
    scale = 1.0 / np.sqrt(d)
    forced = _set_splits(mode, lmax)
    splits = forced or _C.lib().npm_mha_decode_splits(b, hkv, lmax)
    base = _run(qn, kn, vn, lmax, scale, causal, lengths, n, packed=packed)
    name = f'mha_decode_kernel D={d} rows={hq // hkv * t} splits={splits} causal={causal} varlen=1'
    assert base[2] == name
    checked = False
    for page_rows in PC.PAGE_SIZES + (_one_page(lmax),):
        for order in ('identity', 'random'):
            pk, pv, table = PC.build_pool(k, v, lengths, page_rows, order, seed=d + t + page_rows)
            got = _run(qn, pk, pv, lmax, scale, causal, lengths, n, packed=packed, paged=(table, page_rows))
            assert got[2] == name + f' paged={page_rows}'
            _bits_equal(base, got, f'{got[2]} {order} L={lengths.tolist()}')
            if not checked:                                               # follows from equality; stated for one of them
                _check(got[0], got[1], q, k, v, lengths, n, scale, causal, got[2] + f' L={lengths.tolist()} n={n.tolist()}')
                checked = True


@pytest.mark.parametrize('mode', ['one', 'auto', 'many'])
@pytest.mark.parametrize('d,hq,hkv,t,length,b,causal', [(128, 8, 2, 1, 8192, 2, 1), (64, 8, 8, 2, 2049, 3, 1), (16, 8, 1, 4, 129, 64, 0),
                                                        (32, 6, 3, 5, 704, 3, 1), (128, 8, 1, 4, 300, 5, 0)])
def test_paged_uniform_lengths_are_bitwise_the_uniform_entry_point(npm, d, hq, hkv, t, length, b, causal, mode):
    q, k, v = _data(7 + d + t, b, t, hq, hkv, d, length + 5)
    scale = 1.0 / np.sqrt(d)
    _set_splits(mode, length)
    base = _run(q, k, v, length, scale, causal)
    lengths = np.full(b, length)
    for page_rows in PC.PAGE_SIZES + (_one_page(length),):
        pk, pv, table = PC.build_pool(k, v, lengths, page_rows, 'random', seed=page_rows)
        for new_lens in (None, [t] * b):
            got = _run(q, pk, pv, length, scale, causal, lengths, new_lens, paged=(table, page_rows))
            _bits_equal(base, got, f'uniform {got[2]}')
            assert got[2] == base[2] + f' varlen=1 paged={page_rows}'


def test_paged_load_policy_and_pool_layout_do_not_change_a_bit(npm):
    """Either load policy, a pool with more spare pages, another permutation: identical bits."""
    from np_modeling_amd import _C
    lengths, n = np.array([2049, 17, 1, 600, 64]), np.array([2, 1, 0, 2, 2])
    q, k, v = _data(5, 5, 2, 8, 2, 128, 2049)
    scale = 1.0 / np.sqrt(128)
    runs = []
    for nt, seed, spare in ((2, 1, 3), (1, 1, 3), (2, 9, 40)):
        _C.check(_C.lib().npm_set_tuning(NT_KNOB, nt), 'npm_set_tuning')
        pk, pv, table = PC.build_pool(k, v, lengths, 64, 'random', seed=seed, spare=spare)
        runs.append(_run(q, pk, pv, 2049, scale, 1, lengths, n, paged=(table, 64)))
    for other in runs[1:]:
        _bits_equal(runs[0], other, 'policy / layout')


def test_paged_bad_arguments_launch_nothing(npm):
    from np_modeling_amd import _C
    lengths = np.array([8, 20])
    q, k, v = _data(2, 2, 2, 4, 2, 32, 20)
    pk, pv, table = PC.build_pool(k, v, lengths, 16, 'identity')
    _run(q, pk, pv, 20, 0.2, 1, lengths, null_lens=True, paged=(table, 16), expect=BAD)      # kv_lens == NULL
    _run(q, pk, pv, 20, 0.2, 1, lengths, paged=(table, 16), null_table=True, expect=BAD)     # block_table == NULL
    for page_rows in (0, 8, 24, 48):
        _run(q, pk, pv, 20, 0.2, 1, lengths, paged=(table, page_rows), expect=BAD)
    _run(q, pk, pv, 40, 0.2, 1, lengths, paged=(table, 16), expect=BAD)   # the table rows are shorter than d->kv_len needs
    lib, dev = _C.lib(), _ints(lengths)
    buf = npm.device.full([4096], SENTINEL)
    for page_rows in (0, 8, 24, 48):
        assert lib.npm_kv_append_paged(buf.ptr, 64, buf.ptr, 64, 64 * 64, 2, 1, 64, dev.ptr, None, dev.ptr, 1, page_rows) == BAD
        assert lib.npm_kv_gather_paged(buf.ptr, 64, 64 * 64, buf.ptr, 2, 1, 64, dev.ptr, dev.ptr, 1, page_rows) == BAD
    assert lib.npm_kv_append_paged(buf.ptr, 64, buf.ptr, 64, 1024, 2, 1, 64, None, None, dev.ptr, 1, 16) == BAD      # at_lens == NULL
    assert lib.npm_kv_append_paged(buf.ptr, 64, buf.ptr, 64, 1024, 2, 1, 64, dev.ptr, None, None, 1, 16) == BAD      # table == NULL
    assert lib.npm_kv_gather_paged(buf.ptr, 64, 1024, buf.ptr, 2, 1, 64, None, dev.ptr, 1, 16) == BAD                # lens == NULL
    assert lib.npm_kv_gather_paged(buf.ptr, 64, 1024, buf.ptr, 2, 1, 64, dev.ptr, None, 1, 16) == BAD                # table == NULL
    assert lib.npm_kv_append_paged(buf.ptr, 64, buf.ptr, 64, 1024, 2, 1, 14, dev.ptr, None, dev.ptr, 1, 16) == BAD   # row_len % 4
    np.testing.assert_array_equal(buf.numpy(), SENTINEL)


def test_kv_entry_points_empty_and_null_order(npm):
    """The return codes of the five row-copy entry points where no kernel is launched, row by row.  The contiguous three
    (npm_kv_append, npm_kv_append_varlen, npm_kv_gather_varlen): a negative count is a bad argument, an empty call (batch, tokens /
    rows or row_len 0) is NPM_OK even with every pointer NULL.  The paged two: a NULL length array or table, a negative table pitch
    or a bad page size is a bad argument even on an empty call; with those valid an empty call is NPM_OK with NULL src / pool / out.
    A call that has something to copy refuses each NULL pointer.  (NPM_E_NOT_INITIALIZED, which comes before all of it, cannot be
    provoked in a process that has a device: tests/test_paged_host.py checks it where there is none.)"""
    from np_modeling_amd import _C
    lib, ok = _C.lib(), 0
    buf = npm.device.full([64], SENTINEL)
    lens = _ints([0, 0])
    p, n = buf.ptr, lens.ptr
    for batch, count, row in ((-1, 1, 4), (1, -1, 4), (1, 1, -4)):
        assert lib.npm_kv_append(p, 4, p, 4, 16, batch, count, row, 0) == BAD
        assert lib.npm_kv_append_varlen(p, 4, p, 4, 16, batch, count, row, n, None) == BAD
        assert lib.npm_kv_gather_varlen(p, 4, 16, p, batch, count, row, n) == BAD
        assert lib.npm_kv_append_paged(p, 4, p, 4, 64, batch, count, row, n, None, n, 1, 16) == BAD
        assert lib.npm_kv_gather_paged(p, 4, 64, p, batch, count, row, n, n, 1, 16) == BAD
    assert lib.npm_kv_append(p, 4, p, 4, 16, 1, 1, 4, -1) == BAD                                   # at < 0
    assert lib.npm_kv_append(None, 4, None, 4, 16, 0, 1, 4, -1) == BAD                             # ... before the empty call
    for batch, count, row in ((0, 1, 4), (1, 0, 4), (1, 1, 0), (0, 0, 0)):
        assert lib.npm_kv_append(None, 4, None, 4, 16, batch, count, row, 0) == ok
        assert lib.npm_kv_append_varlen(None, 4, None, 4, 16, batch, count, row, None, None) == ok
        assert lib.npm_kv_gather_varlen(None, 4, 16, None, batch, count, row, None) == ok
        for at_lens, table, pitch, page_rows in ((None, n, 1, 16), (n, None, 1, 16), (n, n, -1, 16), (n, n, 1, 0), (n, n, 1, 8),
                                                 (n, n, 1, 24), (n, n, 1, -16)):
            assert lib.npm_kv_append_paged(None, 4, None, 4, 64, batch, count, row, at_lens, None, table, pitch, page_rows) == BAD
            assert lib.npm_kv_gather_paged(None, 4, 64, None, batch, count, row, at_lens, table, pitch, page_rows) == BAD
        assert lib.npm_kv_append_paged(None, 4, None, 4, 64, batch, count, row, n, None, n, 1, 16) == ok
        assert lib.npm_kv_gather_paged(None, 4, 64, None, batch, count, row, n, n, 1, 16) == ok
        assert lib.npm_kv_append_paged(None, 4, None, 4, 64, batch, count, row, n, None, n, 0, 16) == ok      # table_pitch 0 is no error
    for src, dst in ((None, p), (p, None)):                               # something to copy: every pointer is needed
        assert lib.npm_kv_append(src, 4, dst, 4, 16, 1, 1, 4, 0) == BAD
        assert lib.npm_kv_append_varlen(src, 4, dst, 4, 16, 1, 1, 4, n, None) == BAD
        assert lib.npm_kv_gather_varlen(src, 4, 16, dst, 1, 1, 4, n) == BAD
        assert lib.npm_kv_append_paged(src, 4, dst, 4, 64, 1, 1, 4, n, None, n, 1, 16) == BAD
        assert lib.npm_kv_gather_paged(src, 4, 64, dst, 1, 1, 4, n, n, 1, 16) == BAD
    assert lib.npm_kv_append_varlen(p, 4, p, 4, 16, 1, 1, 4, None, None) == BAD                    # at_lens
    assert lib.npm_kv_gather_varlen(p, 4, 16, p, 1, 1, 4, None) == BAD                             # lens
    assert lib.npm_kv_append(p, 4, p, 4, 16, 0, 1, 4, 0) == ok                                     # batch 0 on real memory: nothing copied
    assert lib.npm_kv_append_varlen(p, 4, p, 4, 16, 0, 1, 4, n, None) == ok
    assert lib.npm_kv_gather_varlen(p, 4, 16, p, 0, 1, 4, n) == ok
    assert lib.npm_kv_append_paged(p, 4, p, 4, 64, 0, 1, 4, n, None, n, 1, 16) == ok
    assert lib.npm_kv_gather_paged(p, 4, 64, p, 0, 1, 4, n, n, 1, 16) == ok
    np.testing.assert_array_equal(buf.numpy(), SENTINEL)


# ---- npm_kv_append_paged / npm_kv_gather_paged -------------------------------------------------------------------------------------
@pytest.mark.parametrize('b,t,hkv,d,cap,at,n', [(3, 5, 2, 16, 40, (0, 35, 7), (5, 5, 0)), (1, 1, 8, 128, 9, (4,), (1,)),
                                                (64, 7, 1, 32, 9, None, None), (2, 129, 3, 64, 300, (171, 0), (129, 1)),
                                                (4, 3, 2, 32, 70, (0, 15, 64, 62), (3, 3, 0, 3))])
@pytest.mark.parametrize('packed', [False, True])
@pytest.mark.parametrize('page_rows', [16, 64])
def test_kv_append_paged_then_gather_paged_is_exact(npm, b, t, hkv, d, cap, at, n, packed, page_rows):
    """Rows appended through the table come back from the gather exactly, zeros behind; every other row of the pool -- pages of
    other sequences, rows past the lengths, unused pages -- keeps its sentinel.  ``packed``: the source rows are the K part of a
    packed projection (row pitch larger than the row)."""
    from np_modeling_amd import _C, device as D
    rng = np.random.default_rng(b + t)
    at = rng.integers(0, cap - t + 1, b) if at is None else np.array(at)
    n = rng.integers(0, t + 1, b) if n is None else np.array(n)
    row = hkv * d
    pitch = 3 * row + 8 * d if packed else row
    offset = 8 * d if packed else 0
    src = rng.standard_normal([b * t, pitch]).astype(np.float32)
    per = PC.pages_of(cap, page_rows)
    pages = b * per + 2
    table = rng.permutation(pages)[:b * per].astype(np.int32).reshape(b, per)
    want = np.full([pages, page_rows, row], SENTINEL, dtype=np.float32)
    rows_of = src.reshape(b, t, pitch)[:, :, offset:offset + row]
    for i in range(b):
        for j in range(n[i]):
            want[table[i, (at[i] + j) // page_rows], (at[i] + j) % page_rows] = rows_of[i, j]
    pool = D.full([pages * page_rows * row + GUARD], SENTINEL)
    sd, at_dev, n_dev, table_dev = D.from_host(src), _ints(at), _ints(n), _ints(table)
    _C.check(_C.lib().npm_kv_append_paged(sd.ptr + 4 * offset, pitch, pool.ptr, row, page_rows * row, b, t, row, at_dev.ptr, n_dev.ptr,
                                          table_dev.ptr, per, page_rows), 'npm_kv_append_paged')
    got = _guarded(pool, pages * page_rows * row).reshape(pages, page_rows, row)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    # gather: the first at + n rows of every sequence; what was not appended is the sentinel, what lies behind is zero
    lens = at + n
    rows = int(max(lens.max(), 1))
    host = np.where(got == SENTINEL, np.float32(np.nan), got)             # never-written rows must not be read past a length ...
    for i in range(b):                                                    # ... but below it they are this sequence's rows
        for j in range(lens[i]):
            p, r = table[i, j // page_rows], j % page_rows
            host[p, r] = got[p, r]
    pool.flat_view(0, [pages * page_rows * row]).set(host.ravel())
    out = D.full([b * rows * row + GUARD], SENTINEL)
    lens_dev = _ints(lens)
    junk = table.copy()
    for i in range(b):                                                    # entries past a sequence's last page: an unused page
        junk[i, PC.pages_of(lens[i], page_rows):] = np.setdiff1d(np.arange(pages), table.ravel())[0]
    junk_dev = _ints(junk)
    _C.check(_C.lib().npm_kv_gather_paged(pool.ptr, row, page_rows * row, out.ptr, b, rows, row, lens_dev.ptr, junk_dev.ptr, per,
                                          page_rows), 'npm_kv_gather_paged')
    gathered = _guarded(out, b * rows * row).reshape(b, rows, row)
    for i in range(b):
        assert (gathered[i, lens[i]:] == 0).all()
        for j in range(lens[i]):
            expect = rows_of[i, j - at[i]] if j >= at[i] else np.float32(SENTINEL)
            assert np.array_equal(gathered[i, j], np.broadcast_to(expect, [row])), (i, j)


# ---- MultiHeadAttention: a paged cache against the contiguous one ------------------------------------------------------------------
def _layer_run(att, x_rows, schedule, capacity, **paged):
    from np_modeling_amd import _C
    cache = att.make_cache(len(x_rows), capacity, **paged)
    outs, paths = [], []
    for x, n in VR.padded_calls(x_rows, schedule):
        outs.append(np.asarray(att(x, cache=cache, new_lengths=n)))
        paths.append(att._cached_path)
        if paths[-1] == 'decode':
            want = 'causal=1 varlen=1' + (f' paged={paged["page_size"]}' if paged else '')
            assert _C.last_decode_kernel().endswith(want), (_C.last_decode_kernel(), want)
    assert cache.lengths.tolist() == VR.schedule_rows(schedule).tolist()
    return outs, paths, cache


@pytest.mark.parametrize('heads,kv_heads,f', [(8, 8, 1024), (8, 2, 1024), (8, 1, 512), (4, 4, 64), (6, 3, 192)])
@pytest.mark.parametrize('page_size', [16, 64])
def test_layer_with_a_paged_cache_is_bitwise_the_contiguous_cache(npm, heads, kv_heads, f, page_size):
    """A ragged prompt (the fused forward on the fresh projection), single tokens and a chunk of two (the decode kernel), a second
    chunk too large for the decode kernel (the fused forward on gathered rows), more single tokens.  Only the cache differs: all
    three paths are bitwise here (both caches gather on the third, neither takes a shortcut)."""
    att, p = DC.make_mha(npm, f, heads, kv_heads, seed=heads + f, batch=3)
    schedule = [np.array(n) for n in ([3, 37, 64], [1, 1, 1], [1, 0, 1], [2, 0, 1], [40, 2, 33], [1, 1, 0], [1, 1, 1])]
    total = VR.schedule_rows(schedule)
    rng = np.random.default_rng(f)
    x_rows = [rng.standard_normal([s, f]).astype(np.float32) for s in total]
    want, want_paths, _ = _layer_run(att, x_rows, schedule, int(total.max()) + 5)
    got, paths, cache = _layer_run(att, x_rows, schedule, int(total.max()) + 5, page_size=page_size,
                                   pages=int(sum(PC.pages_of(s, page_size) for s in total)))
    assert paths == want_paths == ['fused_masked', 'decode', 'decode', 'decode', 'fused_masked', 'decode', 'decode']
    assert cache.pages_free == 0                                          # the pool held exactly what the sequences needed
    for i, (a, b) in enumerate(zip(got, want)):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), f'call {i} ({paths[i]}) differs from the contiguous cache'
    for i, (a, b) in enumerate(zip(VR.collect(got, schedule, 3), VR.layer_alone(p, x_rows, schedule))):
        _layer_close(a, b, LAYER_TOL, f'paged {page_size} H{heads}/{kv_heads} sequence {i} vs float64')


# ---- TransformerDecoder.decode -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('norm_first', [True, False])
@pytest.mark.parametrize('kv_heads', [None, 2])
def test_decoder_decode_with_a_paged_self_cache_is_bitwise_the_contiguous_one(npm, norm_first, kv_heads):
    f = 256
    dec, p = DC.make_decoder(npm, f, 4, kv_heads, 384, norm_first, True, seed=11, batch=3, seq_kv=23)
    schedule = [np.array(n) for n in ([45, 2, 17], [1, 1, 1], [1, 1, 0], [1, 0, 0], [3, 0, 1], [1, 0, 1])]
    total = VR.schedule_rows(schedule)
    rng = np.random.default_rng(12)
    q_rows = [rng.standard_normal([s, f]).astype(np.float32) for s in total]
    kv = rng.standard_normal([3, 23, f]).astype(np.float32)
    kv_lengths = np.array([23, 4, 11])
    runs = []
    for kwargs in ({}, dict(page_size=16, pages=7)):
        state = dec.start_decoding(kv, int(total.max()) + 3, kv_lengths=kv_lengths, **kwargs)
        runs.append([np.asarray(dec.decode(x, state, new_lengths=n)) for x, n in VR.padded_calls(q_rows, schedule)])
        assert state.positions.tolist() == total.tolist()
    assert state.self_cache.pages_in_use == 7
    for i, (a, b) in enumerate(zip(*runs)):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), f'step {i} differs from the contiguous cache'
    for i, (got, ref) in enumerate(zip(VR.collect(runs[1], schedule, 3), VR.decoder_alone(p, q_rows, schedule, kv, kv_lengths, norm_first))):
        _layer_close(got, ref, 1e-4, f'paged decode sequence {i} vs float64')


# ---- continuous batching -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('heads,kv_heads,f', [(8, 8, 1024), (8, 2, 512), (4, 1, 64)])
def test_layer_release_and_admit_while_the_others_decode(npm, heads, kv_heads, f):
    att, p = DC.make_mha(npm, f, heads, kv_heads, seed=heads + 1, batch=4)
    total = PC.plan_rows()
    rng = np.random.default_rng(7)
    x_rows = [rng.standard_normal([s, f]).astype(np.float32) for s in total]
    cache = att.make_cache(4, 32, page_size=16, pages=6)
    got = PC.run_continuous(lambda x, n: att(x, cache=cache, new_lengths=n), cache.release, lambda slot: None, cache, x_rows, pad=2.5)
    assert cache.lengths.tolist() == [int(total[0]), int(total[4]), int(total[2]), int(total[3])]
    want = VR.layer_alone(p, x_rows, PC.PLAN)
    for i in range(5):
        sizes = [int(n[i]) for n in PC.PLAN if n[i]]
        alone, _ = DC.run_mha_chunks(att, x_rows[i][None], sizes, capacity=int(total[i]))     # batch 1, a fresh contiguous cache
        _layer_close(got[i], want[i], LAYER_TOL, f'continuous H{heads}/{kv_heads} sequence {i} vs float64')
        _layer_close(got[i], alone[0], 2 * LAYER_TOL, f'continuous H{heads}/{kv_heads} sequence {i} vs alone')


@pytest.mark.parametrize('norm_first', [True, False])
@pytest.mark.parametrize('kv_heads', [None, 2])
def test_decoder_release_and_admit_with_a_longer_memory(npm, norm_first, kv_heads):
    f = 256
    dec, p = DC.make_decoder(npm, f, 4, kv_heads, 384, norm_first, True, seed=13, batch=4, seq_kv=23)
    total = PC.plan_rows()
    rng = np.random.default_rng(8)
    q_rows = [rng.standard_normal([s, f]).astype(np.float32) for s in total]
    kv = rng.standard_normal([5, 40, f]).astype(np.float32)              # the fifth sequence's memory is the longest
    kv_lengths = np.array([23, 4, 11, 17, 40])
    state = dec.start_decoding(kv[:4, :23], 32, kv_lengths=kv_lengths[:4], page_size=16, pages=6, memory_capacity=48)
    assert state.cross_cache.capacity == 48

    def admit(slot):
        dec.admit(state, slot, kv[4:5], kv_length=40)
        assert state.cross_cache.lengths.tolist() == [23, 40, 11, 17]

    got = PC.run_continuous(lambda x, n: dec.decode(x, state, new_lengths=n), state.release, admit, state.self_cache, q_rows)
    assert state.positions.tolist() == [int(total[0]), int(total[4]), int(total[2]), int(total[3])]
    want = VR.decoder_alone(p, q_rows, PC.PLAN, kv, kv_lengths, norm_first)
    for i in range(5):
        alone_state = dec.start_decoding(kv[i:i + 1, :kv_lengths[i]], int(total[i]))          # batch 1, fresh contiguous caches
        alone = np.concatenate([np.asarray(dec.decode(np.ascontiguousarray(c), alone_state))
                                for c in VR.DR_split(q_rows[i][None], [int(n[i]) for n in PC.PLAN])], axis=1)[0]
        _layer_close(got[i], alone, 2 * LAYER_TOL, f'continuous decode sequence {i} vs alone')
        _layer_close(got[i], want[i], 1e-4, f'continuous decode sequence {i} vs float64')
