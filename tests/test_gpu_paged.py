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

import ctypes as C

import numpy as np
import pytest

import attn_range_data as R
import decode_cases as DC
import paged_cases as PC
import varlen_reference as VR

pytestmark = pytest.mark.gpu

GUARD = 64
SENTINEL = 777.0
SPLITS_KNOB, NT_KNOB = 20, 21
LAYER_TOL = 1e-5
BAD = 10002


@pytest.fixture(scope='module')
def npm():
    import np_modeling_amd
    return np_modeling_amd


@pytest.fixture(autouse=True)
def _defaults_afterwards(npm):
    yield
    from np_modeling_amd import _C
    for knob in (SPLITS_KNOB, NT_KNOB):
        _C.check(_C.lib().npm_set_tuning(knob, 0), 'npm_set_tuning')


def _set_splits(mode, lmax):
    from np_modeling_amd import _C
    tiles = (lmax + 15) // 16
    value = {'one': 1, 'auto': 0, 'many': min(tiles + 3, 1024)}.get(mode, mode)
    _C.check(_C.lib().npm_set_tuning(SPLITS_KNOB, int(value)), 'npm_set_tuning')
    return int(value) or None


def _guarded(arr, n):
    np.testing.assert_array_equal(arr.flat_view(n, [arr.size - n]).numpy(), SENTINEL)
    return arr.flat_view(0, [n]).numpy()


def _ints(values):
    from np_modeling_amd import device as D
    return D.bytes_from_host(np.ascontiguousarray(np.asarray(values, dtype=np.int32)))


def _pad_rows(x, packed):
    """[..., rows, Hkv, D] -> [..., rows, Hkv * D (+ 4 floats of NaN padding)], and the row pitch."""
    hkv, d = x.shape[-2:]
    flat = x.reshape(x.shape[:-2] + (hkv * d,))
    if not packed:
        return np.ascontiguousarray(flat), hkv * d
    out = np.full(flat.shape[:-1] + (hkv * d + 4,), np.nan, dtype=np.float32)
    out[..., :hkv * d] = flat
    return out, hkv * d + 4


def _run(q, k, v, lmax, scale, causal, kv_lens=None, new_lens=None, packed=False, paged=None, expect=0, null_lens=False,
         null_table=False):
    """q [B, T, Hq, D]; k / v [B, capacity, Hkv, D] (contiguous) or, with ``paged = (table [B, P], page_rows)``, page pools
    [pages, page_rows, Hkv, D] -> ctx, lse, kernel string.  ``kv_lens`` None: npm_mha_decode_fwd at kv_len = lmax; else the varlen or
    the paged entry point with d->kv_len = lmax.  ``packed``: q sits in a [B, T, Hq + 2 Hkv, D] buffer and the cache rows carry 4
    floats of padding (NaN in both)."""
    from np_modeling_amd import _C, device as D
    b, t, hq, d = q.shape
    rows, hkv = k.shape[1], k.shape[2]
    if packed:
        qp = hq * d + 2 * hkv * d
        qbuf = np.full([b, t, qp], np.nan, dtype=np.float32)
        qbuf[:, :, :hq * d] = q.reshape(b, t, hq * d)
    else:
        qp, qbuf = hq * d, q
    kbuf, kp = _pad_rows(k, packed)
    vbuf, _ = _pad_rows(v, packed)
    qd, kd, vd = D.from_host(qbuf), D.from_host(kbuf), D.from_host(vbuf)
    ctx = D.full([b * t * hq * d + GUARD], SENTINEL)
    lse = D.full([b * hq * t + GUARD], SENTINEL)
    c = _C.npm_mha_decode()
    c.batch, c.heads, c.kv_heads, c.new_tokens, c.kv_len, c.head_dim = b, hq, hkv, t, lmax, d
    c.causal, c.scale = int(causal), scale
    c.q, c.q_pitch = qd.ptr, qp
    c.k, c.k_pitch, c.k_stride_b = kd.ptr, kp, rows * kp
    c.v, c.v_pitch, c.v_stride_b = vd.ptr, kp, rows * kp
    c.ctx, c.ctx_pitch, c.lse = ctx.ptr, hq * d, lse.ptr
    lens = None if null_lens or kv_lens is None else _ints(kv_lens)
    new = None if new_lens is None else _ints(new_lens)
    lens_ptr, new_ptr = (None if x is None else x.ptr for x in (lens, new))
    if paged is not None:
        table, page_rows = paged
        assert table.min() >= 0 and table.max() < k.shape[0], 'every table entry must name a page of the pool'
        table_dev = _ints(table)
        rc = _C.lib().npm_mha_decode_fwd_paged(C.byref(c), lens_ptr, new_ptr, None if null_table else table_dev.ptr, table.shape[1],
                                               page_rows)
    elif kv_lens is None:
        rc = _C.lib().npm_mha_decode_fwd(C.byref(c))
    else:
        rc = _C.lib().npm_mha_decode_fwd_varlen(C.byref(c), lens_ptr, new_ptr)
    if expect:
        assert rc == expect, (rc, _C.lib().npm_last_error())
        np.testing.assert_array_equal(ctx.numpy(), SENTINEL)              # nothing was launched
        return None
    _C.check(rc, 'npm_mha_decode_fwd[_varlen|_paged]')
    return _guarded(ctx, b * t * hq * d).reshape(b, t, hq, d), _guarded(lse, b * hq * t).reshape(b, hq, t), _C.last_decode_kernel()


def _check(got_ctx, got_lse, q, k, v, kv_lens, new_lens, scale, causal, what):
    """tests/test_gpu_varlen.py's check, restated: every valid element against float64 of its sequence alone at tol(X) of that
    sequence; rows without a visible key are ctx == 0, lse == -inf."""
    b, t = q.shape[:2]
    want_ctx, want_lse = VR.decode_attention(q, k, v, kv_lens, new_lens, scale, causal)
    seen = VR.valid_rows(t, kv_lens, new_lens)
    assert (got_ctx[~seen] == 0).all(), f'{what}: ctx of a row without a visible key is not 0'
    assert np.isneginf(got_lse.transpose(0, 2, 1)[~seen]).all(), f'{what}: lse of a row without a visible key is not -inf'
    worst_ctx = worst_lse = 0.0
    for i in np.nonzero(seen.any(axis=1))[0]:
        rows = seen[i]
        g_ctx, g_lse = got_ctx[i, rows].astype(np.float64), got_lse[i][:, rows].astype(np.float64)
        assert np.isfinite(g_ctx).all() and np.isfinite(g_lse).all(), f'{what}: sequence {i} not finite'
        x = R.exponent_magnitude(q[i:i + 1, rows], k[i:i + 1, :kv_lens[i]], scale, want_lse[i:i + 1, :, rows])
        worst_ctx = max(worst_ctx, float((np.abs(g_ctx - want_ctx[i, rows]) / (R.exponent_tol(2e-6, x) * (1.0 + np.abs(want_ctx[i, rows])))).max()))
        worst_lse = max(worst_lse, float(np.abs(g_lse - want_lse[i][:, rows]).max() / R.exponent_tol(3e-6, x)))
    print(f'{what}: ctx {worst_ctx:.3f} of the bound, lse {worst_lse:.3f} of the bound')
    assert worst_ctx <= 1.0, f'{what}: ctx {worst_ctx:.3g} of the bound'
    assert worst_lse <= 1.0, f'{what}: lse {worst_lse:.3g} of the bound'


def _data(seed, b, t, hq, hkv, d, cap):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal([b, t, hq, d]).astype(np.float32), rng.standard_normal([b, cap, hkv, d]).astype(np.float32),
            rng.standard_normal([b, cap, hkv, d]).astype(np.float32))


def _poison(q, k, v, kv_lens, new_lens, fill=np.nan):
    k, v, q = k.copy(), v.copy(), q.copy()
    past = np.arange(k.shape[1])[None, :] >= np.asarray(kv_lens)[:, None]
    k[past], v[past] = fill, fill
    if new_lens is not None:
        q[np.arange(q.shape[1])[None, :] >= np.asarray(new_lens)[:, None]] = fill
    return q, k, v


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
def _layer_close(got, want, tol, what):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape and np.isfinite(got).all(), what
    frac = float((np.abs(got - want) / (tol * (np.abs(want) + max(np.abs(want).max(), 1.0)))).max())
    print(f'{what}: {frac:.3f} of {tol:.1e} (|ref| + max |ref|)')
    assert frac <= 1.0, f'{what}: {frac:.3g} of the bound {tol:.3g}'


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
