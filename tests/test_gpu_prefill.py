"""GPU: the prefill attention kernel -- npm_mha_prefill_fwd (csrc/npm_prefill.hip) through the C ABI, then MultiHeadAttention
and TransformerDecoder.decode / admit with ``device.PREFILL_KERNEL`` on.

The kernel is held to the float64 reference (every sequence alone, tests/varlen_reference.py) with tests/decode_gpu.check
unchanged: ctx |got - ref| <= 2e-6 (1 + |ref|), lse within 3e-6, grown by tests/attn_range_data.py's tol(X) -- the project's bound
for this same contract; tests/test_prefill_host.py holds a float32 model of the kernel's accumulation order to half of it on this
grid.  Three identities are BITWISE: the paged call equals the contiguous one on the same rows (page sizes 16 and 64, identity
and random tables); kv_lens == NULL equals the call with all lengths equal; sequence b inside a batch equals that sequence at
batch 1 with the same new_tokens, and a larger d->kv_len changes nothing.  Against the decode kernel at rows <= 32: both inside
the float64 bound (the decode kernel splits keys over waves and blocks, so not bitwise).

NaN fills every cache row at and past a sequence's length, the padded query rows, every unused page and pool row, the packed
pitches' padding; table entries past a sequence's last page name an all-NaN page (every entry is in range: a kernel that forms
an address from one reads NaN, never out of bounds).  Guard regions keep their sentinel.

Layers: outputs against every sequence alone at tests/test_gpu_paged.py's bounds (1e-5 (|ref| + max |ref|) against float64, 2e-5
between two float32 evaluations, 1e-4 for the decoder against float64) and against the switch-off result at the float32 bound.

A second grid (``prefill_reference.group_cases``) holds the kernel to the same bound and identities where the 64-row tile is
partly filled (Hq / Hkv of 3, 5, 7) and where a group needs a second, partly full head chunk (72, 65): ``q`` is N(0, 1) per (token,
head), so a row stored in another row's slot misses the float64 bound by orders of magnitude.  ``range_cases`` moves every score
of a row by up to +-200 and saturates the softmax (tests/attn_range_data.py) at B 2, L 300, T up to 70; ``repeat_cases`` runs one
call three times and compares bits (the K / V tiles are double buffered in LDS behind one barrier per tile).

Every test names npm_mha_prefill_*, ``PREFILL_KERNEL`` or the path 'prefill': none exists without this feature.
"""

import ctypes as C

import numpy as np
import pytest

import decode_cases as DC
import decode_gpu
import paged_cases as PC
import prefill_reference as PR
import varlen_reference as VR
from decode_gpu import GUARD, SENTINEL
from decode_gpu import check as _check, data as _data, guarded as _guarded, ints as _ints, layer_close as _layer_close
from decode_gpu import pad_rows as _pad_rows, poison as _poison, run as _run_decode

pytestmark = pytest.mark.gpu

LAYER_TOL = 1e-5
BAD, UNSUPPORTED = 10002, 10003


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


def _run(q, k, v, lmax, scale, causal, kv_lens=None, new_lens=None, packed=False, paged=None, expect=0, null_table=False,
         want_lse=True, tweak=None):
    """tests/decode_gpu.run for npm_mha_prefill_fwd: q [B, T, Hq, D]; k / v [B, capacity, Hkv, D] or, with ``paged = (table,
    page_rows)``, page pools -> ctx, lse, kernel string.  ``kv_lens`` None: the uniform call at kv_len = lmax.  ``tweak(c)`` edits
    the descriptor before the call (bad arguments); ``expect``: the call must return that code and leave ctx untouched."""
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
    c.ctx, c.ctx_pitch, c.lse = ctx.ptr, hq * d, lse.ptr if want_lse else None
    if tweak is not None:
        tweak(c)
    lens = None if kv_lens is None else _ints(kv_lens)
    new = None if new_lens is None else _ints(new_lens)
    lens_ptr, new_ptr = (None if x is None else x.ptr for x in (lens, new))
    table_ptr, pitch, page_rows = None, 0, 0
    if paged is not None:
        table, page_rows = paged
        assert table.min() >= 0 and table.max() < k.shape[0], 'every table entry must name a page of the pool'
        table_dev = _ints(table)
        table_ptr, pitch = None if null_table else table_dev.ptr, table.shape[1]
    rc = _C.lib().npm_mha_prefill_fwd(C.byref(c), lens_ptr, new_ptr, table_ptr, pitch, page_rows)
    if expect:
        assert rc == expect, (rc, _C.lib().npm_last_error())
        np.testing.assert_array_equal(ctx.numpy(), SENTINEL)              # nothing was launched
        np.testing.assert_array_equal(lse.numpy(), SENTINEL)
        return None
    _C.check(rc, 'npm_mha_prefill_fwd')
    got_lse = _guarded(lse, b * hq * t).reshape(b, hq, t)
    if not want_lse:
        np.testing.assert_array_equal(got_lse, SENTINEL)
    return _guarded(ctx, b * t * hq * d).reshape(b, t, hq, d), got_lse, _C.last_prefill_kernel()


# ---- npm_mha_prefill_fwd ---------------------------------------------------------------------------------------------------------
def test_prefill_supported_head_sizes(npm):
    from np_modeling_amd import _C, device as D
    for d in range(1, 260):
        assert bool(_C.lib().npm_mha_prefill_supported(d)) == (d in (16, 32, 64, 128))
    assert D.mha_prefill_supported(64) and D.mha_prefill_supported(64, 64) and not D.mha_prefill_supported(64, 32)
    assert not D.mha_prefill_supported(48)


@pytest.mark.parametrize('case', PR.kernel_cases(), ids=PR.case_id)
def test_prefill_kernel_float64_bound_and_bitwise_identities(npm, case):
    d, hq, hkv, t, causal, lengths, n, packed, place = case
    b, lmax = len(lengths), int(lengths.max())
    q, k, v = PR.case_data(case)
    qn, kn, vn = _poison(q, k, v, lengths, n)
    scale = 1.0 / np.sqrt(d)
    base = _run(qn, kn, vn, lmax, scale, causal, lengths, n, packed=packed)
    name = f'mha_prefill_kernel D={d} T={t} rows={PR.ROWS} causal={causal} varlen=1'
    assert base[2] == name
    what = f'{name} L={lengths.tolist()} n={n.tolist()}'
    _check(base[0], base[1], q, k, v, lengths, n, scale, causal, what)
    # 1. paged == contiguous
    for page_rows in PR.PAGE_SIZES:
        for order in ('identity', 'random'):
            pk, pv, table = PC.build_pool(k, v, lengths, page_rows, order, seed=d + t + page_rows)
            got = _run(qn, pk, pv, lmax, scale, causal, lengths, n, packed=packed, paged=(table, page_rows))
            assert got[2] == name + f' paged={page_rows}'
            _bits_equal(base, got, f'{got[2]} {order} L={lengths.tolist()}')
    # 3. a larger upper bound changes nothing; every sequence alone at batch 1 with the same new_tokens
    _bits_equal(base, _run(qn, kn, vn, lmax + 37, scale, causal, lengths, n, packed=packed), what + ' under a larger kv_len')
    for i in range(b):
        alone = _run(qn[i:i + 1], kn[i:i + 1], vn[i:i + 1], int(lengths[i]), scale, causal, lengths[i:i + 1], n[i:i + 1], packed=packed)
        _bits_equal((base[0][i:i + 1], base[1][i:i + 1]), alone, what + f' sequence {i} alone')


@pytest.mark.parametrize('case', PR.group_cases(), ids=PR.case_id)
def test_prefill_kernel_on_uneven_and_multi_chunk_groups(npm, case):
    """The row mapping of a block where gb tb < 64 (rows of the tile that are no row of the call) and where blockIdx.x carries a
    head chunk beside the token tile: the float64 bound, unchanged, is what catches a misplaced (token, head) row."""
    d, hq, hkv, t, causal, lengths, n, packed, place = case
    b, lmax = len(lengths), int(lengths.max())
    q, k, v = PR.case_data(case)
    qn, kn, vn = _poison(q, k, v, lengths, n)
    scale = 1.0 / np.sqrt(d)
    base = _run(qn, kn, vn, lmax, scale, causal, lengths, n, packed=packed)
    name = f'mha_prefill_kernel D={d} T={t} rows={PR.ROWS} causal={causal} varlen=1'
    assert base[2] == name
    what = f'{name} H={hq}/{hkv} tile rows {PR.tile_rows(hq, hkv)} head chunks {PR.head_chunks(hq, hkv)[0]} L={lengths.tolist()} n={n.tolist()}'
    _check(base[0], base[1], q, k, v, lengths, n, scale, causal, what)
    for page_rows, order in ((16, 'random'), (64, 'identity')):          # the full cross is the first grid's
        pk, pv, table = PC.build_pool(k, v, lengths, page_rows, order, seed=d + t + page_rows)
        got = _run(qn, pk, pv, lmax, scale, causal, lengths, n, packed=packed, paged=(table, page_rows))
        assert got[2] == name + f' paged={page_rows}'
        _bits_equal(base, got, f'{got[2]} {order} L={lengths.tolist()}')
    _bits_equal(base, _run(qn, kn, vn, lmax + 37, scale, causal, lengths, n, packed=packed), what + ' under a larger kv_len')
    for i in range(b):
        alone = _run(qn[i:i + 1], kn[i:i + 1], vn[i:i + 1], int(lengths[i]), scale, causal, lengths[i:i + 1], n[i:i + 1], packed=packed)
        _bits_equal((base[0][i:i + 1], base[1][i:i + 1]), alone, what + f' sequence {i} alone')


@pytest.mark.parametrize('d,hq,hkv,t', PR.RANGE_SHAPES)
def test_prefill_shifted_and_saturated_scores(npm, d, hq, hkv, t):
    """tests/test_gpu_decode.py's test of this name for npm_mha_prefill_fwd, at more rows than the decode kernel takes: every score
    of a row moved by up to +-200; nearly one-hot rows whose largest scores sit in the last of 19 key tiles, at keys a causal row
    cannot see.  The paged call on the same rows is bitwise the contiguous one."""
    lengths = np.full(PR.RANGE_BATCH, PR.RANGE_LEN)
    for kind in PR.RANGE_KINDS:
        q, k, v, scale = PR.range_data(d, hq, hkv, t, kind)
        pk, pv, table = PC.build_pool(k, v, lengths, 16, 'random', seed=d + t)
        for causal in (0, 1):
            ctx, lse, kernel = _run(q, k, v, PR.RANGE_LEN, scale, causal)
            assert kernel == f'mha_prefill_kernel D={d} T={t} rows={PR.ROWS} causal={causal}'
            _check(ctx, lse, q, k, v, lengths, None, scale, causal, f'{kind} H={hq}/{hkv} {kernel}')
            got = _run(q, pk, pv, PR.RANGE_LEN, scale, causal, lengths, None, paged=(table, 16))
            assert got[2] == kernel + ' varlen=1 paged=16'
            _bits_equal((ctx, lse), got, f'{kind} {got[2]}')


@pytest.mark.parametrize('case', PR.repeat_cases(), ids=PR.case_id)
def test_prefill_same_call_repeated_is_bitwise_equal(npm, case):
    """Three runs of one npm_mha_prefill_fwd call, contiguous and paged: a block that read a K / V tile from LDS before every
    thread had stored it (or stored into the buffer others still read) would differ from run to run."""
    d, hq, hkv, t, causal, lengths, n, packed, place = case
    lmax = int(lengths.max())
    q, k, v = PR.case_data(case)
    qn, kn, vn = _poison(q, k, v, lengths, n)
    scale = 1.0 / np.sqrt(d)
    pk, pv, table = PC.build_pool(k, v, lengths, 16, 'random', seed=d + t)
    first = _run(qn, kn, vn, lmax, scale, causal, lengths, n)
    _check(first[0], first[1], q, k, v, lengths, n, scale, causal, f'{first[2]} H={hq}/{hkv} L={lengths.tolist()}')
    for repeat in (1, 2):
        _bits_equal(first, _run(qn, kn, vn, lmax, scale, causal, lengths, n), f'{first[2]} run {repeat} against run 0')
    for repeat in (0, 1, 2):
        got = _run(qn, pk, pv, lmax, scale, causal, lengths, n, paged=(table, 16))
        _bits_equal(first, got, f'{got[2]} run {repeat} against the contiguous run 0')


@pytest.mark.parametrize('d,hq,hkv,t,length,b,causal', [(128, 8, 2, 67, 300, 2, 1), (64, 8, 8, 64, 64, 3, 1), (16, 8, 1, 9, 129, 5, 0),
                                                        (32, 6, 3, 33, 33, 3, 1), (128, 8, 1, 19, 47, 2, 0), (64, 8, 8, 131, 700, 2, 1)])
def test_prefill_without_lengths_is_bitwise_the_call_with_all_lengths_equal(npm, d, hq, hkv, t, length, b, causal):
    """2. kv_lens == NULL (needs kv_len >= new_tokens) against kv_lens = [L] * B, new_lens NULL or [T] * B, contiguous and paged."""
    q, k, v = _data(7 + d + t, b, t, hq, hkv, d, length + 5)
    scale = 1.0 / np.sqrt(d)
    base = _run(q, k, v, length, scale, causal)
    assert base[2] == f'mha_prefill_kernel D={d} T={t} rows={PR.ROWS} causal={causal}'
    lengths = np.full(b, length)
    _check(base[0], base[1], q, k, v, lengths, None, scale, causal, base[2])
    for new_lens in (None, [t] * b):
        _bits_equal(base, _run(q, k, v, length, scale, causal, lengths, new_lens), 'uniform against all lengths equal')
        for page_rows in PR.PAGE_SIZES:
            pk, pv, table = PC.build_pool(k, v, lengths, page_rows, 'random', seed=page_rows)
            got = _run(q, pk, pv, length, scale, causal, lengths, new_lens, paged=(table, page_rows))
            _bits_equal(base, got, f'uniform against {got[2]}')
            assert got[2] == base[2] + f' varlen=1 paged={page_rows}'
    without = _run(q, k, v, length, scale, causal, want_lse=False)        # lse is optional
    assert np.array_equal(without[0].view(np.uint32), base[0].view(np.uint32))


_DECODE_CASES = [c for c in VR.kernel_cases() if c[5].max() <= 700][::3]


@pytest.mark.parametrize('case', _DECODE_CASES, ids=VR.case_id)
def test_prefill_kernel_on_the_decode_kernels_shapes(npm, case):
    """rows <= 32: the shapes npm_mha_decode_fwd_varlen takes.  Both kernels inside the float64 bound; the two are then within
    twice that bound of each other, not bitwise (the decode kernel splits the keys)."""
    d, hq, hkv, t, causal, lengths, n, packed, mode = case
    lmax = int(lengths.max())
    q, k, v = _data(d * 1000 + hq * 100 + t * 10 + causal + lmax, len(lengths), t, hq, hkv, d, lmax + 3)
    qn, kn, vn = _poison(q, k, v, lengths, n)
    scale = 1.0 / np.sqrt(d)
    decode_gpu.set_splits(mode, lmax)
    dec = _run_decode(qn, kn, vn, lmax, scale, causal, lengths, n, packed=packed)
    got = _run(qn, kn, vn, lmax, scale, causal, lengths, n, packed=packed)
    assert dec[2].startswith('mha_decode_kernel') and got[2].startswith('mha_prefill_kernel')
    _check(dec[0], dec[1], q, k, v, lengths, n, scale, causal, dec[2])
    _check(got[0], got[1], q, k, v, lengths, n, scale, causal, got[2])


def test_prefill_bad_arguments_launch_nothing(npm):
    lengths = np.array([8, 20])
    q, k, v = _data(2, 2, 40, 4, 2, 32, 24)
    pk, pv, table = PC.build_pool(k, v, lengths, 16, 'identity')
    n = np.array([8, 20])
    _run(q, pk, pv, 20, 0.2, 1, None, n, paged=(table, 16), expect=BAD)                      # a block table without kv_lens
    for page_rows in (0, 8, 24, 48):
        _run(q, pk, pv, 20, 0.2, 1, lengths, n, paged=(table, page_rows), expect=BAD)
    _run(q, pk, pv, 40, 0.2, 1, lengths, n, paged=(table, 16), expect=BAD)                   # the table rows are shorter than d->kv_len needs
    _run(q, k, v, 24, 0.2, 1, expect=BAD)                                                    # uniform: kv_len 24 < new_tokens 40
    _run(q, k, v, -1, 0.2, 1, lengths, n, expect=BAD)

    def field(name, value):
        def tweak(c):
            setattr(c, name, value)
        return tweak

    for name, value in (('heads', 3), ('kv_heads', 0), ('new_tokens', 0), ('scale', 0.0), ('q', None), ('k', None), ('v', None), ('ctx', None),
                        ('q_pitch', 4 * 32 - 4), ('q_pitch', 4 * 32 + 2), ('k_pitch', 2 * 32 - 4), ('v_pitch', 2 * 32 + 1),
                        ('ctx_pitch', 4 * 32 - 4), ('k_stride_b', 24 * 64 + 2), ('batch', 0), ('batch', 65536)):
        _run(q, k, v, 20, 0.2, 1, lengths, n, expect=BAD, tweak=field(name, value))
    _run(q, k, v, 20, 0.2, 1, lengths, n, expect=BAD, tweak=lambda c: setattr(c, 'q', c.q + 4))          # not 16-byte aligned
    for d in (8, 48, 256):
        _run(q, k, v, 20, 0.2, 1, lengths, n, expect=UNSUPPORTED, tweak=field('head_dim', d))


# ---- MultiHeadAttention ----------------------------------------------------------------------------------------------------------
def _layer_run(att, x_rows, schedule, capacity, **paged):
    from np_modeling_amd import _C
    cache = att.make_cache(len(x_rows), capacity, **paged)
    outs, paths = [], []
    for x, n in VR.padded_calls(x_rows, schedule):
        outs.append(np.asarray(att(x, cache=cache, new_lengths=n)))
        paths.append(att._cached_path)
        if paths[-1] == 'prefill':
            want = 'causal=1 varlen=1' + (f' paged={paged["page_size"]}' if paged else '')
            assert _C.last_prefill_kernel().endswith(want), (_C.last_prefill_kernel(), want)
    assert cache.lengths.tolist() == VR.schedule_rows(schedule).tolist()
    return outs, paths, cache


@pytest.mark.parametrize('heads,kv_heads,f', [(8, 8, 1024), (8, 2, 512), (8, 1, 128), (6, 3, 192), (12, 4, 192), (5, 1, 160)])
@pytest.mark.parametrize('page_size', [16, 64])
def test_layer_ragged_prefill_and_second_chunk_into_a_paged_cache(npm, monkeypatch, heads, kv_heads, f, page_size):
    """A ragged prompt of 41 .. 70 tokens into an empty paged cache, single tokens, a second chunk on top, single tokens: with the
    switch on the two chunks run the prefill kernel, and no page beyond the sequences' own is in use."""
    from np_modeling_amd import device as D
    att, p = DC.make_mha(npm, f, heads, kv_heads, seed=heads + f, batch=3)
    schedule = [np.array(n) for n in ([41, 70, 55], [1, 1, 1], [1, 0, 1], [40, 2, 33], [1, 1, 0])]
    total = VR.schedule_rows(schedule)
    rng = np.random.default_rng(f)
    x_rows = [rng.standard_normal([s, f]).astype(np.float32) for s in total]
    pages = int(sum(PC.pages_of(s, page_size) for s in total))
    kwargs = dict(page_size=page_size, pages=pages)
    off, off_paths, _ = _layer_run(att, x_rows, schedule, int(total.max()) + 5, **kwargs)
    monkeypatch.setattr(D, 'PREFILL_KERNEL', True)
    got, paths, cache = _layer_run(att, x_rows, schedule, int(total.max()) + 5, **kwargs)
    assert off_paths == ['fused_masked', 'decode', 'decode', 'fused_masked', 'decode']
    assert paths == ['prefill', 'decode', 'decode', 'prefill', 'decode']
    assert cache.pages_in_use == pages and cache.pages_free == 0
    want = VR.layer_alone(p, x_rows, schedule)
    for i, (a, b, c) in enumerate(zip(VR.collect(got, schedule, 3), want, VR.collect(off, schedule, 3))):
        sizes = [int(n[i]) for n in schedule if n[i]]
        alone, _ = DC.run_mha_chunks(att, x_rows[i][None], sizes, capacity=int(total[i]))       # batch 1, contiguous, switch on
        _layer_close(a, b, LAYER_TOL, f'prefill paged {page_size} H{heads}/{kv_heads} sequence {i} vs float64')
        _layer_close(a, alone[0], 2 * LAYER_TOL, f'prefill paged {page_size} H{heads}/{kv_heads} sequence {i} vs alone')
        _layer_close(a, c, 2 * LAYER_TOL, f'prefill paged {page_size} H{heads}/{kv_heads} sequence {i} vs switch off')


def test_layer_uniform_contiguous_cache_takes_the_kernel_only_on_top_of_rows(npm, monkeypatch):
    """A uniform prefill from empty stays on the fused forward (it reads the projection in place); a chunk on top of cached rows
    runs the prefill kernel's scalar call, with no copy of the valid rows."""
    from np_modeling_amd import _C, device as D
    att, p = DC.make_mha(npm, 256, 4, 2, seed=3, batch=2)
    x = np.random.default_rng(3).standard_normal([2, 90, 256]).astype(np.float32)
    off, off_paths = DC.run_mha_chunks(att, x, [40, 1, 49], capacity=96)
    monkeypatch.setattr(D, 'PREFILL_KERNEL', True)
    got, paths = DC.run_mha_chunks(att, x, [40, 1, 49], capacity=96)
    assert off_paths == ['fused_masked', 'decode', 'fused_masked'] and paths == ['fused_masked', 'decode', 'prefill']
    assert _C.last_prefill_kernel() == f'mha_prefill_kernel D=64 T=49 rows={PR.ROWS} causal=1'
    want = VR.layer_alone(p, list(x), [np.array([40, 40]), np.array([1, 1]), np.array([49, 49])])
    for i in range(2):
        _layer_close(got[i], want[i], LAYER_TOL, f'uniform chunk sequence {i} vs float64')
        _layer_close(got[i], off[i], 2 * LAYER_TOL, f'uniform chunk sequence {i} vs switch off')


@pytest.mark.parametrize('heads,kv_heads,f,below,above', [(4, 4, 256, 32, 33), (4, 1, 512, 8, 9), (12, 4, 192, 10, 11)])
def test_layer_hands_over_from_the_decode_kernel_to_the_prefill_kernel_past_32_rows(npm, monkeypatch, heads, kv_heads, f, below, above):
    """On a contiguous cache that holds rows, with the switch on: (Hq / Hkv) T <= 32 is the decode kernel's chunk, one more row
    is the prefill kernel's -- groups 1 and 4 at exactly 32 and 33 rows, group 3 at 30 and 33."""
    from np_modeling_amd import _C, device as D
    group = heads // kv_heads
    assert group * below <= VR.MAX_ROWS < group * above and group * (below + 1) > VR.MAX_ROWS
    att, p = DC.make_mha(npm, f, heads, kv_heads, seed=heads + below, batch=2)
    sizes = [40, below, above]
    x = np.random.default_rng(f + below).standard_normal([2, sum(sizes), f]).astype(np.float32)
    monkeypatch.setattr(D, 'PREFILL_KERNEL', True)
    got, paths = DC.run_mha_chunks(att, x, sizes, capacity=sum(sizes) + 3)
    assert paths == ['fused_masked', 'decode', 'prefill']
    assert _C.last_prefill_kernel() == f'mha_prefill_kernel D={f // heads} T={above} rows={PR.ROWS} causal=1'
    want = VR.layer_alone(p, list(x), [np.array([s, s]) for s in sizes])
    edges = np.cumsum([0] + sizes)
    for i in range(2):
        for name, lo, hi in (('decode', edges[1], edges[2]), ('prefill', edges[2], edges[3])):
            _layer_close(got[i][lo:hi], want[i][lo:hi], LAYER_TOL, f'hand-over H{heads}/{kv_heads} {name} chunk of {hi - lo} sequence {i} vs float64')


@pytest.mark.parametrize('page_size', [None, 16])
def test_layer_uniform_frozen_cross_cache_shorter_than_the_query(npm, monkeypatch, page_size):
    """kv_lengths=None, 5 memory rows under 40 query rows: the scalar npm_mha_prefill_fwd call needs kv_len >= new_tokens, so
    KVCache.attend takes the per-sequence call."""
    from np_modeling_amd import _C, device as D
    att, p = DC.make_mha(npm, 256, 8, 2, seed=9, batch=3)
    rng = np.random.default_rng(6)
    kv = rng.standard_normal([3, 5, 256]).astype(np.float32)
    x = rng.standard_normal([3, 40, 256]).astype(np.float32)
    paged = {} if page_size is None else dict(page_size=page_size)
    outs = []
    for switch in (False, True):
        monkeypatch.setattr(D, 'PREFILL_KERNEL', switch)
        cache = att.fill_cache(att.make_cache(3, 5, **paged), kv)
        outs.append(np.asarray(att(x, cache=cache)))
        assert att._cached_path == ('prefill' if switch else 'fused_masked')
    assert _C.last_prefill_kernel() == f'mha_prefill_kernel D=32 T=40 rows={PR.ROWS} causal=0 varlen=1' + (f' paged={page_size}' if page_size else '')
    for i, want in enumerate(VR.cross_alone(p, list(x), kv, np.full(3, 5))):
        _layer_close(outs[1][i], want, LAYER_TOL, f'short uniform cross sequence {i} vs float64')
        _layer_close(outs[1][i], outs[0][i], 2 * LAYER_TOL, f'short uniform cross sequence {i} vs switch off')


@pytest.mark.parametrize('page_size', [None, 16])
def test_layer_frozen_cross_cache_with_kv_lengths(npm, monkeypatch, page_size):
    from np_modeling_amd import _C, device as D
    att, p = DC.make_mha(npm, 256, 8, 2, seed=8, batch=3)
    rng = np.random.default_rng(4)
    kv = rng.standard_normal([3, 75, 256]).astype(np.float32)
    kv_lengths = np.array([75, 2, 33])
    n = np.array([40, 0, 17])
    x_rows = [rng.standard_normal([s, 256]).astype(np.float32) for s in n]
    (x, _), = VR.padded_calls(x_rows, [n])
    paged = {} if page_size is None else dict(page_size=page_size)
    outs = []
    for switch in (False, True):
        monkeypatch.setattr(D, 'PREFILL_KERNEL', switch)
        cache = att.fill_cache(att.make_cache(3, 75, **paged), kv, lengths=kv_lengths)
        outs.append(np.asarray(att(x, cache=cache, new_lengths=n)))
        assert att._cached_path == ('prefill' if switch else 'fused_masked')
    assert _C.last_prefill_kernel().endswith('causal=0 varlen=1' + (f' paged={page_size}' if page_size else ''))
    for i, (got, off, want) in enumerate(zip(VR.collect(outs[1:], [n], 3), VR.collect(outs[:1], [n], 3), VR.cross_alone(p, x_rows, kv, kv_lengths))):
        if n[i]:
            _layer_close(got, want, LAYER_TOL, f'cross sequence {i} vs float64')
            _layer_close(got, off, 2 * LAYER_TOL, f'cross sequence {i} vs switch off')


def test_no_gathered_copy_is_allocated(npm, monkeypatch):
    """One long sequence beside short ones in a paged cache, then a 40-token chunk on top.  Switch off: the fused forward gathers
    K and V of every sequence to the longest ([4, 552, 256] floats each, 4 MiB blocks of the pool).  Switch on: the pool grows by
    less than ONE such tensor, and the cache holds the sequences' own pages only."""
    from np_modeling_amd import device as D
    att, _ = DC.make_mha(npm, 256, 4, 4, seed=5, batch=4)
    rng = np.random.default_rng(5)
    first = rng.standard_normal([4, 512, 256]).astype(np.float32)
    chunk = rng.standard_normal([4, 40, 256]).astype(np.float32)
    one_gathered = 4 * 552 * 256 * 4
    growth = {}
    for switch in (True, False):
        monkeypatch.setattr(D, 'PREFILL_KERNEL', switch)
        cache = att.make_cache(4, 600, page_size=64, pages=12)
        att(first, cache=cache, new_lengths=[512, 3, 5, 2])
        D.synchronize()
        D.trim_pool()
        before = D.pool_stats()[1]
        out = np.asarray(att(chunk, cache=cache, new_lengths=[40, 1, 1, 1]))
        growth[switch] = D.pool_stats()[1] - before
        assert np.isfinite(out).all() and att._cached_path == ('prefill' if switch else 'fused_masked')
        assert cache.pages_in_use == 9 + 1 + 1 + 1 and cache.lengths.tolist() == [552, 4, 6, 3]
        del cache, out
    print(f'pool growth of the chunk: {growth[True]} bytes with the prefill kernel, {growth[False]} without')
    assert growth[True] < one_gathered <= growth[False] // 2


# ---- TransformerDecoder: admit a prompt among decoding sequences -----------------------------------------------------------------
_SLOT = (0, 1, 2, 3, 1)           # five logical sequences over four slots: the fifth takes the slot the second gave back
_PLAN = [np.array(n) for n in ([44, 9, 41, 3, 0], [1, 1, 1, 1, 0], [1, 1, 1, 1, 0],
                               [1, 0, 1, 1, 0],                            # slot 1 is empty and rides along
                               [1, 0, 1, 1, 40],                           # the fifth sequence's 40-token prompt beside single tokens
                               [1, 0, 1, 1, 1], [2, 0, 0, 1, 1])]
_RELEASE_AFTER, _ADMIT_AT = 2, 4


def _continuous(dec, state, q_rows, kv, kv_lengths):
    outs, paths = [], []
    for step, (x5, n5) in enumerate(VR.padded_calls(q_rows, _PLAN)):
        if step == _ADMIT_AT:
            dec.admit(state, _SLOT[4], kv[4:5], kv_length=int(kv_lengths[4]))
        x, n = np.zeros([4, x5.shape[1], x5.shape[2]], dtype=np.float32), np.zeros(4, dtype=np.int64)
        for seq in range(5):
            if n5[seq]:
                x[_SLOT[seq]], n[_SLOT[seq]] = x5[seq], n5[seq]
        out = np.asarray(dec.decode(x, state, new_lengths=n))
        assert np.isfinite(out).all(), f'step {step}: not finite'
        paths.append((dec._self_attention._cached_path, dec._cross_attention._cached_path))
        wide = np.zeros((5,) + out.shape[1:], dtype=out.dtype)
        for seq in range(5):
            if n5[seq]:
                wide[seq] = out[_SLOT[seq]]
        outs.append(wide)
        if step == _RELEASE_AFTER:
            pages = state.self_cache.block_table[_SLOT[1]]
            pages = pages[pages >= 0].copy()
            state.release(_SLOT[1])
            PC.poison_pages(state.self_cache, pages)
    return VR.collect(outs, _PLAN, 5), paths


@pytest.mark.parametrize('norm_first', [True, False])
@pytest.mark.parametrize('kv_heads', [None, 2])
def test_decoder_admits_a_40_token_prompt_among_decoding_sequences(npm, monkeypatch, norm_first, kv_heads):
    from np_modeling_amd import device as D
    f = 256
    dec, p = DC.make_decoder(npm, f, 4, kv_heads, 384, norm_first, True, seed=13, batch=4, seq_kv=23)
    total = VR.schedule_rows(_PLAN)
    rng = np.random.default_rng(8)
    q_rows = [rng.standard_normal([s, f]).astype(np.float32) for s in total]
    kv = rng.standard_normal([5, 40, f]).astype(np.float32)
    kv_lengths = np.array([23, 4, 11, 17, 40])
    runs = {}
    for switch in (False, True):
        monkeypatch.setattr(D, 'PREFILL_KERNEL', switch)
        state = dec.start_decoding(kv[:4, :23], 64, kv_lengths=kv_lengths[:4], page_size=16, pages=12, memory_capacity=48)
        runs[switch], paths = _continuous(dec, state, q_rows, kv, kv_lengths)
        assert state.positions.tolist() == [int(total[0]), int(total[4]), int(total[2]), int(total[3])]
        assert state.self_cache.pages_in_use == sum(PC.pages_of(total[i], 16) for i in (0, 4, 2, 3))
        bulk = 'prefill' if switch else 'fused_masked'
        assert paths[0] == (bulk, bulk) and paths[_ADMIT_AT] == (bulk, bulk) and paths[1] == ('decode', 'decode'), paths
    want = VR.decoder_alone(p, q_rows, _PLAN, kv, kv_lengths, norm_first)
    for i in range(5):
        alone_state = dec.start_decoding(kv[i:i + 1, :kv_lengths[i]], int(total[i]))          # batch 1, fresh contiguous caches, switch on
        alone = np.concatenate([np.asarray(dec.decode(np.ascontiguousarray(c), alone_state))
                                for c in VR.DR_split(q_rows[i][None], [int(n[i]) for n in _PLAN])], axis=1)[0]
        _layer_close(runs[True][i], want[i], 1e-4, f'admit sequence {i} vs float64')
        _layer_close(runs[True][i], alone, 2 * LAYER_TOL, f'admit sequence {i} vs alone')
        _layer_close(runs[True][i], runs[False][i], 2 * LAYER_TOL, f'admit sequence {i} vs switch off')
