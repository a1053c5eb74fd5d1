"""GPU: attention over a shared key / value prefix -- npm_mha_prefix_fwd and npm_attn_combine (csrc/npm_prefix.hip) around the
existing paged entry point, through the C ABI, then MultiHeadAttention and TransformerDecoder with ``device.SHARED_PREFIX`` on.

The three launches (the paged call over the rows behind the prefix with the table moved on by P / page_rows slots, the prefix
pass, the combine) are held to the float64 reference of every sequence alone (tests/varlen_reference.py) at the bound
tests/decode_gpu.py::check applies to the decode kernel: ctx |got - ref| <= 2e-6 (1 + |ref|), lse within 3e-6, grown by
tests/attn_range_data.py's tol(X).  The combine adds one rounding level to a structure the decode kernel already has (splits
merged in order): no new tolerance.  Bitwise, with no tolerance: f16 pools equal f32 pools holding the rounded values, a random
page order equals the identity order, two runs are equal, and a sequence's rows in a batch equal that sequence at batch 1 under
the same split counts and d->kv_len.

NaN fills every pool row past a length, every unused page, the table entries past a sequence's last page (an all-NaN page) and
the padded query rows; every table entry is in range.  Guard regions behind ctx, lse and the partials keep their sentinel, and
the partials of rows that are not live are never written.

Every test names an entry point, switch or path that does not exist without this feature.
"""

import ctypes as C

import numpy as np
import pytest

import decode_cases as DC
import decode_gpu
import varlen_reference as VR
from decode_gpu import GUARD, SENTINEL
from decode_gpu import check as _check, guarded as _guarded, ints as _ints, layer_close as _layer_close, set_splits as _set_splits

pytestmark = pytest.mark.gpu

PREFIX_KNOB = 24
LAYER_TOL = 1e-5


@pytest.fixture(scope='module')
def npm():
    import np_modeling_amd
    return np_modeling_amd


@pytest.fixture(autouse=True)
def _defaults_afterwards(npm):
    from np_modeling_amd import _C
    yield
    decode_gpu.reset_knobs()
    _C.check(_C.lib().npm_set_tuning(PREFIX_KNOB, 0), 'npm_set_tuning')


# ---- data: B sequences whose first P rows are the same rows ------------------------------------------------------------------------
def _shared_data(seed, b, t, hq, hkv, d, prefix, suffixes, n):
    """q [B, T, Hq, D], k / v [B, cap, Hkv, D] with k[i, :P] = k[0, :P] for every sequence that brings a token, lengths [B].  A
    sequence with n = 0 has rows of its own (and may be shorter than the prefix): it shares nothing."""
    rng = np.random.default_rng(seed)
    lengths = np.array([prefix + s if n[i] else s for i, s in enumerate(suffixes)], dtype=np.int64)
    cap = int(lengths.max())
    q = rng.standard_normal([b, t, hq, d]).astype(np.float32)
    k, v = (rng.standard_normal([b, cap, hkv, d]).astype(np.float32) for _ in range(2))
    for i in range(b):
        if n[i]:
            k[i, :prefix], v[i, :prefix] = k[0, :prefix], v[0, :prefix]
    return q, k, v, lengths


def _suffixes(b, t, n):
    """Ragged: exactly the new tokens, a few rows, a tile and a bit, a page of 256 and a bit, ..."""
    base = (0, 5, 37, 300, 1, 16, 64)
    return [int(n[i]) + base[i % len(base)] if n[i] else (9, 40)[i % 2] for i in range(b)]


def _new_lens(b, t):
    n = np.full(b, t, dtype=np.int64)
    if b >= 3:
        n[b // 2] = 0                                                     # one sequence rides along
    if t > 1:
        n[-1] = t - 1                                                     # one brings a token less
    return n


def _pool(k, v, lengths, n, prefix, page_rows, order, seed, f16):
    """Page pools in which the sequences with n > 0 NAME THE SAME PAGES for their first P rows.  Returns pool_k, pool_v
    [pages, page_rows, Hkv, D] (float32, or float16 for ``f16``), table int32 [B, per] and the table row of the prefix."""
    b = len(lengths)
    per = max(-(-int(lengths.max()) // page_rows), 1)
    shared = prefix // page_rows
    own = [(-(-int(lengths[i]) // page_rows) - (shared if n[i] else 0)) for i in range(b)]
    need = shared + sum(own)
    pages = need + 4
    rng = np.random.default_rng(seed)
    ids = np.arange(need) if order == 'identity' else rng.permutation(pages)[:need]
    unused = np.setdiff1d(np.arange(pages), ids)
    pools = [np.full((pages, page_rows) + x.shape[2:], np.nan, dtype=np.float32) for x in (k, v)]
    table = np.empty([b, per], dtype=np.int32)
    first_active = int(np.nonzero(n)[0][0])
    at = shared
    for i in range(b):
        row = list(ids[:shared]) if n[i] else []
        row += list(ids[at:at + own[i]])
        at += own[i]
        table[i, :len(row)] = row
        table[i, len(row):] = unused[(i + np.arange(per - len(row))) % len(unused)]
        for j0 in range(0, int(lengths[i]), page_rows):
            take = min(page_rows, int(lengths[i]) - j0)
            for pool, x in zip(pools, (k, v)):
                pool[table[i, j0 // page_rows], :take] = x[i, j0:j0 + take]
    if f16:
        pools = [p.astype(np.float16) for p in pools]
    return pools[0], pools[1], table, first_active


def _run_shared(q, pk, pv, table, first, lengths, n, prefix, page_rows, scale, splits, lmax=None, want_lse=True):
    """The three launches through the C ABI: ctx [B, T, Hq, D], lse [B, Hq, T], and the kernel strings."""
    from np_modeling_amd import _C, device as D
    b, t, hq, d = q.shape
    hkv = pk.shape[2]
    f16 = pk.dtype == np.float16
    row = hkv * d
    lmax = int(lengths.max()) if lmax is None else lmax
    qn = q.copy()
    qn[np.arange(t)[None, :] >= n[:, None]] = np.nan
    qd = D.from_host(qn)
    kd, vd = (D.bytes_from_host(np.ascontiguousarray(p)) for p in (pk, pv))
    ctx = D.full([b * t * hq * d + GUARD], SENTINEL)
    lse = D.full([b * hq * t + GUARD], SENTINEL)
    part = D.full([splits * b * t * hq * (d + 1) + GUARD], SENTINEL)
    part_lse = part.ptr + 4 * splits * b * t * hq * d
    c = _C.npm_mha_decode()
    c.batch, c.heads, c.kv_heads, c.new_tokens, c.kv_len, c.head_dim = b, hq, hkv, t, lmax - prefix, d
    c.causal, c.scale = 1, scale
    c.q, c.q_pitch = qd.ptr, hq * d
    c.k, c.k_pitch, c.k_stride_b = kd.ptr, row, page_rows * row
    c.v, c.v_pitch, c.v_stride_b = vd.ptr, row, page_rows * row
    c.ctx, c.ctx_pitch, c.lse = ctx.ptr, hq * d, lse.ptr
    behind = _ints(np.maximum(lengths - prefix, 0))
    new = _ints(n)
    table_dev = _ints(table)
    suffix_table = table_dev.ptr + 4 * (prefix // page_rows)
    decode = hq // hkv * t <= 32
    entry = {(True, False): 'npm_mha_decode_fwd_paged', (False, False): 'npm_mha_prefill_fwd', (True, True): 'npm_mha_decode_fwd_f16',
             (False, True): 'npm_mha_prefill_fwd_f16'}[(decode, f16)]
    _C.check(getattr(_C.lib(), entry)(C.byref(c), behind.ptr, new.ptr, suffix_table, table.shape[1], page_rows), entry)
    suffix_kernel = _C.last_decode_kernel() if decode else _C.last_prefill_kernel()
    _C.check(_C.lib().npm_mha_prefix_fwd(C.byref(c), new.ptr, table_dev.ptr + 4 * first * table.shape[1], page_rows, prefix, splits,
                                         part.ptr, part_lse, int(f16)), 'npm_mha_prefix_fwd')
    name = _C.last_prefix_kernel()
    assert name == f'mha_prefix_kernel D={d} R={b * t} rows=64 prefix={prefix} splits={splits} paged={page_rows}' + (' kv=f16' if f16 else ''), name
    parts = _guarded(part, splits * b * t * hq * (d + 1)).copy()
    live = np.repeat((np.arange(t)[None, :] < n[:, None]).reshape(1, b * t, 1), splits, axis=0)
    pc = parts[:splits * b * t * hq * d].reshape(splits, b * t, hq, d)
    pl = parts[splits * b * t * hq * d:].reshape(splits, b * t, hq)
    assert (pc[~live[:, :, 0]] == SENTINEL).all() and (pl[~live[:, :, 0]] == SENTINEL).all(), 'a row that is not live wrote a partial'
    assert np.isfinite(pc[live[:, :, 0]]).all() and not np.isnan(pl[live[:, :, 0]]).any()
    _C.check(_C.lib().npm_attn_combine(part.ptr, part_lse, splits, ctx.ptr, hq * d, lse.ptr, b, t, hq, d, new.ptr, int(want_lse)),
             'npm_attn_combine')
    assert np.array_equal(_guarded(part, splits * b * t * hq * (d + 1)).view(np.uint32), parts.view(np.uint32))
    return _guarded(ctx, b * t * hq * d).reshape(b, t, hq, d).copy(), _guarded(lse, b * hq * t).reshape(b, hq, t).copy(), (suffix_kernel, name)


def _splits(mode, b, t, hq, hkv, prefix):
    from np_modeling_amd import _C
    if mode == 'auto':
        return int(_C.lib().npm_mha_prefix_splits(b * t, hq, hkv, prefix))
    return 1 if mode == 'one' else prefix // 16                          # 'tile': one 16-key tile per split


def _bits_equal(a, b, what):
    assert np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32)), f'{what}: ctx differs in bits'
    assert np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32)), f'{what}: lse differs in bits'


# (d, hq, hkv, b, t, prefix, page_rows): every head size and head grouping; (head, row) pairs per K / V head below 16 (2 x 4, 3 x 2),
# no multiple of 16 (10 x 2, 3 x 2 x 2), above 64 (64 x 1 x ..., 5 x 4 x 8); B 64 at D 16; P one page of 16, of 64, of 256, and
# 2048 + 64 (2048 + 256 at page 256); a suffix call that takes the prefill kernel (16 query heads on one K / V head, T 4)
CASES = [(16, 8, 8, 64, 1, 16, 16), (16, 8, 1, 64, 4, 2112, 64), (16, 8, 2, 3, 2, 64, 64), (32, 8, 2, 2, 1, 64, 64),
         (32, 6, 3, 5, 2, 2112, 16), (64, 6, 3, 3, 2, 2112, 64), (64, 8, 8, 2, 4, 16, 16), (64, 16, 1, 3, 4, 64, 16),
         (128, 8, 1, 5, 4, 2112, 64), (128, 8, 8, 3, 1, 64, 16), (128, 8, 2, 5, 2, 256, 256), (32, 8, 1, 2, 2, 2304, 256)]


@pytest.mark.parametrize('mode', ['one', 'auto', 'tile'])
@pytest.mark.parametrize('case', CASES, ids=lambda c: 'D%d-H%d/%d-B%d-T%d-P%d-page%d' % c)
def test_prefix_suffix_and_combine_against_every_sequence_alone(npm, case, mode):
    d, hq, hkv, b, t, prefix, page_rows = case
    n = _new_lens(b, t)
    q, k, v, lengths = _shared_data(d + hq + b + prefix, b, t, hq, hkv, d, prefix, _suffixes(b, t, n), n)
    pk, pv, table, first = _pool(k, v, lengths, n, prefix, page_rows, 'random', seed=b + t, f16=False)
    scale = 1.0 / np.sqrt(d)
    splits = _splits(mode, b, t, hq, hkv, prefix)
    assert 1 <= splits <= prefix // 16
    ctx, lse, names = _run_shared(q, pk, pv, table, first, lengths, n, prefix, page_rows, scale, splits)
    assert f'paged={page_rows}' in names[0]
    _check(ctx, lse, q, k, v, lengths, n, scale, 1, f'{names[1]} + {names[0]} L={lengths.tolist()} n={n.tolist()}')


@pytest.mark.parametrize('case', [CASES[1], CASES[4], CASES[7], CASES[8], CASES[10]], ids=lambda c: 'D%d-H%d/%d-B%d-T%d-P%d-page%d' % c)
def test_prefix_bitwise_f16_page_order_and_repeat(npm, case):
    d, hq, hkv, b, t, prefix, page_rows = case
    n = _new_lens(b, t)
    q, k, v, lengths = _shared_data(3 + d, b, t, hq, hkv, d, prefix, _suffixes(b, t, n), n)
    scale = 1.0 / np.sqrt(d)
    splits = _splits('auto', b, t, hq, hkv, prefix)
    pk, pv, table, first = _pool(k, v, lengths, n, prefix, page_rows, 'identity', seed=1, f16=False)
    base = _run_shared(q, pk, pv, table, first, lengths, n, prefix, page_rows, scale, splits)
    _bits_equal(base, _run_shared(q, pk, pv, table, first, lengths, n, prefix, page_rows, scale, splits), 'a second run')
    rk, rv, rtable, rfirst = _pool(k, v, lengths, n, prefix, page_rows, 'random', seed=7, f16=False)
    assert not np.array_equal(rtable, table)
    _bits_equal(base, _run_shared(q, rk, rv, rtable, rfirst, lengths, n, prefix, page_rows, scale, splits), 'a random page order')
    # f16: the pools hold halves; the f32 call on the rounded values is the same bits
    hk, hv, htable, hfirst = _pool(k, v, lengths, n, prefix, page_rows, 'random', seed=7, f16=True)
    half = _run_shared(q, hk, hv, htable, hfirst, lengths, n, prefix, page_rows, scale, splits)
    assert half[2][1].endswith(' kv=f16') and half[2][0].endswith(' kv=f16')
    rounded = _run_shared(q, hk.astype(np.float32), hv.astype(np.float32), htable, hfirst, lengths, n, prefix, page_rows, scale, splits)
    _bits_equal(half, rounded, 'f16 against f32 on the rounded values')
    _check(half[0], half[1], q, k.astype(np.float16).astype(np.float32), v.astype(np.float16).astype(np.float32), lengths, n, scale, 1,
           f'{half[2][1]} against float64 on the stored values')


@pytest.mark.parametrize('case', [CASES[2], CASES[5], CASES[7], CASES[8]], ids=lambda c: 'D%d-H%d/%d-B%d-T%d-P%d-page%d' % c)
def test_a_sequence_in_a_batch_is_bitwise_that_sequence_at_batch_one(npm, case):
    """Both split knobs forced equal and the same d->kv_len: the partition of the keys is then the same in both calls."""
    d, hq, hkv, b, t, prefix, page_rows = case
    n = _new_lens(b, t)
    q, k, v, lengths = _shared_data(11 + d, b, t, hq, hkv, d, prefix, _suffixes(b, t, n), n)
    scale = 1.0 / np.sqrt(d)
    lmax = int(lengths.max())
    _set_splits(3, lmax - prefix)
    splits = min(5, prefix // 16)
    pk, pv, table, first = _pool(k, v, lengths, n, prefix, page_rows, 'random', seed=2, f16=False)
    batch = _run_shared(q, pk, pv, table, first, lengths, n, prefix, page_rows, scale, splits)
    for i in np.nonzero(n)[0]:
        one = _run_shared(q[i:i + 1], pk, pv, table[i:i + 1], 0, lengths[i:i + 1], n[i:i + 1], prefix, page_rows, scale, splits, lmax=lmax)
        _bits_equal((batch[0][i:i + 1], batch[1][i:i + 1]), one, f'sequence {i} alone')


def test_combine_without_lse_leaves_the_suffix_lse_and_padded_rows_are_zero(npm):
    d, hq, hkv, b, t, prefix, page_rows = 64, 8, 2, 3, 2, 64, 16
    n = np.array([2, 0, 1])
    q, k, v, lengths = _shared_data(5, b, t, hq, hkv, d, prefix, [2, 9, 30], n)
    pk, pv, table, first = _pool(k, v, lengths, n, prefix, page_rows, 'random', seed=3, f16=False)
    scale = 1.0 / np.sqrt(d)
    full = _run_shared(q, pk, pv, table, first, lengths, n, prefix, page_rows, scale, 2)
    bare = _run_shared(q, pk, pv, table, first, lengths, n, prefix, page_rows, scale, 2, want_lse=False)
    assert np.array_equal(full[0].view(np.uint32), bare[0].view(np.uint32))
    assert (full[0][1] == 0).all() and (full[0][2, 1] == 0).all() and np.isneginf(full[1][1]).all() and np.isneginf(full[1][2, :, 1]).all()
    live = np.arange(t)[None, :] < n[:, None]
    assert (bare[1].transpose(0, 2, 1)[live] < full[1].transpose(0, 2, 1)[live]).all()     # the suffix alone weighs less than the whole


def test_prefix_bad_arguments_launch_nothing(npm):
    from np_modeling_amd import _C, device as D
    lib = _C.lib()
    buf = D.full([16 * 64 * 4 + 4096], SENTINEL)
    table = _ints([0, 1, 2, 3])
    c = _C.npm_mha_decode()
    c.batch, c.heads, c.kv_heads, c.new_tokens, c.kv_len, c.head_dim = 2, 4, 2, 1, 0, 32
    c.causal, c.scale = 1, 0.2
    c.q, c.q_pitch = buf.ptr, 128
    c.k, c.k_pitch, c.k_stride_b = buf.ptr, 64, 16 * 64
    c.v, c.v_pitch, c.v_stride_b = buf.ptr, 64, 16 * 64
    part = D.full([4096], SENTINEL)
    ok_args = dict(new=None, table=table.ptr, page=16, prefix=32, splits=2, pc=part.ptr, pl=part.ptr + 4 * 2048, f16=0)

    def call(**kw):
        a = dict(ok_args, **kw)
        return lib.npm_mha_prefix_fwd(C.byref(c), a['new'], a['table'], a['page'], a['prefix'], a['splits'], a['pc'], a['pl'], a['f16'])

    for bad in (dict(table=None), dict(page=8), dict(page=24), dict(prefix=0), dict(prefix=24), dict(prefix=-16), dict(splits=0),
                dict(splits=1025), dict(pc=None), dict(pl=None), dict(pc=part.ptr + 4)):
        rc = call(**bad)
        assert rc == 10002, (bad, rc)
    c.k_pitch, c.k_stride_b = 68, 16 * 68                                 # 4 elements of padding suit floats, not halves (16 bytes)
    assert call(f16=1) == 10002
    c.k_pitch, c.k_stride_b = 64, 16 * 64
    c.head_dim = 24
    assert call() == 10003
    c.head_dim = 32
    for args in ((None, part.ptr, 1, buf.ptr, 128, part.ptr), (part.ptr, None, 1, buf.ptr, 128, part.ptr), (part.ptr, part.ptr, 0, buf.ptr, 128, part.ptr),
                 (part.ptr, part.ptr, 1, None, 128, part.ptr), (part.ptr, part.ptr, 1, buf.ptr, 128, None), (part.ptr, part.ptr, 1, buf.ptr, 100, part.ptr)):
        assert lib.npm_attn_combine(args[0], args[1], args[2], args[3], args[4], args[5], 2, 1, 4, 32, None, 1) == 10002, args
    assert lib.npm_attn_combine(part.ptr, part.ptr, 1, buf.ptr, 128, part.ptr, 2, 1, 4, 24, None, 1) == 10003
    np.testing.assert_array_equal(buf.numpy(), SENTINEL)
    np.testing.assert_array_equal(part.numpy(), SENTINEL)


def test_the_split_rule_fills_the_chip_and_keeps_several_tiles(npm):
    from np_modeling_amd import _C
    lib = _C.lib()
    assert lib.npm_mha_prefix_splits(64, 64, 8, 8192) == 8                 # 8 row tiles x 8 heads x 8 splits = 512 blocks of 64 tiles
    assert lib.npm_mha_prefix_splits(8, 64, 8, 512) == 4                   # never fewer than 8 tiles (128 keys) in a split
    assert lib.npm_mha_prefix_splits(8, 8, 8, 64) == 1
    _C.check(lib.npm_set_tuning(PREFIX_KNOB, 7), 'npm_set_tuning')
    assert lib.npm_mha_prefix_splits(64, 64, 8, 8192) == 7
    assert lib.npm_set_tuning(PREFIX_KNOB, 1025) == 10002 and lib.npm_set_tuning(PREFIX_KNOB, -1) == 10002


# ---- the layer and the decoder with the switch on ----------------------------------------------------------------------------------
def _forked_layer(npm, att, f, dtype, tokens, steps, prompt_rows, page_size, seed, share=True):
    """A prompt into slot 0 of a batch of 4, forked into slots 1 and 2 (``share`` False: three prompts of their own), slot 3
    empty; then ``steps`` calls of ``tokens`` rows.  Outputs per step, the path of each, and the rows of the three sequences."""
    rng = np.random.default_rng(seed)
    prompt = rng.standard_normal([prompt_rows, f]).astype(np.float32)
    tails = [rng.standard_normal([steps * tokens, f]).astype(np.float32) for _ in range(3)]
    cache = att.make_cache(4, prompt_rows + steps * tokens, page_size=page_size, dtype=dtype)
    x = np.zeros([4, prompt_rows, f], dtype=np.float32)
    if share:
        x[0] = prompt
        att(x, cache=cache, new_lengths=[prompt_rows, 0, 0, 0])
        cache.fork(0, 1)
        cache.fork(0, 2)
    else:
        x[:3] = prompt
        att(x, cache=cache, new_lengths=[prompt_rows] * 3 + [0])
    outs, paths = [], []
    for s in range(steps):
        x = np.full([4, tokens, f], 2.5, dtype=np.float32)
        for i in range(3):
            x[i] = tails[i][s * tokens:(s + 1) * tokens]
        outs.append(np.asarray(att(x, cache=cache, new_lengths=[tokens] * 3 + [0])))
        paths.append(att._cached_path)
    return outs, paths, [np.concatenate([prompt, tail]) for tail in tails], cache


@pytest.mark.parametrize('dtype', ['f32', 'f16'])
@pytest.mark.parametrize('heads,kv_heads,f,tokens,path', [(8, 2, 512, 1, 'decode'), (8, 1, 512, 5, 'prefill'), (8, 8, 1024, 2, 'decode')])
def test_layer_with_the_switch_on(npm, monkeypatch, dtype, heads, kv_heads, f, tokens, path):
    """``_cached_path`` is 'decode_shared', or 'prefill_shared' at 40 score rows per K / V head; against float64 at the layer bound
    of tests/test_gpu_paged.py (f32), and against the switch off (two float32 evaluations: twice that bound).  A batch whose
    sequences do not share takes today's path, array_equal to the switch off."""
    D = npm.device
    monkeypatch.setattr(D, 'PREFILL_KERNEL', True)
    monkeypatch.setattr(D, 'PREFILL_KERNEL_F16', True)
    monkeypatch.setattr(D, 'SHARED_PREFIX_MIN_ROWS', 64)
    att, p = DC.make_mha(npm, f, heads, kv_heads, seed=heads + f, batch=4)
    runs = {}
    for on in (False, True):
        monkeypatch.setattr(D, 'SHARED_PREFIX', on)
        runs[on] = _forked_layer(npm, att, f, dtype, tokens, 3, 100, 16, seed=f)
        runs[on, 'own'] = _forked_layer(npm, att, f, dtype, tokens, 3, 100, 16, seed=f, share=False)
    assert runs[True][1] == [path + '_shared'] * 3 and runs[False][1] == [path] * 3
    assert runs[True, 'own'][1] == runs[False, 'own'][1] == [path] * 3
    for a, b in zip(runs[True, 'own'][0], runs[False, 'own'][0]):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), 'sequences that do not share: the switch changed a bit'
    for a, b in zip(runs[False][0], runs[False, 'own'][0]):                # forked (switch off) == each filled on its own
        assert np.array_equal(a[:3].view(np.uint32), b[:3].view(np.uint32))
    rows = runs[True][2]
    want = VR.layer_alone(p, rows, [[100] * 3] + [[tokens] * 3] * 3)
    for i in range(3):
        got = np.concatenate([o[i] for o in runs[True][0]])
        off = np.concatenate([o[i] for o in runs[False][0]])
        _layer_close(got, off, 2 * LAYER_TOL, f'shared {dtype} H{heads}/{kv_heads} T{tokens} sequence {i} vs the switch off')
        if dtype == 'f32':
            _layer_close(got, want[i][100:], LAYER_TOL, f'shared H{heads}/{kv_heads} T{tokens} sequence {i} vs float64')


@pytest.mark.parametrize('norm_first', [True, False])
def test_decoder_fork_and_decode_with_the_switch_on(npm, monkeypatch, norm_first):
    D = npm.device
    monkeypatch.setattr(D, 'SHARED_PREFIX', True)
    monkeypatch.setattr(D, 'SHARED_PREFIX_MIN_ROWS', 32)
    f = 256
    dec, p = DC.make_decoder(npm, f, 4, 2, 384, norm_first, True, seed=17, batch=3, seq_kv=23)
    rng = np.random.default_rng(3)
    kv = rng.standard_normal([3, 23, f]).astype(np.float32)
    prompt = rng.standard_normal([45, f]).astype(np.float32)
    tails = [rng.standard_normal([5, f]).astype(np.float32) for _ in range(3)]
    state = dec.start_decoding(kv, 56, page_size=16)
    q = np.zeros([3, 45, f], dtype=np.float32)
    q[0] = prompt
    dec.decode(q, state, new_lengths=[45, 0, 0])
    dec.fork(state, 0, 1)
    dec.fork(state, 0, 2)
    outs = []
    for s in range(5):
        outs.append(np.asarray(dec.decode(np.stack([tail[s:s + 1] for tail in tails]), state)))
        assert dec._self_attention._cached_path == 'decode_shared'
    assert state.self_cache.pages_in_use == 3 + 2 + 3 and state.self_cache.page_copies == 2
    rows = [np.concatenate([prompt, tail]) for tail in tails]
    want = VR.decoder_alone(p, rows, [[45] * 3] + [[1] * 3] * 5, np.repeat(kv[:1], 3, axis=0), [23] * 3, norm_first)
    for i in range(3):
        _layer_close(np.concatenate([o[i] for o in outs]), want[i][45:], 1e-4, f'shared decode sequence {i} vs float64')
